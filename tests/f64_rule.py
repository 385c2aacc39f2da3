"""The per-tensor float64 rule of tests/test_learner_f64_gpu.py for kernel-level tests, with that module's constants:
with e(x) = ||x - x64|| / ||x64||, a HIP result passes when e(hip) <= max(FACTOR e(aten32), floor) and e(aten32) <= ATEN_MAX,
where aten32 is the same expression in float32 through PyTorch's own ops on the GPU (floor = FLOOR, or HIDDEN_FLOOR for the
hidden and cell states the cell kernels write: their sigmoid / tanh are the hardware exp + reciprocal forms)."""
import numpy as np

import learner_f64
from learner_f64 import ATEN_MAX, FACTOR, FLOOR, HIDDEN_FLOOR  # noqa: F401  (re-exported)


class Table(object):
    """Collects (what, e(hip), e(aten32)) rows; finish() prints them all, then fails if any row missed the rule."""

    def __init__(self, label):
        self.label, self.rows, self.bad = label, [], []

    def rule(self, what, hip, x64, x32, floor=FLOOR):
        e_hip, e32 = learner_f64.rel_err(hip, x64), learner_f64.rel_err(x32, x64)
        allowed = max(FACTOR * e32, floor)
        self.rows.append((what, e_hip, e32))
        if not (np.isfinite(e_hip) and e_hip <= allowed):
            self.bad.append("%s: e(hip) %.3e > allowed %.3e (e(aten32) %.3e)" % (what, e_hip, allowed, e32))
        if not e32 <= ATEN_MAX:
            self.bad.append("%s: e(aten32) %.3e > %.0e: reference and floor disagree" % (what, e32, ATEN_MAX))

    def finish(self):
        for what, e_hip, e32 in self.rows:
            print("%-34s %-22s e(hip) %.3e  e(aten32) %.3e" % (self.label, what, e_hip, e32))
        assert not self.bad, "\n".join([self.label] + self.bad)
        return self.rows


def cell_recurrence(cells, feats, h0, c0, keep, go, gh, dtype, device):
    """The masked recurrence of P nn.LSTMCells or nn.GRUCells, one cell call per step and player, in `dtype` on `device`:
    feats [T, P, N, F], h0 / c0 [P, N, R] (c0 None for GRUCells), keep [T, N] (0 where the env ended at that step; applied AFTER
    the step, as Agent.action_train does), go [T, P, N, R], gh [P, N, R]. Returns a dict of detached tensors: h_seq [T, P, N, R]
    (un-masked step outputs), h_fin / c_fin (masked), and the gradients of sum(h_seq go) + sum(h_fin gh) w.r.t. every cell's
    weight_ih, weight_hh, bias_ih, bias_hh ("weight_ih[p]", ...), "feats", "h0" and (LSTM) "c0"."""
    import torch
    lstm = c0 is not None
    P = len(cells)
    mine = [type(c)(c.input_size, c.hidden_size).to(device=device, dtype=dtype) for c in cells]
    for a, b in zip(mine, cells):
        a.load_state_dict({k: v.detach().to(device=device, dtype=dtype) for k, v in b.state_dict().items()})
    leaf = lambda t: t.detach().to(device=device, dtype=dtype).requires_grad_(True)
    f, h_in = leaf(feats), leaf(h0)
    c_in = leaf(c0) if lstm else None
    k = keep.detach().to(device=device, dtype=dtype)
    h = list(h_in.unbind(0))
    c = list(c_in.unbind(0)) if lstm else None
    outs = []
    for t in range(f.shape[0]):
        kt = k[t].unsqueeze(1)
        if lstm:
            step = [mine[p](f[t, p], (h[p], c[p])) for p in range(P)]
            outs.append(torch.stack([s[0] for s in step], 0))
            h, c = [s[0] * kt for s in step], [s[1] * kt for s in step]
        else:
            step = [mine[p](f[t, p], h[p]) for p in range(P)]
            outs.append(torch.stack(step, 0))
            h = [s * kt for s in step]
    h_seq, h_fin = torch.stack(outs, 0), torch.stack(h, 0)
    names = ["%s[%d]" % (n, p) for p in range(P) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    wrt = [getattr(mine[p], n) for p in range(P) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    names += ["feats", "h0"] + (["c0"] if lstm else [])
    wrt += [f, h_in] + ([c_in] if lstm else [])
    obj = (h_seq * go.to(device=device, dtype=dtype)).sum() + (h_fin * gh.to(device=device, dtype=dtype)).sum()
    out = dict(zip(names, (g.detach() for g in torch.autograd.grad(obj, wrt))))
    out.update(h_seq=h_seq.detach(), h_fin=h_fin.detach())
    if lstm:
        out["c_fin"] = torch.stack(c, 0).detach()
    return out
