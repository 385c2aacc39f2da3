"""CPU checks of the GRU learner's embedding fold and its entry points (include/atr_gru_sums.h):
  * the fold's algebra in float64 against autograd through f + fc_action_tracker(one_hot(a)) -> nn.GRUCell;
  * the new header against the built library and fused.GRU_SUMS_PROTOTYPES (the parsing of tests/test_abi_cpu.py);
  * the build's scratch check covers every k_gru_bptt instantiation;
  * DeferredWeightGrads.add / add_all: row ranges, column blocks, all-or-none, check() keyed on the whole slice."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from conftest import ROOT
from test_abi_cpu import _header_functions, _py_class


def test_fold_algebra_in_float64_against_autograd():
    """T = 3, N = 5, episode ends mid-rollout. With dG = autograd's own dL/d ig [T N, 3R] and S[a] = its sum over the rows with
    tracker action a: S^T E + dG^T f = dW_ih, (S W_ih)^T = d fc_action_tracker.weight, its row sums = the bias gradient —
    1e-12 relative."""
    torch.manual_seed(11)
    T, N, Fd, R, A = 3, 5, 12, 8, 4
    cell = nn.GRUCell(Fd, R).double()
    fa = nn.Linear(A, Fd).double()
    head = torch.randn(T, N, R, dtype=torch.float64)
    f = torch.randn(T, N, Fd, dtype=torch.float64)
    a = torch.randint(0, A, (T, N))
    a[0, 0], a[1, 1], a[2, 2], a[0, 3] = 0, 1, 2, 3                 # every action occurs
    keep = torch.ones(T, N, dtype=torch.float64)
    keep[0, 1] = keep[1, 3] = keep[1, 0] = 0.0                      # episode ends after steps 0 and 1
    h = torch.randn(N, R, dtype=torch.float64)
    igs, loss = [], 0.0
    for t in range(T):
        x = f[t] + fa(nn.functional.one_hot(a[t], A).double())
        ig = x @ cell.weight_ih.t() + cell.bias_ih
        ig.retain_grad()
        igs.append(ig)
        hg = h @ cell.weight_hh.t() + cell.bias_hh
        r = torch.sigmoid(ig[:, :R] + hg[:, :R])
        z = torch.sigmoid(ig[:, R:2 * R] + hg[:, R:2 * R])
        n = torch.tanh(ig[:, 2 * R:] + r * hg[:, 2 * R:])
        h_new = (1 - z) * n + z * h
        with torch.no_grad():                                       # (the expressions above ARE nn.GRUCell's)
            assert float((h_new - cell(x, h)).abs().max()) <= 1e-12
        loss = loss + (h_new * head[t]).sum()
        h = h_new * keep[t].unsqueeze(1)
    loss.backward()
    dG = torch.cat([ig.grad for ig in igs], 0)                      # [T N, 3R]
    rows_a = a.reshape(T * N)
    S = torch.stack([dG[rows_a == k].sum(0) for k in range(A)], 0)  # [4, 3R]
    E = fa.weight.detach().t() + fa.bias.detach()                   # [4, F]: E[a] = fc_action_tracker(one_hot(a))
    W = cell.weight_ih.detach()

    def close(got, want):
        return float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float(cell.weight_ih.grad.abs().max()) > 0 and float(fa.weight.grad.abs().max()) > 0
    assert close(S.t() @ E + dG.t() @ f.reshape(T * N, Fd), cell.weight_ih.grad)
    dfa_w = (S @ W).t()                                             # [F, 4]
    assert close(dfa_w, fa.weight.grad)
    assert close(dfa_w.sum(1), fa.bias.grad)
    assert not close(dG.t() @ f.reshape(T * N, Fd), cell.weight_ih.grad)       # (the raw-feature product alone misses S^T E)


def test_sums_header_library_and_prototype_table_agree():
    from active_tracking_rl_amd import build, fused, vec_env
    build.build()
    assert os.path.join("..", "..", "include", "atr_gru_sums.h") in build.HEADERS
    assert '#include "atr_gru_sums.h"' in open(os.path.join(ROOT, "include", "atr_gru.h")).read()
    txt = open(os.path.join(ROOT, "include", "atr_gru_sums.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", txt).split("\n") if not ln.lstrip().startswith("#"))
    funcs = _header_functions(txt)
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    assert sorted(funcs) == sorted(fused.GRU_SUMS_PROTOTYPES) == ["atr_gru_bptt_act_sums_floats", "atr_gru_bptt_sums"]
    L = fused.lib()
    for name, (res, params) in funcs.items():
        assert hasattr(lib, name), name
        restype, argtypes = fused.GRU_SUMS_PROTOTYPES[name]
        assert _py_class(restype) == res and len(argtypes) == len(params), name
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _py_class(a) == c, (name, i)
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes
    # atr_gru_bptt's arguments up to dh_init, five more, then its P, T, N, R, stream
    bptt = fused.GRU_PROTOTYPES["atr_gru_bptt"][1]
    sums = fused.GRU_SUMS_PROTOTYPES["atr_gru_bptt_sums"][1]
    assert len(sums) == len(bptt) + 5 == 22 and sums[:12] == bptt[:12] and sums[-5:] == bptt[-5:]
    assert not set(fused.GRU_SUMS_PROTOTYPES) & (set(fused.ATR_PROTOTYPES) | set(fused.GRU_PROTOTYPES)
                                                 | set(fused.GRU_STEP_PROTOTYPES))
    assert L.atr_gru_bptt_act_sums_floats(40) == 3 * 4 * 384 and L.atr_gru_bptt_act_sums_floats(16) == 4 * 384
    # refusals come before any launch: missing sums / actions, another action table, a player outside the group
    args = [None] * 4 + [0, None, 0, None, None, None, 0, None]
    for tail in ([0, 4, None, 0, None, 1, 1, 16, 128, None], [0, 5, None, 0, None, 1, 1, 16, 128, None]):
        with pytest.raises(RuntimeError, match=r"^atr_gru_bptt_sums failed \(-1\)$"):
            L.atr_gru_bptt_sums(*(args + tail))


def test_build_checks_every_gru_bptt_instantiation_for_scratch():
    from active_tracking_rl_amd import build
    assert build.NO_SCRATCH_LEARNER == {"gru_hip.hip": "k_gru_bptt"} and "gru_hip.hip" in build.SOURCES
    assert not set(build.NO_SCRATCH) & set(build.NO_SCRATCH_LEARNER)
    rem = lambda name, n: ("x.hip:1:1: remark: Function Name: %s [-Rpass-analysis=kernel-resource-usage]\n"
                           "x.hip:1:1: remark:     ScratchSize [bytes/lane]: %d [-Rpass-analysis=kernel-resource-usage]\n" % (name, n))
    plain, sums = "_ZN3atr10k_gru_bpttILb0EEEvNS_7GruBpttE", "_ZN3atr10k_gru_bpttILb1EEEvNS_7GruBpttE"
    assert build.scratch_users(rem(plain, 0) + rem(sums, 0) + rem("_ZN3atr14k_gru_cell_fwdENS_6GruFwdE", 8), "k_gru_bptt") == []
    assert build.scratch_users(rem(plain, 0) + rem(sums, 24), "k_gru_bptt") == [(sums, 24)]


class _Bucket(object):
    def __init__(self, params):
        self.params = params
        self.grads = [torch.zeros_like(p) for p in params]

    def grad_views(self):
        return self.grads


def test_deferred_weight_grads_takes_row_ranges_and_column_blocks_all_or_none(monkeypatch):
    """DeferredWeightGrads.add_all on CPU stand-ins: CPU operands, a list longer than the room and a full group register
    nothing and raise nothing; then, with the device condition patched out of the way, the record of a row range (destination
    and bias views are the rows, check() is keyed on the WHOLE slice) and the alignment and shape refusals."""
    from active_tracking_rl_amd import fused
    R, Fd, K = 128, 256, 4096
    wih, whh, bih, bhh = torch.zeros(3 * R, Fd), torch.zeros(3 * R, R), torch.zeros(3 * R), torch.zeros(3 * R)
    q = fused.DeferredWeightGrads(_Bucket([wih, whh, bih, bhh]))
    dG, f, hm = torch.zeros(K, 4 * R), torch.zeros(K, Fd), torch.zeros(K, R)
    three = [dict(x1=dG[:, :3 * R], x2=f, weight=wih, biases=(bih,)),
             dict(x1=dG[:, :2 * R], x2=hm, weight=whh, biases=(bhh,), rows=(0, 2 * R)),
             dict(x1=dG[:, 3 * R:], x2=hm, weight=whh, biases=(bhh,), rows=(2 * R, 3 * R))]
    assert q.add_all(three) is None and q.problems == [] and q.registered == set() and q.K is None      # (CPU operands)
    monkeypatch.setattr(fused.DeferredWeightGrads, "MAX", 2)
    assert q.add_all(three) is None and q.problems == []                                                # (no room: not an error)
    q.problems = [None, None]
    assert q.add(dG, f, wih, biases=(bih,)) is None and len(q.problems) == 2                            # (full)
    q.problems = []
    monkeypatch.setattr(fused.DeferredWeightGrads, "MAX", 8)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    rec = q._problem(**three[2])
    assert rec is not None
    (x1, x2, dst, rs, shift, bv, M, N), (whole, bw) = rec
    assert (M, N) == (R, R) and x1.stride(0) == 4 * R and dst.data_ptr() == q.view(whh)[2 * R:].data_ptr()
    assert bv[0].data_ptr() == q.view(bhh)[2 * R:].data_ptr() and bv[0].shape == (R,)
    assert whole.data_ptr() == q.view(whh).data_ptr() and bw[0].data_ptr() == q.view(bhh).data_ptr()
    got = q.add_all(three)
    assert got is not None and len(q.problems) == 3 and q.K == K
    assert q.registered == {q.view(v).data_ptr() for v in (wih, whh, bih, bhh)}
    q.check([q.view(v) for v in (wih, whh, bih, bhh)])
    with pytest.raises(RuntimeError, match="grouped weight gradients"):
        q.check([q.view(wih), q.view(whh)[2 * R:], q.view(bih), q.view(bhh)])
    assert q._problem(x1=dG[:, 1:1 + R], x2=hm, weight=whh, rows=(0, R)) is None                         # (not 16-byte aligned)
    assert q._problem(x1=dG[:, :R], x2=hm, weight=whh, rows=(0, 2 * R)) is None                          # (shape of the rows)
