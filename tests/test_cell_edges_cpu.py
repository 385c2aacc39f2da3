"""tests/cell_edge_spec.py on its own, without a GPU: the ladder, the float64 references against nn.LSTMCell / nn.GRUCell autograd,
the derived bounds E_SIG / E_TANH / bound_* against a float32 emulation of the hardware forms, that the bounds reject the rewrites
they exist for, and that the peaked heads cases are peaked and have a usable float32 reference.

Measured here (numpy float32 emulation, the ladder + 4M log-uniform points in [1e-8, 200]):
  emulated sigmoid  exp2 and rcp correctly rounded: max err 9.3e-08; each on the far side of its exact result: <= 1.24e-07   E_SIG  1.653e-07
  emulated tanh                                             1.8e-07;                                          <= 2.49e-07   E_TANH 3.605e-07
  emulated cells, largest err / allowed over every output and every perturbation: LSTM forward 0.37, backward 0.38 (PRE 0.36), GRU
  forward 0.36, backward 0.50 (dh z, one product: U |v| against 2 U |v|)
  peaked heads in float32 on the CPU: e(aten32) <= 7.4e-06 over every quantity; 2433 .. 3517 of 8195 rows and 314 .. 452 of 777 with
  p_max == 1.0f; smallest log p(a) -90 .. -204
"""
import numpy as np
import pytest
import torch

import cell_edge_spec as spec
from f64_rule import ATEN_MAX, cell_recurrence
from learner_f64 import rel_err
from test_hidden_sizes_gpu import GRAD_NAMES, STAT_NAMES, _heads_reference

MILD = spec.LADDER[np.abs(spec.LADDER) <= 4.0]
PUSHES = [(pe, pr) for pe in (-1, 0, 1) for pr in (-1, 0, 1)]
SATURATED = np.array([44.4, 45.0, 88.8, 89.0, 100.0, 1e4, 3e38], dtype=np.float32)


def _close(a, b, what):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), (what, float((a - b).abs().max()))


# ---- the ladder ----------------------------------------------------------------------------------------------------------------
def test_the_ladder_and_the_draw():
    L = spec.LADDER
    assert np.isfinite(L).all() and L.dtype == np.float32 and np.array_equal(np.sort(L), L)
    for v in (0.0, 2.0 ** -149, 2.0 ** -126, 1e-8, 1e-4, 0.5, 1, 4, 8.3, 8.4, 16.6, 16.7, 20, 44.3, 44.4, 45, 88.7, 88.8, 89, 100, 1e4, 3e38):
        assert np.float32(v) in L and np.float32(-v) in L, v
    assert np.signbit(L[L == 0]).tolist() == [True, False]
    assert float(np.abs(spec.C_LADDER).max()) == float(np.float32(45.0)) and set(spec.C_LADDER.tolist()) <= set(L.tolist())
    assert set(np.abs(spec.C_RANGE_ONLY).tolist()) == {float(np.float32(1e4)), float(np.float32(3e38))}
    x = spec.draw((2048, 512), 1)
    assert x.dtype == np.float32 and np.isfinite(x).all() and np.array_equal(x, spec.draw((2048, 512), 1))
    for v in L[L != 0]:
        assert (x == v).any(), v
    assert (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any()
    off = ~np.isin(x, L)
    assert 0.45 < off.mean() < 0.55 and float(np.abs(x[off]).max()) <= 200.0 and float(np.abs(x[off]).min()) >= 0.99e-8
    assert len(np.unique(np.floor(np.log2(np.abs(x[off]))))) >= 34           # every binade of [1e-8, 200]
    c = spec.draw((512, 128), 2, ladder=spec.C_LADDER, top=64.0)
    assert float(np.abs(c).max()) <= 64.0


# ---- the references against autograd -------------------------------------------------------------------------------------------
def _mild(shape, seed):
    return torch.from_numpy(spec.draw(shape, seed, ladder=MILD, top=4.0).astype(np.float64))


def _setup(T, cell_type, gates, seed):
    P, N, R = 2, 6, 8
    g = torch.Generator().manual_seed(seed)
    cells = []
    for p in range(P):
        c = cell_type(gates * R, R).double()
        with torch.no_grad():
            c.weight_ih.copy_(torch.eye(gates * R))
            c.bias_ih.zero_()
            c.bias_hh.copy_(torch.randn(gates * R, generator=g) * (0.3 if gates == 3 else 0.0))
            c.weight_hh.copy_(torch.randn(gates * R, R, generator=g) * 0.4)
        cells.append(c)
    keep = (torch.rand(T, N, generator=g) > 0.35).double()
    go = torch.randn(T, P, N, R, generator=g).double()
    return P, N, R, cells, keep, go


@pytest.mark.parametrize("T", [1, 3])
def test_the_lstm_references_equal_lstmcell_autograd(T):
    P, N, R, cells, keep, go = _setup(T, torch.nn.LSTMCell, 4, 10 + T)
    feats, h0, c0 = _mild((T, P, N, 4 * R), 20 + T), _mild((P, N, R), 30 + T), _mild((P, N, R), 40 + T)
    assert T == 1 or 0 < int((keep[:-1] == 0).sum())
    want = cell_recurrence(cells, feats, h0, c0, keep, go, torch.zeros(P, N, R), torch.float64, "cpu")
    whh = torch.stack([c.weight_hh.detach() for c in cells], 0)                   # [P, 4R, R]
    h_all, c_all, gates = torch.zeros(P, T + 1, N, R).double(), torch.zeros(P, T + 1, N, R).double(), torch.zeros(P, T, N, 4 * R).double()
    h_all[:, 0], c_all[:, 0] = h0, c0
    for t in range(T):
        k = torch.ones(N).double() if t == 0 else keep[t - 1]
        pre = feats[t] + torch.bmm(k.view(1, N, 1) * h_all[:, t], whh.transpose(1, 2))
        o = spec.lstm_fwd_expr(spec.F64(), *(x.numpy() for x in spec.split4(pre)), c_all[:, t].numpy(), k.view(1, N, 1).numpy())
        gates[:, t] = torch.from_numpy(np.concatenate([o["i"], o["f"], o["g"], o["o"]], -1))
        h_all[:, t + 1], c_all[:, t + 1] = torch.from_numpy(o["h"]), torch.from_numpy(o["c"])
    _close(h_all[:, 1:].transpose(0, 1), want["h_seq"], "h_seq")
    dh = go.transpose(0, 1)
    got = spec.lstm_bptt_ref(keep, gates, c_all, h_all, dh, whh, torch.float64, "cpu")
    _close(got["dG"].transpose(0, 1), want["feats"], "dG")
    _close(got["dh0"], want["h0"], "dh0")
    _close(got["dc0"], want["c0"], "dc0")
    for p in range(P):
        _close(got["dW_hh"][p].t(), want["weight_hh[%d]" % p], "dW_hh")
    # the PRE form of the same: pre-activations in, activated inside
    pre_all = torch.stack([feats[t] + torch.bmm((torch.ones(N).double() if t == 0 else keep[t - 1]).view(1, N, 1) * h_all[:, t],
                                                whh.transpose(1, 2)) for t in range(T)], 1)
    again = spec.lstm_bptt_ref(keep, pre_all, c_all, h_all, dh, whh, torch.float64, "cpu", pre=True)
    _close(again["dG"], got["dG"], "dG from pre-activations")
    # the one-step expressions the per-element bounds propagate through are these
    if T == 1:
        e = spec.lstm_bwd_expr(spec.F64(), [x.numpy() for x in spec.split4(gates[:, 0])], c_all[:, 1].numpy(), c_all[:, 0].numpy(),
                               dh[:, 0].numpy(), np.ones((1, N, 1)))
        _close(np.concatenate([e["di"], e["df"], e["dg"], e["do"]], -1), got["dG"][:, 0], "one-step dG")
        _close(e["dc0"], got["dc0"], "one-step dc0")
        b = spec.bound_lstm_bwd([x.numpy() for x in spec.split4(gates[:, 0])], c_all[:, 1].numpy(), c_all[:, 0].numpy(),
                                dh[:, 0].numpy(), np.ones((1, N, 1)))
        _close(b["df"][0], e["df"], "the bound's own value")


@pytest.mark.parametrize("T", [1, 3])
def test_the_gru_references_equal_grucell_autograd(T):
    P, N, R, cells, keep, go = _setup(T, torch.nn.GRUCell, 3, 50 + T)
    feats, h0 = _mild((T, P, N, 3 * R), 60 + T), _mild((P, N, R), 70 + T)
    want = cell_recurrence(cells, feats, h0, None, keep, go, torch.zeros(P, N, R), torch.float64, "cpu")
    whh = torch.stack([c.weight_hh.detach() for c in cells], 0)                   # [P, 3R, R]
    bhh = torch.stack([c.bias_hh.detach() for c in cells], 0).view(P, 1, 3 * R)
    h_all, acts = torch.zeros(P, T + 1, N, R).double(), torch.zeros(P, T, N, 4 * R).double()
    h_all[:, 0] = h0
    for t in range(T):
        k = (torch.ones(N).double() if t == 0 else keep[t - 1]).view(1, N, 1)
        hg = torch.bmm(k * h_all[:, t], whh.transpose(1, 2)) + bhh
        x = feats[t] + hg
        q = hg[..., 2 * R:]
        o = spec.gru_fwd_expr(spec.F64(), x[..., :R].numpy(), x[..., R:2 * R].numpy(), feats[t][..., 2 * R:].numpy(), q.numpy(),
                              (k * h_all[:, t]).numpy())
        acts[:, t] = torch.from_numpy(np.concatenate([o["r"], o["z"], o["n"], q.numpy()], -1))
        h_all[:, t + 1] = torch.from_numpy(o["h"])
    _close(h_all[:, 1:].transpose(0, 1), want["h_seq"], "h_seq")
    dh = go.transpose(0, 1)
    got = spec.gru_bptt_ref(keep, acts, h_all, dh, whh, torch.float64, "cpu")
    _close(got["dG"][..., :3 * R].transpose(0, 1), want["feats"], "dG")
    _close(got["dh0"], want["h0"], "dh0")
    for p in range(P):
        _close(got["dW_hh"][p].t(), want["weight_hh[%d]" % p], "dW_hh")
        _close(got["db_hh"][p], want["bias_hh[%d]" % p], "db_hh")
    if T == 1:
        r, z, n, q = (x.numpy() for x in spec.split4(acts[:, 0]))
        e = spec.gru_bwd_expr(spec.F64(), r, z, n, q, h_all[:, 0].numpy(), dh[:, 0].numpy())
        _close(np.concatenate([e["dr"], e["dz"], e["dn"], e["dq"]], -1), got["dG"][:, 0], "one-step dG")
        whh0 = torch.zeros_like(whh)
        _close(e["direct"], spec.gru_bptt_ref(keep, acts, h_all, dh, whh0, torch.float64, "cpu")["dh0"], "one-step dh0 at W_hh = 0")


# ---- the emulation inside the derived bounds -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    rng = np.random.default_rng(0)
    n = 4_000_000
    x = np.exp(rng.uniform(np.log(1e-8), np.log(200.0), n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    x = np.concatenate([spec.LADDER, x.astype(np.float32)])
    return x, spec.sigmoid64(x), spec.tanh64(x)


def test_the_derived_bounds_are_what_the_docstring_says():
    assert abs(spec.E_SIG - 1.653e-7) < 1e-10 and abs(spec.E_TANH - 3.605e-7) < 1e-10
    assert abs(spec.K_SIG - 0.2239) < 1e-4 and abs(spec.K_TANH - 0.4477) < 1e-4 and 7.2e-8 < spec.REL_ARG < 7.4e-8


@pytest.mark.parametrize("pe,pr", PUSHES)
def test_the_emulated_forms_stay_within_e_sig_and_e_tanh(sweep, pe, pr):
    x, s64, t64 = sweep
    s, t = spec.emu_sigmoid(x, pe, pr), spec.emu_tanh(x, pe, pr)
    assert np.isfinite(s).all() and np.isfinite(t).all()
    assert float(s.min()) >= 0.0 and float(s.max()) <= 1.0 and float(t.min()) >= -1.0 and float(t.max()) <= 1.0
    es, et = np.abs(s.astype(np.float64) - s64), np.abs(t.astype(np.float64) - t64)
    print("push exp %+d rcp %+d: sigmoid %.3e at %s, tanh %.3e at %s" % (pe, pr, es.max(), spec.where_on_ladder(x[es.argmax()]),
                                                                         et.max(), spec.where_on_ladder(x[et.argmax()])))
    assert float(es.max()) <= spec.E_SIG and float(et.max()) <= spec.E_TANH
    # saturation is exact where the docstring says so
    big = x[np.abs(x) >= 100.0]
    assert np.array_equal(spec.emu_sigmoid(big, pe, pr), (big > 0).astype(np.float32))
    assert np.array_equal(spec.emu_tanh(big, pe, pr), np.sign(big))


def _cell_inputs(R=16, N=2048):
    ig = spec.draw((N, 4 * R), 101)
    cp = spec.draw((N, R), 102, ladder=spec.C_LADDER, top=64.0)
    k = (np.arange(N) % 3 != 0).astype(np.float32).reshape(N, 1)
    dh = np.random.default_rng(103).standard_normal((N, R)).astype(np.float32)
    return ig, cp, k, dh


def _ratios(label, got, want):
    worst = 0.0
    for name in want:
        ratio, at, err = spec.worst(got[name], want[name][0], want[name][1])
        print("%-28s %-7s err / allowed %.3f (err %.3e)" % (label, name, ratio, err))
        worst = max(worst, ratio)
    return worst


def _emu_ops(pe, pr, **forms):
    return spec.Emu32(sig=lambda x: spec.emu_sigmoid(x, pe, pr, form=forms.get("sig", "hw")),
                      tanh=lambda x: spec.emu_tanh(x, pe, pr, form=forms.get("tanh", "hw")))


def _lstm_emulated(ops):
    """Emulated LSTM forward, then backward from ITS stores in both forms -> (got, want) dict pairs per stage."""
    ig, cp, k, dh = _cell_inputs()
    parts = spec.split4(ig)
    fwd = spec.lstm_fwd_expr(ops, *parts, cp, k)
    out = [("lstm forward", fwd, spec.bound_lstm_fwd(*parts, cp, k))]
    if all(np.isfinite(fwd[n]).all() for n in fwd):
        gates = [fwd[n] for n in "ifgo"]
        out.append(("lstm backward", spec.lstm_bwd_expr(ops, gates, fwd["c"], cp, dh, k), spec.bound_lstm_bwd(gates, fwd["c"], cp, dh, k)))
        out.append(("lstm backward PRE", spec.lstm_bwd_expr(ops, parts, fwd["c"], cp, dh, k, activate=True),
                    spec.bound_lstm_bwd(parts, fwd["c"], cp, dh, k, activate=True)))
    return out


def _gru_emulated(ops):
    R, N = 16, 2048
    ig = spec.draw((N, 3 * R), 111)
    hg = spec.draw((N, 3 * R), 112, ladder=spec.C_LADDER, top=64.0)
    hp = spec.draw((N, R), 113, ladder=spec.C_LADDER, top=64.0)
    k = (np.arange(N) % 3 != 0).astype(np.float32).reshape(N, 1)
    dh = np.random.default_rng(114).standard_normal((N, R)).astype(np.float32)
    hm = (k * hg).astype(np.float32)
    args = (spec.f32_sum(ig[:, :R], hm[:, :R]), spec.f32_sum(ig[:, R:2 * R], hm[:, R:2 * R]), ig[:, 2 * R:], hm[:, 2 * R:], k * hp)
    fwd = spec.gru_fwd_expr(ops, *args)
    out = [("gru forward", fwd, spec.bound_gru_fwd(*args))]
    if all(np.isfinite(fwd[n]).all() for n in fwd):
        st = (fwd["r"], fwd["z"], fwd["n"], args[3], args[4], dh)
        out.append(("gru backward", spec.gru_bwd_expr(ops, *st), spec.bound_gru_bwd(*st)))
    return out


@pytest.mark.parametrize("pe,pr", PUSHES)
def test_the_emulated_cells_stay_within_the_propagated_bounds(pe, pr):
    for label, got, want in _lstm_emulated(_emu_ops(pe, pr)) + _gru_emulated(_emu_ops(pe, pr)):
        assert all(np.isfinite(got[n]).all() for n in got), label
        assert _ratios("%s push %+d %+d" % (label, pe, pr), got, want) <= 1.0, label
    stages = [s[0] for s in _lstm_emulated(_emu_ops(pe, pr))]
    assert stages == ["lstm forward", "lstm backward", "lstm backward PRE"]


# ---- the bounds bite -----------------------------------------------------------------------------------------------------------
def test_the_rewrites_are_rejected_and_a_libm_tanh_passes(sweep):
    x, s64, t64 = sweep
    # (a) tanh as (e^2x - 1) / (e^2x + 1): inf / inf from 44.4 up; (b) sigmoid as e^x / (1 + e^x): from 88.8 up
    ta, sb = spec.emu_tanh(spec.LADDER, form="ratio"), spec.emu_sigmoid(spec.LADDER, form="ratio")
    assert np.isnan(ta[np.isin(spec.LADDER, SATURATED)]).all() and np.isfinite(ta[spec.LADDER < 44.35]).all()
    assert np.isnan(sb[np.isin(spec.LADDER, SATURATED[2:])]).all() and np.isfinite(sb[spec.LADDER < 88.75]).all()
    for got, want, bound in ((ta, spec.tanh64(spec.LADDER), spec.E_TANH), (sb, spec.sigmoid64(spec.LADDER), spec.E_SIG)):
        assert spec.worst(got, want, bound)[0] > 1.0
    # through the cell bounds as well
    for ops in (_emu_ops(0, 0, sig="ratio"), _emu_ops(0, 0, tanh="ratio")):
        label, got, want = _lstm_emulated(ops)[0]
        assert _ratios("rewrite: " + label, got, want) > 1.0
        label, got, want = _gru_emulated(ops)[0]
        assert _ratios("rewrite: " + label, got, want) > 1.0
    # a tanh of libm accuracy is inside everything
    assert float(np.abs(spec.emu_tanh(x, form="libm").astype(np.float64) - t64).max()) <= spec.E_TANH
    for label, got, want in _lstm_emulated(_emu_ops(0, 0, tanh="libm")) + _gru_emulated(_emu_ops(0, 0, tanh="libm")):
        assert _ratios("libm tanh: " + label, got, want) <= 1.0, label
    # and an error of 3 E at one point is not
    off = spec.emu_sigmoid(spec.LADDER).astype(np.float64)
    off[30] += 3 * spec.E_SIG
    assert spec.worst(off, spec.sigmoid64(spec.LADDER), spec.E_SIG)[0] > 1.0


# ---- the peaked heads cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aux", [False, True])
@pytest.mark.parametrize("R,rows,A,wfac,rfac", spec.HEADS_CASES)
def test_the_peaked_heads_cases_are_peaked_and_float32_resolves_them(R, rows, A, wfac, rfac, aux):
    x = spec.heads_problem(R, rows, A, wfac, rfac, aux)
    worst = 0.0
    for p in range(2):
        args = (x["hs"][p], x["prm"][p], x["store"][:, p].reshape(rows), x["ret"][:, :, p], x["gae"][:, :, p], x["rew"][:, :, 0],
                x["scale"][p], x["scale_aux"], x["w_ent"][p])
        r64, r32 = _heads_reference(*args, torch.float64), _heads_reference(*args, torch.float32)
        names = [("values", r64["values"], r32["values"]), ("objective", r64["objective"], r32["objective"])]
        names += [(n, r64["stats"][k], r32["stats"][k]) for k, n in enumerate(STAT_NAMES) if not (n == "aux" and len(x["prm"][p]) == 4)]
        names += [(n, a, b) for n, a, b in zip(GRAD_NAMES, r64["grads"], r32["grads"])]
        for n, a, b in names:
            e = rel_err(b, a)
            worst = max(worst, e)
            assert e <= ATEN_MAX, (p, n, e)
        wa, ba = x["prm"][p][0], x["prm"][p][1]
        logp32 = torch.log_softmax(x["hs"][p] @ wa.t() + ba, 1)
        peaked = int((logp32.exp().max(1).values == 1.0).sum())
        lpa = torch.log_softmax(x["hs"][p].double() @ wa.double().t() + ba.double(), 1).gather(1, x["store"][:, p].reshape(rows, 1))
        print("heads R=%d rows=%d A=%d player %d: %d rows with p_max == 1.0f, min log p(a) %.1f, worst e(aten32) so far %.2e"
              % (R, rows, A, p, peaked, float(lpa.min()), worst))
        assert peaked > rows // 4 and float(lpa.min()) < -80.0
        assert float(r64["stats"][2]) >= 0.0 and bool(torch.isfinite(r64["stats"]).all())
