"""-m gpu: the default learner's recurrence backward at kernel level against float64 autograd — the one-launch LSTM BPTT in its
three forms (csrc/bptt_hip.hip: stored gates; stored pre-activations re-activated in registers; those plus the tracker-action
embedding and the by-action column sums of dG), atr_embed_fold (csrc/driver_hip.hip: k_sact_reduce + k_embed_fold) and the autograd
node around them (fused.lstm_sequence_cached), on hand-built stores at R = 128, F = 256.

The reference is tests/lstm_bptt_spec.py (tested on its own by tests/test_lstm_bptt_ref_cpu.py): nn.LSTMCell per step and player in
float64 on the CPU, objective sum(h_seq go); the stores are its forward pass rounded to float32 once. Every comparison is the rule of
tests/f64_rule.py, unchanged: e(hip) <= max(4 e(aten32), floor) and e(aten32) <= 1e-4, aten32 = the same function in float32 on the
GPU. Outputs are NaN-poisoned before every call and checked finite afterwards.

  1 the kernel's three forms: dG, dh0, dc0, dW_hh per player     2 the by-action sums against float64 and against the kernel's own dG
  3 atr_embed_fold alone from random per-tile sums               4 the node: every gradient, what `need` switches off, what was launched

Measured on MI355X over every case (floor = FLOOR = 1e-6 everywhere: the PRE forms, which evaluate four more hardware sigmoid / tanh
per element, stay under it too and get no HIDDEN_FLOOR):
  1 stored gates  dG      e(hip) 8.6e-08 .. 1.1e-07    e(aten32) 2.1e-07 .. 3.5e-07    e(hip) / allowed <= 0.11
                  dh0     e(hip) 2.7e-07 .. 2.9e-07    e(aten32) 4.0e-07 .. 5.1e-07    e(hip) / allowed <= 0.17
                  dc0     e(hip) 9.8e-08 .. 1.2e-07    e(aten32) 1.3e-07 .. 2.3e-07    e(hip) / allowed <= 0.12
                  dW_hh   e(hip) 8.9e-08 .. 8.2e-07    e(aten32) 2.3e-07 .. 8.7e-07    e(hip) / allowed <= 0.24
    PRE, PRE+emb  dG      e(hip) 1.2e-07 .. 1.7e-07    (e(aten32): the same reference)   e(hip) / allowed <= 0.16
                  dh0     e(hip) 2.7e-07 .. 3.2e-07                                      e(hip) / allowed <= 0.17
                  dc0     e(hip) 1.0e-07 .. 1.4e-07                                      e(hip) / allowed <= 0.14
                  dW_hh   e(hip) 1.2e-07 .. 8.2e-07                                      e(hip) / allowed <= 0.24
    (dW_hh's 8.2e-07 is the 2050-row case: that product is torch.bmm's, and aten32's own is 8.7e-07 there)
  2 S[action]             e(hip) 1.4e-07 .. 2.0e-07    e(aten32) 1.9e-07 .. 4.1e-07    e(hip) / allowed <= 0.16
    against the kernel's own dG: err 0 (one row: the sum is the term) .. 8.3e-07; smallest slack under the bound 2.9e-09 at 16 rows
    (3 .. 5 terms per entry), 5.0e-08 at 34, 1.1e-03 at 2050
  3 S                     e(hip) 0 .. 1.1e-07          e(aten32) 0 .. 1.2e-07          e(hip) / allowed <= 0.11
    dwih                  e(hip) 3.9e-08 .. 1.3e-07    e(aten32) 3.7e-08 .. 1.3e-07    e(hip) / allowed <= 0.13
    dfa_w, dfa_b          e(hip) 1.2e-07 .. 1.8e-07    e(aten32) 3.2e-07 .. 4.8e-07    e(hip) / allowed <= 0.12
  4 feats                 e(hip) 3.9e-07 .. 4.0e-07    e(aten32) 4.8e-07 .. 5.1e-07    e(hip) / allowed <= 0.21
    weight_ih, weight_hh  e(hip) 1.8e-07 .. 3.4e-07    e(aten32) 3.2e-07 .. 4.1e-07    e(hip) / allowed <= 0.23
    bias_ih, bias_hh      e(hip) 1.5e-07 .. 1.8e-07    e(aten32) 2.8e-07 .. 3.6e-07    e(hip) / allowed <= 0.15
    fa.weight, fa.bias    e(hip) 1.8e-07 .. 2.5e-07 folded, 3.1e-07 .. 4.5e-07 explicit    e(aten32) 4.2e-07 .. 6.1e-07    <= 0.20

What it resolves: each of these one-line changes, made on a scratch copy of the library and run once on MI355X (never committed),
fails the file; first failing row and its e(hip), with what else failed:
  (a) `dcn = dcc[i]` without `ko[i]` (csrc/bptt_hip.hip)      bptt 2x2x17 gates: dc0[1] 3.5e-01 (dG 2.1e-01, dh0 3.0e-01, dW_hh 2.7e-01);
      every case with T >= 2 in 1, 2 and 4 (31 tests); the T = 1 cases pass, as they must
  (b) `ki[i]` dropped from `d_f`                              bptt 2x2x17 gates: dG[1] 1.3e-01, alone: dh0, dc0 and dW_hh pass, since
      the rows it changes carry k h_prev = 0; sums 2x2x17: S[action 1] 2.0e-01; node: weight_ih 1.1e-01 .. 1.5e-01 (31 tests)
  (c) `ra = ai[i]` regardless of `ok[i]`                      sums 2x2x17 (and 1x1x1, 2x7x37, 2x2x130, 2x1x2050: every ragged last
      tile; 1x1x16 passes): S is not the sum of the kernel's own dG; node-2x2x17 fold: fa.weight 4.1e+00, weight_ih[1] 1.1e+00;
      dG, dh0, dc0, dW_hh and the explicit node untouched (13 tests)
  (d) `bo` not added in the PRE form                          bptt 1x1x1 pre: dG[0] 3.5e-02 (dh0 3.6e-02, dc0 3.0e-02, dW_hh 3.5e-02);
      every case, both PRE forms, the sums and the node; the stored-gates form passes (37 tests)
  (e) the `S[3 * J + j]` term left out of k_embed_fold's dW_ih line (csrc/driver_hip.hip)
                                                              embed_fold tiles=1 J=512 C=256: dwih 2.8e-01 (all 24 shapes, 2.5e-01 ..
      5.6e-01; S, dfa_w, dfa_b pass); node fold: weight_ih[1] 1.3e-01 .. 1.9e-01 (32 tests)
"""
import contextlib

import pytest
import torch

import lstm_bptt_spec as spec
from f64_rule import Table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R, GATES = spec.R, spec.GATES
FORMS = ("gates", "pre", "pre+emb")


@contextlib.contextmanager
def _poisoned_allocations(monkeypatch):
    """torch.empty / torch.empty_like hand out NaN-filled float tensors: whatever the code under test allocates for its outputs is
    poisoned before the kernels write it."""
    real, real_like = torch.empty, torch.empty_like

    def nan(t):
        return t.fill_(float("nan")) if t.is_floating_point() else t
    with monkeypatch.context() as m:
        m.setattr(torch, "empty", lambda *a, **k: nan(real(*a, **k)))
        m.setattr(torch, "empty_like", lambda *a, **k: nan(real_like(*a, **k)))
        yield


_ON_GPU = {}


def _problem(name):
    """(inputs, float64 reference, aten32 reference, stores on the GPU) of a named case: made once, shared, never written."""
    if name not in _ON_GPU:
        x, ref = spec.problem(name)
        x32 = spec.reference(x, torch.float32, DEV)
        _ON_GPU[name] = (x, ref, x32, spec.stores(x, ref, DEV))
    return _ON_GPU[name]


def _bptt(s, case, form, monkeypatch, want_sums=True):
    """fused._lstm_bptt on the stores `s` in one of the three forms -> (dG [P, T, N, 4R], dh0, dc0, dW_hh [P, 4R, R], pre dict)."""
    from active_tracking_rl_amd import fused
    pre, acts = None, s["acts"]
    if form == "pre":
        pre, acts = dict(bias=s["bias"]), s["pre_with_emb"]
    elif form == "pre+emb":
        pre, acts = dict(bias=s["bias"], emb=s["emb"], emb_player=case.emb_player, act=s["act"], want_sums=want_sums), s["pre"]
    with _poisoned_allocations(monkeypatch):
        dG, dh0, dc0, dwhh = fused._lstm_bptt(None, s["keep"], s["h_all"], s["c_all"], acts, s["dh"], whh_nn=s["whh"], pre=pre)
    torch.cuda.synchronize()
    for t in (dG, dh0, dc0, dwhh):
        assert bool(torch.isfinite(t).all())
    return dG.view(case.P, case.T, case.N, GATES), dh0, dc0, dwhh.transpose(1, 2), pre


def _finish(tables, more=()):
    """Every table printed, then one failure that names every row that missed the rule (and what `more` holds)."""
    bad = list(more)
    for tab in tables:
        try:
            tab.finish()
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(spec.CASES))
def test_the_three_forms_of_the_bptt_launch_against_float64(name, monkeypatch):
    """1. fused._lstm_bptt with pre=None, with pre (no embedding table: the embedding's projection is in the stored
    pre-activations) and with pre + emb + want_sums: dG, dh0, dc0 and dW_hh per player under the rule. The player whose dL/dh_seq
    is None has exactly zero gradients. An 8-row embedding table gets no sums (pre["act_sums"] is None)."""
    from active_tracking_rl_amd import fused
    monkeypatch.setattr(fused, "use_fused_bptt", True)
    x, ref, x32, s = _problem(name)
    case = x["case"]
    launched = spec.Spy(monkeypatch, ("atr_lstm_bptt", "atr_lstm_bptt_pre2", "atr_lstm_cell_backward"))
    tables = []
    for form in FORMS:
        dG, dh0, dc0, dwhh, pre = _bptt(s, case, form, monkeypatch)
        if form == "pre+emb":
            if case.n_act == spec.N_ACT:
                assert pre["act_sums"] is not None and pre["act_sums"].numel() == (case.N + 15) // 16 * 4 * GATES
            else:
                assert pre["act_sums"] is None
        tab = Table("bptt %s %s" % (name, form))
        tables.append(tab)
        for p in range(case.P):
            rows = (("dG[%d]" % p, dG[p], ref["dG"][p], x32["dG"][p]), ("dh0[%d]" % p, dh0[p], ref["h0"][p], x32["h0"][p]),
                    ("dc0[%d]" % p, dc0[p], ref["c0"][p], x32["c0"][p]),
                    ("dW_hh[%d]" % p, dwhh[p], ref["weight_hh[%d]" % p], x32["weight_hh[%d]" % p]))
            for what, hip, r64, r32 in rows:
                if p == case.no_dh:
                    assert float(hip.abs().max()) == 0.0 and float(r64.abs().max()) == 0.0, what
                else:
                    tab.rule(what, hip, r64, r32)
    _finish(tables)
    assert launched.calls == ["atr_lstm_bptt", "atr_lstm_bptt_pre2", "atr_lstm_bptt_pre2"]


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, c in spec.CASES.items() if c.n_act == spec.N_ACT])
def test_the_by_action_sums_against_float64_and_the_kernels_own_dg(name, monkeypatch):
    """2. act_sums summed over the tiles in float64, S [4, 4R]: under the rule against the float64 reference dG grouped by action
    (aten32: the float32 reference dG through a float32 one-hot product), per action that a row took; against the float64 sum of the
    kernel's own dG within T N 2^-24 sum|terms| per entry (tests/test_gru_learner_gpu.py's bound: an f32 sum of that many terms in
    any order; rows past N counted nowhere); an absent action's block exactly zero in every tile; the buffer's size; and no sums
    for a table that is not the four-move one (-1)."""
    from active_tracking_rl_amd import fused
    monkeypatch.setattr(fused, "use_fused_bptt", True)
    x, ref, x32, s = _problem(name)
    case = x["case"]
    P, T, N, ep = case.P, case.T, case.N, case.emb_player
    L = fused.lib()
    tiles = (N + 15) // 16
    assert L.atr_lstm_bptt_act_sums_floats(N) == tiles * 4 * 512
    dG, dh0, dc0, _, pre = _bptt(s, case, "pre+emb", monkeypatch)
    sums = pre["act_sums"]
    assert sums.numel() == tiles * 4 * 512 and bool(torch.isfinite(sums).all())
    part = sums.view(tiles, 4, GATES).double().cpu()
    S = part.sum(0)
    act = x["store"][:, 0]
    S64 = spec.by_action(ref["dG"][ep], act)
    S32 = spec.by_action(x32["dG"][ep], s["act"])
    own = dG[ep].double().cpu()
    tab, off = Table("sums %s" % name), []
    for k in range(4):
        m = (act == k).unsqueeze(-1).double()
        if not bool((act == k).any()):
            assert float(part[:, k].abs().max()) == 0.0 and float(S64[k].abs().max()) == 0.0, k
            continue
        tab.rule("S[action %d]" % k, S[k], S64[k], S32[k])
        own64, mag = (own * m).sum((0, 1)), (own.abs() * m).sum((0, 1))
        err, bound = (S[k] - own64).abs(), T * N * 2.0 ** -24 * mag
        print("sums %-12s action %d: %d rows, max err against own dG %.2e, min slack %.2e"
              % (name, k, int((act == k).sum()), float(err.max()), float((bound - err).min())))
        if not bool((err <= bound).all()):
            off.append("S[action %d] is not the sum of the kernel's own dG: err %.3e, %.3e past its bound"
                       % (k, float(err.max()), float((err - bound).max())))
    _finish([tab], off)
    # the four-move table only: an 8-row table with a sums buffer is refused, and nothing is launched
    p_, pn = fused._p, fused._pn
    emb8 = torch.cat([s["emb"], s["emb"]], 0).contiguous()
    dg1, dh1, dc1 = torch.empty_like(dG), torch.empty_like(dh0), torch.empty_like(dc0)
    ps, pa = (T + 1) * N * R, T * N * GATES
    with pytest.raises(RuntimeError, match=r"atr_lstm_bptt_pre2 failed \(-1\)"):
        L.atr_lstm_bptt_pre2(pn(s["dh"][0]), pn(s["dh"][1]) if P > 1 else None, p_(s["keep"]), p_(s["pre"]), pa, p_(s["bias"][0]),
                             p_(s["bias"][1]) if P > 1 else None, p_(emb8), ep, 8, p_(s["act"]), s["act"].stride(0), p_(s["c_all"]),
                             ps, p_(s["whh"][0]), p_(s["whh"][1]) if P > 1 else None, p_(dg1), pa, p_(dh1), p_(dc1), p_(sums),
                             P, T, N, R, fused._stream(dg1))
    torch.cuda.synchronize()


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def _fold_operands(tiles, J, Cc):
    g = torch.Generator().manual_seed(1000 * tiles + J + Cc)
    rnd = lambda *sh: torch.randn(*sh, generator=g)
    return dict(part=rnd(tiles, 4, J).to(DEV), fa_w=(0.3 * rnd(Cc, 4)).to(DEV), fa_b=(0.1 * rnd(Cc)).to(DEV),
                wih=(0.08 * rnd(J, Cc)).to(DEV), dwih0=rnd(J, Cc).to(DEV))


def _fold(o, part=None, fa_w=None, J=None, tiles=None):
    """atr_embed_fold on the operands `o` (overrides: what a refused call gets wrong) -> (dwih, dfa_w, dfa_b, S), poisoned first."""
    from active_tracking_rl_amd import fused
    J0, Cc = o["wih"].shape
    part = o["part"] if part is None else part
    fa_w = o["fa_w"] if fa_w is None else fa_w
    dwih = o["dwih0"].clone()
    nan = lambda *sh: torch.full(sh, float("nan"), device=DEV)
    dfa_w, dfa_b, S = nan(Cc, 4), nan(Cc), nan(4, J0)
    fused.lib().atr_embed_fold(fused._p(part), part.shape[0] if tiles is None else tiles, fused._p(fa_w), fused._p(o["fa_b"]),
                               fused._p(o["wih"]), fused._p(dwih), fused._p(dfa_w), fused._p(dfa_b), fused._p(S),
                               J0 if J is None else J, Cc, fused._stream(dwih))
    torch.cuda.synchronize()
    return dwih, dfa_w, dfa_b, S


@pytest.mark.parametrize("Cc", [256, 196])
@pytest.mark.parametrize("J", [512, 384])
@pytest.mark.parametrize("tiles", [1, 16, 17, 113, 129, 256])
def test_embed_fold_alone_against_float64(tiles, J, Cc):
    """3. atr_embed_fold from random per-tile sums [tiles, 4, J] (J = 4R of the LSTM, 3R of the GRU; C = 256 and a width that is no
    multiple of 64): S = their sum, dwih += S^T E (dwih starts at N(0, 1) values: "=" in place of "+=" misses the rule by O(1)),
    d fa_w = (S wih)^T, d fa_b — each under the rule against the same algebra in float64, aten32 = that algebra in float32 torch
    ops. Tile counts: one; one per reduction group (16); one more; the smallest that enters k_sact_reduce's eight-deep loop (113);
    129 as the 2050-row BPTT case leaves; 256 (two rounds of that loop)."""
    o = _fold_operands(tiles, J, Cc)
    dwih, dfa_w, dfa_b, S = _fold(o)
    want64 = spec.fold_algebra(*(o[k].cpu() for k in ("part", "fa_w", "fa_b", "wih", "dwih0")), torch.float64)
    want32 = spec.fold_algebra(*(o[k] for k in ("part", "fa_w", "fa_b", "wih", "dwih0")), torch.float32)
    tab = Table("embed_fold tiles=%d J=%d C=%d" % (tiles, J, Cc))
    tab.rule("S", S, o["part"].double().sum(0), o["part"].sum(0))
    for what, hip, r64, r32 in zip(("dwih", "dfa_w", "dfa_b"), (dwih, dfa_w, dfa_b), want64, want32):
        assert bool(torch.isfinite(hip).all()), what
        tab.rule(what, hip, r64, r32)
    tab.finish()


def test_embed_fold_refuses_what_it_cannot_read():
    """3. A fa_w that is not 16-byte aligned (the kernel reads its rows as float4), J no multiple of 4 and no tiles: status 1 each."""
    o = _fold_operands(2, 512, 256)
    shifted = torch.zeros(o["fa_w"].numel() + 1, device=DEV)[1:].view(256, 4)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for bad in (dict(fa_w=shifted), dict(J=510), dict(tiles=0)):
        with pytest.raises(RuntimeError, match=r"atr_embed_fold failed \(1\)"):
            _fold(o, **bad)


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
NODE_NAMES = ("atr_lstm_bptt", "atr_lstm_bptt_pre", "atr_lstm_bptt_pre2", "atr_embed_fold", "atr_embed_add", "atr_embed_add_ld",
              "atr_embed_grad", "atr_gemm_tn_grouped", "atr_lstm_cell_backward")


@pytest.mark.parametrize("need", [None, (True, False), (False, True)], ids=["both", "tracker-only", "target-only"])
@pytest.mark.parametrize("fold", [True, False], ids=["fold", "explicit"])
@pytest.mark.parametrize("name", list(spec.NODE_CASES))
def test_the_cached_node_against_float64(name, fold, need, monkeypatch):
    """4. fused.lstm_sequence_cached on the PRE stores, both players, the embedding on player 1: with fold=fc_action_tracker the
    target's features are the raw ones and the node makes fc_action_tracker's gradients (atr_lstm_bptt_pre2 with sums +
    atr_embed_fold, once each, on the spot: T N < 4096); without it the features are f + E[a] through torch ops, whose autograd
    makes them. Every gradient under the rule; what `need` switches off is None, and then one launch per trained player runs."""
    from active_tracking_rl_amd import fused
    monkeypatch.setattr(fused, "use_fused_bptt", True)
    monkeypatch.setattr(fused, "fold_embedding", True)
    x, ref, x32, s = _problem(name)
    case = x["case"]
    P, T, N = case.P, case.T, case.N
    assert P == 2 and case.emb_player == 1 and fused._deferred is None
    lstms = [torch.nn.LSTMCell(spec.FDIM, R).to(DEV) for _ in range(P)]
    for mine, theirs in zip(lstms, x["cells"]):
        mine.load_state_dict(theirs.state_dict())
    fa = torch.nn.Linear(case.n_act, spec.FDIM).to(DEV)
    fa.load_state_dict(x["fa"].state_dict())
    feats = [x["feats"][:, p].reshape(T * N, spec.FDIM).to(DEV).requires_grad_(True) for p in range(P)]
    pre = dict(bias=s["bias"], emb=s["emb"], emb_player=1, act=s["act"])
    assert fused.embed_fold_ok(pre, s["h_all"], s["c_all"], s["keep"], fa)
    f_in = list(feats)
    if not fold:
        f_in[1] = feats[1] + fa(torch.nn.functional.one_hot(s["act"].reshape(T * N), case.n_act).float())
    trained = (True, True) if need is None else need
    spy = spec.Spy(monkeypatch, NODE_NAMES)
    with _poisoned_allocations(monkeypatch):
        h_seq = fused.lstm_sequence_cached(lstms, f_in, s["keep"], s["h_all"], s["c_all"], s["pre"], need=need, pre=pre,
                                           fold=fa if fold else None)
        assert len(h_seq) == P and all(torch.equal(h_seq[p], s["h_all"][p, 1:]) for p in range(P))
        go = x["go"].to(DEV)
        names = ["feats[%d]" % p for p in range(P)] + ["%s[%d]" % (n, p) for p in range(P) for n in spec.PARAMS] + ["fa.weight", "fa.bias"]
        wrt = feats + [getattr(lstms[p], n) for p in range(P) for n in spec.PARAMS] + [fa.weight, fa.bias]
        grads = dict(zip(names, torch.autograd.grad(sum((h_seq[p] * go[:, p]).sum() for p in range(P)), wrt, allow_unused=True)))
    torch.cuda.synchronize()
    folded = fold and trained[1]
    assert spy.count("atr_lstm_bptt_pre2") == 1 and spy.count("atr_embed_fold") == (1 if folded else 0)
    assert not any(c != "atr_lstm_bptt_pre2" and c != "atr_embed_fold" for c in spy.calls), spy.calls
    tab = Table("node %s %s need=%s" % (name, "fold" if fold else "explicit", need))
    for n in names:
        player = 1 if n.startswith("fa.") else int(n[-2])
        want = ref["feats"][:, player].reshape(T * N, -1) if n.startswith("feats") else ref[n]
        want32 = x32["feats"][:, player].reshape(T * N, -1) if n.startswith("feats") else x32[n]
        if not trained[player]:
            assert grads[n] is None, n
            continue
        assert grads[n] is not None and bool(torch.isfinite(grads[n]).all()), n
        tab.rule(n, grads[n], want, want32)
    tab.finish()
