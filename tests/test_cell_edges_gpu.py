"""-m gpu: the cell kernels (csrc/atr_cell.h and everything that includes it, csrc/actor_step_hip.hip's own sigm / tanh_fast, the cell
backward of csrc/lstm_hip.hip, csrc/gru_hip.hip and csrc/bptt_hip.hip) and the heads kernels (csrc/heads_hip.hip) at SATURATED
inputs, per element: pre-activations and cell states drawn from tests/cell_edge_spec.py's ladder (every float range where
sigmoidf_ / tanhf_ change behaviour, up to 3e38), a policy with p_max == 1.0f on a third of its rows. The spec, its references and
its derived bounds E_SIG / E_TANH / bound_* are tested on their own in tests/test_cell_edges_cpu.py.

  1 the activation sweep and the LSTM cell forward (fused.lstm_cell_into): stored gates within E_SIG / E_TANH of float64, c and h
    within bound_*, ranges, a done row independent of its c_prev, cell states of 1e4 and 3e38 finite with the reference's sign
  2 the other entry points (lstm_cell_act_into with bias / emb, lstm_cell_act2_into, the policy half of act_env_step) bit for bit
    against 1;  fused.actor_step_into with the ladder on its bias slots, per element
  3 the GRU cell forward (fused.gru_cell, atr_gru_cell_forward's store) per element
  4 the cell backward at T = 1 per element (per-step kernels and the one-launch kernels, three LSTM forms), signs, PRE == gates
  5 the cell backward at T = 3 and the heads at a peaked policy under tests/f64_rule.py's rule, unchanged
Outputs are NaN-poisoned before every call and checked finite afterwards.

Measured on MI355X (largest err / allowed per test, where on the ladder it sits):
  activation sweep (4M points)   sigmoid 1.06e-07 at x = 3.6 (0.64 of E_SIG = 1.65e-07)   tanh 2.08e-07 at x = -1.9 (0.58 of E_TANH = 3.61e-07)
  lstm_cell_into R=128 / 64      gates 0.62 (1.02e-07 at 3.5)   c 0.28 (3.3e-06 at c_prev = -20)   h 0.20
  actor_step_into                gates 0.41 (tanh, 1.48e-07 at -1.9)   c 0.21   h 0.16
  gru_cell R=128 / 64            r, z 0.65 (1.07e-07 at 3.5)   n 0.27   h 0.30 (2.9e-06 at k h_prev = -16.6)
  backward T=1                   LSTM 0.30 (dc0; every form, per-step and one launch)   GRU 0.50 (dh0 = dh z: one product)
  backward T=3, the rule         LSTM dG 2.3e-07 .. 2.6e-07, dh0 3.4e-07 .. 4.2e-07, dc0 1.2e-07 .. 1.4e-07, dW_hh 2.7e-07 .. 3.0e-07,
                                 S 2.4e-07 .. 2.8e-07 against e(aten32) 7.9e-08 .. 3.1e-07: e(hip) / allowed <= 0.34 (floor 1e-6)
                                 GRU 1.5e-07 .. 3.3e-07 against e(aten32) 1.8e-07 .. 3.3e-07: <= 0.25; the per-step kernels equal aten32
  peaked heads, the rule         values <= 0.08, objective 0.25, policy 0.36, value 0.19, entropy 0.25, dL/dh 0.35, dW_actor 0.33,
                                 db_actor 0.51, dW_critic 0.16, db_critic 0.53, aux head 0.17 of allowed; e(aten32) <= 3.5e-06
  every test runs in 1.3 s or less.

What the file found: with the entropy taken as -sum p (z - lse), lse = max + log(sum), the ENTROPY STATISTIC of the R = 256, A = 8
case (logits beyond 128) missed the rule: e(hip) 1.1e-06 .. 1.9e-06 against allowed 1.0e-06 .. 1.5e-06 (e(aten32) 2.0e-07 .. 3.8e-07),
in heads_loss and heads_loss_pair alike: z - lse rounds at the logits' magnitude, 7.6e-6, and on a peaked row log p of the top action
is all the entropy there is. csrc/heads_hip.hip now takes the statistic's log p as (z - max) - log(sum) (e(hip) 2.0e-10 .. 2.5e-07).
The loss, its gradient and the policy statistic keep z - lse and are bit for bit what they were. (Moving those to the same form was
tried: everything here passed, and two unit-scale cases of tests/test_hidden_sizes_gpu.py then had their policy statistic at
1.04e-06 and 1.16e-06 against allowed 1.00e-06 and 1.05e-06 — a cancelling sum of 16387 signed terms whose last bits moved — and
tests/test_learner_f64_gpu.py::test_ragged_frame_count_against_float64[1001], whose window then no longer resolved one env's share.)

What it resolves: each rewrite made on a scratch copy of the library and run once on MI355X (never committed):
  (a) tanhf_ as (e^2x - 1) / (e^2x + 1) (csrc/atr_cell.h)   11 of 20 tests fail: the activation sweep first (NaN gates from |x| = 44.4
      up), lstm_cell_into R=128 / 64, the other entry points R=128 / 64, gru_cell R=128 / 64, both backward tests at T = 1 and both
      at T = 3 (NaN stores, NaN tanh(c)); actor_step_into (its own tanh_fast) and the eight heads cases pass, as they must
  (b) sigmoidf_ as e^x / (1 + e^x)                          the same 11 tests: NaN gates from x = 88.8 up
  (c) the heads kernel's entropy with logf(p[i])            the 8 heads cases fail, first row loss[0]: statistics [nan, 4.07e+07, nan, 0],
      then entropy not >= 0, non-finite dL/dh, dW_actor, db_actor; the 12 cell tests pass
With (a) or (b) in place all 235 tests of tests/test_fused_stem_gpu.py, test_lstm_bptt_f64_gpu.py, test_gru_gpu.py,
test_gru_learner_f64_gpu.py, test_hidden_sizes_gpu.py and test_learner_f64_gpu.py pass. With (c) 234 pass; the one that fails,
test_ragged_frame_count_against_float64[1001], fails on its own resolution check ("allowed error does not resolve one env's share":
logf(p) moves the last bits of the learner's gradients and with them the window that test picks), not on any value of the heads.
"""
import numpy as np
import pytest
import torch

import cell_edge_spec as spec
from f64_rule import Table
from lstm_bptt_spec import Spy
from test_hidden_sizes_gpu import GRAD_NAMES, STAT_NAMES, _heads_reference
from test_lstm_bptt_f64_gpu import _poisoned_allocations

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A = 4


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def randn(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


class Report(object):
    """Per-element rows (what, largest err / allowed, its err, where on the ladder it sits): printed, then one failure for all."""

    def __init__(self, label):
        self.label, self.rows, self.bad = label, [], []

    def add(self, what, got, ref, allowed, at):
        got = host(got) if torch.is_tensor(got) else got
        ratio, i, err = spec.worst(got, ref, allowed)
        at = np.broadcast_to(np.asarray(at), np.shape(ref)).reshape(-1)[i]
        self.rows.append((what, ratio, err, spec.where_on_ladder(at)))
        if not ratio <= 1.0:
            self.bad.append("%s: err %.3e is %.2f x allowed at input %s (flat index %d)" % (what, err, ratio, self.rows[-1][3], i))

    def check(self, ok, what):
        if not ok:
            self.bad.append(what)

    def finish(self):
        for what, ratio, err, where in self.rows:
            print("%-30s %-16s err / allowed %.3f  err %.3e  at %s" % (self.label, what, ratio, err, where))
        assert not self.bad, "\n".join([self.label] + self.bad)


def _sampler():
    from active_tracking_rl_amd import fused
    s = fused.ActionSampler(torch.device(DEV), seed=5)
    s.begin_block()
    return s


def _actor(R, seed=0):
    torch.manual_seed(seed)
    return torch.nn.Linear(R, A).to(DEV)


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
_FWD = {}


def _lstm_forward(R):
    """The ladder through fused.lstm_cell_into at 2048 rows: (inputs on the host, outputs on the GPU), made once per R."""
    from active_tracking_rl_amd import fused
    if R not in _FWD:
        N = 2048
        ig = spec.draw((N, 4 * R), 1000 + R)
        cp = spec.draw((N, R), 2000 + R, ladder=spec.C_LADDER, top=64.0)
        done = (np.arange(N) % 3 == 0).astype(np.uint8)
        h, c, acts = nan(N, R), nan(N, R), nan(N, 4 * R)
        fused.lstm_cell_into(dev(ig), torch.zeros(N, 4 * R, device=DEV), dev(cp), dev(done), h, c, acts)
        torch.cuda.synchronize()
        _FWD[R] = (ig, cp, done, h, c, acts)
    return _FWD[R]


def _hold_lstm_forward(rep, parts, cp, k, h, c, acts):
    """The per-element checks of one LSTM cell forward: parts = the four float32 pre-activation blocks the kernel activated."""
    R = cp.shape[1]
    for t in (h, c, acts):
        assert bool(torch.isfinite(t).all())
    want = spec.bound_lstm_fwd(*parts, cp, k)
    g = dict(zip("ifgo", (host(x) for x in spec.split4(acts))))
    for name, x in zip("ifgo", parts):
        rep.add("gate " + name, g[name], want[name][0], spec.E_TANH if name == "g" else spec.E_SIG, x)
    rep.add("c", c, want["c"][0], want["c"][1], cp)
    rep.add("h", h, want["h"][0], want["h"][1], want["c"][0])
    for name in "ifo":
        rep.check(float(g[name].min()) >= 0.0 and float(g[name].max()) <= 1.0, "gate %s leaves [0, 1]" % name)
    rep.check(float(np.abs(g["g"]).max()) <= 1.0, "|g| > 1")
    rep.check(float(h.abs().max()) <= 1.0, "|h| > 1")
    return want


def test_the_activation_sweep():
    """4M log-uniform points in [1e-8, 200] of either sign through fused.lstm_cell_into's gate store (8192 rows, R = 128): the
    hardware sigmoid's and tanh's own largest absolute error, against E_SIG / E_TANH."""
    from active_tracking_rl_amd import fused
    N, R = 8192, 128
    rng = np.random.default_rng(7)
    x = (np.exp(rng.uniform(np.log(1e-8), np.log(200.0), (N, 4 * R))) * np.where(rng.random((N, 4 * R)) < 0.5, -1.0, 1.0)).astype(np.float32)
    h, c, acts = nan(N, R), nan(N, R), nan(N, 4 * R)
    fused.lstm_cell_into(dev(x), torch.zeros(N, 4 * R, device=DEV), torch.zeros(N, R, device=DEV), None, h, c, acts)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(acts).all()) and bool(torch.isfinite(h).all()) and bool(torch.isfinite(c).all())
    rep = Report("activation sweep")
    got = host(acts)
    sig = np.ones(4 * R, dtype=bool)
    sig[2 * R:3 * R] = False
    rep.add("sigmoid", got[:, sig], spec.sigmoid64(x[:, sig]), spec.E_SIG, x[:, sig])
    rep.add("tanh", got[:, ~sig], spec.tanh64(x[:, ~sig]), spec.E_TANH, x[:, ~sig])
    rep.check(float(got[:, sig].min()) >= 0.0 and float(got[:, sig].max()) <= 1.0 and float(np.abs(got).max()) <= 1.0, "range")
    rep.finish()


@pytest.mark.parametrize("R", [128, 64])
def test_lstm_cell_forward_on_the_ladder(R):
    from active_tracking_rl_amd import fused
    ig, cp, done, h, c, acts = _lstm_forward(R)
    N = ig.shape[0]
    k = (done == 0).astype(np.float32).reshape(N, 1)
    rep = Report("lstm_cell_into R=%d" % R)
    _hold_lstm_forward(rep, spec.split4(ig), cp, k, h, c, acts)
    # a done row does not read its c_prev: other cell states there, the range-only ones among them, same rows out
    cp2 = cp.copy()
    cp2[done != 0] = np.resize(np.concatenate([spec.C_RANGE_ONLY, spec.C_LADDER[::-1]]), cp2[done != 0].shape)
    h2, c2, a2 = nan(N, R), nan(N, R), nan(N, 4 * R)
    fused.lstm_cell_into(dev(ig), torch.zeros(N, 4 * R, device=DEV), dev(cp2), dev(done), h2, c2, a2)
    torch.cuda.synchronize()
    rep.check(torch.equal(h2, h) and torch.equal(c2, c) and torch.equal(a2, acts), "a done row's result depends on its c_prev")
    # range only: cell states of 1e4 and 3e38 on live rows
    cp3 = np.resize(spec.C_RANGE_ONLY, cp.shape).astype(np.float32)
    h3, c3, a3 = nan(N, R), nan(N, R), nan(N, 4 * R)
    fused.lstm_cell_into(dev(ig), torch.zeros(N, 4 * R, device=DEV), dev(cp3), None, h3, c3, a3)
    torch.cuda.synchronize()
    rep.check(bool(torch.isfinite(h3).all()) and bool(torch.isfinite(c3).all()), "non-finite h or c from a cell state of 1e4 / 3e38")
    want = spec.bound_lstm_fwd(*spec.split4(ig), cp3, np.ones((N, 1), dtype=np.float32))
    for name, got in (("c", host(c3)), ("h", host(h3))):
        ref, allowed = want[name]
        sure = np.abs(ref) > allowed
        rep.check(bool((np.sign(got[sure]) == np.sign(ref[sure])).all()), "range only: %s has not the reference's sign" % name)
        rep.check(sure.mean() > 0.5, "range only: the sign of %s is decided on too few elements" % name)
    rep.check(float(h3.abs().max()) <= 1.0, "range only: |h| > 1")
    rep.finish()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [128, 64])
def test_the_other_lstm_entry_points_bit_for_bit(R):
    """lstm_cell_act_into (bias: the ladder on the 4R bias slots, zeros in ig; emb: the ladder as a 2048-row table read through
    act_in), lstm_cell_act2_into and, at R = 128, the policy half of act_env_step: the states and gates of lstm_cell_into on the
    same pre-activations, bit for bit; their actions only have to be actions."""
    from active_tracking_rl_amd import fused
    ig, cp, done, h, c, acts = _lstm_forward(R)
    N = ig.shape[0]
    zero = torch.zeros(N, 4 * R, device=DEV)
    igd, cpd, doned = dev(ig), dev(cp), dev(done)
    actor = _actor(R)
    bad = []

    def same(tag, got, want):
        for name, a, b in zip(("h", "c", "gates"), got, want):
            if not bool(torch.isfinite(a).all()):
                bad.append("%s: non-finite %s" % (tag, name))
            elif not torch.equal(a, b):
                bad.append("%s: %s differs in %d elements" % (tag, name, int((a != b).sum())))

    def actions_ok(tag, a):
        if not (int(a.min()) >= 0 and int(a.max()) < A):
            bad.append("%s: an action outside [0, %d)" % (tag, A))
    # the ladder on the bias: every row sees the same 4R pre-activations
    bias = spec.draw((4 * R,), 3000 + R)
    hb, cb, ab = nan(N, R), nan(N, R), nan(N, 4 * R)
    fused.lstm_cell_into(dev(np.broadcast_to(bias, (N, 4 * R))), zero, cpd, doned, hb, cb, ab)
    s = _sampler()
    out = [nan(N, R), nan(N, R), nan(N, 4 * R)]
    act = torch.full((N,), -1, dtype=torch.int64, device=DEV)
    fused.lstm_cell_act_into(zero, zero, cpd, doned, *out, s, actor, act, bias=dev(bias))
    same("act_into bias", out, (hb, cb, ab)); actions_ok("act_into bias", act)
    # the ladder as the embedding table, one row per env
    rows = torch.arange(N, device=DEV)
    for tag, b in (("act_into emb", None), ("act_into emb + zero bias", torch.zeros(4 * R, device=DEV))):
        out = [nan(N, R), nan(N, R), nan(N, 4 * R)]
        act.fill_(-1)
        fused.lstm_cell_act_into(zero, zero, cpd, doned, *out, s, actor, act, emb=igd, act_in=rows, bias=b)
        same(tag, out, (h, c, acts)); actions_ok(tag, act)
    # both players in one launch: player 0 the ladder in ig, player 1 the ladder on the bias
    ig2 = torch.stack([igd, zero], 0).contiguous()
    biases = [torch.zeros(4 * R, device=DEV), dev(bias)]
    cp2 = torch.stack([cpd, cpd], 0)
    actors = [actor, _actor(R, 1)]
    h2, c2, a2 = nan(2, N, R), nan(2, N, R), nan(2, N, 4 * R)
    act2 = torch.full((2, N), -1, dtype=torch.int64, device=DEV)
    fused.lstm_cell_act2_into(ig2, torch.zeros_like(ig2), biases, cp2, doned, h2, c2, a2, s, actors, act2)
    same("act2_into[0]", (h2[0], c2[0], a2[0]), (h, c, acts)); same("act2_into[1]", (h2[1], c2[1], a2[1]), (hb, cb, ab))
    actions_ok("act2_into", act2)
    if R == 128:
        h3, c3, a3 = nan(2, N, R), nan(2, N, R), nan(2, N, 4 * R)
        act2.fill_(-1)
        fused.act_env_step(None, [ig2[0], ig2[1]], [zero, zero], biases, [cp2[0], cp2[1]], doned, [h3[0], h3[1]], [c3[0], c3[1]],
                           [a3[0], a3[1]], s, actors, act2)
        same("act_env_step[0]", (h3[0], c3[0], a3[0]), (h, c, acts)); same("act_env_step[1]", (h3[1], c3[1], a3[1]), (hb, cb, ab))
        actions_ok("act_env_step", act2)
    s.end_block()
    torch.cuda.synchronize()
    assert not bad, "\n".join(bad)


def test_actor_step_on_the_ladder():
    """fused.actor_step_into (csrc/actor_step_hip.hip, its own sigm / tanh_fast): f = 0 and h_prev = 0, so the pre-activation of
    every row is exactly the bias, which holds the ladder on its 512 slots; c_prev from C_LADDER, 130 rows (a ragged last tile)."""
    from active_tracking_rl_amd import fused
    N, F_, R = 130, 256, 128
    torch.manual_seed(2)
    lstm = torch.nn.LSTMCell(F_, R).to(DEV)
    bias = spec.draw((4 * R,), 4000)
    cp = spec.draw((N, R), 4001, ladder=spec.C_LADDER, top=64.0)
    done = (np.arange(N) % 3 == 0).astype(np.uint8)
    h, c, acts = nan(N, R), nan(N, R), nan(N, 4 * R)
    fused.actor_step_into(torch.zeros(N, F_, device=DEV), torch.zeros(N, R, device=DEV), dev(cp), dev(done), lstm, dev(bias), h, c, acts)
    torch.cuda.synchronize()
    rep = Report("actor_step_into")
    parts = [np.broadcast_to(b, (N, R)) for b in spec.split4(bias)]
    _hold_lstm_forward(rep, parts, cp, (done == 0).astype(np.float32).reshape(N, 1), h, c, acts)
    rep.finish()


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def _gru_forward(ig, hg, bhh, hp, done, acts=True):
    """atr_gru_cell_forward for one player on host arrays -> (h, acts (r, z, n, q) or None) on the GPU, poisoned first."""
    from active_tracking_rl_amd import fused
    N, R = hp.shape
    h, st = nan(N, R), nan(N, 4 * R) if acts else None
    igd, hgd, bd, hpd = dev(ig), dev(hg), dev(bhh), dev(hp)
    dn = dev(done) if done is not None else None
    fused.lib().atr_gru_cell_forward(fused._p(igd), None, fused._p(hgd), fused._p(bd), None, fused._p(hpd), 0, None, fused._pn(dn),
                                     fused._p(h), 0, fused._pn(st), 0, 1, N, R, fused._stream(igd))
    torch.cuda.synchronize()
    return h, st


def _gru_args(ig, hg, bhh, hp, k):
    """What gru_cell4 activates, from the kernel's float32 inputs: hidden side fma(k, hg, b_hh) rounded once, then ir + hr, iz + hz."""
    R = hp.shape[1]
    hm = (k.astype(np.float64) * hg.astype(np.float64) + bhh.astype(np.float64)).astype(np.float32)
    return (spec.f32_sum(ig[:, :R], hm[:, :R]), spec.f32_sum(ig[:, R:2 * R], hm[:, R:2 * R]), ig[:, 2 * R:], hm[:, 2 * R:],
            (k * hp).astype(np.float32))


@pytest.mark.parametrize("R", [128, 64])
def test_gru_cell_forward_on_the_ladder(R, monkeypatch):
    from active_tracking_rl_amd import fused
    N = 2048
    ig = spec.draw((N, 3 * R), 5000 + R)
    hg = spec.draw((N, 3 * R), 5100 + R, ladder=spec.C_LADDER, top=64.0)
    hp = spec.draw((N, R), 5200 + R, ladder=spec.C_LADDER, top=64.0)
    bhh = randn((3 * R,), 5300 + R, 0.25)
    done = (np.arange(N) % 3 == 0).astype(np.uint8)
    k = (done == 0).astype(np.float32).reshape(N, 1)
    h, st = _gru_forward(ig, hg, bhh, hp, done)
    with _poisoned_allocations(monkeypatch):
        h1 = fused.gru_cell(dev(ig), dev(hg), dev(bhh), dev(hp), done=dev(done))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(st).all()) and torch.equal(h1, h)
    args = _gru_args(ig, hg, bhh, hp, k)
    want = spec.bound_gru_fwd(*args)
    r, z, n, q = (host(x) for x in spec.split4(st))
    rep = Report("gru_cell R=%d" % R)
    rep.add("r", r, want["r"][0], spec.E_SIG, args[0])
    rep.add("z", z, want["z"][0], spec.E_SIG, args[1])
    rep.add("n", n, want["n"][0], want["n"][1], args[2])
    rep.add("h", h, want["h"][0], want["h"][1], args[4])
    rep.check(np.array_equal(q, args[3]), "the stored q is not fma(k, hg_n, b_hn)")
    rep.check(float(min(r.min(), z.min())) >= 0.0 and float(max(r.max(), z.max())) <= 1.0 and float(np.abs(n).max()) <= 1.0, "range")
    # h' = (1 - z) n + z (k h): between n and k h_prev up to the bound
    lo, hi = np.minimum(want["n"][0], args[4]) - want["h"][1], np.maximum(want["n"][0], args[4]) + want["h"][1]
    rep.check(bool(((host(h) >= lo) & (host(h) <= hi)).all()), "h' outside [n, k h_prev]")
    rep.finish()


# ---- 4 and 5: stores written by the forward kernels from ladder inputs ---------------------------------------------------------
P, N_B, R_B = 2, 34, 128
_STORES = {}


def _keep(T, seed):
    keep = (np.random.default_rng(seed).random((T, N_B)) > 0.3).astype(np.float32)
    assert T == 1 or 0 < (keep[:-1] == 0).sum() < keep[:-1].size
    return keep


def _lstm_stores(T):
    """P = 2 players, 34 rows (a ragged third 16-row tile), R = 128, T steps: float32 pre-activations from the ladder, a bias per
    player and the tracker-action embedding on player 1 ((pre + bias) + emb[act], the PRE forms' order), run through
    fused.lstm_cell_act_into step by step (hg = 0: the backward reads the stores, whatever recurrence made them)."""
    from active_tracking_rl_amd import fused
    if T not in _STORES:
        R, N = R_B, N_B
        pre = spec.draw((P, T, N, 4 * R), 6000 + T)
        bias = randn((P, 4 * R), 6100 + T, 0.5)
        emb = randn((A, 4 * R), 6200 + T, 0.5)
        act = np.random.default_rng(6300 + T).integers(0, A, (T, N))
        keep = _keep(T, 6400 + T)
        h_all, c_all, gates = nan(P, T + 1, N, R), nan(P, T + 1, N, R), nan(P, T, N, 4 * R)
        h_all[:, 0] = dev(spec.draw((P, N, R), 6500 + T, ladder=spec.C_LADDER[np.abs(spec.C_LADDER) <= 1.0], top=1.0))
        c_all[:, 0] = dev(spec.draw((P, N, R), 6600 + T, ladder=spec.C_LADDER, top=64.0))
        pred, biasd, embd, actd, keepd = dev(pre), dev(bias), dev(emb), dev(act), dev(keep)
        zero = torch.zeros(N, 4 * R, device=DEV)
        s, actor, drawn = _sampler(), _actor(R), torch.zeros(N, dtype=torch.int64, device=DEV)
        for t in range(T):
            done = (keepd[t - 1] == 0).to(torch.uint8) if t else None
            for p in range(P):
                fused.lstm_cell_act_into(pred[p, t], zero, c_all[p, t], done, h_all[p, t + 1], c_all[p, t + 1], gates[p, t], s, actor,
                                         drawn, emb=embd if p == 1 else None, act_in=actd[t] if p == 1 else None, bias=biasd[p])
        s.end_block()
        torch.cuda.synchronize()
        for t_ in (h_all, c_all, gates):
            assert bool(torch.isfinite(t_).all())
        x = spec.f32_sum(pre, bias.reshape(P, 1, 1, 4 * R))               # what the PRE form activates without the embedding,
        x_emb = x.copy()                                                  # and with it on player 1
        x_emb[1] = spec.f32_sum(x[1], emb[act])
        g = torch.Generator().manual_seed(6700 + T)
        whh = torch.zeros(P, 4 * R, R) if T == 1 else torch.randn(P, 4 * R, R, generator=g) * 0.1
        _STORES[T] = dict(T=T, pre=pred, bias=[biasd[0], biasd[1]], emb=embd, act=actd, keep=keepd, h_all=h_all, c_all=c_all,
                          gates=gates, x=x, x_emb=x_emb, dh=torch.randn(P, T, N, R, generator=g).to(DEV), whh=whh.to(DEV),
                          act_host=act)
    return _STORES[T]


def _lstm_bptt(s, form, monkeypatch, fused_launch=True):
    """fused._lstm_bptt on the stores in one of its forms -> (dG [P, T, N, 4R], dh0, dc0, dW_hh [P, R, 4R], by-action sums or None)."""
    from active_tracking_rl_amd import fused
    monkeypatch.setattr(fused, "use_fused_bptt", fused_launch)
    pre, acts = None, s["gates"]
    if form == "pre":
        pre, acts = dict(bias=s["bias"]), s["pre"]
    elif form == "pre+emb":
        pre, acts = dict(bias=s["bias"], emb=s["emb"], emb_player=1, act=s["act"], want_sums=True), s["pre"]
    names = ("atr_lstm_bptt", "atr_lstm_bptt_pre2", "atr_lstm_cell_backward")
    spy = Spy(monkeypatch, names)
    with _poisoned_allocations(monkeypatch):
        dG, dh0, dc0, dwhh = fused._lstm_bptt(s["whh"].transpose(1, 2).contiguous(), s["keep"], s["h_all"], s["c_all"], acts,
                                              [s["dh"][0], s["dh"][1]], whh_nn=[s["whh"][0], s["whh"][1]], pre=pre)
    torch.cuda.synchronize()
    want = {"gates": "atr_lstm_bptt", "pre": "atr_lstm_bptt_pre2", "pre+emb": "atr_lstm_bptt_pre2"}[form] if fused_launch \
        else "atr_lstm_cell_backward"
    assert set(spy.calls) == {want}, spy.calls
    for t in (dG, dh0, dc0, dwhh):
        assert bool(torch.isfinite(t).all())
    sums = None
    if form == "pre+emb":
        sums = pre["act_sums"]
        assert sums is not None and bool(torch.isfinite(sums).all())
        sums = sums.view(-1, 4, 4 * R_B).double().sum(0)
    return dG.view(P, s["T"], N_B, 4 * R_B), dh0, dc0, dwhh, sums


def _same_sign(rep, what, got, ref):
    """No derivative factor negative: sigma (1 - sigma) >= 0 and 1 - t^2 >= 0 at every point, so no entry's sign is the opposite
    of the reference's."""
    rep.check(bool((host(got).astype(np.float64) * ref >= 0.0).all()), "%s: an entry with the opposite sign of the reference" % what)


def test_lstm_cell_backward_at_one_step_per_element(monkeypatch):
    """T = 1, W_hh = 0: no product in any expression. The per-step kernel (k_lstm_cell_bwd) and the one-launch kernel in its three
    forms on the forward kernels' own stores: dG and dc0 per element within bound_lstm_bwd, dh0 exactly zero."""
    s = _lstm_stores(1)
    gates, c, cp, dh = host(s["gates"][:, 0]), host(s["c_all"][:, 1]), host(s["c_all"][:, 0]), host(s["dh"][:, 0])
    one = np.ones((1, N_B, 1), dtype=np.float32)
    for part in spec.split4(gates):
        assert float(part.min()) >= -1.0 and float(part.max()) <= 1.0
    stored = spec.bound_lstm_bwd(spec.split4(gates), c, cp, dh, one)
    re_act = {"pre": spec.bound_lstm_bwd(spec.split4(s["x"][:, 0]), c, cp, dh, one, activate=True),
              "pre+emb": spec.bound_lstm_bwd(spec.split4(s["x_emb"][:, 0]), c, cp, dh, one, activate=True)}
    at = dict(di=gates[..., :R_B], df=cp, dg=gates[..., 2 * R_B:3 * R_B], do=c, dc0=c)
    got = {}
    bad = []
    for label, form, launch in (("per-step", "gates", False), ("one launch gates", "gates", True), ("one launch pre", "pre", True),
                                ("one launch pre+emb", "pre+emb", True)):
        dG, dh0, dc0, _, _ = _lstm_bptt(s, form, monkeypatch, launch)
        got[label] = dG
        want = stored if form == "gates" else re_act[form]
        rep = Report("lstm backward T=1 " + label)
        for name, blk in zip(("di", "df", "dg", "do"), spec.split4(dG[:, 0])):
            rep.add(name, blk, want[name][0], want[name][1], at[name])
            _same_sign(rep, name, blk, want[name][0])
        rep.add("dc0", dc0, want["dc0"][0], want["dc0"][1], at["dc0"])
        _same_sign(rep, "dc0", dc0, want["dc0"][0])
        rep.check(float(dh0.abs().max()) == 0.0, "dh0 is not zero at W_hh = 0")
        try:
            rep.finish()
        except AssertionError as e:
            bad.append(str(e))
    # re-activated in registers from the same float32 sums: the forward kernel's own gates, bit for bit
    if not torch.equal(got["one launch pre+emb"], got["one launch gates"]):
        bad.append("PRE + emb: dG differs from the stored-gates form")
    if not torch.equal(got["one launch pre"][0], got["one launch gates"][0]):
        bad.append("PRE: dG of the player without embedding differs from the stored-gates form")
    assert not bad, "\n".join(bad)


def _gru_stores(T):
    from active_tracking_rl_amd import fused
    key = ("gru", T)
    if key not in _STORES:
        R, N = R_B, N_B
        ig = spec.draw((P, T, N, 3 * R), 7000 + T)
        hg = spec.draw((P, T, N, 3 * R), 7100 + T, ladder=spec.C_LADDER, top=64.0)
        bhh = randn((P, 3 * R), 7200 + T, 0.25)
        keep = _keep(T, 7300 + T)
        h_all, acts = nan(P, T + 1, N, R), nan(P, T, N, 4 * R)
        h_all[:, 0] = dev(spec.draw((P, N, R), 7400 + T, ladder=spec.C_LADDER, top=64.0))
        for t in range(T):
            done = (keep[t - 1] == 0).astype(np.uint8) if t else None
            for p in range(P):
                h, st = _gru_forward(ig[p, t], hg[p, t], bhh[p], host(h_all[p, t]), done)
                h_all[p, t + 1], acts[p, t] = h, st
        assert bool(torch.isfinite(h_all).all()) and bool(torch.isfinite(acts).all())
        g = torch.Generator().manual_seed(7500 + T)
        whh = torch.zeros(P, 3 * R, R) if T == 1 else torch.randn(P, 3 * R, R, generator=g) * 0.1
        act = np.random.default_rng(7600 + T).integers(0, A, (T, N))
        _STORES[key] = dict(T=T, keep=dev(keep), h_all=h_all, acts=acts, dh=torch.randn(P, T, N, R, generator=g).to(DEV),
                            whh=whh.to(DEV), act=dev(act), act_host=act)
    return _STORES[key]


def _gru_bptt(s, monkeypatch, fused_launch, sums=False):
    """fused._gru_bptt -> (dG [P, T, N, 4R], dh0, dW_hh [P, R, 3R], db_hh [P, 3R], by-action sums of player 1 or None)."""
    from active_tracking_rl_amd import fused
    monkeypatch.setattr(fused, "use_fused_gru_bptt", fused_launch)
    spy = Spy(monkeypatch, ("atr_gru_bptt", "atr_gru_bptt_sums", "atr_gru_cell_backward"))
    info = dict(emb_player=1, act=s["act"]) if sums else None
    with _poisoned_allocations(monkeypatch):
        dG, dh0, dwhh, dbhh = fused._gru_bptt(s["whh"].transpose(1, 2).contiguous(), s["keep"], s["h_all"], s["acts"],
                                              [s["dh"][0], s["dh"][1]], sums=info)
    torch.cuda.synchronize()
    want = ("atr_gru_bptt_sums" if sums else "atr_gru_bptt") if fused_launch else "atr_gru_cell_backward"
    assert set(spy.calls) == {want}, spy.calls
    for t in (dG, dh0, dwhh, dbhh):
        assert bool(torch.isfinite(t).all())
    S = None
    if sums:
        assert info["act_sums"] is not None and bool(torch.isfinite(info["act_sums"]).all())
        S = info["act_sums"].view(-1, 4, 3 * R_B).double().sum(0)
    return dG.view(P, s["T"], N_B, 4 * R_B), dh0, dwhh, dbhh, S


def test_gru_cell_backward_at_one_step_per_element(monkeypatch):
    """T = 1, W_hh = 0: k_gru_cell_bwd and the one-launch k_gru_bptt on atr_gru_cell_forward's own store: dG = (dr, dz, dn, dq) and
    dh0 = dh z per element within bound_gru_bwd."""
    s = _gru_stores(1)
    r, z, n, q = (host(x) for x in spec.split4(s["acts"][:, 0]))
    hp, dh = host(s["h_all"][:, 0]), host(s["dh"][:, 0])
    want = spec.bound_gru_bwd(r, z, n, q, hp, dh)
    at = dict(dr=q, dz=hp, dn=n, dq=r, direct=z)
    bad = []
    for label, launch in (("per-step", False), ("one launch", True)):
        dG, dh0, _, _, _ = _gru_bptt(s, monkeypatch, launch)
        rep = Report("gru backward T=1 " + label)
        for name, blk in zip(("dr", "dz", "dn", "dq"), spec.split4(dG[:, 0])):
            rep.add(name, blk, want[name][0], want[name][1], at[name])
            _same_sign(rep, name, blk, want[name][0])
        rep.add("dh0", dh0, want["direct"][0], want["direct"][1], at["direct"])
        _same_sign(rep, "dh0", dh0, want["direct"][0])
        try:
            rep.finish()
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def _finish(tables):
    bad = []
    for tab in tables:
        try:
            tab.finish()
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


def test_lstm_cell_backward_over_three_steps_under_the_rule(monkeypatch):
    """T = 3 with a keep mask and a random W_hh: dG, dh0, dc0, dW_hh per player and the by-action sums under tests/f64_rule.py's
    rule; reference = the same backward over the same stores in float64 on the CPU, floor = it in float32 through PyTorch's ops."""
    s = _lstm_stores(3)
    cpu = {k: s[k].cpu() for k in ("keep", "gates", "c_all", "h_all", "dh", "whh")}
    common = lambda d: (d["keep"], d["c_all"], d["h_all"], d["dh"], d["whh"])
    refs = {}
    for form, acts in (("gates", None), ("pre", s["x"]), ("pre+emb", s["x_emb"])):
        a64 = cpu["gates"] if acts is None else torch.from_numpy(acts)
        a32 = s["gates"] if acts is None else dev(acts)
        k, c, h, d, w = common(cpu)
        r64 = spec.lstm_bptt_ref(k, a64, c, h, d, w, torch.float64, "cpu", pre=acts is not None, act=s["act_host"])
        k, c, h, d, w = common(s)
        r32 = spec.lstm_bptt_ref(k, a32, c, h, d, w, torch.float32, DEV, pre=acts is not None, act=s["act_host"])
        refs[form] = (r64, r32)
    tables = []
    for label, form, launch in (("per-step", "gates", False), ("one launch gates", "gates", True), ("one launch pre", "pre", True),
                                ("one launch pre+emb", "pre+emb", True)):
        dG, dh0, dc0, dwhh, S = _lstm_bptt(s, form, monkeypatch, launch)
        r64, r32 = refs[form]
        tab = Table("lstm backward T=3 " + label)
        tables.append(tab)
        for p in range(P):
            for what, hip, key in (("dG", dG, "dG"), ("dh0", dh0, "dh0"), ("dc0", dc0, "dc0"), ("dW_hh", dwhh, "dW_hh")):
                tab.rule("%s[%d]" % (what, p), hip[p], r64[key][p], r32[key][p])
        if S is not None:
            for a in range(A):
                assert bool((s["act"] == a).any())
                tab.rule("S[action %d]" % a, S[a], r64["S"][1][a], r32["S"][1][a])
    _finish(tables)


def test_gru_cell_backward_over_three_steps_under_the_rule(monkeypatch):
    """The GRU's: dG, dh0, dW_hh, db_hh per player and the one-launch kernel's by-action sums of dG's input-side columns."""
    s = _gru_stores(3)
    args = lambda d, dt, where: spec.gru_bptt_ref(*(d[k] if where != "cpu" else d[k].cpu() for k in ("keep", "acts", "h_all", "dh", "whh")),
                                                  dt, where)
    r64, r32 = args(s, torch.float64, "cpu"), args(s, torch.float32, DEV)
    onehot = torch.nn.functional.one_hot(torch.from_numpy(s["act_host"]).reshape(-1), A)
    by_action = lambda r: torch.matmul(onehot.to(r["dG"].dtype).to(r["dG"].device).t(), r["dG"][1].reshape(-1, 4 * R_B)[:, :3 * R_B])
    tables = []
    for label, launch, sums in (("per-step", False, False), ("one launch", True, False), ("one launch + sums", True, True)):
        dG, dh0, dwhh, dbhh, S = _gru_bptt(s, monkeypatch, launch, sums)
        tab = Table("gru backward T=3 " + label)
        tables.append(tab)
        for p in range(P):
            for what, hip, key in (("dG", dG, "dG"), ("dh0", dh0, "dh0"), ("dW_hh", dwhh, "dW_hh"), ("db_hh", dbhh, "db_hh")):
                tab.rule("%s[%d]" % (what, p), hip[p], r64[key][p], r32[key][p])
        if S is not None:
            s64, s32 = by_action(r64), by_action(r32)
            for a in range(A):
                tab.rule("S[action %d]" % a, S[a], s64[a], s32[a])
    _finish(tables)


@pytest.mark.parametrize("aux", [False, True])
@pytest.mark.parametrize("R,rows,n_act,wfac,rfac", spec.HEADS_CASES)
def test_heads_kernels_at_a_peaked_policy(R, rows, n_act, wfac, rfac, aux, monkeypatch):
    """fused.heads_values, heads_loss and heads_loss_pair in the layout of tests/test_hidden_sizes_gpu.py for a trained policy
    (spec.heads_problem: more than a quarter of the rows with p_max == 1.0f, log p(a) below -80): objective, the four statistics,
    dL/dh and every head gradient under the rule; the statistics finite and the entropy not negative."""
    from active_tracking_rl_amd import fused
    x = spec.heads_problem(R, rows, n_act, wfac, rfac, aux)
    T, N = x["T"], x["N"]

    def linear(w, b):
        lin = torch.nn.Linear(w.shape[1], w.shape[0]).to(DEV)
        with torch.no_grad():
            lin.weight.copy_(w); lin.bias.copy_(b)
        return lin
    actors = [linear(*x["prm"][p][0:2]) for p in range(2)]
    critics = [linear(*x["prm"][p][2:4]) for p in range(2)]
    auxes = [None, linear(*x["prm"][1][4:6]) if aux else None]
    prm = [[actors[p].weight, actors[p].bias, critics[p].weight, critics[p].bias] +
           ([auxes[p].weight, auxes[p].bias] if auxes[p] is not None else []) for p in range(2)]
    hs = [x["hs"][p].to(DEV).requires_grad_(True) for p in range(2)]
    store = x["store"].to(DEV)
    actions = store.transpose(1, 2)
    ret, gae, rew = x["ret"].to(DEV), x["gae"].to(DEV), x["rew"].to(DEV)
    scale, scale_aux, w_ent = x["scale"], x["scale_aux"], x["w_ent"]
    ref = []
    for dt, where in ((torch.float64, "cpu"), (torch.float32, DEV)):
        mv = (lambda t: t.detach().cpu()) if where == "cpu" else (lambda t: t)
        ref.append([_heads_reference(mv(hs[p]), [mv(t) for t in prm[p]], mv(store[:, p].reshape(rows)), mv(ret[:, :, p]), mv(gae[:, :, p]),
                                     mv(rew[:, :, 0]), scale[p], scale_aux, w_ent[p], dt) for p in range(2)])
    tab = Table("peaked heads R=%d A=%d aux=%d rows=%d" % (R, n_act, aux, rows))
    val = torch.zeros(T + 1, N, 2, 1, device=DEV)
    for p in range(2):
        fused.heads_values(hs[p].detach(), critics[p], val, p)
        tab.rule("values[%d]" % p, val[:T, :, p].reshape(rows), ref[0][p]["values"], ref[1][p]["values"])
    bad = []

    def hold(tag, p, term, stats, grads):
        if not (bool(torch.isfinite(stats).all()) and bool(torch.isfinite(term))):
            bad.append("%s[%d]: a non-finite statistic or objective: %s" % (tag, p, stats.tolist()))
        if not float(stats[2]) >= 0.0:
            bad.append("%s[%d]: negative entropy %r" % (tag, p, float(stats[2])))
        tab.rule("%s[%d] objective" % (tag, p), term, ref[0][p]["objective"], ref[1][p]["objective"])
        for k, name in enumerate(STAT_NAMES):
            tab.rule("%s[%d] %s" % (tag, p, name), stats[k], ref[0][p]["stats"][k], ref[1][p]["stats"][k])
        assert len(grads) == len(ref[0][p]["grads"])
        for name, g, g64, g32 in zip(GRAD_NAMES, grads, ref[0][p]["grads"], ref[1][p]["grads"]):
            if not bool(torch.isfinite(g).all()):
                bad.append("%s[%d]: non-finite %s" % (tag, p, name))
            tab.rule("%s[%d] %s" % (tag, p, name), g.reshape(g64.shape), g64, g32)
    with _poisoned_allocations(monkeypatch):
        for p in range(2):
            lp, st = fused.heads_loss(hs[p], actors[p], critics[p], auxes[p], store[:, p].reshape(rows), ret, gae, val, p,
                                      rew if auxes[p] is not None else None, 0, scale[p], scale_aux if auxes[p] is not None else 0.0,
                                      w_ent[p], unit_coeff=True)
            hold("loss", p, lp, st, torch.autograd.grad(lp, [hs[p]] + prm[p]))
        cfg = [dict(actions=actions[:, :, p], ret=ret, gae=gae, val=val, off=p, r_aux=rew if auxes[p] is not None else None, aux_off=0,
                    scale=scale[p], scale_aux=scale_aux if auxes[p] is not None else 0.0, w_ent=w_ent[p], stats_scale=0.5)
               for p in range(2)]
        l0, l1, st = fused.heads_loss_pair(hs, actors, critics, auxes, cfg)
        one = torch.ones((), device=DEV)
        got = torch.autograd.grad([l0, l1], hs + prm[0] + prm[1], grad_outputs=[one, one])
    hold("pair", 0, l0, st[0] / 0.5, [got[0]] + list(got[2:2 + len(prm[0])]))
    hold("pair", 1, l1, st[1] / 0.5, [got[1]] + list(got[2 + len(prm[0]):]))
    try:
        tab.finish()
    except AssertionError as e:
        bad.append(str(e))
    assert not bad, "\n".join(bad)
