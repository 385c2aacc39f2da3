"""-m gpu: the GRU cores' learner (maze-gru, tat-maze-gru) against the float64 evaluation of the same rollout
(tests/learner_f64.py), by the rule and with the helpers of tests/test_learner_f64_gpu.py.

tests/test_gru_fused_gpu.py and tests/test_gru_learner_gpu.py hold the cached GRU learner to the project's own float32 learner
without a cache, at 2e-4 max|ref| per parameter: both share csrc/gru_hip.hip, the heads kernels, the stem backward and the GAE, and
that criterion does not resolve one env's share of a gradient. Here every GRU-specific piece is held to a reference that reaches no
project kernel: the one-launch BPTT (atr_gru_bptt, R = 128), the rollout's fused step (k_gru_step: h_all, acts = (r, z, n, q), the
[features | k h_prev] rows), fused.gru_sequence_cached, atr_gru_bptt_sums + atr_embed_fold, the grouped weight-gradient launch with
three problems per trained player and its colsum bias slices (bias_hh written as [0:2R] and [2R:3R]), boot_values on a GRU cache, and
the co-run dW plan over GRU problem records.

Every case: Track2D-BlockPartialPZR-v0 with a 37-step TimeLimit (PZR37), R = 128, u8 observations, aux 'reward' for tat-maze-gru and
'none' for maze-gru, every 1-D parameter drawn from N(0, 0.1) before the first rollout (_make's bias_noise: b_hn sits inside
r * (W_hn h + b_hn) and starts at zero, where a mistake in its handling cannot show), windows with episode ends at >= 3 distinct
steps, the full _check (every bucket slice, the four loss terms, boot_values, h_all per player where a cache exists), and an
assertion that the case ran the path it is named after.

Gradients, loss terms and bootstrap values: the rule of tests/test_learner_f64_gpu.py unchanged (learner_f64.FACTOR / FLOOR /
ATEN_MAX / RESOLUTION). Hidden states: k_gru_step's stored h_all measured e(hip) 1.91e-7 .. 2.30e-7 per player over the cached cases
(c to f) against e(aten32) 1.18e-7 .. 1.97e-7 — within 4 e(aten32), let alone max(4 e(aten32), HIDDEN_FLOOR) — so HIDDEN_FLOOR = 4e-6
is used as it is (learner_f64.py says what a one-step-late done mask gives against it). The measured figures of each case are in
its docstring.

Three arithmetic-only changes, made one at a time in a scratch build, and what the case named then reported:
  * action 3's column sum left out of k_embed_fold's dW_ih term — case c, mode -1: player1 lstm.weight_ih e(hip) 1.9e-01 against
    1.9e-06 allowed (9.9e4 x), nothing else;
  * the third GRU problem's colsum0 pointed at bias_hh[0:R] instead of bias_hh[2R:3R] (DeferredWeightGrads._problem) — case d,
    mode -1: lstm.bias_hh of both players e(hip) 1.2 / 1.4 against 1e-06 allowed (1.2e6 x / 1.4e6 x);
  * b_hn dropped from the q column of model.gru_step_consts — case c: every tensor, e.g. h_all 3.1e-01 / 2.9e-01 against 4e-06
    (7.8e4 x), player1 lstm.weight_hh 2.3e-01 against 1e-06 (2.3e5 x), boot_values 2.1e-01 (2.1e5 x).
tests/test_gru_learner_gpu.py and tests/test_gru_fused_gpu.py fail under each of the three as well (the second through the NaN
their bucket was filled with, which the misplaced column sum never overwrites): changes of this size are not where the two
criteria differ. They differ below 2e-4 max|ref|: one env's share of a gradient at 512 envs is 5e-4 .. 2e-2 of its NORM here, and
this module allows 1e-6 .. 3e-6 of it."""
import pytest

from test_gru_learner_gpu import _Spy
from test_learner_f64_gpu import PZR37, _eager, _headline, _make, _probe_forward, _run

pytestmark = pytest.mark.gpu
R = 128


def _gru_player(network, n, steps, fused_gru, **kw):
    player, opt, args = _make(network=network, n=n, steps=steps, rnn_out=R, fused_gru=fused_gru, bias_noise=True,
                              **dict(PZR37, aux="reward" if "tat" in network else "none"), **kw)
    m = player.model
    assert m.gru_core and m.tat == ("tat" in network) and bool(m.fused_gru_step) == bool(fused_gru)
    for p in (m.player0, m.player1):
        b_hn, b_ih = p.lstm.bias_hh.detach()[2 * R:], p.lstm.bias_ih.detach()
        assert float(b_hn.std()) > 0.05 and float(b_ih.std()) > 0.05, "b_hn and the rest moved off zero"
    return player, opt, args


def _bias_slices(model, bucket):
    """Per player the data pointers of the bucket's gradient slices a GRU player's three problems write their column sums to."""
    views = {p.data_ptr(): v for p, v in zip(bucket.params, bucket.grad_views())}
    named = dict(model.named_parameters())
    out = []
    for p in (0, 1):
        bih, bhh = (views[named["player%d.lstm.%s" % (p, k)].data_ptr()] for k in ("bias_ih", "bias_hh"))
        assert bhh.numel() == 3 * R
        out.append(sorted([bih.data_ptr(), bhh.data_ptr(), bhh[2 * R:].data_ptr()]))
    return out


def _assert_grouped(spy, model, bucket, mode, fold, passes):
    """What `passes` learner passes launched at a grouped shape: per pass ONE grouped launch of the two fc products and three
    problems per trained player (column blocks of dG: ld1 = 4R) whose colsum0 are that player's bias_ih, bias_hh[0:2R] and
    bias_hh[2R:3R] slices of the bucket; no weight-gradient GEMM beside it; the BPTT launch with the by-action sums and the fold
    where the tracker-aware target is trained, the plain one-launch BPTT otherwise."""
    trained = [0, 1] if mode == -1 else [mode]
    assert spy.count("atr_gemm_tn_grouped") == passes == len(spy.groups) and spy.count("atr_gemm_tn") == 0
    assert spy.count("atr_gru_bptt_sums") == (passes if fold else 0) and spy.count("atr_embed_fold") == (passes if fold else 0)
    assert spy.count("atr_gru_bptt") == (0 if fold else passes)
    assert not any(c.startswith("atr_embed_add") or c.startswith("atr_embed_grad") for c in spy.calls)
    slices = _bias_slices(model, bucket)
    for group in spy.groups:
        assert len(group) == 3 * len(trained) + 2
        gru = [g for g in group if g["ld1"] == 4 * R]
        assert len(gru) == 3 * len(trained) and all(g["colsum1"] is None for g in gru)
        got = sorted(g["colsum0"] for g in gru)
        assert got == sorted(ptr for p in trained for ptr in slices[p]), "the colsum bias slices of the trained players"


def _eager_passes(spy):
    """The learner passes of _eager: two real iterations and then one per window tried."""
    n = spy.count("atr_gru_bptt") + spy.count("atr_gru_bptt_sums")
    assert n >= 3
    return n


@pytest.mark.parametrize("network", ["maze-gru", "tat-maze-gru"])
def test_uncached_gru_learner_at_128_against_float64(network, monkeypatch):
    """Cases a, b. 130 envs x 8 steps, switch off, eager, mode -1: fused.gru_sequence with the ONE-launch atr_gru_bptt (R = 128; the
    R = 64 case of test_learner_at_other_hidden_sizes_against_float64 takes the per-step backward), no cache; tat-maze-gru adds the
    explicit action embedding. The bootstrap value comes from the model's own forward.
    Measured on MI355X (largest e(hip) / allowed per case and the tensor it belongs to):
      case                      gradients                     loss terms  boot_values        h_all e(hip)
      maze-gru                  0.59 player0 lstm.weight_hh   0.16        2.9e-07 (0.28)     (no cache)
      tat-maze-gru              0.60 player0 lstm.weight_hh   0.18        2.2e-07 (0.22)     (no cache)
    lstm.weight_hh: e(hip) 5.9e-07 / 6.0e-07 against e(aten32) 9.6e-08 / 9.8e-08 (the floor of 1e-6 decides); its one-env share is
    3.2e-03 / 1.5e-02."""
    player, opt, args = _gru_player(network, 130, 8, False)
    try:
        _probe_forward(player.model)
        spy = _Spy(monkeypatch)
        _eager(player, opt, args, -1, "%s R=128 uncached eager" % network)
        assert player._cache is None
        passes = _eager_passes(spy)
        assert spy.count("atr_gru_bptt") == passes and spy.count("atr_gru_bptt_sums") == 0 and spy.count("atr_embed_fold") == 0
        assert spy.count("atr_gemm_tn_grouped") == 0
    finally:
        player.env.close()


@pytest.mark.parametrize("mode", [-1, 1])
def test_cached_gru_learner_below_the_grouped_launch_against_float64(mode, monkeypatch):
    """Case c. tat-maze-gru, --fused-gru, 130 envs x 8 steps = 1040 rows, eager: the rollout through k_gru_step into the cache,
    fused.gru_sequence_cached, atr_gru_bptt_sums + atr_embed_fold on the spot, the weight gradients on the spot, boot_values on the
    GRU cache. 130 is a multiple of no tile.
    Measured on MI355X (as above; hidden states against HIDDEN_FLOOR, see the note at the head of this module):
      case                      gradients                     loss terms  boot_values        h_all e(hip)
      mode -1                   0.60 player0 lstm.weight_hh   0.12        1.4e-07 (0.14)     2.1e-07 .. 2.1e-07 (0.05)
      mode 1                    0.57 player1 lstm.weight_hh   0.31        1.4e-07 (0.14)     2.0e-07 .. 2.1e-07 (0.05)"""
    player, opt, args = _gru_player("tat-maze-gru", 130, 8, True)
    try:
        spy = _Spy(monkeypatch)
        _eager(player, opt, args, mode, "tat-maze-gru 130x8 cached eager mode %d" % mode)
        assert player._cache is not None and player._cache.gru and player.model.env_step_fused_seen is True
        assert getattr(player._cache, "boot", None) is not None, "boot_values ran on the GRU cache"
        passes = _eager_passes(spy)
        assert spy.count("atr_gru_bptt_sums") == passes == spy.count("atr_embed_fold") and spy.count("atr_gru_bptt") == 0
        assert spy.count("atr_gemm_tn_grouped") == 0
        assert not any(c.startswith("atr_embed_add") or c.startswith("atr_embed_grad") for c in spy.calls)
    finally:
        player.env.close()


@pytest.mark.parametrize("network,mode", [("tat-maze-gru", -1), ("tat-maze-gru", 0), ("tat-maze-gru", 1), ("maze-gru", -1)])
def test_captured_gru_learner_grouped_launch_against_float64(network, mode, monkeypatch):
    """Cases d, e. --fused-gru, 512 envs x 8 steps = 4096 rows, GraphedIteration: the grouped launch with three problems per trained
    player and the colsum bias slices; the optimizer owns both players, so modes 0 / 1 leave the untrained player's slices exactly
    zero. tat-maze-gru trains the target through atr_gru_bptt_sums and the fold as the grouped launch's post-flush hook; maze-gru
    (and tat-maze-gru in mode 0) through atr_gru_bptt. tat-maze-gru mode -1 runs with gamma = 0.99, tau = 0.95.
    Measured on MI355X (as above). The resolution condition holds at 512 envs: the smallest one-env share of a RESOLVED tensor is
    4.5e-04 (player0 lstm.weight_hh, tat-maze-gru mode 0) against 10 x 1e-06 allowed.
      case                      gradients                     loss terms  boot_values        h_all e(hip)
      tat-maze-gru, mode -1     0.14 player1 actor bias       0.17        1.0e-07 (0.10)     2.1e-07 .. 2.1e-07 (0.05)
      tat-maze-gru, mode 0      0.19 player0 conv1.bias       0.16        1.2e-07 (0.12)     2.1e-07 .. 2.1e-07 (0.05)
      tat-maze-gru, mode 1      0.16 player1 critic bias      0.15        1.9e-07 (0.19)     2.1e-07 .. 2.1e-07 (0.05)
      maze-gru, mode -1         0.20 player0 critic bias      0.13        1.0e-07 (0.10)     2.1e-07 .. 2.3e-07 (0.06)
    lstm.bias_hh (the two colsum slices): e(hip) 5.3e-08 .. 9.9e-08 against e(aten32) 5.9e-08 .. 9.6e-08."""
    coef = dict(tau=0.95, gamma=0.99) if (network, mode) == ("tat-maze-gru", -1) else {}
    player, opt, args = _gru_player(network, 512, 8, True, **coef)
    assert (args.gamma, args.tau) == ((0.99, 0.95) if coef else (0.9, 1.0))
    try:
        spy = _Spy(monkeypatch)
        _run(player, opt, args, mode, "%s 512x8 captured mode %d" % (network, mode), spy=spy)
        assert player._cache is not None and player._cache.gru and player.model.env_step_fused_seen is True
        # (two warm-up iterations and the capture issued their launches through the library's entry points)
        _assert_grouped(spy, player.model, opt.bucket, mode, fold="tat" in network and mode != 0, passes=3)
    finally:
        player.env.close()


def test_gru_learner_synchronous_and_pipelined_corun_against_float64(monkeypatch):
    """Case f. tat-maze-gru, --fused-gru, 1024 envs x 4 steps = 4096 rows (what train.captured_learner_ok allows), mode -1: the
    synchronous captured graph, then the same rollout transplanted into a PipelinedIteration replica whose learner graph holds the
    co-run dW plan (train.CORUN_MIN_ENVS) over the GRU problem records; 1024 rows per step is a row count the 512-env cases never
    give the tile loops. One float64 reference for both.
    Measured on MI355X (as above). The resolution condition holds at 1024 envs: the smallest one-env share of a RESOLVED tensor is
    2.9e-03 (player0 conv2.weight) against 10 x 1.2e-06 allowed at the most (lstm.weight_hh, e(aten32) 2.9e-07).
      case                      gradients                     loss terms  boot_values        h_all e(hip)
      synchronous               0.20 player1 conv1.bias       0.23        8.9e-08 (0.09)     1.9e-07 .. 1.9e-07 (0.05)
      pipelined co-run          0.20 player1 conv1.bias       0.23        8.9e-08 (0.09)     (the synchronous rollout's)
    The co-run plan moves the grouped launch's outputs only: encoder.fc.weight 1.35e-07 -> 1.38e-07 / 1.26e-07 -> 1.28e-07,
    lstm.weight_ih 1.36e-07 -> 1.38e-07, lstm.bias_hh 1.06e-07 -> 1.00e-07 / 9.3e-08 -> 9.1e-08; every other slice's figure is the synchronous learner's."""
    from active_tracking_rl_amd.train import CORUN_MIN_ENVS, captured_learner_ok
    assert captured_learner_ok(1024, 4) and CORUN_MIN_ENVS == 1024
    mode = -1
    player, opt, args = _gru_player("tat-maze-gru", 1024, 4, True)
    try:
        spy = _Spy(monkeypatch)
        it_p = _headline(player, opt, args, mode, "tat-maze-gru 1024x4")
        spy.recording = False
        assert it_p.corun
        assert all(a._cache is not None and a._cache.gru for a in [player] + list(it_p.players))
        assert player.model.env_step_fused_seen is True and it_p.players[0].model.env_step_fused_seen is True
        # master: 2 warm-up passes of either schedule + the synchronous capture; replicas: one capture each + replica 0's again
        assert spy.count("atr_gemm_tn_grouped") == len(spy.groups) == 8 and spy.count("atr_gemm_tn") == 0
        assert spy.count("atr_gru_bptt_sums") == 8 == spy.count("atr_embed_fold") and spy.count("atr_gru_bptt") == 0
        own = {id(b): _bias_slices(a.model, b) for a, b in zip(it_p.players, it_p.buckets)}
        own[id(opt.bucket)] = _bias_slices(player.model, opt.bucket)
        wanted = [sorted(s[0] + s[1]) for s in own.values()]
        for group in spy.groups:
            gru = [g for g in group if g["ld1"] == 4 * R]
            assert len(group) == 8 and len(gru) == 6
            assert sorted(g["colsum0"] for g in gru) in wanted, "the colsum bias slices of one bucket"
    finally:
        player.env.close()
