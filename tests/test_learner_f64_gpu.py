"""-m gpu: the learner's gradient bucket against a float64 evaluation of the same rollout (tests/learner_f64.py).

Each case builds a player the way the drivers do, runs real iterations (rollout + learner + update) until the rollout
window holds episode ends at 3 or more distinct steps, then replays that iteration's captured rollout + learner without
its update and compares, tensor by tensor, what the HIP learner produced with the float64 reference of the CPU path:

  * every parameter's slice of the flat gradient bucket;
  * the four loss terms (policy, value, entropy, |aux|, averaged over envs) the learner reports;
  * the bootstrap values V(s_T) of the learner's bootstrap step;
  * the hidden states the rollout stored (h_all[:, 1:]): the forward kernels that fed the cached learner.

Tolerance, per tensor, with e(x) = ||x - x64|| / ||x64||: e(hip) <= max(4 e(aten32), 1e-6) and e(aten32) <= 1e-4, where
aten32 is the same evaluation in float32 on the GPU through PyTorch's own kernels (every project kernel off). Resolution:
for the stem, fc and both LSTM weights of each trained player the allowed error is at least 10x smaller than the share
of ONE env's loss terms in that gradient, so a kernel that drops or doubles one env's contribution fails. Where the
float64 gradient is zero (the untrained player in training modes 0 / 1) the bucket must be exactly zero.

Hidden sizes other than 128 (--rnn-out 64 / 96 / 256, maze-gru at 64) and tau != 1: the last test of the module and the mode -1 case
of the 512-env test; their measured figures are in those tests' docstrings. With the tau factor removed from k_gae in a scratch build
the 512-env mode -1 case fails (as do the tau != 1 cases of tests/test_fused_stem_gpu.py's GAE test).

The GRU cores at R = 128 — the one-launch GRU BPTT, the --fused-gru cache, its fold, grouped and co-run paths — are held to the same
rule with these helpers in tests/test_gru_learner_f64_gpu.py."""
import numpy as np
import pytest
import torch

import learner_f64

pytestmark = pytest.mark.gpu

from learner_f64 import ATEN_MAX, FACTOR, FLOOR, HIDDEN_FLOOR, RESOLUTION  # noqa: E402  (stated there once; tests/f64_rule.py reads them too)
RESOLVED = ("encoder.conv1.weight", "encoder.conv2.weight", "encoder.fc.weight", "lstm.weight_ih", "lstm.weight_hh")


def _probe_boot(model):
    """Keep a copy of the values the learner's bootstrap step writes (one copy launch appended to that step)."""
    orig = model.boot_values

    def boot_values(states, cache, done, v_out):
        out = orig(states, cache, done, v_out)
        model.boot_probe = v_out.detach().clone()
        return out
    model.boot_values = boot_values


def _probe_forward(model):
    """Where the learner's bootstrap step is the model's own forward (hidden sizes without a heads kernel, cores without a
    rollout cache): keep its values and the tracker action it drew. Rollouts act through model.act, so the last call is it."""
    orig = model.forward

    def forward(inputs, test=False):
        out = orig(inputs, test)
        model.boot_probe, model.boot_action = out[0].detach().clone(), out[1][0].detach().clone()
        return out
    model.forward = forward


BIAS_NOISE_SEED = 1234


def _make(env_id, n, network, aux, train_mode, steps=20, seed=31, max_steps=500, mixed=False, rnn_out=128, tau=None, gamma=None,
          fused_gru=False, bias_noise=False):
    """fused_gru: the --fused-gru switch (the GRU cores' cached, env-fused rollout step). bias_noise: every 1-D parameter (the cell's
    b_ih / b_hh — b_hn among them —, the fc and head biases: all zero at initialisation) drawn from N(0, 0.1) under a fixed seed, in
    place (the parameters are views of the bucket's flat tensor), before any rollout, warm-up or capture."""
    from active_tracking_rl_amd import registry
    from active_tracking_rl_amd.environment import VecEnv
    from active_tracking_rl_amd.train import default_args, make_player
    over = dict(rnn_out=rnn_out)
    if fused_gru:
        over["fused_gru"] = True
    if tau is not None:
        over["tau"] = tau
    if gamma is not None:
        over["gamma"] = gamma
    args = default_args(env=env_id, network=network, aux=aux, train_mode=train_mode, num_envs=n, num_steps=steps, seed=seed,
                        **over)
    args.gpu_ids = [0]
    over = {}
    if max_steps != 500:
        over["max_episode_steps"] = max_steps
    if mixed:
        over["map_type_per_env"] = np.array([registry.MAP_CODE["Block" if i % 2 == 0 else "Maze"] for i in range(n)], np.uint8)
    env = VecEnv(env_id, n, device="cuda:0", seed=seed, obs_u8=True, **over)
    player, opt = make_player(args, torch.device("cuda:0"), 0, 1, env=env)
    if bias_noise:
        g = torch.Generator(device="cuda:0").manual_seed(BIAS_NOISE_SEED)
        flat = opt.bucket.flat.data_ptr(), opt.bucket.flat.data_ptr() + opt.bucket.flat.numel() * 4
        with torch.no_grad():
            for p in player.model.parameters():
                if p.dim() == 1:
                    p.normal_(0, 0.1, generator=g)
                    assert flat[0] <= p.data_ptr() < flat[1], "a parameter that left the bucket's flat tensor"
    _probe_boot(player.model)
    return player, opt, args


def _snapshot(player, **kw):
    """learner_f64.snapshot; on a GRU cache (model._new_cache_gru: h_all [2, T+1, N, R] as the LSTM cache lays it out, c_all the zero
    tensor no launch writes, the bootstrap draw in cache.boot.actions[0]) the cell state it starts from must be exactly zero."""
    snap = learner_f64.snapshot(player, **kw)
    if getattr(player._cache, "gru", False):
        assert float(snap["c0"].abs().max()) == 0.0 and float(player._cache.c_all.abs().max()) == 0.0, "a GRU cache's c_all is zero"
        assert snap["h0"].shape == snap["c0"].shape == (2, player._cache.N, player._cache.h_all.shape[-1])
    return snap


def _window(it, player, opt, mode, max_iters=80):
    """Real iterations of the synchronous captured graph until the rollout window holds episode ends at >= 3 distinct
    steps; that last iteration's rollout + learner are replayed without its update (the bucket then holds its gradient)."""
    g = it.g_rolls[mode]
    for i in range(max_iters):
        opt.bucket.grad.zero_()
        g.replay()
        torch.cuda.synchronize()
        steps = int((player._buf[2].sum(1) > 0).sum())
        if steps >= min(3, player._buf[2].shape[0]):
            return i
        it.g_opt.replay()
    raise AssertionError("no window with episode ends at 3 distinct steps in %d iterations" % max_iters)


def _bucket_grads(model, bucket):
    names = {id(p): n for n, p in model.named_parameters()}
    return {names[id(p)]: v.detach().clone() for p, v in zip(bucket.params, bucket.grad_views())}


def _stats(stats):
    pl, vl, en, pr = stats
    return dict(policy=pl.reshape(2), value=vl.reshape(2), entropy=en.reshape(2), aux=pr.reshape(-1)[:1])


def _check(label, ref, floor, share, mode, hip_grads, hip_terms, hip_boot, hip_h=None):
    """The per-tensor rule of the module docstring; returns the table rows it checked."""
    rows, bad = [], []

    def rule(what, hip, x64, x32, need_resolution=None, floor_=FLOOR):
        e_hip, e32 = learner_f64.rel_err(hip, x64), learner_f64.rel_err(x32, x64)
        allowed = max(FACTOR * e32, floor_)
        rows.append((label, what, e_hip, e32, need_resolution))
        if not (np.isfinite(e_hip) and e_hip <= allowed):
            bad.append("%s: e(hip) %.3e > allowed %.3e (e(aten32) %.3e)" % (what, e_hip, allowed, e32))
        if e32 > ATEN_MAX:
            bad.append("%s: e(aten32) %.3e > %.0e: reference and floor disagree" % (what, e32, ATEN_MAX))
        if need_resolution is not None and not allowed * RESOLUTION <= need_resolution:
            bad.append("%s: allowed error %.3e does not resolve one env's share %.3e" % (what, allowed, need_resolution))

    trained = [p for p in (0, 1) if mode in (-1, p)]
    n_zero = 0
    for name, hip in hip_grads.items():
        x64 = ref["grads"][name]
        if float(x64.norm()) == 0.0:
            # (the untrained player of modes 0 / 1: nothing may leak into its slices)
            assert float(hip.abs().max()) == 0.0, (label, name, "non-zero gradient where the loss does not reach")
            n_zero += 1
            continue
        res = None
        if any(name == "player%d.%s" % (p, r) for p in trained for r in RESOLVED):
            res = share[name]
        rule(name, hip, x64, floor["grads"][name], res)
    if mode in (0, 1):
        assert n_zero > 0 or all(n.startswith("player%d." % mode) for n in hip_grads), label
    for k in learner_f64.TERMS:
        rule("loss." + k, hip_terms[k], ref["terms"][k], floor["terms"][k])
    rule("boot_values", hip_boot, ref["boot_v"], floor["boot_v"])
    if hip_h is not None:
        for p in (0, 1):
            rule("h_all.player%d" % p, hip_h[:, p], ref["h"][:, p], floor["h"][:, p], floor_=HIDDEN_FLOOR)
    for r in rows:
        print("%-28s %-36s e(hip) %.3e  e(aten32) %.3e  one-env share %s" %
              (r[0], r[1], r[2], r[3], "%.3e" % r[4] if r[4] is not None else "-"))
    assert not bad, "\n".join([label] + bad)
    return rows


def _references(snap, mode):
    ref = learner_f64.reference(snap, mode)
    floor = learner_f64.reference(snap, mode, dtype=torch.float32, device="cuda:0")
    n = snap["dones"].shape[1]
    one = learner_f64.reference(snap, mode, envs=[0])
    share = {k: float(one["grads"][k].norm()) / n / max(float(ref["grads"][k].norm()), 1e-300) for k in ref["grads"]}
    return ref, floor, share


def _run(player, opt, args, mode, label, spy=None):
    """Synchronous captured graph: >= 2 real iterations (the eager warm-up, kept), then the window. spy (an object with a
    `recording` flag): records while the warm-up iterations and the capture issue their launches, not after."""
    from active_tracking_rl_amd.train import GraphedIteration
    it = GraphedIteration(player, opt, args, mode=mode, keep_warmup_updates=True)
    if spy is not None:
        spy.recording = False
    it.run(mode)
    _window(it, player, opt, mode)
    # (R = 256: the bootstrap step is the model's own forward, whose draw _probe_forward kept)
    in_cache = getattr(player._cache, "boot", None) is not None
    snap = _snapshot(player, boot_action=None if (in_cache or not player.model.tat) else player.model.boot_action)
    hip = _bucket_grads(player.model, opt.bucket)
    h = player._cache.h_all[:, 1:].transpose(0, 1)
    ref, floor, share = _references(snap, mode)
    _check(label, ref, floor, share, mode, hip, _stats(it.stats_by_mode[mode]), player.model.boot_probe, h)
    return player


def test_headline_learner_synchronous_and_pipelined_against_float64():
    """Track2D-BlockPartialPZR-v0, 4096 envs x 20 steps, tat-maze-lstm, u8 observations, mode -1: the timed region's
    learner. Synchronous captured graph (k_stem_bwd16 over 81920 frames per player, k_lstm_bptt on the stored
    pre-activations, the embedding fold as the grouped dW launch's post-flush hook at K = 81920, strided dReLU,
    heads_loss_pair), then the same rollout handed to a PipelinedIteration replica whose learner graph was captured with
    the co-run dW plan: one float64 reference for both."""
    mode = -1
    player, opt, args = _make("Track2D-BlockPartialPZR-v0", 4096, "tat-maze-lstm", "reward", mode)
    try:
        _headline(player, opt, args, mode, "pzr4096")
        cache = player._cache               # (the window's: nothing ran on the master after it)
        assert cache.pre_all is not None and cache.fh_all is not None
    finally:
        player.env.close()


def _headline(player, opt, args, mode, label):
    """One rollout window through the synchronous captured graph, then the same rollout transplanted into a PipelinedIteration
    replica whose learner graph was captured with the co-run dW plan: one float64 reference for both. Returns the schedule."""
    from test_drivers_gpu import _transplant_rollout
    from active_tracking_rl_amd.train import GraphedIteration, PipelinedIteration
    it_p = PipelinedIteration(player, opt, args, mode=mode, serial=True)      # (first: it warms up eagerly on the master)
    assert it_p.corun, "co-run dW is the pipelined learner's form from train.CORUN_MIN_ENVS envs up"
    it = GraphedIteration(player, opt, args, mode=mode, keep_warmup_updates=True)
    rep = it_p.players[0]
    _probe_boot(rep.model)
    rep.model._sampler.seed = player.model._sampler.seed         # the bootstrap step's draw: same Philox key
    it_p._capture(mode, 0)
    it.run(mode)
    _window(it, player, opt, mode)
    cache = player._cache
    assert player._buf[0].dtype == torch.uint8
    snap = _snapshot(player)
    hip_sync = _bucket_grads(player.model, opt.bucket)
    boot_sync = player.model.boot_probe.clone()
    h = cache.h_all[:, 1:].transpose(0, 1).clone()
    moved = _transplant_rollout({k: v for k, v in vars(player).items() if k not in ("model", "env", "args")},
                                {k: v for k, v in vars(rep).items() if k not in ("model", "env", "args")})
    assert moved >= 8, moved
    rep.model._sampler.counter.copy_(player.model._sampler.counter)
    it_p.buckets[0].flat.copy_(opt.bucket.flat)                  # the weights the synchronous learner used
    it_p.buckets[0].grad.zero_()
    it_p.graphs[(mode, 0)][1].replay()
    torch.cuda.synchronize()
    assert torch.equal(rep._cache.boot.actions[0], cache.boot.actions[0]), "the two bootstrap steps drew differently"
    hip_pipe = _bucket_grads(rep.model, it_p.buckets[0])
    ref, floor, share = _references(snap, mode)
    _check(label + " synchronous", ref, floor, share, mode, hip_sync, _stats(it.stats_by_mode[mode]), boot_sync, h)
    _check(label + " pipelined co-run", ref, floor, share, mode, hip_pipe, _stats(it_p.graphs[(mode, 0)][2]),
           rep.model.boot_probe)
    return it_p


@pytest.mark.parametrize("mode", [-1, 0, 1])
def test_pair_kernel_learner_512_against_float64(mode):
    """512 envs (<= 512-row path): pair kernels, k_embed_add / k_embed_grad_*, BPTT on activated gates, the wave-per-frame
    stem backward. The optimizer owns both players, so modes 0 / 1 leave the untrained player's slices exactly zero.
    Mode -1 runs with gamma = 0.99, tau = 0.95 (every other case of this module has tau = 1, where k_gae's tau factor is
    invisible); modes 0 / 1 keep the defaults 0.9 / 1."""
    coef = dict(tau=0.95, gamma=0.99) if mode == -1 else {}
    player, opt, args = _make("Track2D-BlockPartialPZR-v0", 512, "tat-maze-lstm", "reward", -1, **coef)
    assert (args.gamma, args.tau) == ((0.99, 0.95) if mode == -1 else (0.9, 1.0))
    try:
        _run(player, opt, args, mode, "pzr512 mode %d" % mode)
        assert player._cache.fh_all is None and player._cache.acts is not None
    finally:
        player.env.close()


def test_three_step_window_runs_the_eager_learner_and_matches_float64():
    """1024 envs x 3 steps = 3072 rows: one-GEMM rollout with stored pre-activations, below the grouped dW launch's
    threshold (the fold follows the product on the spot). Captured in a hipGraph, this learner wrote the tracker-aware
    target's lstm.bias_ih / bias_hh (e = 24.6) and encoder.fc.bias (e = 1.0) slices of the bucket wrong, while every weight
    gradient and the same learner run eagerly were right: the drivers refuse to capture at such shapes
    (train.captured_learner_ok) and main.py runs the eager loop there. Checked here: the refusal, and the eager learner —
    rollout + Agent.compute_grads into the bucket, what that loop runs — against float64."""
    from active_tracking_rl_amd.train import GraphedIteration, PipelinedIteration, captured_learner_ok, rollout
    assert not captured_learner_ok(1024, 3) and captured_learner_ok(512, 3) and captured_learner_ok(1024, 4)
    mode = -1
    player, opt, args = _make("Track2D-BlockPartialPZR-v0", 1024, "tat-maze-lstm", "reward", -1, steps=3)
    try:
        for cls in (GraphedIteration, PipelinedIteration):
            with pytest.raises(RuntimeError, match="captured learner is not supported"):
                cls(player, opt, args, mode=mode)
        for _ in range(2):                                  # real iterations, with updates
            rollout(player, args.num_steps)
            player.optimize(None, opt, player.model, mode, player.device)
        for _ in range(80):
            rollout(player, args.num_steps)
            opt.bucket.grad.zero_()
            stats = player.compute_grads(opt, mode)
            torch.cuda.synchronize()
            if int((player._buf[2].sum(1) > 0).sum()) >= 3:
                break
            opt.step()
        else:
            raise AssertionError("no window with episode ends at all 3 steps")
        assert player._cache.pre_all is not None and player._cache.fh_all is not None
        snap = _snapshot(player)
        ref, floor, share = _references(snap, mode)
        _check("pzr1024x3 eager", ref, floor, share, mode, _bucket_grads(player.model, opt.bucket), _stats(stats),
               player.model.boot_probe, player._cache.h_all[:, 1:].transpose(0, 1))
    finally:
        player.env.close()


@pytest.mark.parametrize("n", [1001, 1002])
def test_ragged_frame_count_against_float64(n):
    """n envs x 20 steps: 20020 / 20040 frames per tracker launch, not a multiple of 16 — the ragged last pass of the 16-frame
    stem kernels and a ragged K tail of k_gemm_tn on the one-GEMM path. 1001 keeps float observations (the byte rollout store
    needs an even count); 1002 runs on the u8 frames the headline uses."""
    player, opt, args = _make("Track2D-BlockPartialPZR-v0", n, "tat-maze-lstm", "reward", -1)
    try:
        _run(player, opt, args, -1, "pzr%d ragged" % n)
        assert player._cache.fh_all is not None
        assert player._buf[0].dtype == (torch.float32 if n % 2 else torch.uint8)
    finally:
        player.env.close()


@pytest.mark.parametrize("name", ["mazenav1024_mode0", "adv2048_mixed", "pzr1024_timelimit37"])
def test_baseline_configurations_against_float64(name):
    """configs[3] (Track2D-MazePartialNav-v0, 1024 envs, maze-lstm, mode 0: Nav targets, two-GEMM cell), configs[4]
    (Track2D-BlockPartialAdv-v0, 2048 envs, maze-lstm, mode -1, Block / Maze maps mixed), and PZR 1024 with a 37-step
    TimeLimit (many time-limit ends inside one window)."""
    if name == "mazenav1024_mode0":
        player, opt, args = _make("Track2D-MazePartialNav-v0", 1024, "maze-lstm", "none", 0)
        mode = 0
    elif name == "adv2048_mixed":
        player, opt, args = _make("Track2D-BlockPartialAdv-v0", 2048, "maze-lstm", "none", -1, mixed=True)
        mode = -1
    else:
        player, opt, args = _make("Track2D-BlockPartialPZR-v0", 1024, "tat-maze-lstm", "reward", -1, max_steps=37)
        mode = -1
    try:
        _run(player, opt, args, mode, name)
    finally:
        player.env.close()


def _eager(player, opt, args, mode, label):
    """The eager loop (rollout + Agent.compute_grads into the bucket; two real updates first) until the window holds episode
    ends at >= 3 distinct steps, then the full rule of _check on that window."""
    from active_tracking_rl_amd.train import rollout
    for _ in range(2):
        rollout(player, args.num_steps)
        player.optimize(None, opt, player.model, mode, player.device)
    for _ in range(80):
        rollout(player, args.num_steps)
        acts = torch.stack(player.actions, 0).clone() if player._cache is None else None
        opt.bucket.grad.zero_()
        stats = player.compute_grads(opt, mode)
        torch.cuda.synchronize()
        if int((player._buf[2].sum(1) > 0).sum()) >= 3:
            break
        opt.step()
    else:
        raise AssertionError("no window with episode ends at 3 distinct steps")
    cache = player._cache
    in_cache = cache is not None and getattr(cache, "boot", None) is not None
    boot_action = None if (in_cache or not player.model.tat) else player.model.boot_action
    snap = _snapshot(player, boot_action=boot_action, actions=acts)
    ref, floor, share = _references(snap, mode)
    h = cache.h_all[:, 1:].transpose(0, 1) if cache is not None else None
    _check(label, ref, floor, share, mode, _bucket_grads(player.model, opt.bucket), _stats(stats), player.model.boot_probe, h)
    return player


PZR37 = dict(env_id="Track2D-BlockPartialPZR-v0", aux="reward", train_mode=-1, max_steps=37)   # every window holds episode ends
OTHER_SIZES = ([("eager", "tat-maze-lstm", R, -1) for R in (64, 256)] + [("eager", "tat-maze-lstm", 64, m) for m in (0, 1)] +
               [("eager", "maze-gru", 64, -1), ("eager", "tat-maze-lstm", 96, -1)] +
               [("captured", "tat-maze-lstm", R, -1) for R in (64, 256)])


@pytest.mark.parametrize("leg,network,R,mode", OTHER_SIZES)
def test_learner_at_other_hidden_sizes_against_float64(leg, network, R, mode):
    """--rnn-out off 128, Track2D-BlockPartialPZR-v0 with a 37-step TimeLimit, aux reward.
    eager: 130 envs x 8 steps through rollout + Agent.compute_grads. R = 64 / 256: the generic cell kernels of the rollout, the
    per-step BPTT (atr_lstm_cell_backward + bmm: the one-launch kernel is R = 128's), the heads kernels at 16 / 64 lanes per
    row, the weight gradients on the spot. R = 96 (model.hidden_size_support: a cache, no heads kernel): the tensor heads over
    the cached recurrence, the bootstrap value through the model's own forward. maze-gru at R = 64: no cache, gru_sequence.
    captured: 1024 envs x 4 steps = 4096 rows (what train.captured_learner_ok allows) through GraphedIteration.
    The captured learner meets the rule at both sizes (no gradient anywhere near the bias-gradient fault of captured_learner_ok,
    which stays as it is): capture is not refused off R = 128.
    R = 256 takes its bootstrap values from the model's own forward (model.hidden_size_support: fused_boot), inside the captured
    graph too: through one more step of the rollout's cell kernels the eager case measured e = 1.321e-06 against 1.226e-06 allowed.
    Measured on MI355X (largest e(hip) / allowed per case and the tensor it belongs to; hidden states against HIDDEN_FLOOR):
      case                      gradients                     loss terms  boot_values        h_all e(hip)
      eager 64, mode -1         0.64 lstm.weight_hh           0.28        7.9e-07 (0.66)     6.4e-07 .. 1.1e-06 (0.28)
      eager 64, mode 0          0.64 lstm.weight_hh           0.29        8.8e-07 (0.73)     6.3e-07 .. 1.1e-06 (0.28)
      eager 64, mode 1          0.51 lstm.weight_hh           0.21        7.2e-07 (0.54)     6.4e-07 .. 1.1e-06 (0.27)
      eager 256, mode -1        0.74 actor weight             0.18        5.8e-07 (0.49)     1.2e-06 .. 1.8e-06 (0.44)
      eager 96, mode -1         0.63 lstm.weight_hh           0.19        2.4e-07 (0.24)     7.5e-07 .. 1.0e-06 (0.25)
      eager maze-gru 64         0.62 lstm.weight_hh           0.21        5.4e-07 (0.36)     (no cache)
      captured 64               0.45 actor weight             0.41        5.3e-07 (0.53)     6.3e-07 .. 1.1e-06 (0.27)
      captured 256              0.61 actor weight             0.16        4.7e-07 (0.46)     1.2e-06 .. 1.7e-06 (0.43)
    lstm.weight_hh of captured 64 (4096 rows, fused.bmm_tn's chunked sum): e(hip) 1.95e-07 against e(aten32) 2.74e-07."""
    n, steps = (130, 8) if leg == "eager" else (1024, 4)
    # (maze-gru has no reward head: aux "none", as every case of a network without one in this module)
    player, opt, args = _make(network=network, n=n, steps=steps, rnn_out=R, **dict(PZR37, aux="reward" if "tat" in network else "none"))
    try:
        label = "%s R=%d %s mode %d" % (network, R, leg, mode)
        _probe_forward(player.model)
        if leg == "eager":
            _eager(player, opt, args, mode, label)
            assert (player._cache is None) == ("gru" in network)
        else:
            _run(player, opt, args, mode, label)
    finally:
        player.env.close()
