"""-m gpu: the tracking statistics on the device. The kernel's tables are integers, so they must EQUAL the host model's
(tracking_stats.classify): on synthetic stores at the shapes where the kernel can go wrong, across split calls, a drain and two
replays of a captured graph; on real rollouts, where the bins must also equal the bins of the true positions read back from the
env after every step; and inside the replayed graphs of both training schedules, which must train the same weights with the
statistics attached and without."""
import functools
import os

import numpy as np
import pytest
import torch

import tracking_stats_spec as ts
from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T = 20
LIMIT = 13        # a short TimeLimit: episodes end inside a 40-step walk


@functools.lru_cache(maxsize=None)
def _store(steps, n, seed, n_actions=4):
    return ts.synthetic_store(steps, n, seed, n_actions)


def _fresh(n):
    return (torch.full((n,), -1, dtype=torch.int32, device=DEV), torch.zeros(176, dtype=torch.int64, device=DEV),
            torch.zeros((2, 170, 8), dtype=torch.int64, device=DEV))


def _launch(obs, rew, done, act, carry, hist, act_hist, flags=0, n_actions=4):
    """atr_track_stats on device tensors as they are: obs [T+1, N, 2, 13, 13], rew [T, N, 2], done [T, N], act [T, N, 2] | None."""
    from active_tracking_rl_amd import tracking_stats
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    assert obs.stride(4) == 1 and obs.stride(3) == 13
    tracking_stats.track_stats(obs.data_ptr(), obs.dtype == torch.uint8, obs.stride()[:3], rew.data_ptr(), rew.stride(), done.data_ptr(),
                               done.stride(), act.data_ptr() if act is not None else 0, act.stride() if act is not None else (0, 0, 0),
                               carry.data_ptr(), hist.data_ptr(), act_hist.data_ptr(), done.shape[0], done.shape[1], n_actions, flags,
                               stream)


def _inside(big_shape, cut, value, fill):
    """`value` copied into the slice `cut` of a larger tensor filled with `fill`: a view with the store's strides and an offset."""
    big = torch.full(big_shape, fill, dtype=value.dtype, device=DEV)
    view = big[cut]
    view.copy_(value)
    assert view.shape == value.shape and view.data_ptr() != big.data_ptr()
    return view


def _got(carry, hist, act_hist):
    torch.cuda.synchronize()
    return hist.cpu().numpy(), act_hist.cpu().numpy(), carry.cpu().numpy()


@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("steps", [1, 2, 20])
@pytest.mark.parametrize("n", [1, 3, 5, 67])
def test_kernel_equals_the_host_model(n, steps, u8):
    """Two successive calls per variant on synthetic stores that hold every kind of sample (each inconsistent form and
    out-of-range actions included), continuing carry and tables: (a) contiguous tensors, actions [T, N, 2], auto-reset store;
    (b) every input a slice of a larger poisoned store (non-unit strides), actions a view of a [T, 2, N] store, flags bit 0 set,
    8 actions; (c) no actions. One env, a partial workgroup (4 envs each) and more than one wave's worth of envs."""
    from active_tracking_rl_amd import tracking_stats
    dt = torch.uint8 if u8 else torch.float32
    for variant, flags, n_actions in (("a", 0, 4), ("b", 1, 8), ("c", 0, 4)):
        state, want = _fresh(n), (None, None, None)
        for call in range(2):
            obs, rew, done, act, kinds = _store(steps, n, 100 * call + 7 * n + steps, n_actions)
            d_obs, d_rew, d_done = torch.from_numpy(obs).to(DEV).to(dt), torch.from_numpy(rew).to(DEV), torch.from_numpy(done).to(DEV)
            d_act = torch.from_numpy(act).to(DEV)
            if variant == "b":
                d_obs = _inside((steps + 3, n + 2, 3, 13, 13), (slice(1, steps + 2), slice(1, n + 1), slice(1, 3)), d_obs, 4)
                d_rew = _inside((steps + 2, n + 3, 3), (slice(2, steps + 2), slice(2, n + 2), slice(0, 2)), d_rew, 1.0)
                d_done = _inside((steps + 1, n + 4), (slice(1, steps + 1), slice(3, n + 3)), d_done, 1)
                d_act = d_act.permute(0, 2, 1).contiguous().permute(0, 2, 1)           # [T, 2, N] storage read as [T, N, 2]
                assert n == 1 or d_act.stride() == (2 * n, 1, n)                       # (torch is free with a size-1 dimension's stride)
            elif variant == "c":
                d_act = None
            _launch(d_obs, d_rew, d_done, d_act, *state, flags=flags, n_actions=n_actions)
            want = tracking_stats.classify(obs, rew, done, act if d_act is not None else None, carry=want[2], flags=flags,
                                           n_actions=n_actions, hist=want[0], act_hist=want[1])
            ts.assert_tables_equal(_got(*state), want, (variant, call))
        assert want[0][ts.SAMPLES] == 2 * steps * n
        if steps * n >= 60:     # (the comparison was not one of empty tables)
            assert want[0][ts.INCONSISTENT] > 0 and want[0][:169].sum() > 0 and want[0][ts.OUT] > 0 and want[0][ts.CENTRE] > 0
            assert (want[1].sum() > 0) == (variant != "c") and (want[0][ts.TERMINAL] > 0) == (flags == 0)


def test_split_calls_drain_and_graph_replays():
    """67 envs x 20 steps: the split 7 + 13 equals one call counter for counter; the drain hands both tables out and leaves
    zeros and the carry as it was; two replays of a captured graph (one stream, no branches) count what two consecutive updates
    count — the offset bins exactly twice one update's, the actions of the second replay paired across the boundary."""
    from active_tracking_rl_amd import tracking_stats
    n = 67
    obs, rew, done, act, _ = _store(T, n, 5)
    d_obs, d_rew, d_done, d_act = (torch.from_numpy(x).to(DEV) for x in (obs, rew, done, act))
    one = tracking_stats.classify(obs, rew, done, act)
    whole = _fresh(n)
    _launch(d_obs, d_rew, d_done, d_act, *whole)
    ts.assert_tables_equal(_got(*whole), one, "one call")
    split = _fresh(n)
    _launch(d_obs[:8], d_rew[:7], d_done[:7], d_act[:7], *split)
    _launch(d_obs[7:], d_rew[7:], d_done[7:], d_act[7:], *split)
    ts.assert_tables_equal(_got(*split), one, "7 + 13")
    out_h, out_a = torch.full((176,), -1, dtype=torch.int64, device=DEV), torch.full((2, 170, 8), -1, dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    tracking_stats.track_stats_drain(split[1].data_ptr(), split[2].data_ptr(), out_h.data_ptr(), out_a.data_ptr(), stream)
    torch.cuda.synchronize()
    assert np.array_equal(out_h.cpu().numpy(), one[0]) and np.array_equal(out_a.cpu().numpy(), one[1])
    assert not split[1].cpu().numpy().any() and not split[2].cpu().numpy().any()
    assert np.array_equal(split[0].cpu().numpy(), one[2])
    # a captured update, replayed twice from a fresh carry
    graphed = _fresh(n)
    side = torch.cuda.Stream(device=DEV)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        _launch(d_obs, d_rew, d_done, d_act, *graphed)
    torch.cuda.synchronize()
    assert not graphed[1].cpu().numpy().any()                 # (capturing launched nothing)
    g.replay()
    g.replay()
    two = tracking_stats.classify(obs, rew, done, act, carry=one[2], hist=one[0], act_hist=one[1])
    got = _got(*graphed)
    ts.assert_tables_equal(got, two, "two replays")
    assert np.array_equal(got[0][:171], 2 * one[0][:171]) and got[0][ts.SAMPLES] == 2 * T * n
    assert got[1].sum() > 2 * one[1].sum()                    # the second replay's first actions found a state to pair with


def _env(env_id, n, seed=1, **kw):
    from active_tracking_rl_amd.environment import VecEnv
    return VecEnv(env_id, n, device=DEV, seed=seed, max_episode_steps=LIMIT, **kw)


@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("env_id", ["Track2D-BlockPartialPZR-v0", "Track2D-MazePartialAdv-v0"])
def test_real_rollouts_against_true_positions(env_id, u8, auto_reset):
    """64 envs, 40 random steps written into the rollout store; the positions are read back after every step. Every sample's
    bin equals the bin of its true positions — except done steps of the auto-reset handle, which are TERMINAL (the store holds
    the next episode's first observation); on the auto_reset=False handle they are binned like any other. INCONSISTENT is 0,
    and the device tables equal the host model's."""
    from active_tracking_rl_amd import tracking_stats
    n, steps = 64, 40
    env = _env(env_id, n, seed=7, obs_u8=u8, auto_reset=auto_reset)
    try:
        assert env.obs_u8 == u8
        st = tracking_stats.TrackingStats(env, torch.device(DEV))
        assert st.flags == (0 if auto_reset else 1) and st.n_actions == 4 and env.tracking_stats is st
        buf = env.rollout_buffers(steps)
        assert buf[0].dtype == (torch.uint8 if u8 else torch.float32)
        buf[0][0].copy_(env.reset().reshape(buf[0][0].shape))
        gen = torch.Generator(device=DEV)
        gen.manual_seed(3)
        acts = torch.randint(0, 4, (steps, 2, n), device=DEV, generator=gen)
        pos = np.zeros((steps, n, 2, 2), np.int64)
        for t in range(steps):
            _, _, done, _ = env.step([acts[t, 0], acts[t, 1]], out=(buf[0][t + 1], buf[1][t], buf[2][t]))
            pos[t] = env.core.get_state()["pos"]
            if not auto_reset and bool(done.any()):
                env.core.reset(mask=done)
        st.update(buf[0], buf[1], buf[2], acts.permute(0, 2, 1))
        obs, rew, done = (b.cpu().numpy() for b in buf)
        want = tracking_stats.classify(obs, rew, done, acts.permute(0, 2, 1).cpu().numpy(), flags=st.flags)
        ts.assert_tables_equal(_got(st.carry, st.hist, st.act_hist), want, env_id)
        true_bins = ts.bin_of_positions(pos)
        if auto_reset:
            true_bins[done != 0] = ts.TERMINAL
        hist = want[0]
        print("%s u8=%s auto_reset=%s: in view %d, out %d, co-located %d, terminal %d, paired actions %d"
              % (env_id, u8, auto_reset, hist[:169].sum(), hist[ts.OUT], hist[ts.CENTRE], hist[ts.TERMINAL], want[1][0].sum()))
        assert np.array_equal(tracking_stats.sample_bins(obs, rew, done, st.flags), true_bins)
        assert np.array_equal(hist[:171], np.bincount(true_bins.ravel(), minlength=171))
        assert hist[ts.INCONSISTENT] == 0 and hist[ts.SAMPLES] == steps * n and done.sum() >= n
        assert (hist[ts.TERMINAL] == done.sum()) if auto_reset else (hist[ts.TERMINAL] == 0)
        hist_d, act_d = st.drain()
        torch.cuda.synchronize()
        assert np.array_equal(hist_d.cpu().numpy(), want[0]) and np.array_equal(act_d.cpu().numpy(), want[1])
        assert not st.hist.cpu().numpy().any() and not st.act_hist.cpu().numpy().any()
    finally:
        env.close()


def test_attachment_rules():
    """Refused: a second object on one shard, stacked frames (no rollout store), windows that are not 13 x 13. Agent.reset()
    sets the carry of an attached object to -1."""
    from active_tracking_rl_amd import tracking_stats
    from active_tracking_rl_amd.train import default_args, make_player
    env = _env("Track2D-BlockPartialPZR-v0", 64, obs_u8=True)
    try:
        st = tracking_stats.TrackingStats(env, torch.device(DEV))
        with pytest.raises(RuntimeError, match="already has tracking statistics"):
            tracking_stats.TrackingStats(env, torch.device(DEV))
        args = default_args(env="Track2D-BlockPartialPZR-v0", num_envs=64, num_steps=T)
        args.gpu_ids = [0]
        st.carry.fill_(5)
        player, _ = make_player(args, torch.device(DEV), 0, 1, env=env)          # (make_player resets the shard)
        torch.cuda.synchronize()
        assert (st.carry.cpu().numpy() == -1).all()
        st.detach()
        assert env.tracking_stats is None
    finally:
        env.close()
    for env_id, kw, text in (("Track2D-BlockPartialPZR-v0", dict(stack_frames=2), "rollout store"),
                             ("Track2D-BlockFullPZR-v0", {}, "13 x 13")):
        env = _env(env_id, 4, **kw)
        try:
            with pytest.raises(RuntimeError, match=text):
                tracking_stats.TrackingStats(env, torch.device(DEV))
            assert getattr(env, "tracking_stats", None) is None
        finally:
            env.close()


def _train(schedule, attach, tmp_path=None, n=64, iters=4):
    from active_tracking_rl_amd import tracking_stats
    from active_tracking_rl_amd.train import GraphedIteration, PipelinedIteration, default_args, make_player
    from active_tracking_rl_amd.utils import ScalarWriter
    args = default_args(env="Track2D-BlockPartialPZR-v0", num_envs=n, num_steps=T, seed=2, network="tat-maze-lstm", aux="reward",
                        train_mode=-1)
    args.gpu_ids = [0]
    env = _env("Track2D-BlockPartialPZR-v0", n, seed=2, obs_u8=True)
    try:
        player, opt = make_player(args, torch.device(DEV), 0, 1, env=env)
        st = tracking_stats.TrackingStats(env, torch.device(DEV)) if attach else None
        it = (GraphedIteration if schedule == "synchronous" else PipelinedIteration)(player, opt, args)
        for _ in range(iters):
            it.run()
        it.finish()
        torch.cuda.synchronize()
        weights = opt.bucket.flat.detach().clone()
        if not attach:
            return weights, None
        tables = (st.hist.cpu().numpy().copy(), st.act_hist.cpu().numpy().copy(), st.carry.cpu().numpy().copy())
        writer = ScalarWriter(os.path.join(str(tmp_path), "scalars"))
        summary = st.record(writer, 1234, 0, str(tmp_path))
        writer.close()
        return weights, (tables, summary)
    finally:
        env.close()


@pytest.mark.parametrize("schedule", ["synchronous", "pipelined"])
def test_counts_inside_the_replayed_schedules(schedule, tmp_path):
    """4 replayed iterations (after the schedule's two warm-up iterations) of 64 envs x 20 steps with the object attached:
    SAMPLES = iterations x T x N, INCONSISTENT = 0, and per player the paired actions are SAMPLES - TERMINAL - N — every
    non-terminal sample's state is followed by an action except the run's last one per env — plus the envs whose LAST sample
    was terminal (their carry is -1 at the end: they are in TERMINAL and in N at once; with none of those this is the plain
    formula). record() writes the scalars, the heat map and the raw tables. Without the object the same seed trains
    bit-identical weights: the hook is inert."""
    import json
    from active_tracking_rl_amd import tracking_stats
    n, iters = 64, 4
    with_stats, ((hist, act_hist, carry), summary) = _train(schedule, True, tmp_path, n, iters)
    without, _ = _train(schedule, False, None, n, iters)
    assert torch.isfinite(without).all() and torch.equal(with_stats, without)
    samples = (2 + iters) * T * n
    ended_terminal = int((carry == -1).sum())
    print("%s: samples %d, terminal %d, in view %d, out %d, co-located %d, paired %d / %d, envs ending on a terminal sample %d"
          % (schedule, hist[ts.SAMPLES], hist[ts.TERMINAL], hist[:169].sum(), hist[ts.OUT], hist[ts.CENTRE], act_hist[0].sum(),
             act_hist[1].sum(), ended_terminal))
    assert hist[ts.SAMPLES] == samples and hist[ts.INCONSISTENT] == 0 and hist[:171].sum() == samples
    assert hist[ts.TERMINAL] >= n                              # (the 13-step limit: every env finished several episodes)
    assert act_hist[0].sum() == act_hist[1].sum() == samples - hist[ts.TERMINAL] - n + ended_terminal
    assert not act_hist[:, :, 4:].any()
    assert summary == tracking_stats.summarize(hist, act_hist) and summary["samples"] == samples
    assert 0.0 < summary["in_view_rate"] <= 1.0 and 0.0 <= summary["tracker_toward_rate"] <= 1.0
    heat = os.path.join(str(tmp_path), "heatmaps")
    assert os.path.getsize(os.path.join(heat, "target_offset_1234.png")) > 100
    raw = np.load(os.path.join(heat, "target_offset_1234.npz"))
    assert np.array_equal(raw["hist"], hist) and np.array_equal(raw["act_hist"], act_hist)
    tags = {json.loads(ln)["tag"] for ln in open(os.path.join(str(tmp_path), "scalars", "scalars.jsonl"))}
    assert {"train/in_view_rate", "train/in_range_rate", "train/colocated_rate", "train/mean_distance", "train/tracker_toward_rate",
            "train/target_away_rate"} <= tags <= set(tracking_stats.TAGS)
