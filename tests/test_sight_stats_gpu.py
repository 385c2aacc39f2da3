"""-m gpu: the sight statistics on the device. The kernel's table is integers, so it must EQUAL the host model's
(sight_stats.classify): on synthetic stores at the shapes where the kernel can go wrong, in every memory layout, across split
calls, a drain and two replays of a captured graph, and on hand-made windows; on real rollouts, where the class read from the
window must also equal the class read from the env's TRUE map and positions; and inside the replayed graphs of a training
schedule, beside the tracking statistics, which must train the same weights with the statistics attached and without."""
import functools
import os

import numpy as np
import pytest
import torch

import sight_spec as sp
from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T = 20
LIMIT = 13        # a short TimeLimit: episodes end inside a 40-step walk


@functools.lru_cache(maxsize=None)
def _store(steps, n, seed):
    return sp.synthetic_store(steps, n, seed)[:3]


def _fresh(n, carry=-1):
    return torch.full((n,), carry, dtype=torch.int32, device=DEV), torch.zeros(776, dtype=torch.int64, device=DEV)


def _launch(obs, rew, done, carry, tab, flags=0):
    """atr_sight_stats on device tensors as they are: obs [T+1, N, 2, 13, 13], rew [T, N, 2], done [T, N]."""
    from active_tracking_rl_amd import sight_stats
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    assert obs.stride(4) == 1 and obs.stride(3) == 13
    sight_stats.sight_stats(obs.data_ptr(), obs.dtype == torch.uint8, obs.stride()[:3], rew.data_ptr(), rew.stride(), done.data_ptr(),
                            done.stride(), carry.data_ptr(), tab.data_ptr(), done.shape[0], done.shape[1], flags, stream)


def _dev(obs, rew, done, dt=torch.uint8):
    return torch.from_numpy(obs).to(DEV).to(dt), torch.from_numpy(rew).to(DEV), torch.from_numpy(done).to(DEV)


def _got(carry, tab):
    torch.cuda.synchronize()
    return tab.cpu().numpy(), carry.cpu().numpy()


@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("n", [1, 3, 5, 37, 257])
def test_kernel_equals_the_host_model(n, u8):
    """Synthetic stores that hold every kind of sample, N no multiple of the 4 envs of a workgroup (nor of 64), T around the
    10-step chunk (1, 2, 7, 20, 23), both flags, uint8 and float32: two successive calls per case, continuing carry and table,
    the first from a carry with out-of-range values. The table identities hold, and SEEN is tracking_stats' offset histogram."""
    from active_tracking_rl_amd import sight_stats, tracking_stats
    dt = torch.uint8 if u8 else torch.float32
    for steps in (1, 2, 7, 20, 23):
        for flags in (0, 1):
            start = np.resize(np.array([-1, 0, 1, 2, 3, -7, 1 << 30], np.int32), n)
            carry, tab = _fresh(n)
            carry.copy_(torch.from_numpy(start))
            want, hist = (None, start), None
            for call in range(2):
                obs, rew, done = _store(steps, n, 100 * call + 7 * n + steps)
                _launch(*_dev(obs, rew, done, dt), carry, tab, flags=flags)
                want = sight_stats.classify(obs, rew, done, carry=want[1], flags=flags, tab=want[0])
                sp.assert_equal(_got(carry, tab), want, (steps, flags, call))
                hist = tracking_stats.classify(obs, rew, done, flags=flags, hist=hist)[0]
            sp.check_identities(want[0], hist)
            assert want[0][sp.SAMPLES] == 2 * steps * n
            if steps * n >= 140:     # (the comparison was not one of empty tables)
                t = want[0]
                assert t[sp.BLOCKED:sp.BLOCKED + 169].sum() > 0 and t[sp.NOPATH:sp.NOPATH + 169].sum() > 0 and t[sp.OUT] > 0
                assert t[sp.PATH + 3:sp.PATH + 169].sum() > 0 and t[sp.DETOUR + 1:sp.TRANS].sum() > 0 and t[sp.TRANS:sp.TRANS + 9].sum() > 0
                assert t[sp.INCONSISTENT] > 0 and t[sp.SEEN + 84] > 0 and (t[sp.TERMINAL] > 0) == (flags == 0)


def test_memory_layouts():
    """Windows at all four byte alignments (a uint8 store sliced at byte offsets 0 .. 3 of a flat allocation), a strided slice of
    a larger poisoned store (every input, both dtypes), and a stacked list of per-step tensors."""
    from active_tracking_rl_amd import sight_stats
    n, steps = 37, 23
    obs, rew, done = _store(steps, n, 11)
    want = sight_stats.classify(obs, rew, done)
    d_obs, d_rew, d_done = _dev(obs, rew, done)
    for off in range(4):
        flat = torch.full((d_obs.numel() + 8,), 1, dtype=torch.uint8, device=DEV)
        view = flat[off:off + d_obs.numel()].view(d_obs.shape)
        view.copy_(d_obs)
        assert view.data_ptr() % 4 == (flat.data_ptr() + off) % 4 and flat.data_ptr() % 4 == 0
        state = _fresh(n)
        _launch(view, d_rew, d_done, *state)
        sp.assert_equal(_got(*state), want, ("byte offset", off))
    for dt in (torch.uint8, torch.float32):
        big_o = torch.full((steps + 3, n + 2, 3, 13, 13), 1, dtype=dt, device=DEV)
        big_r = torch.full((steps + 2, n + 3, 3), 1.0, dtype=torch.float32, device=DEV)
        big_d = torch.full((steps + 1, n + 4), 1, dtype=torch.uint8, device=DEV)
        v_o, v_r, v_d = big_o[1:steps + 2, 1:n + 1, 1:3], big_r[2:steps + 2, 2:n + 2, 0:2], big_d[1:steps + 1, 3:n + 3]
        v_o.copy_(d_obs.to(dt))
        v_r.copy_(d_rew)
        v_d.copy_(d_done)
        assert not v_o.is_contiguous() and not v_r.is_contiguous() and not v_d.is_contiguous()
        state = _fresh(n)
        _launch(v_o, v_r, v_d, *state, flags=1)
        sp.assert_equal(_got(*state), sight_stats.classify(obs, rew, done, flags=1), ("slice", dt))
    stacked = (torch.stack([d_obs[t].clone() for t in range(steps + 1)]), torch.stack([d_rew[t].clone() for t in range(steps)]),
               torch.stack([d_done[t].clone() for t in range(steps)]))
    state = _fresh(n)
    _launch(*stacked, *state)
    sp.assert_equal(_got(*state), want, "stacked list")


def test_split_calls_drain_and_graph_replays():
    """67 envs x 20 steps: the split 7 + 13 equals one call counter for counter; a drain between the two parts loses and doubles
    nothing (drained + rest = whole) and leaves the carry untouched; the drain hands the table out and leaves zeros; two replays
    of a captured graph (one stream, no branches) count what two host-model calls with the carry passed on count."""
    from active_tracking_rl_amd import sight_stats
    n = 67
    obs, rew, done = _store(T, n, 5)
    d_obs, d_rew, d_done = _dev(obs, rew, done)
    one = sight_stats.classify(obs, rew, done)
    whole = _fresh(n)
    _launch(d_obs, d_rew, d_done, *whole)
    sp.assert_equal(_got(*whole), one, "one call")
    split = _fresh(n)
    _launch(d_obs[:8], d_rew[:7], d_done[:7], *split)
    _launch(d_obs[7:], d_rew[7:], d_done[7:], *split)
    sp.assert_equal(_got(*split), one, "7 + 13")
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    first = sight_stats.classify(obs[:8], rew[:7], done[:7])
    drained = _fresh(n)
    out = torch.full((776,), -1, dtype=torch.int64, device=DEV)
    _launch(d_obs[:8], d_rew[:7], d_done[:7], *drained)
    sight_stats.sight_stats_drain(drained[1].data_ptr(), out.data_ptr(), stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), first[0]) and not drained[1].cpu().numpy().any()
    assert np.array_equal(drained[0].cpu().numpy(), first[1])                 # the carry is untouched
    _launch(d_obs[7:], d_rew[7:], d_done[7:], *drained)
    rest, carry = _got(*drained)
    assert np.array_equal(out.cpu().numpy() + rest, one[0]) and np.array_equal(carry, one[1])
    # a captured update, replayed twice from a fresh carry
    graphed = _fresh(n)
    side = torch.cuda.Stream(device=DEV)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        _launch(d_obs, d_rew, d_done, *graphed)
    torch.cuda.synchronize()
    assert not graphed[1].cpu().numpy().any()                 # (capturing launched nothing)
    g.replay()
    g.replay()
    two = sight_stats.classify(obs, rew, done, carry=one[1], tab=one[0])
    got = _got(*graphed)
    sp.assert_equal(got, two, "two replays")
    assert np.array_equal(got[0][:sp.TRANS], 2 * one[0][:sp.TRANS]) and got[0][sp.SAMPLES] == 2 * T * n
    assert got[0][sp.TRANS:sp.TRANS + 9].sum() > 2 * one[0][sp.TRANS:sp.TRANS + 9].sum()      # the second replay's first samples found a state


def test_hand_made_windows():
    """The hand-made windows of the CPU file as one store, one sample per env: a wall on each single line cell of every offset
    (BLOCKED), walls everywhere but the line (CLEAR), enclosed targets (NOPATH), wall-free windows (P = |dr| + |dc|), and the
    64-step corridor at the LAST env; then the corridor at the last env AND last step of a 23-step store."""
    from active_tracking_rl_amd import sight_stats
    samples = [sp.wall_on_line_cell(dr, dc, k) for dr, dc in sp.OFFSETS for k in range(len(sp.line(dr, dc)))]
    n_line = len(samples)
    samples += [sp.walls_off_the_line(dr, dc) for dr, dc in sp.OFFSETS]
    samples += [sp.enclosed(dr, dc) for dr, dc in ((2, 0), (-3, 4), (6, 6), (-6, 0), (1, 1), (0, -5))]
    samples += [sp.pair(np.zeros((13, 13), np.uint8), dr, dc) for dr, dc in sp.OFFSETS]
    long_obs, long_rew, dr, dc, P = sp.longest_window()
    samples.append((long_obs, long_rew))
    obs, rew, done = sp.store_of(samples)
    want = sight_stats.classify(obs, rew, done)
    sp.assert_equal(want, sp.loop_model(obs, rew, done)[:2], "host model against the loop")
    # every line-cell wall and the corridor block; so do the enclosures whose wall falls on the line: (2, 0), (-6, 0), (0, -5)
    assert want[0][sp.BLOCKED:sp.BLOCKED + 169].sum() == n_line + 1 + 3 and want[0][sp.PATH + P] == 1 and P == 64
    assert want[0][sp.NOPATH:sp.NOPATH + 169].sum() == 6 + (168 - 24)        # enclosed, and the off-line walls of the 144 oblique offsets
    for dt in (torch.uint8, torch.float32):
        state = _fresh(len(samples))
        _launch(*_dev(obs, rew, done, dt), *state)
        sp.assert_equal(_got(*state), want, ("hand-made", dt))
    n, steps = 5, 23
    obs, rew, done = (x.copy() for x in _store(steps, n, 3))
    obs.reshape(steps + 1, n, 2, 169)[steps, n - 1] = long_obs
    rew[steps - 1, n - 1, 0], done[steps - 1, n - 1] = long_rew, 0
    want = sight_stats.classify(obs, rew, done, flags=1)
    assert want[0][sp.PATH + P] == 1 and want[1][n - 1] == sp.BLOCKED_CLASS
    state = _fresh(n)
    _launch(*_dev(obs, rew, done), *state, flags=1)
    sp.assert_equal(_got(*state), want, "corridor at the last env and step")


def _env(env_id, n, seed=1, **kw):
    from active_tracking_rl_amd.environment import VecEnv
    return VecEnv(env_id, n, device=DEV, seed=seed, max_episode_steps=LIMIT, **kw)


def _true_class(grid, side, pos):
    """The sight class from the env's TRUE map [82, 82] and positions [2, 2], cells outside the side x side map as walls."""
    (r0, c0), (r1, c1) = pos
    dr, dc = int(r1 - r0), int(c1 - c0)
    if abs(dr) > 6 or abs(dc) > 6:
        return sp.OUT_CLASS
    for r, c in sp.line(dr, dc):
        rr, cc = int(r0) + r - 6, int(c0) + c - 6
        if not (0 <= rr < side and 0 <= cc < side) or grid[rr, cc] == 1:
            return sp.BLOCKED_CLASS
    return sp.CLEAR


@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("env_id", ["Track2D-BlockPartialPZR-v0", "Track2D-MazePartialNav-v0"])
def test_real_rollouts(env_id, auto_reset):
    """64 envs, 40 random steps written into the rollout store through VecEnv: the device table and carry equal the host
    model's. On the auto_reset=False handle the map and the positions are read back after every step: for the non-done samples
    the sight class computed from the TRUE map equals the class computed from the window — the statistic means what it says."""
    from active_tracking_rl_amd import sight_stats
    n, steps = 64, 40
    env = _env(env_id, n, seed=7, obs_u8=True, auto_reset=auto_reset)
    try:
        st = sight_stats.SightStats(env, torch.device(DEV))
        assert st.flags == (0 if auto_reset else 1) and env.sight_stats is st
        buf = env.rollout_buffers(steps)
        buf[0][0].copy_(env.reset().reshape(buf[0][0].shape))
        gen = torch.Generator(device=DEV)
        gen.manual_seed(3)
        acts = torch.randint(0, 4, (steps, 2, n), device=DEV, generator=gen)
        true = np.full((steps, n), -1, np.int32)
        for t in range(steps):
            _, _, done, _ = env.step([acts[t, 0], acts[t, 1]], out=(buf[0][t + 1], buf[1][t], buf[2][t]))
            if not auto_reset:
                state, maps = env.core.get_state(), env.core.get_maps()
                true[t] = [_true_class(maps[e], int(state["side"][e]), state["pos"][e]) for e in range(n)]
                if bool(done.any()):
                    env.core.reset(mask=done)
        st.update(buf[0], buf[1], buf[2])
        obs, rew, done = (b.cpu().numpy() for b in buf)
        want = sight_stats.classify(obs, rew, done, flags=st.flags)
        sp.assert_equal(_got(st.carry, st.tab), want, env_id)
        tab = want[0]
        sp.check_identities(tab)
        print("%s auto_reset=%s: in view %d, blocked %d, no path %d, out %d, terminal %d, transitions %s"
              % (env_id, auto_reset, tab[:169].sum(), tab[sp.BLOCKED:sp.BLOCKED + 169].sum(), tab[sp.NOPATH:sp.NOPATH + 169].sum(),
                 tab[sp.OUT], tab[sp.TERMINAL], tab[sp.TRANS:sp.TRANS + 9].tolist()))
        assert tab[sp.INCONSISTENT] == 0 and tab[sp.SAMPLES] == steps * n and tab[:169].sum() > 0
        if not auto_reset:
            classes = sp.loop_model(obs, rew, done, flags=1)[2]
            live = done == 0
            assert live.sum() > steps * n // 2 and (classes[live] >= 0).all()
            assert np.array_equal(classes[live], true[live]), np.argwhere((classes != true) & live)[:5].tolist()
            assert (true[live] == sp.BLOCKED_CLASS).any() and (true[live] == sp.CLEAR).any()
        out = st.drain()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want[0]) and not st.tab.cpu().numpy().any()
        assert np.array_equal(st.carry.cpu().numpy(), want[1])
    finally:
        env.close()


def test_attachment_rules():
    """Refused: a second object on one shard, stacked frames (no rollout store), windows that are not 13 x 13. Attaching beside
    tracking statistics works. Agent.reset() sets the carry of an attached object to -1."""
    from active_tracking_rl_amd import sight_stats, tracking_stats
    from active_tracking_rl_amd.train import default_args, make_player
    env = _env("Track2D-BlockPartialPZR-v0", 64, obs_u8=True)
    try:
        tracking_stats.TrackingStats(env, torch.device(DEV))
        st = sight_stats.SightStats(env, torch.device(DEV))
        with pytest.raises(RuntimeError, match="already has sight statistics"):
            sight_stats.SightStats(env, torch.device(DEV))
        args = default_args(env="Track2D-BlockPartialPZR-v0", num_envs=64, num_steps=T)
        args.gpu_ids = [0]
        st.carry.fill_(2)
        player, _ = make_player(args, torch.device(DEV), 0, 1, env=env)          # (make_player resets the shard)
        torch.cuda.synchronize()
        assert (st.carry.cpu().numpy() == -1).all()
        st.detach()
        assert env.sight_stats is None and env.tracking_stats is not None
    finally:
        env.close()
    for env_id, kw, text in (("Track2D-BlockPartialPZR-v0", dict(stack_frames=2), "rollout store"),
                             ("Track2D-BlockFullPZR-v0", {}, "13 x 13")):
        env = _env(env_id, 4, **kw)
        try:
            with pytest.raises(RuntimeError, match=text):
                sight_stats.SightStats(env, torch.device(DEV))
            assert getattr(env, "sight_stats", None) is None
        finally:
            env.close()


def _train(attach, tmp_path=None, n=64, iters=3):
    from active_tracking_rl_amd import sight_stats, tracking_stats
    from active_tracking_rl_amd.train import GraphedIteration, captured_learner_ok, default_args, make_player
    from active_tracking_rl_amd.utils import ScalarWriter
    assert captured_learner_ok(n, T)
    args = default_args(env="Track2D-BlockPartialPZR-v0", num_envs=n, num_steps=T, seed=2, network="tat-maze-lstm", aux="reward",
                        train_mode=-1)
    args.gpu_ids = [0]
    env = _env("Track2D-BlockPartialPZR-v0", n, seed=2, obs_u8=True)
    try:
        player, opt = make_player(args, torch.device(DEV), 0, 1, env=env)
        st = sight_stats.SightStats(env, torch.device(DEV)) if attach else None
        tr = tracking_stats.TrackingStats(env, torch.device(DEV)) if attach else None
        it = GraphedIteration(player, opt, args)
        for _ in range(iters):
            it.run()
        it.finish()
        torch.cuda.synchronize()
        bucket = (opt.bucket.flat.detach().clone(), opt.bucket.grad.detach().clone())
        if not attach:
            return bucket, None
        tab, hist = st.tab.cpu().numpy().copy(), tr.hist.cpu().numpy().copy()
        writer = ScalarWriter(os.path.join(str(tmp_path), "scalars"))
        summary = st.record(writer, 1234, 0, str(tmp_path))
        writer.close()
        return bucket, (tab, hist, summary)
    finally:
        env.close()


def test_counts_inside_the_replayed_schedule(tmp_path):
    """3 replayed iterations (after the schedule's two warm-up iterations) of 64 envs x 20 steps — the shape the tracking
    statistics' schedule test uses; train.captured_learner_ok admits it — with SightStats and TrackingStats both attached:
    SAMPLES = iterations x T x N, INCONSISTENT = 0, the SEEN segment is the tracking statistics' offset histogram, record()
    returns finite rates in [0, 1] and writes the scalars, the occlusion map and the raw table. Without the objects the same seed
    gives the same weights and the same gradient bucket, bit for bit: the hook is inert."""
    import json
    from active_tracking_rl_amd import sight_stats
    n, iters = 64, 3
    with_stats, (tab, hist, summary) = _train(True, tmp_path, n, iters)
    without, _ = _train(False, None, n, iters)
    for a, b in zip(with_stats, without):
        assert torch.isfinite(b).all() and torch.equal(a, b)
    samples = (2 + iters) * T * n
    print("samples %d, in view %d, blocked %d, no path %d, out %d, terminal %d, transitions %s, mean path %.2f"
          % (tab[sp.SAMPLES], tab[:169].sum(), summary["blocked"], summary["no_path"], tab[sp.OUT], tab[sp.TERMINAL],
             tab[sp.TRANS:sp.TRANS + 9].tolist(), summary["mean_path"]))
    assert tab[sp.SAMPLES] == samples == hist[172] and tab[sp.INCONSISTENT] == 0 and tab[sp.TERMINAL] >= n
    sp.check_identities(tab, hist)
    assert tab[:169].sum() == hist[:169].sum() > 0 and tab[sp.OUT] == hist[169] and tab[sp.TERMINAL] == hist[170]
    assert summary == sight_stats.summarize(tab) and summary["samples"] == samples
    for key in ("sight_clear_rate", "occluded_rate", "no_path_rate", "unseen_rate", "lost_to_occlusion_rate", "lost_to_range_rate",
                "reacquire_rate"):
        assert np.isfinite(summary[key]) and 0.0 <= summary[key] <= 1.0, key
    assert np.isfinite(summary["mean_path"]) and summary["mean_path"] >= 1.0 and summary["mean_detour"] >= 0.0
    heat = os.path.join(str(tmp_path), "heatmaps")
    assert os.path.getsize(os.path.join(heat, "occlusion_1234.png")) > 100
    assert np.array_equal(np.load(os.path.join(heat, "occlusion_1234.npz"))["tab"], tab)
    tags = {json.loads(ln)["tag"] for ln in open(os.path.join(str(tmp_path), "scalars", "scalars.jsonl"))}
    assert tags == set(sight_stats.TAGS)
