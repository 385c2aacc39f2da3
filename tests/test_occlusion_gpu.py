"""-m gpu: occluded observations on the device. Everything is integers (or floats that hold them), so everything is compared for
EQUALITY with tests/occlusion_spec.py: the kernel on random windows in every layout the ABI addresses, with guard bytes; the byte
windows' shared dwords under an in-place run; VecEnv(occlusion=True) against a plain twin of the same seed, observation for
observation, and the gym-protocol env on both episode sources; the rollout store and the learner on it; the store inside the replayed graphs of both schedules; the statistics on an
occluded store; and the fall-backs of the graphed evaluator and the fused GRU step, which the occluded env step rules out."""
import functools

import numpy as np
import pytest
import torch

import occlusion_spec as sp
from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PZR = "Track2D-BlockPartialPZR-v0"
RAM = "Track2D-BlockPartialRam-v0"
LIMIT = 13        # a short TimeLimit: episodes end (and auto-reset) inside a 40-step walk
POISON = 165


@functools.lru_cache(maxsize=None)
def _case(n, density, seed):
    """(windows u8 [n, 2, 13, 13], their spec) — computed once per case and shared."""
    w = sp.random_windows(2 * n, density, seed).reshape(n, 2, 13, 13)
    want = sp.occlude(w)
    w.setflags(write=False)
    want.setflags(write=False)
    return w, want


def _guarded(windows, guard, dt):
    """A poisoned device buffer with `guard` elements before and after the dense windows; (buffer, the windows' view)."""
    n = windows.size
    buf = torch.full((guard + n + guard,), POISON, dtype=dt, device=DEV)
    view = buf[guard:guard + n].view(windows.shape)
    view.copy_(torch.from_numpy(np.array(windows)).to(DEV).to(dt))
    return buf, view


def _guards_intact(buf, guard):
    return bool((buf[:guard] == POISON).all()) and bool((buf[-guard:] == POISON).all())


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("n", [1, 3, 5, 64, 257])
def test_kernel_equals_the_spec(n, u8):
    """Random windows over {0, 1, 2, 4} at wall densities 0.05, 0.15 and 0.4, as a dense [n, 2, 169] store behind 37, 38 and 39
    guard elements (byte windows: every alignment of a window's first byte occurs): out of place into a second guarded buffer
    (the source unchanged), in place (equal to out of place), guards untouched; then as a strided slice [n, 1:3] of a poisoned
    [n, 5, 169] store, of which only the addressed windows change; and with another `hidden` value."""
    from active_tracking_rl_amd import occlusion
    dt = torch.uint8 if u8 else torch.float32
    for k, density in enumerate((0.05, 0.15, 0.4)):
        guard = 37 + k
        w, want = _case(n, density, 100 + k)
        src_buf, src = _guarded(w, guard, dt)
        dst_buf = torch.full_like(src_buf, POISON)
        dst = dst_buf[guard:guard + w.size].view(w.shape)
        occlusion.occlude_windows(src.data_ptr(), dst.data_ptr(), u8, n, 2, 338, 169, 5, _stream())
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy(), want.astype(dst.cpu().numpy().dtype)), (n, density, "out of place")
        assert np.array_equal(src.cpu().numpy(), w.astype(src.cpu().numpy().dtype)) and _guards_intact(dst_buf, guard)
        assert occlusion.occlude_(src) is src
        torch.cuda.synchronize()
        assert torch.equal(src, dst) and _guards_intact(src_buf, guard), (n, density, "in place")
        # a strided slice of a larger store
        store = torch.full((n, 5, 13, 13), POISON, dtype=dt, device=DEV)
        store[:, 1:3].copy_(torch.from_numpy(np.array(w)).to(DEV).to(dt))
        occlusion.occlude_(store[:, 1:3], hidden=7)
        torch.cuda.synchronize()
        got = store.cpu().numpy()
        assert np.array_equal(got[:, 1:3], sp.occlude(w, hidden=7).astype(got.dtype)), (n, density, "slice")
        assert (got[:, 0] == POISON).all() and (got[:, 3:] == POISON).all()


def test_windows_that_share_dwords_in_place():
    """4096 dense byte windows, one byte off dword alignment, in place. In every window a wall at (5, 5) hides cell 0 and a wall at
    (7, 7) hides cell 168, so both ragged ends of every window are stored, next to the neighbouring windows' end bytes, which
    other wavefronts are storing at the same time and which hold other values. The whole buffer equals the spec."""
    from active_tracking_rl_amd import occlusion
    n = 4096
    rs = np.random.RandomState(5)
    w = sp.random_windows(n, 0.1, 6)
    w[:, 5, 5] = w[:, 7, 7] = 1
    w[:, 0, 0] = rs.choice([0, 2, 4], n)
    w[:, 12, 12] = rs.choice([0, 2, 4], n)
    w[:, 0, 1] = rs.choice([0, 2, 4], n)            # (the neighbours inside the shared dwords differ from window to window)
    w[:, 12, 11] = rs.choice([0, 2, 4], n)
    want = sp.occlude(w)
    assert (want[:, 0, 0] == 5).all() and (want[:, 12, 12] == 5).all()
    buf, view = _guarded(w, 1, torch.uint8)
    assert view.data_ptr() % 4 == 1
    occlusion.occlude_(view)
    torch.cuda.synchronize()
    assert np.array_equal(view.cpu().numpy(), want) and _guards_intact(buf, 1)


def _raw(obs):
    """[N, 2, 1, 1, 13, 13] as VecEnv hands it out (no stack, no rescale) -> numpy [N, 2, 13, 13]."""
    a = obs.cpu().numpy()
    return a.reshape(a.shape[0], 2, 13, 13)


def _rescaled(x):
    """VecEnv._stack's rescaling, with the same device operations (what is under test is that it comes AFTER the occlusion)."""
    return torch.from_numpy(x.astype(np.float32)).to(DEV).clamp(0.0, 255.0).mul(2.0).div(255.0).add(-1.0).cpu().numpy()


@pytest.mark.parametrize("env_id,u8,kw", [(PZR, True, {}), (PZR, False, {}), (RAM, True, {}),
                                          (PZR, False, dict(stack_frames=2, rescale=True))],
                         ids=["pzr-u8", "pzr-f32", "ram-u8", "pzr-stack2-rescale"])
def test_env_equals_its_plain_twin(env_id, u8, kw):
    """VecEnv(occlusion=True) and a plain VecEnv of the same seed under the same 40 random actions, 70 envs, TimeLimit 13 (every
    env auto-resets three times): rewards and done flags identical; every observation — reset(), observe(), step(), observe()
    after the last step — equals the spec of the plain twin's, in the env's own dtype; with two stacked, rescaled frames the
    raw windows are occluded first and then rescaled and stacked."""
    from active_tracking_rl_amd.environment import VecEnv
    n, steps = 70, 40
    occ = VecEnv(env_id, n, device=DEV, seed=9, obs_u8=u8, max_episode_steps=LIMIT, occlusion=True, **kw)
    plain = VecEnv(env_id, n, device=DEV, seed=9, obs_u8=u8, max_episode_steps=LIMIT)
    try:
        assert occ.occlusion and not plain.occlusion and occ.obs_u8 == plain.obs_u8 == (u8 and not kw)
        assert occ.fused_step_out(tuple(b[0] for b in plain.rollout_buffers(1))) is None
        stacked = bool(kw)
        frames = [None]

        def expect(plain_obs, done=None, fill=False, peek=False):
            cur = sp.occlude(_raw(plain_obs))
            if not stacked:
                return cur.reshape(n, 2, 1, 1, 13, 13)
            cur = _rescaled(cur)
            if peek:
                return frames[0]
            if fill:
                frames[0] = np.stack([cur, cur], 2)
            else:
                nxt = np.stack([frames[0][:, :, 1], cur], 2)
                d = done.astype(bool)
                nxt[d] = np.stack([cur, cur], 2)[d]
                frames[0] = nxt
            return frames[0].reshape(n, 2, 2, 1, 13, 13)

        def same(got, want, what):
            g = got.cpu().numpy()
            assert g.dtype == (np.uint8 if occ.obs_u8 else np.float32) and g.shape == want.reshape(g.shape).shape, what
            assert np.array_equal(g, want.reshape(g.shape).astype(g.dtype)), what

        same(occ.reset(), expect(plain.reset(), fill=True), "reset")
        same(occ.observe(), expect(plain.observe(), peek=True) if stacked else expect(plain.observe()), "observe after reset")
        gen = torch.Generator(device=DEV)
        gen.manual_seed(4)
        acts = torch.randint(0, 4, (steps, 2, n), device=DEV, generator=gen)
        ends = hidden = 0
        for t in range(steps):
            a = [acts[t, 0]] if env_id == RAM else [acts[t, 0], acts[t, 1]]
            o, r, d, _ = occ.step(a)
            p, r2, d2, _ = plain.step(a)
            assert torch.equal(r, r2) and torch.equal(d, d2), t
            want = expect(p, done=d2.cpu().numpy())
            same(o, want, "step %d" % t)
            ends += int(d.sum())
            hidden += int((sp.occlude(_raw(p)) != _raw(p)).sum())
        same(occ.observe(), expect(plain.observe(), peek=True) if stacked else expect(plain.observe()), "observe after the walk")
        assert ends >= 3 * n and hidden > 0
        assert occ.core.faults() == 0 and plain.core.faults() == 0
    finally:
        occ.close()
        plain.close()


@pytest.mark.parametrize("rng", ["philox", "numpy"])
def test_gym_protocol_env_equals_its_plain_twin(rng):
    """Track2DEnv(occlusion=True) under the reference's gym protocol, on the device generators and in the reference-exact mode
    (whose reset goes through t2d_inject and observe(), a path of its own): reset and 30 steps against a plain twin of the same
    seed — observations equal the spec of the twin's, rewards, done flags and distances are the twin's."""
    from active_tracking_rl_amd.environment import Track2DEnv
    occ = Track2DEnv("Track2D-BlockPartialNav-v0", device=DEV, seed=3, rng=rng, occlusion=True)
    plain = Track2DEnv("Track2D-BlockPartialNav-v0", device=DEV, seed=3, rng=rng)
    try:
        rs = np.random.RandomState(2)
        hidden = 0
        for episode in range(2):
            o, p = occ.reset(), plain.reset()
            assert o.dtype == p.dtype == np.float32 and o.shape == p.shape == (2, 1, 1, 13, 13)
            assert np.array_equal(o, sp.occlude(p)), (rng, episode, "reset")
            for t in range(15):
                a = rs.randint(0, 4, 2)
                o, r, d, info = occ.step(a)
                p, r2, d2, info2 = plain.step(a)
                assert np.array_equal(o, sp.occlude(p)), (rng, episode, t)
                assert np.array_equal(r, r2) and d == d2 and info["distance"] == info2["distance"]
                hidden += int((o != p).sum())
                if d:
                    break
        assert hidden > 0
    finally:
        occ.close()
        plain.close()


def _twin_store(env_id, n, seed, actions, first=None, **kw):
    """The spec of a plain env's walk under `actions` [T, 2, N]: (obs u8 [T+1, N, 2, 13, 13], rew [T, N, 2], done [T, N]). first: a
    snapshot blob (EnvSnapshot.to_bytes) of the state the walk starts from instead of the twin's own reset."""
    from active_tracking_rl_amd.environment import VecEnv
    plain = VecEnv(env_id, n, device=DEV, seed=seed, obs_u8=True, **kw)
    try:
        obs0 = plain.reset()
        if first is not None:
            plain.core.snapshot().load_bytes(first).restore()
            obs0 = plain.observe()
        obs, rew, done = [_raw(obs0)], [], []
        for t in range(actions.shape[0]):
            o, r, d, _ = plain.step([actions[t, 0].contiguous(), actions[t, 1].contiguous()])
            obs.append(_raw(o))
            rew.append(r.cpu().numpy())
            done.append(d.cpu().numpy())
        assert plain.core.faults() == 0
        return sp.occlude(np.stack(obs)), np.stack(rew), np.stack(done)
    finally:
        plain.close()


def _store_equals(player, want, what):
    obs, rew, done = (b.cpu().numpy() for b in player._buf)
    assert obs.dtype == np.uint8 and np.array_equal(obs, want[0]), what
    assert np.array_equal(rew, want[1]) and np.array_equal(done, want[2]), what
    return obs


def test_large_batch_rollout_and_learner_on_an_occluded_store():
    """1024 envs x 6 steps with occlusion=True, above cat_gemm_min_rows: the env steps in a launch of its own (as RPF ids do), so
    the cache keeps the two-GEMM form and the model never steps the env; every slot of the byte store equals the spec of a plain
    twin driven by the stored actions; the cached learner agrees with the recompute learner at the tolerances of
    test_large_batch_rollout_with_a_separate_env_step_keeps_the_two_gemm_cell."""
    from active_tracking_rl_amd.train import default_args, make_player, rollout
    from test_drivers_gpu import _check_grads
    args = default_args(env=PZR, num_envs=1024, num_steps=6, network="tat-maze-lstm", seed=7, train_mode=-1, occlusion=True)
    args.gpu_ids = [0]
    player, optimizer = make_player(args, torch.device(DEV), 0, 1)
    try:
        assert player.env.occlusion and player.env.obs_u8
        assert player.model.cat_gate_gemm and args.num_envs >= player.model.cat_gemm_min_rows
        rollout(player, args.num_steps, fast=True)
        torch.cuda.synchronize()
        assert player._cache is not None and player._cache.fh_all is None
        assert not player.model.env_stepped and not player.model.env_step_fused_seen
        want = _twin_store(PZR, 1024, args.seed, player._cache.actions)
        obs = _store_equals(player, want, "rollout store")
        assert (obs == 5).any()
        outs = []
        cache = player._cache
        for cached in (True, False):
            player._cache = cache if cached else None
            torch.manual_seed(5)
            if getattr(player.model, "_sampler", None) is not None:
                player.model._sampler.counter.zero_()
                player.model._sampler._last = None
            loss, pl, vl, ent, pred = player.loss_recompute(args.train_mode)
            player._cache = cache
            grads = torch.autograd.grad(loss, list(player.model.parameters()), allow_unused=True)
            outs.append((loss.detach(), grads))
        torch.testing.assert_close(outs[0][0], outs[1][0], rtol=1e-4, atol=1e-5)
        _check_grads(outs[0][1], outs[1][1])
        assert player.env.core.faults() == 0
    finally:
        player.env.close()


@pytest.mark.parametrize("schedule", ["synchronous", "pipelined"])
def test_the_launch_replays_inside_the_captured_schedules(schedule):
    """GraphedIteration / PipelinedIteration, 256 envs x 10 steps, three iterations with the occlusion launch inside the captured
    rollout: the bucket is finite, the env kernels flag no fault, and the store of the last replay equals the spec of its own raw
    twin — a plain env put into the state the shard had before that replay (a snapshot blob) and driven by the replay's stored
    actions."""
    from active_tracking_rl_amd.train import GraphedIteration, PipelinedIteration, default_args, make_player
    n, T = 256, 10
    args = default_args(env=PZR, num_envs=n, num_steps=T, seed=2, network="tat-maze-lstm", aux="reward", train_mode=-1,
                        occlusion=True)
    args.gpu_ids = [0]
    player, opt = make_player(args, torch.device(DEV), 0, 1)
    env = player.env
    try:
        assert env.occlusion
        it = (GraphedIteration if schedule == "synchronous" else PipelinedIteration)(player, opt, args)
        it.run()
        it.run()
        it.finish()
        torch.cuda.synchronize()
        blob = env.core.snapshot().save().to_bytes()
        it.run()
        it.finish()
        torch.cuda.synchronize()
        last = it.player if schedule == "synchronous" else it.players[(it.i - 1) & 1]
        assert torch.isfinite(opt.bucket.flat).all() and torch.isfinite(opt.bucket.grad).all()
        assert env.core.faults() == 0
        assert not last.model.env_stepped and last._cache.fh_all is None
        want = _twin_store(PZR, n, args.seed, last._cache.actions, first=blob)
        obs = _store_equals(last, want, schedule)
        assert (obs == 5).any()
    finally:
        env.close()


def test_statistics_on_an_occluded_store():
    """256 envs x 20 steps x 3 rollouts under the same random actions, occluded and plain (TimeLimit 13: TERMINAL samples occur):
    on the occluded store TrackingStats and SightStats count not one INCONSISTENT sample — a hidden target is hidden from both
    players, so it reads OUT — and their SAMPLES and TERMINAL totals equal the plain twin's; what the occluded store counts less in
    view it counts more OUT, and no more than the plain store has BLOCKED (hidden needs the near line blocked)."""
    from active_tracking_rl_amd import sight_stats, tracking_stats
    from active_tracking_rl_amd.environment import VecEnv
    n, T, rollouts = 256, 20, 3
    envs = [VecEnv(PZR, n, device=DEV, seed=3, obs_u8=True, max_episode_steps=LIMIT, occlusion=o) for o in (True, False)]
    try:
        dev = torch.device(DEV)
        stats = [(tracking_stats.TrackingStats(e, dev), sight_stats.SightStats(e, dev)) for e in envs]
        bufs = [e.rollout_buffers(T) for e in envs]
        for e, b in zip(envs, bufs):
            b[0][0].copy_(e.reset().reshape(b[0][0].shape))
        gen = torch.Generator(device=DEV)
        gen.manual_seed(8)
        for k in range(rollouts):
            acts = torch.randint(0, 4, (T, 2, n), device=DEV, generator=gen)
            for e, b, (tr, si) in zip(envs, bufs, stats):
                if k:
                    b[0][0].copy_(b[0][T])
                for t in range(T):
                    e.step([acts[t, 0], acts[t, 1]], out=(b[0][t + 1], b[1][t], b[2][t]))
                tr.update(b[0], b[1], b[2], acts.permute(0, 2, 1))
                si.update(b[0], b[1], b[2])
            assert torch.equal(bufs[0][1], bufs[1][1]) and torch.equal(bufs[0][2], bufs[1][2])
            assert np.array_equal(bufs[0][0].cpu().numpy(), sp.occlude(bufs[1][0].cpu().numpy())), k
        torch.cuda.synchronize()
        (h_o, s_o), (h_p, s_p) = [(tr.hist.cpu().numpy(), si.tab.cpu().numpy()) for tr, si in stats]
        TS, SS = tracking_stats, sight_stats
        print("occluded: in view %d, out %d | plain: in view %d, out %d, blocked %d | terminal %d, samples %d"
              % (s_o[:169].sum(), s_o[SS.OUT], s_p[:169].sum(), s_p[SS.OUT], s_p[SS.BLOCKED:SS.BLOCKED + 169].sum(), s_o[SS.TERMINAL],
                 s_o[SS.SAMPLES]))
        assert h_o[TS.INCONSISTENT] == 0 and s_o[SS.INCONSISTENT] == 0 and h_p[TS.INCONSISTENT] == 0 and s_p[SS.INCONSISTENT] == 0
        assert h_o[TS.SAMPLES] == h_p[TS.SAMPLES] == s_o[SS.SAMPLES] == s_p[SS.SAMPLES] == rollouts * T * n
        assert h_o[TS.TERMINAL] == h_p[TS.TERMINAL] == s_o[SS.TERMINAL] == s_p[SS.TERMINAL] > 0
        lost = int(s_p[:169].sum() - s_o[:169].sum())
        assert lost == s_o[SS.OUT] - s_p[SS.OUT] == h_o[TS.OUT] - h_p[TS.OUT]
        assert 0 <= lost <= s_p[SS.BLOCKED:SS.BLOCKED + 169].sum()
        assert (s_o[:169] <= s_p[:169]).all()
    finally:
        for e in envs:
            e.close()


def test_graphed_evaluation_and_the_fused_gru_step_fall_back(caplog):
    """With occlusion the env step cannot run inside the policy step's last launch: evaluator.supported is False, test.evaluate
    with graphed=True warns once and returns the eager round's finite scores, and a --fused-gru model rolls out without a cache
    (and trains)."""
    import logging
    import greedy_eval_spec as gs
    from active_tracking_rl_amd import evaluator
    from active_tracking_rl_amd.environment import VecEnv
    from active_tracking_rl_amd.test import evaluate
    from active_tracking_rl_amd.train import default_args, make_player, rollout
    nav = "Track2D-BlockPartialNav-v0"
    args = gs.fixture_args(nav, 6, occlusion=True)
    args.gpu_ids = [0]
    model = gs.fixture_model(args, DEV)
    for occ, want in ((False, True), (True, False)):
        env = VecEnv(nav, 8, device=DEV, seed=1, env_id_base=gs.EVAL_BASE, obs_u8=True, occlusion=occ)
        try:
            assert evaluator.supported(env, model) is want
        finally:
            env.close()
    with caplog.at_level(logging.WARNING):
        rsum, length = evaluate(model, nav, args, torch.device(DEV), 6, graphed=True)
    assert rsum.shape == (6, 2) and length.shape == (6,) and np.isfinite(rsum).all() and (length >= 1).all()
    assert sum("falls back to the eager round" in r.getMessage() for r in caplog.records) == 1
    gargs = default_args(env=PZR, network="tat-maze-gru", aux="reward", num_envs=64, num_steps=3, seed=23, fused_gru=True,
                         occlusion=True)
    gargs.gpu_ids = [0]
    pl, opt = make_player(gargs, torch.device(DEV))
    try:
        w0 = opt.bucket.flat.clone()
        rollout(pl, gargs.num_steps)
        assert pl.env.occlusion and pl.model.fused_gru_step and pl._cache is None and pl.model.env_step_fused_seen is False
        assert (pl._buf[0] == 5).any()
        pl.optimize(None, opt, pl.model, gargs.train_mode, torch.device(DEV))
        torch.cuda.synchronize()
        assert torch.isfinite(opt.bucket.flat).all() and not torch.equal(opt.bucket.flat, w0)
    finally:
        pl.env.close()
