"""-m gpu: footprints on the device. Everything is integers (or floats that hold them), so everything is compared for EQUALITY with
tests/footprints_spec.py: the kernel on crafted states in every layout the ABI addresses, with guard bytes, under every mode, role
set and a range of trail lengths; VecEnv(footprints=...) against a plain twin of the same seed with the trail tracked on the host
from the twin's positions (occlusion_spec and fov_spec first, where the env runs those passes); the gym-protocol env on both
episode sources; the slots of a byte rollout store; clone / restore; five env steps captured in one graph and replayed; and the
rollout store of the eager loop and of both graphed schedules."""
import functools
import itertools

import numpy as np
import pytest
import torch

import footprints_spec as sp
import fov_spec
import occlusion_spec
from conftest import ROOT  # noqa: F401
from test_fov_gpu import ENV_CASES, LIMIT, PZR, RAM, _HostFov

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAV = "Track2D-BlockPartialNav-v0"
POISON = 165      # (no value of footprints_spec.VALUES, and not a `value` any test passes)
SIDE = 82
E = sp.EMPTY


@functools.lru_cache(maxsize=None)
def _maps():
    """Two 82 x 82 maps: an empty one, and one with walls on about a third of its cells."""
    walls = (np.random.RandomState(5).random_sample((SIDE, SIDE)) < 0.3).astype(np.uint8)
    maps = np.stack([np.zeros((SIDE, SIDE), np.uint8), walls])
    maps.setflags(write=False)
    return maps


@functools.lru_cache(maxsize=None)
def _state(n):
    """(mazes [n, 82, 82], pos [n, 2, 2]) — env e on map e % 2; the players within 8 cells of each other, every fourth env on one
    of the map's border rows or columns so that padding is in the window; their own cells free. Once per n, shared."""
    rs = np.random.RandomState(300 + n)
    mazes = np.array(_maps()[np.arange(n) % 2])
    pos = np.zeros((n, 2, 2), np.int32)
    for e in range(n):
        pos[e, 0] = rs.randint(0, SIDE, 2)
        if e % 4 == 0:
            pos[e, 0, rs.randint(0, 2)] = (0, SIDE - 1)[rs.randint(0, 2)]
        pos[e, 1] = np.clip(pos[e, 0] + rs.randint(-8, 9, 2), 0, SIDE - 1)
        for p in range(2):
            mazes[e, pos[e, p, 0], pos[e, p, 1]] = 0
    mazes.setflags(write=False)
    pos.setflags(write=False)
    return mazes, pos


def _handle(n, action_type="VonNeumann"):
    """A handle of n envs in the crafted state, and the windows it draws of it, float32 [n, 2, 13, 13] on the host."""
    from active_tracking_rl_amd.vec_env import VecTrack2D
    mazes, pos = _state(n)
    core = VecTrack2D(num_envs=n, map_type="Block", target_mode="Adv", level=1, auto_reset=False, max_episode_steps=500,
                      device=DEV, action_type=action_type)
    core.reset()
    core.inject(mazes, pos.reshape(n, 4))
    true = core.observe().cpu().numpy()
    assert np.array_equal(core.get_state()["pos"], pos)
    return core, true


def _guarded(windows, guard, dt):
    """A poisoned device buffer with `guard` elements before and after the dense windows; (buffer, the windows' view)."""
    n = windows.size
    buf = torch.full((guard + n + guard,), POISON, dtype=dt, device=DEV)
    view = buf[guard:guard + n].view(windows.shape)
    view.copy_(torch.from_numpy(np.array(windows)).to(DEV).to(dt))
    return buf, view


def _guards_intact(buf, guard):
    return bool((buf[:guard] == POISON).all()) and bool((buf[-guard:] == POISON).all())


def _dev(a, dt=None):
    t = torch.from_numpy(np.array(a)).to(DEV)
    return t if dt is None else t.to(dt)


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 130])
def test_kernel_equals_the_spec(n, u8):
    """Crafted states through VecTrack2D.inject — an empty map and one with walls, positions on the map's border rows included —
    and, over the windows the handle draws of them, random cells over {0, 1, 2, 4, 5, 255} on half of the cells, so that "reads 0"
    meets every value at a print; random trails with EMPTY entries, duplicate cells and cells outside the window. A dense
    [n, 2, 169] store behind 37 .. 39 poisoned guard elements (byte windows: with an odd count every alignment of a window's first
    byte occurs), for K in 1, 2, 31, 63, roles 1, 2, 3 and the three modes, `value` 6 and 9, done flags given on every other
    STEP call: the store and the trail equal the spec, the guards are intact, PEEK leaves the trail byte for byte, the handle's
    fault word is 0. Then the slice [:, 1:3] of a poisoned [n, 5, 13, 13] store (env stride 845), of which only the addressed
    windows change; and on an all-zero store exactly the spec's cells changed."""
    from active_tracking_rl_amd import footprints
    dt = torch.uint8 if u8 else torch.float32
    npdt = np.uint8 if u8 else np.float32
    _, pos = _state(n)
    core, true = _handle(n)
    try:
        rs = np.random.RandomState(400 + n)
        guard = 37 + n % 3
        painted = 0
        for i, (k, roles, mode) in enumerate(itertools.product((1, 2, 31, 63), (1, 2, 3), (sp.PEEK, sp.STEP, sp.BEGIN))):
            value = 9 if i % 2 else 6
            w = np.where(rs.random_sample(true.shape) < 0.5, sp.random_windows(n, 500 + i), true).astype(npdt)
            trail = sp.random_trail(n, k, pos, 600 + i)
            done = (rs.random_sample(n) < 0.4).astype(np.uint8) * rs.choice([1, 7, 255], n).astype(np.uint8) if i % 4 < 2 else None
            want_w, want_t = sp.call(w, trail, pos, mode, done, roles, value)
            buf, view = _guarded(w, guard, dt)
            dtrail = _dev(trail)
            assert footprints.mark_(view, dtrail, core, mode, None if done is None else _dev(done), roles, value) is view
            torch.cuda.synchronize()
            what = (n, k, roles, mode)
            assert np.array_equal(view.cpu().numpy(), want_w) and _guards_intact(buf, guard), what
            assert np.array_equal(dtrail.cpu().numpy(), want_t), what
            if mode == sp.PEEK:
                assert dtrail.cpu().numpy().tobytes() == trail.tobytes(), what
            painted += int((want_w != w).sum())
        assert painted > 0
        # a slice of a larger store
        k = 31
        w = np.where(rs.random_sample(true.shape) < 0.5, sp.random_windows(n, 77), true).astype(npdt)
        trail = sp.random_trail(n, k, pos, 78)
        want_w, want_t = sp.call(w, trail, pos, sp.STEP, None, 3)
        wide = torch.full((n, 5, 13, 13), POISON, dtype=dt, device=DEV)
        wide[:, 1:3].copy_(_dev(w, dt))
        dtrail = _dev(trail)
        footprints.mark_(wide[:, 1:3], dtrail, core, sp.STEP, None, 3)
        # an all-zero store: exactly the cells the positions and the trail name
        blank = torch.zeros((n, 2, 13, 13), dtype=dt, device=DEV)
        footprints.mark_(blank, _dev(want_t), core, sp.PEEK, None, 3)
        torch.cuda.synchronize()
        got = wide.cpu().numpy()
        assert np.array_equal(got[:, 1:3], want_w) and (got[:, 0] == POISON).all() and (got[:, 3:] == POISON).all()
        assert np.array_equal(dtrail.cpu().numpy(), want_t)
        assert np.array_equal(blank.cpu().numpy() == 6, sp.paintable(want_t, pos, 3)) and (blank.cpu().numpy() % 6 == 0).all()
        assert core.faults() == 0
    finally:
        core.close()


def test_binding_refusals_on_the_device():
    """What the entry point refuses from the handle's state, and what mark_ refuses about its tensors."""
    from active_tracking_rl_amd import footprints
    from active_tracking_rl_amd.vec_env import VecTrack2D
    core, _ = _handle(4, action_type="Moore")           # (a Moore handle is fine: the rule never looks at an action)
    fresh = VecTrack2D(num_envs=4, map_type="Block", target_mode="Adv", level=1, device=DEV)
    full = VecTrack2D(num_envs=4, map_type="Block", target_mode="Adv", level=1, device=DEV, obs_type="Full", auto_reset=False)
    try:
        obs = torch.zeros((4, 2, 13, 13), dtype=torch.uint8, device=DEV)
        trail = footprints.new_trail(4, 4, DEV)
        footprints.mark_(obs, trail, core, sp.BEGIN)
        with pytest.raises(RuntimeError, match="call t2d_reset"):
            footprints.mark_(obs, trail, fresh, sp.BEGIN)
        full.reset()
        with pytest.raises(RuntimeError, match="observes the whole map"):
            footprints.mark_(obs, trail, full, sp.BEGIN)
        with pytest.raises(ValueError, match="windows overlap"):
            footprints.mark_(torch.zeros(169 * 4 + 8, dtype=torch.uint8, device=DEV).as_strided((4, 2, 13, 13), (169, 4, 13, 1)),
                             trail, core, sp.PEEK)
        for bad in (trail[:3], trail.view(torch.int16), trail[:, :, :1], footprints.new_trail(4, 4, "cpu"),
                    footprints.new_trail(8, 4, DEV)[::2]):
            with pytest.raises(ValueError, match="trail must be a contiguous uint16"):
                footprints.mark_(obs, bad, core, sp.PEEK)
        with pytest.raises(ValueError, match="done must be a contiguous uint8"):
            footprints.mark_(obs, trail, core, sp.STEP, torch.zeros(5, dtype=torch.uint8, device=DEV))
        with pytest.raises(ValueError, match="mode must be"):
            footprints.mark_(obs, trail, core, 3)
        with pytest.raises(ValueError, match="obs holds 3 envs"):
            footprints.mark_(obs[:3], trail[:3].contiguous(), core, sp.PEEK)
        torch.cuda.synchronize()
        assert core.faults() == 0
    finally:
        for c in (core, fresh, full):
            c.close()


class _HostPrints(object):
    """What VecEnv(footprints=K) must hand out, from a plain twin's observations and positions: the trail tracked on the host
    (footprints_spec.record), after occlusion_spec and fov_spec where the env runs those passes."""

    def __init__(self, n, k, roles, fov=None, occlusion=False, auto_reset=True, scripted=False):
        self.n, self.k, self.occlusion, self.auto_reset = n, k, occlusion, auto_reset
        self.roles = 1 if scripted else roles
        self.fov = _HostFov(n, fov, auto_reset=auto_reset, scripted=scripted) if fov is not None else None
        self.trail = sp.new_trail(n, k)
        self.hidden_prints = 0

    def reset(self):
        if self.fov is not None:
            self.fov.reset()

    def see(self, raw, pos, mode, actions=None, done=None):
        """raw [N, 2, 13, 13] and pos [N, 2, 2] of the plain twin -> the windows."""
        w = raw
        if self.occlusion:
            w = occlusion_spec.occlude(w)
        if self.fov is not None:
            w = self.fov.see(w, actions, done)
        self.trail = sp.record(self.trail, pos, mode, done if self.auto_reset else None)
        can = sp.paintable(self.trail, pos, self.roles)
        self.hidden_prints += int((can & (w == 5)).sum())
        return sp.paint(w, self.trail, pos, self.roles)


TWIN_CASES = dict(ENV_CASES)
TWIN_CASES["pzr-occlusion-fov90"] = (PZR, dict(obs_u8=True, occlusion=True, fov=90), dict(max_episode_steps=LIMIT))
TWIN_CASES["pzr-moore"] = (PZR, dict(action_type="Moore"), dict(max_episode_steps=LIMIT))
del TWIN_CASES["pzr-own-limit"]       # (a case of the field-of-view tests' own: the id's TimeLimit ends few episodes in 40 steps)


@pytest.mark.parametrize("case", list(TWIN_CASES))
def test_env_equals_its_plain_twin(case):
    """VecEnv(footprints=4, footprints_for="both") and a plain VecEnv of the same id and seed under the same 40 random actions, 65
    envs, TimeLimit 13: rewards and done flags identical; every observation — reset(), observe() after it, every step(),
    observe() after the last step — equals the spec applied on the host to the plain twin's windows with the twin's positions
    (get_state() after every call), and env._trail equals the host's after every step. Without the auto-reset no done flag reaches
    the pass, and a reset() half way starts every trail afresh. With occlusion (and fov=90) the plain windows go through
    occlusion_spec (and fov_spec) first: prints on cells that read 5 stay hidden, and some do. A scripted (Ram) target's window
    is never painted (the env is created with footprints_for="tracker": "both" is refused there). A Moore handle takes actions
    in 0 .. 7."""
    from active_tracking_rl_amd.environment import VecEnv
    env_id, kw, both = TWIN_CASES[case]
    n, steps, k = 65, 40, 4
    plain_kw = {key: v for key, v in kw.items() if key not in ("occlusion", "fov")}
    who = "tracker" if env_id == RAM else "both"
    env = VecEnv(env_id, n, device=DEV, seed=9, footprints=k, footprints_for=who, **kw, **both)
    plain = VecEnv(env_id, n, device=DEV, seed=9, **plain_kw, **both)
    try:
        assert env.footprints == k and plain.footprints is None and plain._trail is None
        assert env._trail.shape == (n, 2, k + 1) and env._trail.dtype == torch.uint16 and (env._trail.cpu().numpy() == E).all()
        bufs = plain.rollout_buffers(1)
        if bufs is not None:
            assert env.fused_step_out(tuple(b[0] for b in (bufs[0][1:], bufs[1], bufs[2]))) is None
        auto = kw.get("auto_reset", True)
        fov = (kw["fov"], kw["fov"]) if "fov" in kw else None
        host = _HostPrints(n, k, 3, fov=fov, occlusion=kw.get("occlusion", False), auto_reset=auto, scripted=env_id == RAM)
        stack = kw.get("stack_frames", 1)
        frames = [None]

        def expect(windows, done=None, fill=False, peek=False):
            cur = windows.astype(np.float32)
            if stack == 1:
                return cur.reshape(n, 2, 1, 1, 13, 13)
            if fill:
                frames[0] = np.stack([cur, cur], 2)
            elif not peek:
                nxt = np.stack([frames[0][:, :, 1], cur], 2)
                d = done.astype(bool)
                nxt[d] = np.stack([cur, cur], 2)[d]
                frames[0] = nxt
            return frames[0].reshape(n, 2, 2, 1, 13, 13)

        def same(got, want, what):
            g = got.cpu().numpy()
            assert g.dtype == (np.uint8 if env.obs_u8 else np.float32) and g.shape == want.shape, what
            assert np.array_equal(g, want.astype(g.dtype)), what

        def plain_windows(obs):
            a = obs.cpu().numpy()
            return a.reshape(n, 2, stack, 13, 13)[:, :, -1]

        where = lambda: plain.core.get_state()["pos"]
        same(env.reset(), expect(host.see(plain_windows(plain.reset()), where(), sp.BEGIN), fill=True), "reset")
        same(env.observe(), expect(host.see(plain_windows(plain.observe()), where(), sp.PEEK), peek=True), "observe after reset")
        gen = torch.Generator(device=DEV)
        gen.manual_seed(4)
        acts = torch.randint(0, 8 if case == "pzr-moore" else 4, (steps, 2, n), device=DEV, generator=gen)
        acts_h = acts.cpu().numpy()
        ends = painted = 0
        for t in range(steps):
            if not auto and t == steps // 2:
                host.reset()
                same(env.reset(), expect(host.see(plain_windows(plain.reset()), where(), sp.BEGIN), fill=True), "reset half way")
            a = [acts[t, 0]] if env_id == RAM else [acts[t, 0], acts[t, 1]]
            o, r, d, _ = env.step(a)
            p, r2, d2, _ = plain.step(a)
            assert torch.equal(r, r2) and torch.equal(d, d2), t
            dh = d2.cpu().numpy()
            raw = plain_windows(p)
            seen = host.see(raw, where(), sp.STEP, (acts_h[t, 0], acts_h[t, 1]), dh)
            same(o, expect(seen, done=dh), "step %d" % t)
            assert np.array_equal(env._trail.cpu().numpy(), host.trail), t
            ends += int(dh.astype(bool).sum())
            painted += int((seen == 6).sum())
            if env_id == RAM:
                assert not (seen[:, 1] == 6).any()
        before = env._trail.clone().view(torch.int16)
        same(env.observe(), expect(host.see(plain_windows(plain.observe()), where(), sp.PEEK), peek=True), "observe after the walk")
        assert torch.equal(env._trail.view(torch.int16), before)
        print("%s: %d episode ends in %d steps x %d envs, %d cells painted, %d prints hidden under a 5"
              % (case, ends, steps, n, painted, host.hidden_prints))
        assert painted > 0 and ends >= (3 * n if auto else n)
        if kw.get("occlusion") or "fov" in kw:
            assert host.hidden_prints > 0
        assert env.core.faults() == 0 and plain.core.faults() == 0
    finally:
        env.close()
        plain.close()


@pytest.mark.parametrize("rng", ["philox", "numpy"])
@pytest.mark.parametrize("env_id", [PZR, NAV], ids=["pzr", "nav"])
def test_gym_protocol_env_equals_its_plain_twin(env_id, rng):
    """Track2DEnv(footprints=4) under the reference's gym protocol, on the device generators and in the reference-exact mode
    (whose reset goes through t2d_inject and observe(), a path of its own), with a model-driven and with a scripted (Nav) target:
    two episodes of reset and 15 steps against a plain twin of the same seed — observations equal the spec of the twin's,
    rewards, done flags and distances are the twin's, every reset starts with no prints."""
    from active_tracking_rl_amd.environment import Track2DEnv
    who = "both" if env_id == PZR else "tracker"
    env = Track2DEnv(env_id, device=DEV, seed=3, rng=rng, footprints=4, footprints_for=who)
    plain = Track2DEnv(env_id, device=DEV, seed=3, rng=rng)
    try:
        host = _HostPrints(1, 4, 3, auto_reset=False, scripted=env_id != PZR)
        where = lambda: plain.vec.core.get_state()["pos"]
        rs = np.random.RandomState(2)
        painted = 0
        for episode in range(2):
            o, p = env.reset(), plain.reset()
            assert o.dtype == p.dtype == np.float32 and o.shape == p.shape == (2, 1, 1, 13, 13)
            assert np.array_equal(o.reshape(1, 2, 13, 13), host.see(p.reshape(1, 2, 13, 13), where(), sp.BEGIN)), (episode, "reset")
            assert np.array_equal(o, p) and (env.vec._trail.cpu().numpy()[0, :, 1:] == E).all()
            for t in range(15):
                a = rs.randint(0, 4, 2)
                o, r, d, info = env.step(a)
                p, r2, d2, info2 = plain.step(a)
                want = host.see(p.reshape(1, 2, 13, 13), where(), sp.STEP)
                assert np.array_equal(o.reshape(1, 2, 13, 13), want), (episode, t)
                assert np.array_equal(env.vec._trail.cpu().numpy(), host.trail), (episode, t)
                assert np.array_equal(r, r2) and d == d2 and info["distance"] == info2["distance"]
                painted += int((o != p).sum())
                if d:
                    break
        assert painted > 0
    finally:
        env.close()
        plain.close()


def test_rollout_slot_bytes():
    """64 envs with obs_u8 (bytes) and footprints=4 for both, stepping straight into the slots of a rollout store (`out=`): every
    slot equals the spec on the plain twin's."""
    from active_tracking_rl_amd.environment import VecEnv
    n, steps = 64, 16         # (past the TimeLimit of 13: every env restarts inside the store)
    env = VecEnv(PZR, n, device=DEV, seed=5, obs_u8=True, max_episode_steps=LIMIT, footprints=4, footprints_for="both")
    plain = VecEnv(PZR, n, device=DEV, seed=5, obs_u8=True, max_episode_steps=LIMIT)
    try:
        assert env.obs_u8
        host = _HostPrints(n, 4, 3)
        raw = lambda o: o.cpu().numpy().reshape(n, 2, 13, 13)
        where = lambda: plain.core.get_state()["pos"]
        store, rew, done = env.rollout_buffers(steps)
        assert store.dtype == torch.uint8
        store[0].copy_(env.reset().reshape(store[0].shape))
        want = [host.see(raw(plain.reset()), where(), sp.BEGIN)]
        gen = torch.Generator(device=DEV)
        gen.manual_seed(6)
        acts = torch.randint(0, 4, (steps, 2, n), device=DEV, generator=gen)
        for t in range(steps):
            env.step([acts[t, 0], acts[t, 1]], out=(store[t + 1], rew[t], done[t]))
            p, r2, d2, _ = plain.step([acts[t, 0], acts[t, 1]])
            assert torch.equal(rew[t], r2) and torch.equal(done[t], d2)
            want.append(host.see(raw(p), where(), sp.STEP, None, d2.cpu().numpy()))
        assert np.array_equal(store.cpu().numpy(), np.stack(want)) and (store == 6).any() and int(done.sum()) > 0
        assert np.array_equal(env._trail.cpu().numpy(), host.trail)
    finally:
        env.close()
        plain.close()


def test_clone_and_restore_repeat_a_continuation():
    """10 steps, clone_state(), 12 more steps recorded (episodes end in between), restore_state(): the trail is the clone's, and
    the same 12 actions give the same observations, rewards, done flags and trails bit for bit. A masked restore puts back the
    masked envs' rows only."""
    from active_tracking_rl_amd.environment import VecEnv
    n = 65
    env = VecEnv(PZR, n, device=DEV, seed=3, max_episode_steps=LIMIT, footprints=4, footprints_for="both")
    try:
        gen = torch.Generator(device=DEV)
        gen.manual_seed(11)
        acts = torch.randint(0, 4, (22, 2, n), device=DEV, generator=gen)
        i16 = lambda t: t.view(torch.int16)
        env.reset()
        for t in range(10):
            env.step([acts[t, 0], acts[t, 1]])
        state = env.clone_state()
        at_clone = i16(env._trail.clone())
        address = env._trail.data_ptr()
        assert (at_clone[:, :, 1:] != -1).any() and state["trail"] is not env._trail

        def walk():
            out = []
            for t in range(10, 22):
                o, r, d, _ = env.step([acts[t, 0], acts[t, 1]])
                out.append((o.clone(), r.clone(), d.clone(), i16(env._trail.clone())))
            return out
        first = walk()
        assert sum(int(x[2].sum()) for x in first) > 0 and not torch.equal(i16(env._trail), at_clone)
        env.restore_state(state)
        assert torch.equal(i16(env._trail), at_clone) and env._trail.data_ptr() == address
        for a, b in zip(first, walk()):
            assert all(torch.equal(x, y) for x, y in zip(a, b))
        moved = i16(env._trail.clone())
        mask = torch.arange(n, device=DEV) % 3 == 0
        env.restore_state(state, mask=mask)
        assert torch.equal(i16(env._trail)[mask], at_clone[mask]) and torch.equal(i16(env._trail)[~mask], moved[~mask])
        assert not torch.equal(at_clone[~mask], moved[~mask]) and env._trail.data_ptr() == address
        assert env.core.faults() == 0
    finally:
        env.close()


def test_five_steps_captured_in_one_graph_replay_with_fresh_actions():
    """Five VecEnv.step calls on static action tensors inside one torch.cuda.graph, replayed three times with fresh actions
    copied in: all fifteen observations, with rewards, done flags and the trail after each replay, equal the spec on a plain twin
    that takes the same fifteen steps eagerly. The trail is state the replays carry."""
    from active_tracking_rl_amd.environment import VecEnv
    n, T, replays = 65, 5, 3
    env = VecEnv(PZR, n, device=DEV, seed=8, max_episode_steps=LIMIT, footprints=4, footprints_for="both")
    plain = VecEnv(PZR, n, device=DEV, seed=8, max_episode_steps=LIMIT)
    try:
        host = _HostPrints(n, 4, 3)
        raw = lambda o: o.cpu().numpy().reshape(n, 2, 13, 13)
        where = lambda: plain.core.get_state()["pos"]
        gen = torch.Generator(device=DEV)
        gen.manual_seed(12)
        fresh = torch.randint(0, 4, (replays + 1, T, 2, n), device=DEV, generator=gen)
        env.reset()
        host.see(raw(plain.reset()), where(), sp.BEGIN)
        static = fresh[replays].clone()

        def five(e):
            out = [e.step([static[t, 0], static[t, 1]]) for t in range(T)]
            e.flush()
            return out

        def compare(got, k):
            """The plain twin takes the five steps one by one (its positions are read after each), `got` is compared."""
            ends = 0
            for t in range(T):
                p, r2, d2, _ = plain.step([static[t, 0], static[t, 1]])
                dh = d2.cpu().numpy()
                o, r, d, _ = got[t]
                assert np.array_equal(raw(o), host.see(raw(p), where(), sp.STEP, None, dh)), (k, t)
                assert torch.equal(r, r2) and torch.equal(d, d2), (k, t)
                ends += int(dh.astype(bool).sum())
            plain.flush()
            assert np.array_equal(env._trail.cpu().numpy(), host.trail), k
            return ends
        compare(five(env), "eager")        # (one eager pass first: code objects are loaded before the capture)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            outs = five(env)
        ends = 0
        for k in range(replays):
            static.copy_(fresh[k])
            g.replay()
            torch.cuda.synchronize()
            ends += compare(outs, k)
        assert ends > 0 and env.core.faults() == 0 and plain.core.faults() == 0
        del g
    finally:
        env.close()
        plain.close()


def _twin_walk(n, seed, actions, first):
    """A plain byte env put into the state of the snapshot blob `first` and driven by `actions` [T, 2, N]:
    (raw obs u8 [T+1, N, 2, 13, 13], pos [T+1, N, 2, 2], rew [T, N, 2], done [T, N])."""
    from active_tracking_rl_amd.environment import VecEnv
    plain = VecEnv(PZR, n, device=DEV, seed=seed, obs_u8=True)
    try:
        plain.reset()
        plain.core.snapshot().load_bytes(first).restore()
        raw = lambda o: o.cpu().numpy().reshape(n, 2, 13, 13)
        obs, pos, rew, done = [raw(plain.observe())], [plain.core.get_state()["pos"]], [], []
        for t in range(actions.shape[0]):
            o, r, d, _ = plain.step([actions[t, 0].contiguous(), actions[t, 1].contiguous()])
            obs.append(raw(o))
            pos.append(plain.core.get_state()["pos"])
            rew.append(r.cpu().numpy())
            done.append(d.cpu().numpy())
        assert plain.core.faults() == 0
        return np.stack(obs), np.stack(pos), np.stack(rew), np.stack(done)
    finally:
        plain.close()


def _store_equals_the_spec(player, n, seed, blob, trail0, what):
    """The rollout store of `player` against its own raw twin: a plain env started from the snapshot `blob`, driven by the stored
    actions, painted on the host from the trail the shard had before the rollout."""
    acts = player._cache.actions
    raw, pos, rew, done = _twin_walk(n, seed, acts, blob)
    host = _HostPrints(n, 4, 1)
    host.trail = np.array(trail0)
    want = [host.see(raw[0], pos[0], sp.PEEK)]
    for t in range(acts.shape[0]):
        want.append(host.see(raw[t + 1], pos[t + 1], sp.STEP, None, done[t]))
    obs, r, d = (b.cpu().numpy() for b in player._buf)
    assert obs.dtype == np.uint8 and np.array_equal(obs, np.stack(want)), what
    assert np.array_equal(r, rew) and np.array_equal(d, done), what
    assert np.array_equal(player.env._trail.cpu().numpy(), host.trail), what
    assert (obs == 6).any() and not (obs[:, :, 1] == 6).any() and (np.stack(want) != raw).any()


@pytest.mark.parametrize("schedule", ["eager", "synchronous", "pipelined"])
def test_training_stores_what_the_players_see(schedule):
    """64 envs x 5 steps, tat-maze-lstm, footprints=4 (for the tracker): two iterations of the eager loop (rollout + optimize) and
    of each graphed schedule, with the footprint launch inside the captured rollout. Every window of the second iteration's
    rollout store equals the spec applied to its own raw twin — a plain env put into the state the shard had before that iteration
    (a snapshot blob, and the trail read at that moment) and driven by the iteration's stored actions; the env never takes the
    fused step; the bucket and the loss terms are finite and the env kernels flag no fault."""
    from active_tracking_rl_amd.train import GraphedIteration, PipelinedIteration, default_args, make_player, rollout
    n, T = 64, 5
    args = default_args(env=PZR, num_envs=n, num_steps=T, seed=2, network="tat-maze-lstm", aux="reward", train_mode=-1, footprints=4)
    args.gpu_ids = [0]
    player, opt = make_player(args, torch.device(DEV), 0, 1)
    env = player.env
    try:
        assert env.footprints == 4 and env._footprint_roles == 1 and env.obs_u8

        def mark():
            torch.cuda.synchronize()
            return env.core.snapshot().save().to_bytes(), env._trail.cpu().numpy()
        if schedule == "eager":
            optimize = lambda: player.optimize(None, opt, player.model, args.train_mode, torch.device(DEV))
            rollout(player, T)
            optimize()
            blob, trail0 = mark()
            rollout(player, T)
            torch.cuda.synchronize()
            last = player
            _store_equals_the_spec(last, n, args.seed, blob, trail0, schedule)
            stats = optimize()
        else:
            it = (GraphedIteration if schedule == "synchronous" else PipelinedIteration)(player, opt, args)
            it.run()
            it.finish()
            blob, trail0 = mark()
            stats = it.run()
            it.finish()
            torch.cuda.synchronize()
            last = it.player if schedule == "synchronous" else it.players[(it.i - 1) & 1]
            _store_equals_the_spec(last, n, args.seed, blob, trail0, schedule)
        torch.cuda.synchronize()
        assert not last.model.env_stepped and not last.model.env_step_fused_seen
        assert all(bool(torch.isfinite(s).all()) for s in stats)
        assert torch.isfinite(opt.bucket.flat).all() and torch.isfinite(opt.bucket.grad).all()
        assert env.core.faults() == 0
    finally:
        env.close()
