"""-m gpu: sensor noise on the device. Every draw is an integer function of (key, global env id, clock, player), so everything is
compared for EQUALITY with tests/noise_spec.py: the kernel on the occluded windows of a stepped handle in every layout the ABI
addresses, with guard bytes, under ADVANCE, ADVANCE, PEEK on one clock, for every role set and the thresholds' corner cases;
VecEnv(sensor_noise=...) against a twin of the same seed and flags without it; the gym-protocol env; the slots of a byte rollout
store; clone / restore; five env steps captured in one graph and replayed; and the rollout store of the eager loop and of both
graphed schedules."""
import functools

import numpy as np
import pytest
import torch

import ego_spec
import noise_spec as sp
from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PZR = "Track2D-BlockPartialPZR-v0"
RAM = "Track2D-BlockPartialRam-v0"
NAV = "Track2D-BlockPartialNav-v0"
LIMIT = 13        # a short TimeLimit: episodes end (and auto-reset) inside a 30-step walk
POISON = 165      # (no value a window holds)
ONE = sp.ONE
KEY = sp.key_of(1)
RATES = {"flicker": .05, "miss": .1, "ghost": .5}
MID = (sp.threshold_of(.05), sp.threshold_of(.1), sp.threshold_of(.5))
THRESHOLDS = ((0, 0, 0), (ONE, 0, 0), (0, ONE, ONE), (ONE, ONE, ONE), MID)
BASE = 1000


@functools.lru_cache(maxsize=None)
def _occluded_windows(n):
    """(float32 [n, 2, 13, 13] on the host, read-only): the windows of a Block/Adv handle of n envs at env_id_base 1000 after 6
    random steps, with the occlusion pass applied, so that 5s are present. Once per n, shared."""
    from active_tracking_rl_amd import occlusion
    from active_tracking_rl_amd.vec_env import VecTrack2D
    core = VecTrack2D(num_envs=n, map_type="Block", target_mode="Adv", level=1, auto_reset=False, max_episode_steps=500,
                      device=DEV, env_id_base=BASE, seed=3)
    try:
        core.reset()
        gen = torch.Generator(device=DEV)
        gen.manual_seed(n)
        for _ in range(6):
            a = torch.randint(0, 4, (2, n), device=DEV, generator=gen)
            core.step(a[0], a[1])
        obs = core.observe().clone()
        occlusion.occlude_(obs)
        torch.cuda.synchronize()
        w = obs.cpu().numpy()
        assert core.faults() == 0
    finally:
        core.close()
    assert (w == 0).any() and (w == 1).any() and ((w == 5).any() or n < 5)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _planted_windows(n):
    """The same with 6 / 7 / 8 / 255 planted in a sixth of the cells (the centre included in some windows)."""
    rs = np.random.RandomState(70 + n)
    w = np.array(_occluded_windows(n))
    plant = rs.random_sample(w.shape) < 1 / 6
    w[plant] = rs.choice([6, 7, 8, 255], int(plant.sum()))
    w.setflags(write=False)
    return w


def _core(n, base=BASE):
    from active_tracking_rl_amd.vec_env import VecTrack2D
    core = VecTrack2D(num_envs=n, map_type="Block", target_mode="Adv", level=1, auto_reset=False, max_episode_steps=500,
                      device=DEV, env_id_base=base)
    core.reset()
    return core


def _dev(a, dt=None):
    t = torch.from_numpy(np.array(a)).to(DEV)
    return t if dt is None else t.to(dt)


def _clock_dev(clock):
    return _dev(np.asarray(clock, np.uint32).view(np.int32)).view(torch.uint32)


def _clock_host(clock):
    return clock.view(torch.int32).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, 130])
def test_kernel_equals_the_spec(n, u8):
    """The occluded windows of a stepped handle, and the same with 6 / 7 / 8 / 255 planted, on a handle at env_id_base 1000: for
    every threshold triple of the corner cases and the mid rates, and roles 1, 2, 3, three calls ADVANCE, ADVANCE, PEEK on one
    clock (started at different values per window, one of them 0xFFFFFFFF so that it wraps), each on a fresh copy of the windows
    in a dense store behind 37 .. 39 poisoned guard elements: the store and the clock equal the spec after every call, the guards
    are intact, a window whose role bit is clear is untouched and its clock too. Then the layouts: byte windows at odd addresses
    with a canary byte before and after every window, float windows with strides larger than 169 (a slice of a poisoned
    [n, 5, 13, 13] store), of which only the addressed windows change."""
    from active_tracking_rl_amd import noise
    dt = torch.uint8 if u8 else torch.float32
    npdt = np.uint8 if u8 else np.float32
    core = _core(n)
    try:
        guard = 37 + n % 3
        rs = np.random.RandomState(900 + n)
        changed = 0
        for wi, source in enumerate((_occluded_windows, _planted_windows)):
            w = source(n).astype(npdt)
            for ti, t in enumerate(THRESHOLDS):
                for roles in (1, 2, 3):
                    clock = rs.randint(0, 1000, (n, 2)).astype(np.uint32)
                    clock[0, 0] = 0xFFFFFFFF
                    dclock = _clock_dev(clock)
                    for mode in (sp.ADVANCE, sp.ADVANCE, sp.PEEK):
                        want_w, want_c = sp.apply(w, clock, KEY, t, roles, mode, env_base=BASE)
                        buf = torch.full((guard + w.size + guard,), POISON, dtype=dt, device=DEV)
                        view = buf[guard:guard + w.size].view(w.shape)
                        view.copy_(_dev(w, dt))
                        assert noise.noise_(view, dclock, core, mode, KEY, t, roles) is view
                        torch.cuda.synchronize()
                        what = (n, wi, t, roles, mode)
                        got = view.cpu().numpy()
                        assert np.array_equal(got, want_w), what
                        assert bool((buf[:guard] == POISON).all()) and bool((buf[-guard:] == POISON).all()), what
                        assert np.array_equal(_clock_host(dclock), want_c), what
                        for q in range(2):
                            if not (roles >> q) & 1:
                                assert np.array_equal(got[:, q], w[:, q]) and np.array_equal(want_c[:, q], clock[:, q]), what
                        if t == (0, 0, 0):
                            assert got.tobytes() == w.tobytes(), what
                        if mode == sp.PEEK:
                            assert np.array_equal(want_c, clock) and np.array_equal(got, prev), what
                        changed += int((got != w).sum())
                        clock, prev = want_c, got
                    assert clock[0, 0] == (1 if roles & 1 else 0xFFFFFFFF)
        assert changed > 0
        w = _planted_windows(n).astype(npdt)
        clock = np.full((n, 2), 5, np.uint32)
        want_w, want_c = sp.apply(w, clock, KEY, MID if n > 3 else (ONE, ONE, ONE), 3, sp.ADVANCE, env_base=BASE)
        t = MID if n > 3 else (ONE, ONE, ONE)
        dclock = _clock_dev(clock)
        if u8:
            # windows that start at odd addresses, a canary byte before and after each: [n, 2, 171] rows behind one odd byte
            buf = torch.full((1 + n * 2 * 171,), POISON, dtype=dt, device=DEV)
            rows = buf[1:].view(n, 2, 171)
            view = rows[:, :, 1:170].unflatten(2, (13, 13))
            assert view.stride() == (342, 171, 13, 1)          # (171 is odd: the windows start at even and at odd addresses)
            view.copy_(_dev(w, dt))
            noise.noise_(view, dclock, core, sp.ADVANCE, KEY, t, 3)
            torch.cuda.synchronize()
            rows_h = rows.cpu().numpy()
            assert np.array_equal(rows_h[:, :, 1:170].reshape(w.shape), want_w)
            assert (rows_h[:, :, 0] == POISON).all() and (rows_h[:, :, 170] == POISON).all() and int(buf[0]) == POISON
            # ... and the same one byte further on: the other parity
            buf2 = torch.full((2 + n * 2 * 171,), POISON, dtype=dt, device=DEV)
            rows2 = buf2[2:].view(n, 2, 171)
            view2 = rows2[:, :, 1:170].unflatten(2, (13, 13))
            view2.copy_(_dev(w, dt))
            noise.noise_(view2, dclock, core, sp.PEEK, KEY, t, 3)
            torch.cuda.synchronize()
            rows_h = rows2.cpu().numpy()
            assert np.array_equal(rows_h[:, :, 1:170].reshape(w.shape), want_w)
            assert (rows_h[:, :, 0] == POISON).all() and (rows_h[:, :, 170] == POISON).all() and (buf2[:2] == POISON).all()
        else:
            wide = torch.full((n, 5, 13, 13), POISON, dtype=dt, device=DEV)
            wide[:, 1:3].copy_(_dev(w, dt))
            noise.noise_(wide[:, 1:3], dclock, core, sp.ADVANCE, KEY, t, 3)
            torch.cuda.synchronize()
            got = wide.cpu().numpy()
            assert np.array_equal(got[:, 1:3], want_w) and (got[:, 0] == POISON).all() and (got[:, 3:] == POISON).all()
        assert np.array_equal(_clock_host(dclock), want_c) and (want_w != w).any()
        assert core.faults() == 0
    finally:
        core.close()


def test_shards_draw_the_same_words():
    """One handle of 8 envs at base 0 and two handles of 4 at bases 0 and 4 give the same windows."""
    from active_tracking_rl_amd import noise
    w = _planted_windows(5)
    w = np.concatenate([w, w[:3]]).astype(np.uint8)
    want, _ = sp.apply(w, np.zeros((8, 2), np.uint32), KEY, MID, 3, sp.ADVANCE, env_base=0)
    whole, lo, hi = _core(8, 0), _core(4, 0), _core(4, 4)
    try:
        a, b, c = _dev(w), _dev(w[:4]), _dev(w[4:])
        noise.noise_(a, noise.new_clock(8, DEV), whole, sp.ADVANCE, KEY, MID, 3)
        noise.noise_(b, noise.new_clock(4, DEV), lo, sp.ADVANCE, KEY, MID, 3)
        noise.noise_(c, noise.new_clock(4, DEV), hi, sp.ADVANCE, KEY, MID, 3)
        torch.cuda.synchronize()
        assert np.array_equal(a.cpu().numpy(), want) and torch.equal(a, torch.cat([b, c])) and (want != w).any()
    finally:
        for core in (whole, lo, hi):
            core.close()


def test_binding_refusals_on_the_device():
    """What the entry point refuses from the handle's state, and what noise_ refuses about its tensors."""
    from active_tracking_rl_amd import noise
    from active_tracking_rl_amd.vec_env import VecTrack2D
    core = _core(4)
    fresh = VecTrack2D(num_envs=4, map_type="Block", target_mode="Adv", level=1, device=DEV)
    full = VecTrack2D(num_envs=4, map_type="Block", target_mode="Adv", level=1, device=DEV, obs_type="Full", auto_reset=False)
    try:
        obs = torch.zeros((4, 2, 13, 13), dtype=torch.uint8, device=DEV)
        clock = noise.new_clock(4, DEV)
        noise.noise_(obs, clock, core, sp.ADVANCE, KEY, MID)
        with pytest.raises(RuntimeError, match="call t2d_reset"):
            noise.noise_(obs, clock, fresh, sp.ADVANCE, KEY, MID)
        full.reset()
        with pytest.raises(RuntimeError, match="observes the whole map"):
            noise.noise_(obs, clock, full, sp.ADVANCE, KEY, MID)
        with pytest.raises(ValueError, match="windows overlap"):
            noise.noise_(torch.zeros(169 * 4 + 8, dtype=torch.uint8, device=DEV).as_strided((4, 2, 13, 13), (169, 4, 13, 1)),
                         clock, core, sp.PEEK, KEY, MID)
        for bad in (clock[:3], clock.view(torch.int32), noise.new_clock(4, "cpu"), noise.new_clock(8, DEV)[::2],
                    torch.zeros((4, 3), dtype=torch.int32, device=DEV).view(torch.uint32)[:, :2]):
            with pytest.raises(ValueError, match="clock must be a contiguous uint32"):
                noise.noise_(obs, bad, core, sp.PEEK, KEY, MID)
        with pytest.raises(ValueError, match="mode must be"):
            noise.noise_(obs, clock, core, 2, KEY, MID)
        with pytest.raises(ValueError, match="obs holds 3 envs"):
            noise.noise_(obs[:3], clock[:3].contiguous(), core, sp.PEEK, KEY, MID)
        with pytest.raises(ValueError, match="obs must be uint8 / float32"):
            noise.noise_(obs.to(torch.int32), clock, core, sp.PEEK, KEY, MID)
        with pytest.raises(RuntimeError, match="flicker threshold 16777217 outside"):
            noise.noise_(obs, clock, core, sp.PEEK, KEY, (ONE + 1, 0, 0))
        torch.cuda.synchronize()
        assert _clock_host(clock).tolist() == [[1, 0]] * 4 and core.faults() == 0
    finally:
        for c in (core, fresh, full):
            c.close()


ON = dict(max_episode_steps=LIMIT)
STACK = dict(occlusion=True, fov=90, footprints=4, footprints_for="both", map_memory=True)
TWIN_CASES = {
    "alone": (PZR, {}, 3),
    "alone-bytes": (PZR, dict(obs_u8=True), 3),
    "occlusion": (PZR, dict(occlusion=True), 3),
    "occlusion-bytes-target-only": (PZR, dict(occlusion=True, obs_u8=True, noise_for="target"), 2),
    "stack": (PZR, dict(STACK), 3),
    "stack-bytes-tracker-only": (PZR, dict(STACK, obs_u8=True, noise_for="tracker"), 1),
    "stack-ego": (PZR, dict(STACK, egocentric=True), 3),
    "stack-ego-bytes": (PZR, dict(STACK, egocentric=True, obs_u8=True), 3),
    "scripted": (RAM, dict(occlusion=True), 1),
    "scripted-bytes-ego": (RAM, dict(occlusion=True, obs_u8=True, egocentric=True, footprints=4), 1),
}


@pytest.mark.parametrize("case", list(TWIN_CASES))
def test_env_equals_its_plain_twin(case):
    """VecEnv(sensor_noise=...) and a twin of the same id, seed and flags without it (and without the egocentric view) under the
    same 30 random actions, 6 envs, auto-reset, TimeLimit 13 (every env restarts inside the run): rewards and done flags identical;
    every observation — reset(), observe() after it, every step(), observe() after every step — equals the spec applied on the
    host to the twin's windows with the clock the spec predicts (reset: 1, step t: t + 2; the clock runs on across episodes), and
    env._noise_clock equals it. observe() repeats the step's windows and leaves the clock. Where the env is egocentric the twin
    takes the env's absolute actions and the spec's output is turned with ego_spec's map. A scripted (Ram) target's window is
    never touched, nor its clock."""
    from active_tracking_rl_amd import noise
    from active_tracking_rl_amd.environment import VecEnv
    env_id, kw, roles = TWIN_CASES[case]
    n, steps, seed = 6, 30, 9
    ego = kw.get("egocentric")
    twin_kw = {k: v for k, v in kw.items() if k not in ("egocentric", "noise_for")}
    env = VecEnv(env_id, n, device=DEV, seed=seed, sensor_noise=RATES, **kw, **ON)
    twin = VecEnv(env_id, n, device=DEV, seed=seed, **twin_kw, **ON)
    try:
        scripted = env_id == RAM
        ego_roles = 0 if not ego else 1 if scripted else 3
        assert env._noise_roles == roles and env.noise_for == {1: "tracker", 2: "target", 3: "both"}[roles]
        assert env._noise_thresholds == MID == noise.thresholds_of(RATES) and env._noise_key == sp.key_of(seed) == noise.key_of(seed)
        assert twin.sensor_noise is None and twin._noise_clock is None and env._ego_roles == ego_roles
        assert env._noise_clock.dtype == torch.uint32 and tuple(env._noise_clock.shape) == (n, 2)
        assert env.obs_u8 == twin.obs_u8 == bool(kw.get("obs_u8"))
        address = env._noise_clock.data_ptr()
        bufs = twin.rollout_buffers(1)
        assert env.fused_step_out(tuple(b[0] for b in (bufs[0][1:], bufs[1], bufs[2]))) is None
        raw = lambda o: o.cpu().numpy().reshape(n, 2, 13, 13)
        clock = [np.zeros((n, 2), np.uint32)]
        changed = [0]

        def same(got, plain, mode, what):
            want, clock[0] = sp.apply(plain, clock[0], sp.key_of(seed), MID, roles, mode, env_base=0)
            changed[0] += int((want != plain).sum())
            for q in range(2):
                if not (roles >> q) & 1:
                    assert np.array_equal(want[:, q], plain[:, q]) and not clock[0][:, q].any(), what
            if ego_roles:
                want = ego_spec.view_all(want, env._facing.cpu().numpy(), ego_roles)
            g = got.cpu().numpy()
            assert g.dtype == (np.uint8 if env.obs_u8 else np.float32) and g.shape == (n, 2, 1, 1, 13, 13), what
            assert np.array_equal(g.reshape(n, 2, 13, 13), want.astype(g.dtype)), what
            assert np.array_equal(_clock_host(env._noise_clock), clock[0]), what

        same(env.reset(), raw(twin.reset()), sp.ADVANCE, "reset")
        same(env.observe(), raw(twin.observe()), sp.PEEK, "observe after reset")
        gen = torch.Generator(device=DEV)
        gen.manual_seed(4)
        acts = torch.randint(0, 4, (steps, 2, n), device=DEV, generator=gen)
        ends = 0
        for t in range(steps):
            a = [acts[t, 0]] if scripted else [acts[t, 0], acts[t, 1]]
            o, r, d, _ = env.step(a)
            o = o.clone()
            if ego_roles:           # the twin takes the absolute moves the env made of the relative ones
                ab = env._ego_abs[torch.int64]
                a = [ab[0].clone()] if scripted else [ab[0].clone(), ab[1].clone()]
            p, r2, d2, _ = twin.step(a)
            assert torch.equal(r, r2) and torch.equal(d, d2), t
            same(o, raw(p), sp.ADVANCE, "step %d" % t)
            assert (clock[0][:, [q for q in range(2) if (roles >> q) & 1]] == t + 2).all()
            again = env.observe()
            assert torch.equal(again, o), t
            same(again, raw(twin.observe()), sp.PEEK, "observe after step %d" % t)
            ends += int(d2.sum())
        print("%s: %d episode ends in %d steps x %d envs, %d cells changed by the noise" % (case, ends, steps, n, changed[0]))
        assert changed[0] > 100 and ends >= n and env._noise_clock.data_ptr() == address
        assert env.core.faults() == 0 and twin.core.faults() == 0
    finally:
        env.close()
        twin.close()


@pytest.mark.parametrize("env_id", [PZR, NAV], ids=["pzr", "nav"])
def test_gym_protocol_env_equals_its_twin(env_id):
    """Track2DEnv(sensor_noise=...) under the reference's gym protocol with a model-driven (PZR) and a scripted (Nav) target: two
    episodes of reset and 15 steps against a twin of the same seed without the noise — observations equal the spec of the twin's,
    rewards, done flags and distances are the twin's, the clock runs on over the second reset."""
    from active_tracking_rl_amd.environment import Track2DEnv
    seed = 3
    env = Track2DEnv(env_id, device=DEV, seed=seed, occlusion=True, sensor_noise=RATES)
    twin = Track2DEnv(env_id, device=DEV, seed=seed, occlusion=True)
    try:
        roles = 3 if env_id == PZR else 1
        assert env.vec._noise_roles == roles
        rs = np.random.RandomState(2)
        clock = np.zeros((1, 2), np.uint32)
        changed = calls = 0
        for episode in range(2):
            o, p = env.reset(), twin.reset()
            assert o.dtype == p.dtype == np.float32 and o.shape == p.shape == (2, 1, 1, 13, 13)
            want, clock = sp.apply(p.reshape(1, 2, 13, 13), clock, sp.key_of(seed), MID, roles, sp.ADVANCE)
            calls += 1
            assert np.array_equal(o.reshape(1, 2, 13, 13), want), (episode, "reset")
            for t in range(15):
                a = rs.randint(0, 4, 2)
                o, r, d, info = env.step(a)
                p, r2, d2, info2 = twin.step(a)
                want, clock = sp.apply(p.reshape(1, 2, 13, 13), clock, sp.key_of(seed), MID, roles, sp.ADVANCE)
                calls += 1
                assert np.array_equal(o.reshape(1, 2, 13, 13), want), (episode, t)
                assert np.array_equal(_clock_host(env.vec._noise_clock), clock), (episode, t)
                assert np.array_equal(r, r2) and d == d2 and info["distance"] == info2["distance"]
                changed += int((o != p).sum())
                if roles == 1:
                    assert np.array_equal(o[1], p[1])
                if d:
                    break
        assert changed > 0 and clock[0, 0] == calls and clock[0, 1] == (calls if roles == 3 else 0)
    finally:
        env.close()
        twin.close()


def test_rollout_slot_bytes():
    """64 envs with obs_u8 (bytes) and the noise for both, stepping straight into the slots of a rollout store (`out=`): every slot
    equals the spec on the plain twin's."""
    from active_tracking_rl_amd.environment import VecEnv
    n, steps, seed = 64, 16, 5         # (past the TimeLimit of 13: every env restarts inside the store)
    env = VecEnv(PZR, n, device=DEV, seed=seed, obs_u8=True, sensor_noise=RATES, **ON)
    plain = VecEnv(PZR, n, device=DEV, seed=seed, obs_u8=True, **ON)
    try:
        assert env.obs_u8 and env._noise_roles == 3
        raw = lambda o: o.cpu().numpy().reshape(n, 2, 13, 13)
        store, rew, done = env.rollout_buffers(steps)
        assert store.dtype == torch.uint8
        store[0].copy_(env.reset().reshape(store[0].shape))
        w, clock = sp.apply(raw(plain.reset()), np.zeros((n, 2), np.uint32), sp.key_of(seed), MID, 3, sp.ADVANCE)
        want, plains = [w], [raw(plain.observe())]
        gen = torch.Generator(device=DEV)
        gen.manual_seed(6)
        acts = torch.randint(0, 4, (steps, 2, n), device=DEV, generator=gen)
        for t in range(steps):
            env.step([acts[t, 0], acts[t, 1]], out=(store[t + 1], rew[t], done[t]))
            p, r2, d2, _ = plain.step([acts[t, 0], acts[t, 1]])
            assert torch.equal(rew[t], r2) and torch.equal(done[t], d2)
            w, clock = sp.apply(raw(p), clock, sp.key_of(seed), MID, 3, sp.ADVANCE)
            want.append(w)
            plains.append(raw(p))
        assert np.array_equal(store.cpu().numpy(), np.stack(want)) and int(done.sum()) > 0
        assert (np.stack(want) != np.stack(plains)).sum() > 1000 and np.array_equal(_clock_host(env._noise_clock), clock)
    finally:
        env.close()
        plain.close()


def test_clone_and_restore_repeat_a_continuation():
    """10 steps, clone_state(), 12 more steps recorded (episodes end in between), restore_state(): the clock is the clone's, in the
    same tensor, and the same 12 actions give the same observations — noise included — rewards, done flags and clocks bit for bit.
    A masked restore puts back the masked envs' clocks only, and the masked envs alone repeat."""
    from active_tracking_rl_amd.environment import VecEnv
    n = 6
    env = VecEnv(PZR, n, device=DEV, seed=3, occlusion=True, sensor_noise=RATES, **ON)
    try:
        gen = torch.Generator(device=DEV)
        gen.manual_seed(11)
        acts = torch.randint(0, 4, (22, 2, n), device=DEV, generator=gen)
        i32 = lambda t: t.view(torch.int32)
        env.reset()
        for t in range(10):
            env.step([acts[t, 0], acts[t, 1]])
        state = env.clone_state()
        at_clone = i32(env._noise_clock.clone())
        address = env._noise_clock.data_ptr()
        assert (at_clone == 11).all() and state["noise_clock"] is not env._noise_clock

        def walk():
            out = []
            for t in range(10, 22):
                o, r, d, _ = env.step([acts[t, 0], acts[t, 1]])
                out.append((o.clone(), r.clone(), d.clone(), i32(env._noise_clock.clone())))
            return out
        first = walk()
        assert sum(int(x[2].sum()) for x in first) > 0 and (i32(env._noise_clock) == 23).all()
        env.restore_state(state)
        assert torch.equal(i32(env._noise_clock), at_clone) and env._noise_clock.data_ptr() == address
        for a, b in zip(first, walk()):
            assert all(torch.equal(x, y) for x, y in zip(a, b))
        mask = torch.arange(n, device=DEV) % 3 == 0
        env.restore_state(state, mask=mask)
        assert (i32(env._noise_clock)[mask] == 11).all() and (i32(env._noise_clock)[~mask] == 23).all()
        assert env._noise_clock.data_ptr() == address
        third = walk()
        for a, b in zip(first, third):
            assert all(torch.equal(x[mask], y[mask]) for x, y in zip(a, b))
        assert any(not torch.equal(a[0][~mask], b[0][~mask]) for a, b in zip(first, third))
        assert env.core.faults() == 0
    finally:
        env.close()


def test_shard_state_carries_the_clock():
    """Agent.shard_state() holds the clock as env_noise_clock and load_shard_state() puts it back in place."""
    from active_tracking_rl_amd.train import default_args, make_player, rollout

    def player():
        args = default_args(env=PZR, network="tat-maze-lstm", aux="reward", num_envs=64, num_steps=5, seed=23, noise_flicker=.05,
                            noise_ghost=.5)
        args.gpu_ids = [0]
        return make_player(args, torch.device(DEV))[0]
    P, Q = player(), player()
    try:
        assert P.env._noise_roles == 3 and P.env._noise_thresholds == (MID[0], 0, MID[2])
        rollout(P, 5)
        P.clear_actions()
        torch.cuda.synchronize()
        d = P.shard_state()
        at_save = _clock_host(P.env._noise_clock).copy()
        assert d["env_noise_clock"].dtype == torch.uint32 and not d["env_noise_clock"].is_cuda
        assert (at_save == at_save[0, 0]).all() and at_save[0, 0] >= 6          # (a reset and five steps at the least)
        rollout(P, 5)
        address = Q.env._noise_clock.data_ptr()
        Q.load_shard_state(d)
        assert Q.env._noise_clock.data_ptr() == address and np.array_equal(_clock_host(Q.env._noise_clock), at_save)
        rollout(Q, 5)
        torch.cuda.synchronize()
        for i, (x, y) in enumerate(zip(Q._buf, P._buf)):
            assert torch.equal(x, y), i
        with pytest.raises(ValueError, match="saved noise clock has shape"):
            Q.load_shard_state(dict(d, env_noise_clock=d["env_noise_clock"][:32]))
    finally:
        P.env.close()
        Q.env.close()


def test_five_steps_captured_in_one_graph_replay_with_fresh_actions():
    """Five VecEnv.step calls on static action tensors inside one torch.cuda.graph, replayed twice with fresh actions copied in:
    all ten observations, with rewards and done flags and the clock after each replay, equal the spec on a twin that takes the
    same steps eagerly. The clock lives on the device: the second replay draws other words than the first — with the first
    replay's clock its windows would not be the ones the graph wrote."""
    from active_tracking_rl_amd.environment import VecEnv
    n, T, replays, seed = 6, 5, 2, 8
    kw = dict(occlusion=True, **ON)
    env = VecEnv(PZR, n, device=DEV, seed=seed, sensor_noise=RATES, **kw)
    twin = VecEnv(PZR, n, device=DEV, seed=seed, **kw)
    try:
        raw = lambda o: o.cpu().numpy().reshape(n, 2, 13, 13)
        gen = torch.Generator(device=DEV)
        gen.manual_seed(12)
        fresh = torch.randint(0, 4, (replays + 1, T, 2, n), device=DEV, generator=gen)
        env.reset()
        twin.reset()
        clock = [np.ones((n, 2), np.uint32)]
        static = fresh[replays].clone()

        def five(e):
            out = [e.step([static[t, 0], static[t, 1]]) for t in range(T)]
            e.flush()
            return out

        def compare(got, k):
            """The twin takes the five steps one by one, `got` is compared; returns how many cells a stale clock (the one the
            pass before this one started from) would get wrong."""
            stale, off = clock[0] - np.uint32(T), 0
            for t in range(T):
                p, r2, d2, _ = twin.step([static[t, 0], static[t, 1]])
                o, r, d, _ = got[t]
                want, clock[0] = sp.apply(raw(p), clock[0], sp.key_of(seed), MID, 3, sp.ADVANCE)
                other, stale = sp.apply(raw(p), stale, sp.key_of(seed), MID, 3, sp.ADVANCE)
                assert np.array_equal(raw(o), want), (k, t)
                assert torch.equal(r, r2) and torch.equal(d, d2), (k, t)
                off += int((other != want).sum())
            twin.flush()
            assert np.array_equal(_clock_host(env._noise_clock), clock[0]), k
            return off
        compare(five(env), "eager")        # (one eager pass first: code objects are loaded before the capture)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            outs = five(env)
        for k in range(replays):
            static.copy_(fresh[k])
            g.replay()
            torch.cuda.synchronize()
            assert compare(outs, k) > 0, k
        assert (clock[0] == 1 + 3 * T).all() and env.core.faults() == 0 and twin.core.faults() == 0
        del g
    finally:
        env.close()
        twin.close()


def _twin_walk(n, seed, actions, first):
    """A plain byte env put into the state of the snapshot blob `first` and driven by `actions` [T, 2, N]:
    (raw obs u8 [T+1, N, 2, 13, 13], rew [T, N, 2], done [T, N])."""
    from active_tracking_rl_amd.environment import VecEnv
    plain = VecEnv(PZR, n, device=DEV, seed=seed, obs_u8=True)
    try:
        plain.reset()
        plain.core.snapshot().load_bytes(first).restore()
        raw = lambda o: o.cpu().numpy().reshape(n, 2, 13, 13)
        obs, rew, done = [raw(plain.observe())], [], []
        for t in range(actions.shape[0]):
            o, r, d, _ = plain.step([actions[t, 0].contiguous(), actions[t, 1].contiguous()])
            obs.append(raw(o))
            rew.append(r.cpu().numpy())
            done.append(d.cpu().numpy())
        assert plain.core.faults() == 0
        return np.stack(obs), np.stack(rew), np.stack(done)
    finally:
        plain.close()


def _store_equals_the_spec(player, n, seed, blob, clock0, what):
    """The rollout store of `player` against its own raw twin: a plain env started from the snapshot `blob`, driven by the stored
    actions, disturbed on the host from the clock the shard had before the rollout (slot 0 is a second look: PEEK)."""
    acts = player._cache.actions
    raw, rew, done = _twin_walk(n, seed, acts, blob)
    w, clock = sp.apply(raw[0], clock0, sp.key_of(seed), MID, 3, sp.PEEK)
    want = [w]
    for t in range(acts.shape[0]):
        w, clock = sp.apply(raw[t + 1], clock, sp.key_of(seed), MID, 3, sp.ADVANCE)
        want.append(w)
    obs, r, d = (b.cpu().numpy() for b in player._buf)
    assert obs.dtype == np.uint8 and np.array_equal(obs, np.stack(want)), what
    assert np.array_equal(r, rew) and np.array_equal(d, done), what
    assert np.array_equal(_clock_host(player.env._noise_clock), clock), what
    assert (np.stack(want) != raw).sum() > 1000


@pytest.mark.parametrize("schedule", ["eager", "synchronous", "pipelined"])
def test_training_stores_what_the_players_see(schedule):
    """64 envs x 5 steps, tat-maze-lstm, the three rates: two iterations of the eager loop (rollout + optimize) and of each graphed
    schedule, with the noise launch inside the captured rollout. Every window of the second iteration's rollout store equals the
    spec applied to its own raw twin — a plain env put into the state the shard had before that iteration (a snapshot blob, and the
    clock read at that moment) and driven by the iteration's stored actions; the env never takes the fused step; the bucket and
    the loss terms are finite and the env kernels flag no fault."""
    from active_tracking_rl_amd.train import GraphedIteration, PipelinedIteration, default_args, make_player, rollout
    n, T = 64, 5
    args = default_args(env=PZR, num_envs=n, num_steps=T, seed=2, network="tat-maze-lstm", aux="reward", train_mode=-1,
                        noise_flicker=RATES["flicker"], noise_miss=RATES["miss"], noise_ghost=RATES["ghost"])
    args.gpu_ids = [0]
    player, opt = make_player(args, torch.device(DEV), 0, 1)
    env = player.env
    try:
        assert env.noise_for == "both" and env._noise_roles == 3 and env.obs_u8 and env._noise_thresholds == MID

        def mark():
            torch.cuda.synchronize()
            return env.core.snapshot().save().to_bytes(), _clock_host(env._noise_clock).copy()
        if schedule == "eager":
            optimize = lambda: player.optimize(None, opt, player.model, args.train_mode, torch.device(DEV))
            rollout(player, T)
            optimize()
            blob, clock0 = mark()
            rollout(player, T)
            torch.cuda.synchronize()
            last = player
            _store_equals_the_spec(last, n, args.seed, blob, clock0, schedule)
            stats = optimize()
        else:
            it = (GraphedIteration if schedule == "synchronous" else PipelinedIteration)(player, opt, args)
            it.run()
            it.finish()
            blob, clock0 = mark()
            stats = it.run()
            it.finish()
            torch.cuda.synchronize()
            last = it.player if schedule == "synchronous" else it.players[(it.i - 1) & 1]
            _store_equals_the_spec(last, n, args.seed, blob, clock0, schedule)
        torch.cuda.synchronize()
        assert not last.model.env_stepped and not last.model.env_step_fused_seen
        assert all(bool(torch.isfinite(s).all()) for s in stats)
        assert torch.isfinite(opt.bucket.flat).all() and torch.isfinite(opt.bucket.grad).all()
        assert env.core.faults() == 0
    finally:
        env.close()
