"""-m gpu: facing and field of view on the device. Everything is integers (or floats that hold them), so everything is compared for
EQUALITY with tests/fov_spec.py: the kernel on random windows in every layout the ABI addresses, with guard bytes, under every
facing, aperture pair and near radius; the turn rule under the three action dtypes; VecEnv(fov=...) against a plain twin of the
same seed with the facing tracked on the host, and the gym-protocol env on both episode sources; five env steps captured in one graph and replayed; and the rollout store of the
eager loop and of both graphed schedules."""
import functools
import itertools

import numpy as np
import pytest
import torch

import fov_spec as sp
import occlusion_spec
from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PZR = "Track2D-BlockPartialPZR-v0"
RAM = "Track2D-BlockPartialRam-v0"
LIMIT = 13        # a short TimeLimit: episodes end (and auto-reset) inside a 40-step walk
POISON = 165      # (no value of fov_spec.VALUES, and not a `hidden` any test passes)
PAIRS = tuple(itertools.product(sp.APERTURES, repeat=2))


@functools.lru_cache(maxsize=None)
def _case(n):
    """(windows u8 [n, 2, 13, 13] over {0, 1, 2, 4, 5, 255}, facings u8 [n, 2] over {0, 1, 2, 3, NONE}) — once per n, shared."""
    w = sp.random_windows(n, 2, 100 + n)
    f = np.array(sp.FACINGS, np.uint8)[np.random.RandomState(200 + n).randint(0, 5, (n, 2))]
    f.reshape(-1)[:5] = sp.FACINGS[:f.size]     # (from three envs up every facing occurs, whatever n draws)
    w.setflags(write=False)
    f.setflags(write=False)
    return w, f


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


def _dev(a, dt=None):
    t = torch.from_numpy(np.array(a)).to(DEV)
    return t if dt is None else t.to(dt)


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 130])
def test_kernel_equals_the_spec(n, u8):
    """Random windows over {0, 1, 2, 4, 5, 255} and random facings (NONE included) as a dense [n, 2, 169] store behind 37 .. 39
    guard elements (byte windows: with an odd count every alignment of a window's first byte occurs), for all 16 aperture pairs
    and near 0, 1, 6, without actions and done flags (nobody turns): in place the store equals the spec — a player of aperture 360
    keeps its window byte for byte — and the guards and facings are untouched; src -> dst into a poisoned buffer every window of a
    restricted player equals the spec, a 360 player's window of dst is still poison, and src is unchanged. Then in place on an
    all-poison store: exactly the hidden cells were stored, every other cell is still poison."""
    from active_tracking_rl_amd import fov
    dt = torch.uint8 if u8 else torch.float32
    npdt = np.uint8 if u8 else np.float32
    w, f = _case(n)
    guard = 37 + n % 3
    facing = _dev(f)
    for k, ((ap0, ap1), near) in enumerate(itertools.product(PAIRS, (0, 1, 6))):
        hidden = 5 if k % 4 else 9
        want = sp.restrict(w, f, (ap0, ap1), near, hidden).astype(npdt)
        buf, view = _guarded(w, guard, dt)
        assert fov.restrict_(view, facing, apertures=(ap0, ap1), near=near, hidden=hidden) is view
        dst_buf = torch.full_like(buf, POISON)
        dst = dst_buf[guard:guard + w.size].view(w.shape)
        src_buf, src = _guarded(w, guard, dt)
        fov.fov_windows(src.data_ptr(), dst.data_ptr(), u8, n, 2, 338, 169, facing.data_ptr(), None, None, 0, None, ap0, ap1, near,
                        hidden, _stream())
        torch.cuda.synchronize()
        what = (n, ap0, ap1, near)
        assert np.array_equal(view.cpu().numpy(), want) and _guards_intact(buf, guard), what + ("in place",)
        got = dst.cpu().numpy()
        for p, ap in enumerate((ap0, ap1)):
            if ap == 360:
                assert (got[:, p] == POISON).all() and np.array_equal(want[:, p], w[:, p].astype(npdt)), what + ("360", p)
            else:
                assert np.array_equal(got[:, p], want[:, p]), what + ("out of place", p)
        assert _guards_intact(dst_buf, guard) and np.array_equal(src.cpu().numpy(), w.astype(npdt)) and _guards_intact(src_buf, guard)
        assert np.array_equal(facing.cpu().numpy(), f), what
    # in place stores the hidden cells and nothing else
    blank = torch.full((n, 2, 13, 13), POISON, dtype=dt, device=DEV)
    fov.restrict_(blank, facing, apertures=(90, 270), near=1)
    torch.cuda.synchronize()
    assert np.array_equal(blank.cpu().numpy(), sp.restrict(np.full((n, 2, 13, 13), POISON, npdt), f, (90, 270), 1))


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("n", [3, 65])
def test_strided_stores(n, u8):
    """Slot 1 of a poisoned [3, n, 2, 13, 13] rollout store (byte slots of an odd n start off dword alignment), of which only that
    slot changes; the slice [n, 1:3] of a poisoned [n, 5, 13, 13] store (an env stride of five windows), of which only the
    addressed windows change; and player 0 alone as [n, 0:1] of a dense store with a facing tensor [n, 1]."""
    from active_tracking_rl_amd import fov
    dt = torch.uint8 if u8 else torch.float32
    w, f = _case(n)
    facing = _dev(f)
    want = sp.restrict(w, f, (90, 180), 1)
    store = torch.full((3, n, 2, 13, 13), POISON, dtype=dt, device=DEV)
    store[1].copy_(_dev(w, dt))
    fov.restrict_(store[1], facing, apertures=(90, 180))
    wide = torch.full((n, 5, 13, 13), POISON, dtype=dt, device=DEV)
    wide[:, 1:3].copy_(_dev(w, dt))
    fov.restrict_(wide[:, 1:3], facing, apertures=(90, 180))
    solo = _dev(w, dt)
    facing0 = _dev(np.ascontiguousarray(f[:, :1]))
    fov.restrict_(solo[:, 0:1], facing0, apertures=(270, 90), near=0)
    torch.cuda.synchronize()
    got = store.cpu().numpy()
    assert np.array_equal(got[1], want.astype(got.dtype)) and (got[0] == POISON).all() and (got[2] == POISON).all()
    got = wide.cpu().numpy()
    assert np.array_equal(got[:, 1:3], want.astype(got.dtype)) and (got[:, 0] == POISON).all() and (got[:, 3:] == POISON).all()
    got = solo.cpu().numpy()
    assert np.array_equal(got[:, :1], sp.restrict(w[:, :1], f[:, :1], (270,), 0).astype(got.dtype))
    assert np.array_equal(got[:, 1], w[:, 1].astype(got.dtype))
    with pytest.raises(ValueError, match="windows overlap"):
        fov.restrict_(torch.zeros(169 * 4 + 8, dtype=dt, device=DEV).as_strided((4, 2, 13, 13), (169, 4, 13, 1)), facing[:4].contiguous())


@pytest.mark.parametrize("dt", [torch.uint8, torch.int32, torch.int64], ids=["u8", "i32", "i64"])
def test_turn_rule(dt):
    """65 envs x 2 players, four calls in a row on one facing tensor, each with fresh actions in and out of 0 .. 3 (-1 .. 8, large
    values of either sign; 4 .. 8 and 255 for bytes): with done flags, without them (NULL), with player 1's actions NULL, and with
    no actions at all but done flags. After every call the facings and the windows (restricted by the UPDATED facing, apertures
    (90, 360): player 1 keeps turning, its window keeps its bytes) equal the spec's."""
    from active_tracking_rl_amd import fov
    n = 65
    rs = np.random.RandomState(7)
    w, f = _case(n)
    facing = _dev(f)
    host = np.array(f)
    pool = np.array([0, 1, 2, 3, 4, 5, 8, 255] if dt == torch.uint8 else [0, 1, 2, 3, -1, 4, 8, -(2 ** 31), 2 ** 31 - 1])
    if dt == torch.int64:
        pool = np.concatenate([pool, [2 ** 32, 2 ** 32 + 1, -(2 ** 63), 2 ** 63 - 1]])      # (not 0 / 1 once truncated to 32 bits)
    npdt = {torch.uint8: np.uint8, torch.int32: np.int32, torch.int64: np.int64}[dt]
    for call, (give1, give_done, give0) in enumerate(((True, True, True), (True, False, True), (False, True, True),
                                                      (False, True, False))):
        a = pool[rs.randint(0, len(pool), (2, n))].astype(npdt)
        d = (rs.random_sample(n) < 0.3).astype(np.uint8) * rs.choice([1, 7, 255], n).astype(np.uint8)
        acts = (_dev(a[0]) if give0 else None, _dev(a[1]) if give1 else None)
        done = _dev(d) if give_done else None
        obs = _dev(w)
        fov.restrict_(obs, facing, acts, done, apertures=(90, 360), near=1)
        torch.cuda.synchronize()
        want, host = sp.step(w, host, (a[0] if give0 else None, a[1] if give1 else None), d if give_done else None, (90, 360), 1)
        assert np.array_equal(facing.cpu().numpy(), host), (call, "facing")
        assert np.array_equal(obs.cpu().numpy(), want) and np.array_equal(want[:, 1], w[:, 1]), (call, "windows")
    assert set(np.unique(host)) <= set(sp.FACINGS) and (host != np.array(f)).any()


def _raw(obs):
    """[N, 2, 1, 1, 13, 13] as VecEnv hands it out (no stack, no rescale) -> numpy [N, 2, 13, 13]."""
    a = obs.cpu().numpy()
    return a.reshape(a.shape[0], 2, 13, 13)


class _HostFov(object):
    """What VecEnv(fov=...) must hand out, from a plain twin's observations: the facing tracked on the host (fov_spec.turn_all),
    occlusion_spec first where the env occludes."""

    def __init__(self, n, apertures, near=1, occlusion=False, auto_reset=True, scripted=False):
        self.n, self.near, self.occlusion, self.auto_reset, self.scripted = n, near, occlusion, auto_reset, scripted
        self.apertures = (apertures[0], 360) if scripted else apertures
        self.reset()

    def reset(self):
        self.facing = np.full((self.n, 2), sp.NONE, np.uint8)

    def see(self, raw, actions=None, done=None):
        """raw [N, 2, 13, 13] of the plain twin -> the windows; actions: (a0 [N], a1 [N]) of a step, None for reset / observe."""
        if actions is not None:
            a0, a1 = actions
            self.facing = sp.turn_all(self.facing, (a0, None if self.scripted else a1), done if self.auto_reset else None)
        if self.occlusion:
            raw = occlusion_spec.occlude(raw)
        return sp.restrict(raw, self.facing, self.apertures, self.near)


ENV_CASES = {
    "pzr-f32": (PZR, dict(), dict(max_episode_steps=LIMIT)),
    "pzr-u8": (PZR, dict(obs_u8=True), dict(max_episode_steps=LIMIT)),
    "pzr-own-limit": (PZR, dict(obs_u8=True), dict()),
    "pzr-no-auto-reset": (PZR, dict(auto_reset=False), dict(max_episode_steps=LIMIT)),
    "pzr-occlusion": (PZR, dict(obs_u8=True, occlusion=True), dict(max_episode_steps=LIMIT)),
    "ram": (RAM, dict(obs_u8=True), dict(max_episode_steps=LIMIT)),
    "pzr-stack2": (PZR, dict(stack_frames=2), dict(max_episode_steps=LIMIT)),
}


@pytest.mark.parametrize("case", list(ENV_CASES))
def test_env_equals_its_plain_twin(case):
    """VecEnv(fov=(90, 180)) and a plain VecEnv of the same id and seed under the same 40 random actions, 65 envs: rewards and
    done flags identical; every observation — reset(), observe() after it, every step(), observe() after the last step (which
    repeats it and turns nobody) — equals the spec applied on the host, with the facing tracked there, to the plain twin's, in
    the env's own dtype. The TimeLimit is 13, so that every env ends an episode (and, with the in-launch auto-reset, starts the
    next one looking all round) three times inside the walk; the case "pzr-own-limit" runs under the id's own limit, where seed 9
    ends 28 episodes inside the 40 steps (measured on the device; asserted as "some"). Without the auto-reset no done flag reaches the pass, and a reset() half way starts everybody from NONE. With
    occlusion the plain windows go through occlusion_spec first. A scripted (Ram) target's window 1 is the plain twin's, and its
    facing stays NONE. With two stacked frames the windows are restricted first and stacked then. (obs_u8 asks for bytes; 65
    envs keep float observations, as every odd batch does: the byte path through the env is the rollout store's, below.)"""
    from active_tracking_rl_amd.environment import VecEnv
    env_id, kw, both = ENV_CASES[case]
    n, steps = 65, 40
    plain_kw = {k: v for k, v in kw.items() if k != "occlusion"}
    env = VecEnv(env_id, n, device=DEV, seed=9, fov=(90, 180), **kw, **both)
    plain = VecEnv(env_id, n, device=DEV, seed=9, **plain_kw, **both)
    try:
        assert env.fov == (90, 180) and env.fov_near == 1 and plain.fov is None and plain._facing is None
        assert env.obs_u8 == plain.obs_u8 and env._facing.shape == (n, 2) and env._facing.dtype == torch.uint8
        bufs = plain.rollout_buffers(1)
        if bufs is not None:
            assert env.fused_step_out(tuple(b[0] for b in (bufs[0][1:], bufs[1], bufs[2]))) is None
        auto = kw.get("auto_reset", True)
        host = _HostFov(n, (90, 180), occlusion=kw.get("occlusion", False), auto_reset=auto, scripted=env_id == RAM)
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

        same(env.reset(), expect(host.see(plain_windows(plain.reset())), fill=True), "reset")
        same(env.observe(), expect(host.see(plain_windows(plain.observe())), peek=True), "observe after reset")
        gen = torch.Generator(device=DEV)
        gen.manual_seed(4)
        acts = torch.randint(0, 4, (steps, 2, n), device=DEV, generator=gen)
        acts_h = acts.cpu().numpy()
        ends = hidden = 0
        for t in range(steps):
            if not auto and t == steps // 2:
                host.reset()
                same(env.reset(), expect(host.see(plain_windows(plain.reset())), fill=True), "reset half way")
            a = [acts[t, 0]] if env_id == RAM else [acts[t, 0], acts[t, 1]]
            o, r, d, _ = env.step(a)
            p, r2, d2, _ = plain.step(a)
            assert torch.equal(r, r2) and torch.equal(d, d2), t
            dh = d2.cpu().numpy()
            raw = plain_windows(p)
            seen = host.see(raw, (acts_h[t, 0], acts_h[t, 1]), dh)
            same(o, expect(seen, done=dh), "step %d" % t)
            assert np.array_equal(env._facing.cpu().numpy(), host.facing), t
            ends += int(dh.astype(bool).sum())
            hidden += int((seen != raw).sum())
            if env_id == RAM:
                assert np.array_equal(seen[:, 1], raw[:, 1]) and (host.facing[:, 1] == sp.NONE).all()
        before = env._facing.clone()
        same(env.observe(), expect(host.see(plain_windows(plain.observe())), peek=True), "observe after the walk")
        assert torch.equal(env._facing, before) and hidden > 0
        print("%s: %d episode ends in %d steps x %d envs, %d cells hidden" % (case, ends, steps, n, hidden))
        assert ends >= (1 if case == "pzr-own-limit" else 3 * n if auto else n)
        assert env.core.faults() == 0 and plain.core.faults() == 0
    finally:
        env.close()
        plain.close()


@pytest.mark.parametrize("rng", ["philox", "numpy"])
@pytest.mark.parametrize("env_id", [PZR, "Track2D-BlockPartialNav-v0"], ids=["pzr", "nav"])
def test_gym_protocol_env_equals_its_plain_twin(env_id, rng):
    """Track2DEnv(fov=90) under the reference's gym protocol, on the device generators and in the reference-exact mode (whose
    reset goes through t2d_inject and observe(), a path of its own), with a model-driven and with a scripted (Nav) target, which
    the host drives in the reference-exact mode: two episodes of reset and 15 steps against a plain twin of the same seed —
    observations equal the spec of the twin's (the scripted target's window is the twin's), rewards, done flags and distances
    are the twin's, and every reset starts from NONE."""
    from active_tracking_rl_amd.environment import Track2DEnv
    env = Track2DEnv(env_id, device=DEV, seed=3, rng=rng, fov=90)
    plain = Track2DEnv(env_id, device=DEV, seed=3, rng=rng)
    try:
        host = _HostFov(1, (90, 90), auto_reset=False, scripted=env_id != PZR)
        rs = np.random.RandomState(2)
        hidden = 0
        for episode in range(2):
            host.reset()
            o, p = env.reset(), plain.reset()
            assert o.dtype == p.dtype == np.float32 and o.shape == p.shape == (2, 1, 1, 13, 13)
            assert np.array_equal(o, p) and (env.vec._facing == sp.NONE).all(), (episode, "reset")
            for t in range(15):
                a = rs.randint(0, 4, 2)
                o, r, d, info = env.step(a)
                p, r2, d2, info2 = plain.step(a)
                want = host.see(p.reshape(1, 2, 13, 13), (a[:1], a[1:]))
                assert np.array_equal(o.reshape(1, 2, 13, 13), want), (episode, t)
                assert np.array_equal(r, r2) and d == d2 and info["distance"] == info2["distance"]
                hidden += int((o != p).sum())
                if d:
                    break
        assert hidden > 0
    finally:
        env.close()
        plain.close()


def test_rollout_slot_bytes_and_near_and_a_single_aperture():
    """64 envs with obs_u8 (bytes) and fov=270, fov_near=0, stepping straight into the slots of a rollout store (`out=`): every
    slot equals the spec on the plain twin's."""
    from active_tracking_rl_amd.environment import VecEnv
    n, steps = 64, 16         # (past the TimeLimit of 13: every env restarts inside the store)
    env = VecEnv(PZR, n, device=DEV, seed=5, obs_u8=True, max_episode_steps=LIMIT, fov=270, fov_near=0)
    plain = VecEnv(PZR, n, device=DEV, seed=5, obs_u8=True, max_episode_steps=LIMIT)
    try:
        assert env.obs_u8 and env.fov == (270, 270) and env.fov_near == 0
        host = _HostFov(n, (270, 270), near=0)
        store, rew, done = env.rollout_buffers(steps)
        assert store.dtype == torch.uint8
        store[0].copy_(env.reset().reshape(store[0].shape))
        want = [host.see(_raw(plain.reset()))]
        gen = torch.Generator(device=DEV)
        gen.manual_seed(6)
        acts = torch.randint(0, 4, (steps, 2, n), device=DEV, generator=gen)
        for t in range(steps):
            env.step([acts[t, 0], acts[t, 1]], out=(store[t + 1], rew[t], done[t]))
            p, r2, d2, _ = plain.step([acts[t, 0], acts[t, 1]])
            assert torch.equal(rew[t], r2) and torch.equal(done[t], d2)
            want.append(host.see(_raw(p), (acts[t, 0].cpu().numpy(), acts[t, 1].cpu().numpy()), d2.cpu().numpy()))
        assert np.array_equal(store.cpu().numpy(), np.stack(want)) and (store == 5).any() and int(done.sum()) > 0
    finally:
        env.close()
        plain.close()


def test_clone_and_restore_repeat_a_continuation():
    """10 steps, clone_state(), 12 more steps recorded (episodes end in between), restore_state(): the facings are the clone's,
    and the same 12 actions give the same observations, rewards, done flags and facings bit for bit. A masked restore puts back
    the masked envs' facings only."""
    from active_tracking_rl_amd.environment import VecEnv
    n = 65
    env = VecEnv(PZR, n, device=DEV, seed=3, max_episode_steps=LIMIT, fov=(90, 180))
    try:
        gen = torch.Generator(device=DEV)
        gen.manual_seed(11)
        acts = torch.randint(0, 4, (22, 2, n), device=DEV, generator=gen)
        env.reset()
        for t in range(10):
            env.step([acts[t, 0], acts[t, 1]])
        state = env.clone_state()
        at_clone = env._facing.clone()
        assert (at_clone != sp.NONE).any() and state["facing"] is not env._facing

        def walk():
            out = []
            for t in range(10, 22):
                o, r, d, _ = env.step([acts[t, 0], acts[t, 1]])
                out.append((o.clone(), r.clone(), d.clone(), env._facing.clone()))
            return out
        first = walk()
        assert sum(int(x[2].sum()) for x in first) > 0 and not torch.equal(env._facing, at_clone)
        env.restore_state(state)
        assert torch.equal(env._facing, at_clone)
        for a, b in zip(first, walk()):
            assert all(torch.equal(x, y) for x, y in zip(a, b))
        moved = env._facing.clone()
        mask = torch.arange(n, device=DEV) % 3 == 0
        env.restore_state(state, mask=mask)
        assert torch.equal(env._facing[mask], at_clone[mask]) and torch.equal(env._facing[~mask], moved[~mask])
        assert env.core.faults() == 0
    finally:
        env.close()


def test_five_steps_captured_in_one_graph_replay_with_fresh_actions():
    """Five VecEnv.step calls on static action tensors inside one torch.cuda.graph (the stamps of the env's generator restarted
    before the capture and at its end, as train.rollout does for a rollout that is no whole stamp cycle), replayed three times
    with fresh actions copied in: all fifteen observations, with rewards, done flags and the facing after each replay, equal the
    spec on a plain twin that takes the same fifteen steps eagerly. The facing tensor is state the replays carry."""
    from active_tracking_rl_amd.environment import VecEnv
    n, T, replays = 65, 5, 3
    env = VecEnv(PZR, n, device=DEV, seed=8, max_episode_steps=LIMIT, fov=(90, 180))
    plain = VecEnv(PZR, n, device=DEV, seed=8, max_episode_steps=LIMIT)
    try:
        host = _HostFov(n, (90, 180))
        gen = torch.Generator(device=DEV)
        gen.manual_seed(12)
        fresh = torch.randint(0, 4, (replays + 1, T, 2, n), device=DEV, generator=gen)
        env.reset()
        host.see(_raw(plain.reset()))
        static = fresh[replays].clone()

        def five(e):
            out = [e.step([static[t, 0], static[t, 1]]) for t in range(T)]
            e.flush()
            return out

        def compare(got, k):
            acts_h = static.cpu().numpy()
            ends = 0
            for t, ((o, r, d, _), (p, r2, d2, _)) in enumerate(zip(got, five(plain))):
                dh = d2.cpu().numpy()
                assert np.array_equal(_raw(o), host.see(_raw(p), (acts_h[t, 0], acts_h[t, 1]), dh)), (k, t)
                assert torch.equal(r, r2) and torch.equal(d, d2), (k, t)
                ends += int(dh.astype(bool).sum())
            assert np.array_equal(env._facing.cpu().numpy(), host.facing), k
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
    (raw obs u8 [T+1, N, 2, 13, 13], rew [T, N, 2], done [T, N])."""
    from active_tracking_rl_amd.environment import VecEnv
    plain = VecEnv(PZR, n, device=DEV, seed=seed, obs_u8=True)
    try:
        plain.reset()
        plain.core.snapshot().load_bytes(first).restore()
        obs, rew, done = [_raw(plain.observe())], [], []
        for t in range(actions.shape[0]):
            o, r, d, _ = plain.step([actions[t, 0].contiguous(), actions[t, 1].contiguous()])
            obs.append(_raw(o))
            rew.append(r.cpu().numpy())
            done.append(d.cpu().numpy())
        assert plain.core.faults() == 0
        return np.stack(obs), np.stack(rew), np.stack(done)
    finally:
        plain.close()


def _store_equals_the_spec(player, n, seed, blob, facing0, what):
    """The rollout store of `player` against its own raw twin: a plain env started from the snapshot `blob`, driven by the stored
    actions, restricted on the host from the facing the shard had before the rollout."""
    acts = player._cache.actions
    raw, rew, done = _twin_walk(n, seed, acts, blob)
    a = acts.cpu().numpy()
    host = _HostFov(n, (90, 90))
    host.facing = np.array(facing0)
    want = [host.see(raw[0])]
    for t in range(a.shape[0]):
        want.append(host.see(raw[t + 1], (a[t, 0], a[t, 1]), done[t]))
    obs, r, d = (b.cpu().numpy() for b in player._buf)
    assert obs.dtype == np.uint8 and np.array_equal(obs, np.stack(want)), what
    assert np.array_equal(r, rew) and np.array_equal(d, done), what
    assert np.array_equal(player.env._facing.cpu().numpy(), host.facing), what
    assert (obs == 5).any() and (np.stack(want) != raw).any()


@pytest.mark.parametrize("schedule", ["eager", "synchronous", "pipelined"])
def test_training_stores_what_the_players_see(schedule):
    """64 envs x 5 steps, tat-maze-lstm, fov=90: two iterations of the eager loop (rollout + optimize) and of each graphed
    schedule, with the field-of-view launch inside the captured rollout. Every window of the second iteration's rollout store
    equals the spec applied to its own raw twin — a plain env put into the state the shard had before that iteration (a snapshot
    blob, and the facing bytes read at that moment) and driven by the iteration's stored actions; the env never takes the fused
    step; the bucket and the loss terms are finite and the env kernels flag no fault."""
    from active_tracking_rl_amd.train import GraphedIteration, PipelinedIteration, default_args, make_player, rollout
    n, T = 64, 5
    args = default_args(env=PZR, num_envs=n, num_steps=T, seed=2, network="tat-maze-lstm", aux="reward", train_mode=-1, fov=90)
    args.gpu_ids = [0]
    player, opt = make_player(args, torch.device(DEV), 0, 1)
    env = player.env
    try:
        assert env.fov == (90, 90) and env.obs_u8
        def mark():
            torch.cuda.synchronize()
            return env.core.snapshot().save().to_bytes(), env._facing.cpu().numpy()
        if schedule == "eager":
            optimize = lambda: player.optimize(None, opt, player.model, args.train_mode, torch.device(DEV))
            rollout(player, T)
            optimize()
            blob, facing0 = mark()
            rollout(player, T)
            torch.cuda.synchronize()
            last = player
            _store_equals_the_spec(last, n, args.seed, blob, facing0, schedule)
            stats = optimize()
        else:
            it = (GraphedIteration if schedule == "synchronous" else PipelinedIteration)(player, opt, args)
            it.run()
            it.finish()
            blob, facing0 = mark()
            stats = it.run()
            it.finish()
            torch.cuda.synchronize()
            last = it.player if schedule == "synchronous" else it.players[(it.i - 1) & 1]
            _store_equals_the_spec(last, n, args.seed, blob, facing0, schedule)
        torch.cuda.synchronize()
        assert not last.model.env_stepped and not last.model.env_step_fused_seen
        assert all(bool(torch.isfinite(s).all()) for s in stats)
        assert torch.isfinite(opt.bucket.flat).all() and torch.isfinite(opt.bucket.grad).all()
        assert env.core.faults() == 0
    finally:
        env.close()
