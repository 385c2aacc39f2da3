"""-m gpu: the egocentric view on the device. Everything is integers (or floats that hold them), so everything is compared for
EQUALITY with tests/ego_spec.py: atr_ego_windows on windows of distinct cells in every layout the ABI addresses, with guard bytes,
under every facing byte, in place and out of place, for every `roles`; its turn rule under the three action dtypes;
atr_ego_actions over every facing x action; VecEnv(egocentric=...) on relative actions against a twin with the same options minus
`egocentric`, on the same seed, stepped with the spec's absolute actions; the gym-protocol env on both episode sources; snapshots;
five env steps captured in one graph and replayed; the rollout store of the eager loop and of both graphed schedules; and an
evaluation round of the heuristic players."""
import functools

import numpy as np
import pytest
import torch

import ego_spec as sp
import fov_spec
from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PZR = "Track2D-BlockPartialPZR-v0"
RAM = "Track2D-BlockPartialRam-v0"
NAV = "Track2D-BlockPartialNav-v0"
LIMIT = 13        # a short TimeLimit: episodes end (and auto-reset) inside a 40-step walk
POISON = 253      # (no cell of _case holds it: they stay below 251)
NPDT = {torch.uint8: np.uint8, torch.int32: np.int32, torch.int64: np.int64}


@functools.lru_cache(maxsize=None)
def _case(n, p=2):
    """(windows u8 [n, p, 13, 13] with cell c of window k = (c * 7 + k) % 251: 169 different values per window, so any misplaced
    cell shows; facing bytes u8 [n, p] over {0, 1, 2, 3, 255, 7}) — once per (n, p), shared."""
    k = np.arange(n * p).reshape(n, p, 1)
    w = ((np.arange(169).reshape(1, 1, 169) * 7 + k) % 251).astype(np.uint8).reshape(n, p, 13, 13)
    f = np.array(sp.FACINGS, np.uint8)[np.random.RandomState(200 + n + p).randint(0, len(sp.FACINGS), (n, p))]
    f.reshape(-1)[:len(sp.FACINGS)] = sp.FACINGS[:f.size]     # (from three envs up every byte occurs, whatever n draws)
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
    """Windows of distinct cells and facing bytes over {0, 1, 2, 3, 255, 7} as a dense [n, P, 169] store (P = 1 and 2) behind
    37 .. 39 guard elements (byte windows: 169 is odd, so every alignment of a window's first byte occurs), for roles 1, 2, 3,
    without actions and done flags (nobody turns). In place: the store equals the spec — a player outside `roles` keeps its window
    byte for byte — and guards and facings are untouched. src -> dst into a poisoned buffer: every window of a player in `roles`
    equals the spec (every cell written, heading 0 included), another player's window of dst is still poison, src is unchanged."""
    from active_tracking_rl_amd import ego
    dt = torch.uint8 if u8 else torch.float32
    npdt = np.uint8 if u8 else np.float32
    guard = 37 + n % 3
    for p in (1, 2):
        w, f = _case(n, p)
        facing = _dev(f)
        for roles in (1, 2, 3):
            want = sp.view_all(w, f, roles).astype(npdt)
            buf, view = _guarded(w, guard, dt)
            assert ego.turn_(view, facing, roles=roles) is view
            dst_buf = torch.full_like(buf, POISON)
            dst = dst_buf[guard:guard + w.size].view(w.shape)
            src_buf, src = _guarded(w, guard, dt)
            ego.ego_windows(src.data_ptr(), dst.data_ptr(), u8, n, p, 169 * p, 169, facing.data_ptr(), None, None, 0, None, roles,
                            _stream())
            torch.cuda.synchronize()
            what = (n, p, roles)
            assert np.array_equal(view.cpu().numpy(), want) and _guards_intact(buf, guard), what + ("in place",)
            got = dst.cpu().numpy()
            for q in range(p):
                if (roles >> q) & 1:
                    assert np.array_equal(got[:, q], want[:, q]), what + ("out of place", q)
                else:
                    assert (got[:, q] == POISON).all() and np.array_equal(want[:, q], w[:, q].astype(npdt)), what + ("outside", q)
            assert _guards_intact(dst_buf, guard) and np.array_equal(src.cpu().numpy(), w.astype(npdt)) and _guards_intact(src_buf, guard)
            assert np.array_equal(facing.cpu().numpy(), f), what
    w, f = _case(n, 2)
    if n >= 3:
        assert (sp.view_all(w, f) != w).any()


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("n", [3, 65])
def test_strided_stores(n, u8):
    """Slot 1 of a poisoned [3, n, 2, 13, 13] rollout store (byte slots of an odd n start off dword alignment), of which only that
    slot changes; the slice [n, 1:3] of a poisoned [n, 5, 13, 13] store (an env stride of five windows), of which only the
    addressed windows change; and player 0 alone as [n, 0:1] of a dense store with a facing tensor [n, 1]."""
    from active_tracking_rl_amd import ego
    dt = torch.uint8 if u8 else torch.float32
    w, f = _case(n)
    facing = _dev(f)
    want = sp.view_all(w, f)
    store = torch.full((3, n, 2, 13, 13), POISON, dtype=dt, device=DEV)
    store[1].copy_(_dev(w, dt))
    ego.turn_(store[1], facing)
    wide = torch.full((n, 5, 13, 13), POISON, dtype=dt, device=DEV)
    wide[:, 1:3].copy_(_dev(w, dt))
    ego.turn_(wide[:, 1:3], facing)
    solo = _dev(w, dt)
    facing0 = _dev(np.ascontiguousarray(f[:, 1:]))
    ego.turn_(solo[:, 0:1], facing0, roles=1)
    torch.cuda.synchronize()
    got = store.cpu().numpy()
    assert np.array_equal(got[1], want.astype(got.dtype)) and (got[0] == POISON).all() and (got[2] == POISON).all()
    got = wide.cpu().numpy()
    assert np.array_equal(got[:, 1:3], want.astype(got.dtype)) and (got[:, 0] == POISON).all() and (got[:, 3:] == POISON).all()
    got = solo.cpu().numpy()
    assert np.array_equal(got[:, :1], sp.view_all(w[:, :1], f[:, 1:]).astype(got.dtype))
    assert np.array_equal(got[:, 1], w[:, 1].astype(got.dtype))
    with pytest.raises(ValueError, match="windows overlap"):
        ego.turn_(torch.zeros(169 * 4 + 8, dtype=dt, device=DEV).as_strided((4, 2, 13, 13), (169, 4, 13, 1)), facing[:4].contiguous())


@pytest.mark.parametrize("dt", [torch.uint8, torch.int32, torch.int64], ids=["u8", "i32", "i64"])
def test_turn_rule(dt):
    """65 envs x 2 players, six calls in a row on one facing tensor, each with fresh actions in and out of 0 .. 3 (-1 .. 8, large
    values of either sign; 4 .. 8 and 255 for bytes): with done flags, without them (NULL), with player 1's actions NULL, with no
    actions at all but done flags, and for roles 1 and 2. After every call the facings (the bytes of a player outside `roles`
    untouched) and the windows (turned by the UPDATED facing) equal the spec's."""
    from active_tracking_rl_amd import ego
    n = 65
    rs = np.random.RandomState(7)
    w, f = _case(n)
    facing = _dev(f)
    host = np.array(f)
    pool = np.array([0, 1, 2, 3, 4, 5, 8, 255] if dt == torch.uint8 else [0, 1, 2, 3, -1, 4, 8, -(2 ** 31), 2 ** 31 - 1])
    if dt == torch.int64:
        pool = np.concatenate([pool, [2 ** 32, 2 ** 32 + 1, -(2 ** 63), 2 ** 63 - 1]])      # (not 0 / 1 once truncated to 32 bits)
    for call, (give0, give1, give_done, roles) in enumerate(((True, True, True, 3), (True, True, False, 3), (True, False, True, 3),
                                                             (False, False, True, 3), (True, True, True, 1), (True, True, False, 2))):
        a = pool[rs.randint(0, len(pool), (2, n))].astype(NPDT[dt])
        d = (rs.random_sample(n) < 0.3).astype(np.uint8) * rs.choice([1, 7, 255], n).astype(np.uint8)
        acts = (_dev(a[0]) if give0 else None, _dev(a[1]) if give1 else None)
        done = _dev(d) if give_done else None
        obs = _dev(w)
        ego.turn_(obs, facing, acts, done, roles=roles)
        torch.cuda.synchronize()
        before = host
        want, host = sp.windows_call(w, host, (a[0] if give0 else None, a[1] if give1 else None), d if give_done else None, roles)
        assert np.array_equal(facing.cpu().numpy(), host), (call, "facing")
        assert np.array_equal(obs.cpu().numpy(), want), (call, "windows")
        for q in range(2):
            if not (roles >> q) & 1:
                assert np.array_equal(host[:, q], before[:, q]) and np.array_equal(want[:, q], w[:, q]), (call, q)
    assert set(np.unique(host)) <= set(sp.FACINGS) and (host != np.array(f)).any()


def _action_case(n, dt):
    """facing bytes [n, 2] and relative actions (r0 [n], r1 [n]) that run through every facing byte x action -1 .. 8 (bytes: 255
    for -1), player 1 three combinations ahead of player 0."""
    acts = [255 if dt == torch.uint8 else -1] + list(range(9))
    combos = [(f, a) for f in sp.FACINGS for a in acts]
    pick = lambda shift: [combos[(i + shift) % len(combos)] for i in range(n)]
    c0, c1 = pick(0), pick(3)
    facing = np.array([[x[0], y[0]] for x, y in zip(c0, c1)], np.uint8)
    rel = (np.array([x[1] for x in c0]).astype(NPDT[dt]), np.array([y[1] for y in c1]).astype(NPDT[dt]))
    return facing, rel


@pytest.mark.parametrize("dt", [torch.uint8, torch.int32, torch.int64], ids=["u8", "i32", "i64"])
def test_actions_equal_the_spec(dt):
    """atr_ego_actions at n = 130 (every facing byte x action -1 .. 8 occurs for both players; two workgroups) for roles 1, 2, 3:
    out of place into poisoned outputs, in place (abs_p is rel_p), and with a NULL second pair (the poisoned second output stays
    poison); at n = 1 one launch per combination. The facing bytes are unchanged, and so are the inputs of an out-of-place call."""
    from active_tracking_rl_amd import ego
    n = 130
    fh, rel = _action_case(n, dt)
    facing = _dev(fh)
    for roles in (1, 2, 3):
        want = sp.abs_all(fh, rel, roles)
        r0, r1 = _dev(rel[0]), _dev(rel[1])
        o0, o1 = torch.full_like(r0, 99), torch.full_like(r1, 99)
        out = ego.to_absolute((r0, r1), facing, roles, (o0, o1))
        assert out[0] is o0 and out[1] is o1
        i0, i1 = r0.clone(), r1.clone()
        ego.to_absolute((i0, i1), facing, roles, (i0, i1))
        s0, s1 = torch.full_like(r0, 99), torch.full_like(r1, 99)
        ego.to_absolute((r0, None), facing, roles, (s0, None))
        torch.cuda.synchronize()
        for got, p in ((o0, 0), (o1, 1), (i0, 0), (i1, 1), (s0, 0)):
            assert np.array_equal(got.cpu().numpy().astype(np.int64), want[p].astype(NPDT[dt]).astype(np.int64)), (roles, p)
        assert (s1 == 99).all() and np.array_equal(r0.cpu().numpy(), rel[0]) and np.array_equal(r1.cpu().numpy(), rel[1])
        assert np.array_equal(facing.cpu().numpy(), fh)
    assert all((sp.abs_all(fh, rel, 3)[p] != rel[p].astype(np.int64)).any() for p in range(2))
    f1, rel1 = _action_case(60, dt)
    for i in range(60):
        roles = (3, 1, 2)[i % 3]
        fi = np.ascontiguousarray(f1[i:i + 1])
        ri = (rel1[0][i:i + 1], rel1[1][i:i + 1])
        facing = _dev(fi)
        o0, o1 = _dev(ri[0]), _dev(ri[1])
        ego.to_absolute((o0, o1), facing, roles, (o0, o1))
        want = sp.abs_all(fi, ri, roles)
        assert int(o0.cpu()[0]) == int(want[0].astype(NPDT[dt])[0]) and int(o1.cpu()[0]) == int(want[1].astype(NPDT[dt])[0]), i
        assert np.array_equal(facing.cpu().numpy(), fi)


ENV_CASES = {
    "plain": (PZR, 6, dict(obs_u8=True), True),
    "occlusion": (PZR, 6, dict(obs_u8=True, occlusion=True), True),
    "fov90": (PZR, 6, dict(obs_u8=True, fov=90), True),
    "fov180-360": (PZR, 6, dict(obs_u8=True, fov=(180, 360)), True),
    "footprints": (PZR, 6, dict(obs_u8=True, footprints=4, footprints_for="both"), True),
    "all-three": (PZR, 6, dict(obs_u8=True, occlusion=True, fov=90, footprints=4, footprints_for="both"), True),
    "stack2": (PZR, 6, dict(stack_frames=2), True),
    "f32-odd": (PZR, 7, dict(obs_u8=True), True),
    "ram": (RAM, 6, dict(obs_u8=True), True),
    "tracker-only": (PZR, 6, dict(obs_u8=True), "tracker"),
    "tracker-only-fov90": (PZR, 6, dict(obs_u8=True, fov=90), "tracker"),
}


@pytest.mark.parametrize("case", list(ENV_CASES))
def test_env_equals_its_plain_twin(case):
    """VecEnv(egocentric=...) under 40 fixed pseudo-random RELATIVE actions and a twin with the same options minus `egocentric`,
    on the same seed, stepped with the spec's ABSOLUTE actions (ego_spec.EnvModel: read with the heading each step starts from):
    rewards and done flags bit-equal; every observation — reset(), observe() after it, every step(), observe() after the walk —
    equals spec.view of the twin's under the spec's facing, the first windows after in-launch restarts included (TimeLimit 13:
    every env restarts three times); the env's facing bytes are the model's; the env never offers the fused step; its
    absolute-action buffers hold the spec's. With fov=90 and a heading in 0 .. 3 the 5-mask of an egocentric window is the spec's
    heading-0 cone, for every env at every step: the property the feature exists for. A Ram target's window is the twin's. With
    two stacked frames the windows are turned first and stacked then."""
    from active_tracking_rl_amd.environment import VecEnv
    env_id, n, kw, who = ENV_CASES[case]
    steps = 40
    env = VecEnv(env_id, n, device=DEV, seed=9, egocentric=who, max_episode_steps=LIMIT, **kw)
    twin = VecEnv(env_id, n, device=DEV, seed=9, max_episode_steps=LIMIT, **kw)
    try:
        scripted = env_id == RAM
        roles = 1 if scripted or who == "tracker" else 3
        assert env._ego_roles == roles and env.egocentric == ("tracker" if roles == 1 else "both")
        assert twin.egocentric is None and twin._ego_roles == 0 and twin._ego_abs is None
        assert env.obs_u8 == twin.obs_u8 and (env.obs_u8 or case != "plain") and not (env.obs_u8 and n % 2)
        assert env._facing.shape == (n, 2) and env._facing.dtype == torch.uint8 and (twin._facing is None) == ("fov" not in kw)
        assert sorted(env._ego_abs, key=str) == sorted(NPDT, key=str) and all(t.shape == (2, n) for t in env._ego_abs.values())
        bufs = twin.rollout_buffers(1)
        if bufs is not None:
            assert env.fused_step_out(tuple(b[0] for b in (bufs[0][1:], bufs[1], bufs[2]))) is None
        model = sp.EnvModel(n, roles=roles, scripted=scripted, fov="fov" in kw)
        stack = kw.get("stack_frames", 1)
        frames = [None]
        cone = fov_spec.hidden_cells(0, 90, 1)

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

        def twin_windows(obs):
            a = obs.cpu().numpy()
            return a.reshape(n, 2, stack, 13, 13)[:, :, -1]

        same(env.reset(), expect(model.see(twin_windows(twin.reset())), fill=True), "reset")
        same(env.observe(), expect(model.see(twin_windows(twin.observe())), peek=True), "observe after reset")
        rel_h = np.random.RandomState(4).randint(0, 4, (steps, 2, n))
        rel = _dev(rel_h)
        ends = turned = cones = 0
        for t in range(steps):
            abs_h = model.absolute((rel_h[t, 0], rel_h[t, 1]))
            o, r, d, _ = env.step([rel[t, 0]] if scripted else [rel[t, 0], rel[t, 1]])
            a = [_dev(abs_h[0])] if scripted else [_dev(abs_h[0]), _dev(abs_h[1])]
            p, r2, d2, _ = twin.step(a)
            assert torch.equal(r, r2) and torch.equal(d, d2), t
            dh = d2.cpu().numpy()
            model.stepped(abs_h, dh)
            raw = twin_windows(p)
            seen = model.see(raw)
            same(o, expect(seen, done=dh), "step %d" % t)
            assert np.array_equal(env._facing.cpu().numpy(), model.facing), t
            if twin._facing is not None:
                assert torch.equal(env._facing, twin._facing), t
            got_abs = env._ego_abs[torch.int64].cpu().numpy()
            assert np.array_equal(got_abs[0], abs_h[0]) and (scripted or np.array_equal(got_abs[1], abs_h[1])), t
            ends += int(dh.astype(bool).sum())
            turned += int((seen != raw).sum())
            if scripted:
                assert np.array_equal(seen[:, 1], raw[:, 1]) and (model.facing[:, 1] == sp.NONE).all()
            if who == "tracker":
                assert np.array_equal(seen[:, 1], raw[:, 1])
            if case in ("fov90", "tracker-only-fov90"):
                for e in range(n):
                    for q in range(2 if roles == 3 else 1):
                        if model.facing[e, q] <= 3:
                            assert np.array_equal(seen[e, q] == 5, cone), (t, e, q)
                            cones += 1
            for q in range(2):          # what a compass-frame player hands to step() to make the moves `m`
                m = rel[t, q]
                want_rel = [sp.to_rel(model.facing[e, q], rel_h[t, q, e]) if (roles >> q) & 1 else rel_h[t, q, e] for e in range(n)]
                assert env.relative_actions(m, q).cpu().tolist() == want_rel, (t, q)
        before = env._facing.clone()
        same(env.observe(), expect(model.see(twin_windows(twin.observe())), peek=True), "observe after the walk")
        assert torch.equal(env._facing, before) and turned > 0
        print("%s: %d episode ends in %d steps x %d envs, %d cells differ from the twin's, %d cones checked"
              % (case, ends, steps, n, turned, cones))
        assert ends >= 3 * n and (cones > 0 or "fov90" not in case)
        assert env.core.faults() == 0 and twin.core.faults() == 0
    finally:
        env.close()
        twin.close()


@pytest.mark.parametrize("rng", ["philox", "numpy"])
@pytest.mark.parametrize("env_id", [PZR, NAV], ids=["pzr", "nav"])
def test_gym_protocol_env_equals_its_plain_twin(env_id, rng):
    """Track2DEnv(egocentric=True) under the reference's gym protocol, on the device generators and in the reference-exact mode
    (whose reset goes through t2d_inject and observe(), a path of its own), with a model-driven and with a scripted (Nav) target,
    which the host drives in the reference-exact mode: two episodes of reset and 15 steps on relative actions against a plain
    twin of the same seed on the spec's absolute ones — observations equal the spec's view of the twin's (the scripted target's
    window is the twin's), rewards, done flags and distances are the twin's, and every reset starts from NONE."""
    from active_tracking_rl_amd.environment import Track2DEnv
    env = Track2DEnv(env_id, device=DEV, seed=3, rng=rng, egocentric=True)
    twin = Track2DEnv(env_id, device=DEV, seed=3, rng=rng)
    try:
        scripted = env_id != PZR
        assert env.vec._ego_roles == (1 if scripted else 3)
        model = sp.EnvModel(1, roles=1 if scripted else 3, scripted=scripted, auto_reset=False)
        rs = np.random.RandomState(2)
        turned = 0
        for episode in range(2):
            model.reset()
            o, p = env.reset(), twin.reset()
            assert o.dtype == p.dtype == np.float32 and o.shape == p.shape == (2, 1, 1, 13, 13)
            assert np.array_equal(o, p) and (env.vec._facing == sp.NONE).all(), (episode, "reset")
            for t in range(15):
                a = rs.randint(0, 4, 2)
                abs_a = model.absolute((a[:1], a[1:]))
                o, r, d, info = env.step(a)
                p, r2, d2, info2 = twin.step([int(abs_a[0][0]), int(abs_a[1][0])])
                model.stepped(abs_a, None)
                want = model.see(p.reshape(1, 2, 13, 13))
                assert np.array_equal(o.reshape(1, 2, 13, 13), want), (episode, t)
                assert np.array_equal(r, r2) and d == d2 and info["distance"] == info2["distance"]
                assert np.array_equal(env.vec._facing.cpu().numpy()[:, :1], model.facing[:, :1])
                turned += int((o != p).sum())
                if d:
                    break
        assert turned > 0
    finally:
        env.close()
        twin.close()


def test_clone_and_restore_repeat_a_continuation():
    """`egocentric` alone (the facing tensor exists without fov): 10 steps, clone_state(), 12 more steps recorded (episodes end in
    between), restore_state(): the facings are the clone's, and the same 12 relative actions give the same observations, rewards,
    done flags and facings bit for bit. A masked restore puts back the masked envs' facings only."""
    from active_tracking_rl_amd.environment import VecEnv
    n = 65
    env = VecEnv(PZR, n, device=DEV, seed=3, max_episode_steps=LIMIT, egocentric="both")
    try:
        assert env.fov is None and env._facing is not None
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


def _raw(obs):
    """[N, 2, 1, 1, 13, 13] as VecEnv hands it out (no stack, no rescale) -> numpy [N, 2, 13, 13]."""
    a = obs.cpu().numpy()
    return a.reshape(a.shape[0], 2, 13, 13)


def test_five_steps_captured_in_one_graph_replay_with_fresh_actions():
    """Five VecEnv.step calls on static relative-action tensors inside one torch.cuda.graph, replayed three times with fresh
    relative actions copied in: all fifteen observations, with rewards, done flags and the facing after each replay, equal the
    spec on a plain twin that takes the same fifteen steps eagerly on the spec's absolute actions. The facing tensor is state the
    replays carry; the absolute-action buffers are where they were before the capture."""
    from active_tracking_rl_amd.environment import VecEnv
    n, T, replays = 65, 5, 3
    env = VecEnv(PZR, n, device=DEV, seed=8, max_episode_steps=LIMIT, egocentric=True)
    twin = VecEnv(PZR, n, device=DEV, seed=8, max_episode_steps=LIMIT)
    try:
        model = sp.EnvModel(n)
        gen = torch.Generator(device=DEV)
        gen.manual_seed(12)
        fresh = torch.randint(0, 4, (replays + 1, T, 2, n), device=DEV, generator=gen)
        env.reset()
        twin.reset()
        static = fresh[replays].clone()
        where = {dt: t.data_ptr() for dt, t in env._ego_abs.items()}

        def five():
            out = [env.step([static[t, 0], static[t, 1]]) for t in range(T)]
            env.flush()
            return out

        def compare(got, k):
            rel_h = static.cpu().numpy()
            ends = 0
            for t, (o, r, d, _) in enumerate(got):
                abs_h = model.absolute((rel_h[t, 0], rel_h[t, 1]))
                p, r2, d2, _ = twin.step([_dev(abs_h[0]), _dev(abs_h[1])])
                dh = d2.cpu().numpy()
                model.stepped(abs_h, dh)
                assert np.array_equal(_raw(o), model.see(_raw(p))), (k, t)
                assert torch.equal(r, r2) and torch.equal(d, d2), (k, t)
                ends += int(dh.astype(bool).sum())
            twin.flush()
            assert np.array_equal(env._facing.cpu().numpy(), model.facing), k
            return ends
        compare(five(), "eager")        # (one eager pass first: code objects are loaded before the capture)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            outs = five()
        ends = 0
        for k in range(replays):
            static.copy_(fresh[k])
            g.replay()
            torch.cuda.synchronize()
            ends += compare(outs, k)
        assert {dt: t.data_ptr() for dt, t in env._ego_abs.items()} == where
        assert ends > 0 and (model.facing <= 3).any() and env.core.faults() == 0 and twin.core.faults() == 0
        del g
    finally:
        env.close()
        twin.close()


def _store_equals_the_spec(player, n, seed, blob, facing0, what):
    """The rollout store of `player` against its own raw twin: a plain byte env put into the state of the snapshot `blob` and
    driven by the spec's absolute actions of the STORED (relative) actions, from the facing the shard had before the rollout."""
    from active_tracking_rl_amd.environment import VecEnv
    rel = player._cache.actions.cpu().numpy()             # [T, 2, N]
    model = sp.EnvModel(n)
    model.facing = np.array(facing0)
    twin = VecEnv(PZR, n, device=DEV, seed=seed, obs_u8=True)
    try:
        twin.reset()
        twin.core.snapshot().load_bytes(blob).restore()
        raws = [_raw(twin.observe())]
        want, rew, done, differ = [model.see(raws[0])], [], [], 0
        for t in range(rel.shape[0]):
            abs_h = model.absolute((rel[t, 0], rel[t, 1]))
            differ += int((abs_h[0] != rel[t, 0]).sum() + (abs_h[1] != rel[t, 1]).sum())
            o, r, d, _ = twin.step([_dev(abs_h[0]), _dev(abs_h[1])])
            dh = d.cpu().numpy()
            model.stepped(abs_h, dh)
            raws.append(_raw(o))
            want.append(model.see(raws[-1]))
            rew.append(r.cpu().numpy())
            done.append(dh)
        assert twin.core.faults() == 0
    finally:
        twin.close()
    obs, r, d = (b.cpu().numpy() for b in player._buf)
    assert obs.dtype == np.uint8 and np.array_equal(obs, np.stack(want)), what
    assert np.array_equal(r, np.stack(rew)) and np.array_equal(d, np.stack(done)), what
    assert np.array_equal(player.env._facing.cpu().numpy(), model.facing), what
    # the store holds the relative actions: their absolute ones differ somewhere, and so do the turned windows from the raw ones
    assert differ > 0 and (np.stack(want) != np.stack(raws)).any(), what
    assert set(np.unique(rel)) <= {0, 1, 2, 3}


@pytest.mark.parametrize("schedule", ["eager", "synchronous", "pipelined"])
def test_training_stores_what_the_players_see(schedule):
    """64 envs x 5 steps, tat-maze-lstm, egocentric: two iterations of the eager loop (rollout + optimize) and of each graphed
    schedule, with both launches inside the captured rollout. Every window of the second iteration's rollout store equals the
    spec applied to its own raw twin — a plain env put into the state the shard had before that iteration (a snapshot blob, and
    the facing bytes read at that moment) and driven by the absolute actions the spec makes of the iteration's STORED actions,
    which are the relative ones; the env never takes the fused step; the bucket and the loss terms are finite and the env kernels
    flag no fault."""
    from active_tracking_rl_amd.train import GraphedIteration, PipelinedIteration, default_args, make_player, rollout
    n, T = 64, 5
    args = default_args(env=PZR, num_envs=n, num_steps=T, seed=2, network="tat-maze-lstm", aux="reward", train_mode=-1, egocentric=True)
    args.gpu_ids = [0]
    player, opt = make_player(args, torch.device(DEV), 0, 1)
    env = player.env
    try:
        assert env.egocentric == "both" and env.fov is None and env.obs_u8

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


@pytest.mark.parametrize("env_id,players", [(NAV, dict(heuristic_tracker="pursuit")),
                                            (PZR, dict(heuristic_tracker="pursuit", heuristic_target="evade"))], ids=["nav", "pzr"])
def test_heuristic_players_play_the_same_episodes(env_id, players):
    """An eager evaluation round of the heuristic players (they plan in the compass frame; Agent hands their moves to
    VecEnv.relative_actions) on an egocentric env and on a plain env of the same seed: episode lengths and returns are equal."""
    import greedy_eval_spec as gs
    from active_tracking_rl_amd.test import evaluate
    plain = evaluate(None, env_id, gs.fixture_args(env_id, 8), torch.device(DEV), episodes=8, **players)
    ego = evaluate(None, env_id, gs.fixture_args(env_id, 8, egocentric=True), torch.device(DEV), episodes=8, **players)
    print("lengths", ego[1], "tracker returns", ego[0][:, 0])
    assert np.array_equal(plain[1], ego[1]) and np.array_equal(plain[0], ego[0])
    assert ego[1].shape == (8,) and (ego[1] > 1).all()
