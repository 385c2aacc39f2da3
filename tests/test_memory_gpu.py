"""-m gpu: map memory on the device. Everything is integers (or floats that hold them), so everything is compared for EQUALITY with
tests/memory_spec.py: the kernel on injected states whose window rows straddle each word seam of a tile row and hang off every edge
of the map, in every layout the ABI addresses, with guard bytes round the windows and guard words round the tiles, under every
mode and role set; VecEnv(map_memory=...) against a twin of the same seed and flags without it, with the seen sets tracked on the
host from the twin's own windows, positions and maps; observe(); clone / restore; the shard file; the gym-protocol env on both
episode sources; five env steps captured in one graph and replayed; and the rollout store of the eager loop and of both graphed
schedules."""
import functools

import numpy as np
import pytest
import torch

import ego_spec
import memory_spec as sp
from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PZR = "Track2D-BlockPartialPZR-v0"
MAZE = "Track2D-MazePartialPZR-v0"
ROOMS = "Track2D-RoomsPartialPZR-v3"
RAM = "Track2D-BlockPartialRam-v0"
NAV = "Track2D-BlockPartialNav-v0"
LIMIT = 13        # a short TimeLimit: episodes end (and auto-reset) inside a 40-step walk
POISON = 165      # (no value of memory_spec.VALUES, and neither paint value)
WORD = 0x5AA5A55A       # the guard words round the tiles
GUARD_WORDS = 8   # (a multiple of 4: the tiles stay 16-byte aligned)
S = sp.MAX_SIDE


def _special(side):
    """Player cells whose window rows straddle the word seams 31 | 32 and 63 | 64 (columns 26, 32, 58, 64: the window's first or
    last column on either side of a seam), hang off every edge and corner, or lie well inside."""
    return [(0, 0), (side - 1, side - 1), (3, 26), (40, 32), (side - 1, 58), (0, 64), (50, side - 1), (side - 1, 0), (31, 31),
            (64, 5), (6, 6), (12, side - 7), (37, 37), (5, 63), (70, 69), (75, 25)]


@functools.lru_cache(maxsize=None)
def _state(n, side, rnd):
    """(mazes u8 [n, side, side] with walls on about a third of the cells, pos [n, 2, 2] out of _special, rotating with the round;
    the players' own cells free). Once per (n, side, round), shared and read-only."""
    rs = np.random.RandomState(1000 * side + 10 * rnd + n)
    mazes = (rs.random_sample((n, side, side)) < 0.3).astype(np.uint8)
    cells = _special(side)
    pos = np.zeros((n, 2, 2), np.int32)
    for e in range(n):
        pos[e, 0] = cells[(rnd + e) % len(cells)]
        pos[e, 1] = cells[(rnd + e + 7) % len(cells)]
        for p in range(2):
            mazes[e, pos[e, p, 0], pos[e, p, 1]] = 0
    mazes.setflags(write=False)
    pos.setflags(write=False)
    return mazes, pos


def _walls(mazes):
    """bool [n, 82, 82] of u8 [n, side, side]."""
    out = np.zeros((mazes.shape[0], S, S), bool)
    out[:, :mazes.shape[1], :mazes.shape[2]] = mazes != 0
    return out


def _guarded(windows, guard, dt):
    """A poisoned device buffer with `guard` elements before and after the dense windows; (buffer, the windows' view)."""
    n = windows.size
    buf = torch.full((guard + n + guard,), POISON, dtype=dt, device=DEV)
    view = buf[guard:guard + n].view(windows.shape)
    view.copy_(torch.from_numpy(np.array(windows)).to(DEV).to(dt))
    return buf, view


def _guarded_tiles(tiles):
    """uint32 [n, 2, 256] on the device between two runs of GUARD_WORDS guard words; (buffer as int32, the tiles' uint32 view)."""
    n = tiles.size
    buf = torch.full((GUARD_WORDS + n + GUARD_WORDS,), WORD, dtype=torch.int32, device=DEV)
    view = buf[GUARD_WORDS:GUARD_WORDS + n].view(tiles.shape)
    view.copy_(torch.from_numpy(np.array(tiles).view(np.int32)).to(DEV))
    return buf, view.view(torch.uint32)


def _tiles(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _dev(a, dt=None):
    t = torch.from_numpy(np.array(a)).to(DEV)
    return t if dt is None else t.to(dt)


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("side", [81, 82])
@pytest.mark.parametrize("n", [1, 3, 5])
def test_kernel_equals_the_spec(n, side, u8):
    """Sixteen rounds of injected states (VecTrack2D.inject: random walls, the players on the cells of _special, rotating, so that
    with n = 1 every one of them is met by both players), windows drawn from {0, 1, 2, 4, 5, 6} with 5 twice as likely, seen tiles
    that start with random bits inside the square. Every round calls the kernel twice from the same start: on a dense [n, 2, 169]
    store behind 37 .. 39 poisoned guard elements (byte windows: with an odd count every alignment of a window's first byte
    occurs), and on the slice [:, 1:3] of a poisoned [n, 5, 13, 13] store (env stride 845). Roles 1, 2, 3 x the three modes all
    occur, done flags mixed, given and not given; values 7 / 8 and 9 / 200. Windows AND tiles equal the spec; the guards round the
    windows and round the tiles are intact; the window and the tile of a player outside `roles` are byte for byte what they were;
    memory.unpack of the tiles is the spec's set; 7s and 8s occur; the handle's fault word is 0."""
    from active_tracking_rl_amd import memory
    from active_tracking_rl_amd.vec_env import VecTrack2D
    dt = torch.uint8 if u8 else torch.float32
    npdt = np.uint8 if u8 else np.float32
    core = VecTrack2D(num_envs=n, map_type="Block", target_mode="Adv", level=1, auto_reset=False, max_episode_steps=500, device=DEV)
    try:
        core.reset()
        rs = np.random.RandomState(77 * n + side)
        guard = 37 + n % 3
        sevens = eights = kept5 = 0
        for rnd in range(16):
            mazes, pos = _state(n, side, rnd)
            core.inject(mazes, pos.reshape(n, 4))
            st = core.get_state()
            assert np.array_equal(st["pos"], pos) and (st["side"] == side).all()
            assert np.array_equal(core.get_maps()[:, :side, :side], mazes)
            walls, sides = _walls(mazes), np.full(n, side)
            roles, mode = rnd % 3 + 1, (rnd // 3) % 3
            done = None if rnd % 2 else (rs.random_sample(n) < 0.5).astype(np.uint8) * rs.choice([1, 7, 255], n).astype(np.uint8)
            wv, fv = (9, 200) if rnd % 4 == 3 else (sp.WALL, sp.FREE)
            w = sp.random_windows(n, 500 + rnd + 100 * n, npdt)
            seen0 = np.zeros((n, 2, S, S), bool)
            seen0[:, :, :side, :side] = rs.random_sample((n, 2, side, side)) < 0.3
            tiles0 = sp.pack(seen0)
            want_w, want_s = sp.call(w, seen0, walls, pos, sides, mode, done, roles, sp.HIDDEN, wv, fv)
            want_t = sp.pack(want_s)
            assert not want_s[:, :, side:].any() and not want_s[:, :, :, side:].any()
            ddone = None if done is None else _dev(done)
            what = (n, side, rnd, roles, mode)
            # dense, guarded
            buf, view = _guarded(w, guard, dt)
            tbuf, dseen = _guarded_tiles(tiles0)
            assert memory.remember_(view, dseen, core, mode, ddone, roles, sp.HIDDEN, wv, fv) is view
            torch.cuda.synchronize()
            assert np.array_equal(view.cpu().numpy(), want_w), what
            assert bool((buf[:guard] == POISON).all()) and bool((buf[-guard:] == POISON).all()), what
            assert np.array_equal(_tiles(dseen), want_t), what
            assert bool((tbuf[:GUARD_WORDS] == WORD).all()) and bool((tbuf[-GUARD_WORDS:] == WORD).all()), what
            assert np.array_equal(memory.unpack(dseen, side).cpu().numpy(), want_s[:, :, :side, :side]), what
            for p in range(2):
                if not (roles >> p) & 1:        # a wave outside `roles` changes nothing
                    assert np.array_equal(view.cpu().numpy()[:, p], w[:, p]) and np.array_equal(_tiles(dseen)[:, p], tiles0[:, p]), what
            # a slice of a larger store
            wide = torch.full((n, 5, 13, 13), POISON, dtype=dt, device=DEV)
            wide[:, 1:3].copy_(_dev(w, dt))
            tbuf2, dseen2 = _guarded_tiles(tiles0)
            memory.remember_(wide[:, 1:3], dseen2, core, mode, ddone, roles, sp.HIDDEN, wv, fv)
            torch.cuda.synchronize()
            got = wide.cpu().numpy()
            assert np.array_equal(got[:, 1:3], want_w) and (got[:, 0] == POISON).all() and (got[:, 3:] == POISON).all(), what
            assert np.array_equal(_tiles(dseen2), want_t), what
            assert bool((tbuf2[:GUARD_WORDS] == WORD).all()) and bool((tbuf2[-GUARD_WORDS:] == WORD).all()), what
            # idempotent: a KEEP call on the painted windows changes neither the windows nor the tiles
            memory.remember_(view, dseen, core, sp.KEEP, None, roles, sp.HIDDEN, wv, fv)
            torch.cuda.synchronize()
            assert np.array_equal(view.cpu().numpy(), want_w) and np.array_equal(_tiles(dseen), want_t), what
            sevens += int((want_w == wv).sum())
            eights += int((want_w == fv).sum())
            kept5 += int((want_w == sp.HIDDEN).sum())
        print("n %d side %d: %d wall cells, %d free cells painted, %d cells stay hidden" % (n, side, sevens, eights, kept5))
        assert sevens > 0 and eights > 0 and kept5 > 0 and core.faults() == 0
    finally:
        core.close()


def test_binding_refusals_on_the_device():
    """What the entry point refuses from the handle's state, and what remember_ refuses about its tensors; a Moore handle is
    fine."""
    from active_tracking_rl_amd import memory
    from active_tracking_rl_amd.vec_env import VecTrack2D
    mk = lambda **kw: VecTrack2D(num_envs=4, map_type="Block", target_mode="Adv", level=1, device=DEV, **kw)
    core, fresh, full = mk(auto_reset=False, action_type="Moore"), mk(), mk(obs_type="Full", auto_reset=False)
    try:
        core.reset()
        obs = torch.full((4, 2, 13, 13), 5, dtype=torch.uint8, device=DEV)
        seen = memory.new_seen(4, DEV)
        memory.remember_(obs, seen, core, sp.BEGIN)
        with pytest.raises(RuntimeError, match="call t2d_reset"):
            memory.remember_(obs, seen, fresh, sp.BEGIN)
        full.reset()
        with pytest.raises(RuntimeError, match="observes the whole map"):
            memory.remember_(obs, seen, full, sp.BEGIN)
        with pytest.raises(ValueError, match="windows overlap"):
            memory.remember_(torch.zeros(169 * 4 + 8, dtype=torch.uint8, device=DEV).as_strided((4, 2, 13, 13), (169, 4, 13, 1)),
                             seen, core, sp.KEEP)
        for bad in (seen[:3], seen.view(torch.int32), seen[:, :, :128], memory.new_seen(4, "cpu"), memory.new_seen(8, DEV)[::2]):
            with pytest.raises(ValueError, match="seen must be a contiguous uint32"):
                memory.remember_(obs, bad, core, sp.KEEP)
        with pytest.raises(ValueError, match="done must be a contiguous uint8"):
            memory.remember_(obs, seen, core, sp.STEP, torch.zeros(5, dtype=torch.uint8, device=DEV))
        with pytest.raises(ValueError, match="mode must be"):
            memory.remember_(obs, seen, core, 3)
        with pytest.raises(ValueError, match="obs holds 3 envs"):
            memory.remember_(obs[:3], seen[:3].contiguous(), core, sp.KEEP)
        with pytest.raises(RuntimeError, match="equal to hidden"):
            memory.remember_(obs, seen, core, sp.KEEP, None, 3, 5, 5, 8)
        torch.cuda.synchronize()
        assert not _tiles(seen).any() and core.faults() == 0        # (all-hidden windows: nothing was recorded)
    finally:
        for c in (core, fresh, full):
            c.close()


class _Host(object):
    """What VecEnv(map_memory=...) must hand out, from the windows, positions and maps of a twin without it."""

    def __init__(self, twin, roles):
        self.twin, self.n = twin, twin.num_envs
        self.model = sp.Model(self.n, roles)

    def world(self):
        core = self.twin.core
        st = core.get_state()
        return core.get_maps() != 0, st["pos"], st["side"]

    def begin(self, w):
        return self.model.begin(w, *self.world())

    def step(self, w, done):
        return self.model.step(w, *self.world(), done if self.twin.core.auto_reset else None)

    def keep(self, w):
        return self.model.keep(w, *self.world())

    def tiles(self):
        return sp.pack(self.model.seen)


ON = dict(max_episode_steps=LIMIT)
TWIN_CASES = {
    "block-occlusion": (PZR, 5, dict(occlusion=True), True),
    "block-cone": (PZR, 3, dict(fov=90), True),
    "block-both": (PZR, 5, dict(occlusion=True, fov=90), True),
    "block-bytes": (PZR, 4, dict(obs_u8=True, occlusion=True, fov=(180, 90)), True),
    "block-footprints-ego": (PZR, 3, dict(occlusion=True, fov=90, footprints=4, footprints_for="both", egocentric=True), True),
    "block-tracker-only": (PZR, 3, dict(occlusion=True), "tracker"),
    "block-target-only-ego": (PZR, 1, dict(fov=180, egocentric="both"), "target"),
    "maze-occlusion": (MAZE, 3, dict(occlusion=True), True),
    "maze-cone-ego": (MAZE, 1, dict(fov=90, egocentric=True), "both"),
    "rooms-both": (ROOMS, 3, dict(occlusion=True, fov=90), True),
    "ram-occlusion": (RAM, 3, dict(occlusion=True), True),
    "ram-cone-ego": (RAM, 5, dict(fov=90, egocentric=True), "tracker"),
    "moore-occlusion": (PZR, 3, dict(occlusion=True, action_type="Moore"), True),
    "no-auto-reset": (PZR, 3, dict(occlusion=True, auto_reset=False), True),
}


@pytest.mark.parametrize("case", list(TWIN_CASES))
def test_env_equals_its_twin(case):
    """VecEnv(map_memory=...) and a twin of the same id, seed and flags without it under the same 40 random actions, TimeLimit 13
    (every env restarts three times inside the run): rewards and done flags identical; every observation — reset(), observe()
    after it, every step(), observe() after the last step — equals the spec applied on the host to the twin's windows with the
    twin's positions, sides and maps (read after every call), and env._seen equals the host's sets after every step, bit for bit;
    observe() leaves env._seen as it was. Where the env is egocentric the twin is not: it takes the env's absolute actions, and the
    env's window equals the spec's window turned by the env's facing. Without the auto-reset no done flag reaches the pass, and a
    reset() half way empties every tile. A scripted (Ram) target's window and tile are never touched. 7s and 8s both occur."""
    from active_tracking_rl_amd.environment import VecEnv
    env_id, n, kw, who = TWIN_CASES[case]
    steps = 40
    ego = kw.get("egocentric")
    twin_kw = {k: v for k, v in kw.items() if k != "egocentric"}
    env = VecEnv(env_id, n, device=DEV, seed=9, map_memory=who, **kw, **ON)
    twin = VecEnv(env_id, n, device=DEV, seed=9, **twin_kw, **ON)
    try:
        scripted = env_id == RAM
        roles = 1 if scripted and who is True else {True: 3, "tracker": 1, "target": 2, "both": 3}[who]
        ego_roles = 0 if not ego else 1 if scripted else 3
        assert env._memory_roles == roles and env.map_memory == {1: "tracker", 2: "target", 3: "both"}[roles]
        assert twin.map_memory is None and twin._seen is None and env._ego_roles == ego_roles
        assert env._seen.shape == (n, 2, 256) and env._seen.dtype == torch.uint32 and not _tiles(env._seen).any()
        assert env.obs_u8 == twin.obs_u8 == bool(kw.get("obs_u8"))
        address = env._seen.data_ptr()
        bufs = twin.rollout_buffers(1)
        assert env.fused_step_out(tuple(b[0] for b in (bufs[0][1:], bufs[1], bufs[2]))) is None
        host = _Host(twin, roles)
        auto = kw.get("auto_reset", True)
        raw = lambda o: o.cpu().numpy().reshape(n, 2, 13, 13)

        def same(got, want, what):
            if ego_roles:
                want = ego_spec.view_all(want, env._facing.cpu().numpy(), ego_roles)
            g = got.cpu().numpy()
            assert g.dtype == (np.uint8 if env.obs_u8 else np.float32) and g.shape == (n, 2, 1, 1, 13, 13), what
            assert np.array_equal(g.reshape(n, 2, 13, 13), want.astype(g.dtype)), what
            assert np.array_equal(_tiles(env._seen), host.tiles()), what

        same(env.reset(), host.begin(raw(twin.reset())), "reset")
        same(env.observe(), host.keep(raw(twin.observe())), "observe after reset")
        gen = torch.Generator(device=DEV)
        gen.manual_seed(4)
        acts = torch.randint(0, 8 if "action_type" in kw else 4, (steps, 2, n), device=DEV, generator=gen)
        ends = sevens = eights = 0
        for t in range(steps):
            if not auto and t == steps // 2:
                same(env.reset(), host.begin(raw(twin.reset())), "reset half way")
            a = [acts[t, 0]] if scripted else [acts[t, 0], acts[t, 1]]
            o, r, d, _ = env.step(a)
            if ego_roles:           # the twin takes the absolute moves the env made of the relative ones
                ab = env._ego_abs[torch.int64]
                a = [ab[0].clone()] if scripted else [ab[0].clone(), ab[1].clone()]
            p, r2, d2, _ = twin.step(a)
            assert torch.equal(r, r2) and torch.equal(d, d2), t
            dh = d2.cpu().numpy()
            plain = raw(p)
            want = host.step(plain, dh)
            same(o, want, "step %d" % t)
            assert np.array_equal(want[plain != 5], plain[plain != 5]) and set(np.unique(want[plain == 5])) <= {5, 7, 8}, t
            for q in range(2):
                if not (roles >> q) & 1:
                    assert np.array_equal(want[:, q], plain[:, q]) and not _tiles(env._seen)[:, q].any(), t
            ends += int(dh.astype(bool).sum())
            sevens += int((want == 7).sum())
            eights += int((want == 8).sum())
            if twin._facing is not None:
                assert torch.equal(env._facing, twin._facing), t
        before = _tiles(env._seen).copy()
        same(env.observe(), host.keep(raw(twin.observe())), "observe after the walk")
        assert np.array_equal(_tiles(env._seen), before) and env._seen.data_ptr() == address
        cells = env.seen_cells()
        side = env.core.map_side
        assert cells.dtype == torch.bool and tuple(cells.shape) == (n, 2, side, side)
        assert np.array_equal(cells.cpu().numpy(), host.model.seen[:, :, :side, :side]) and not host.model.seen[:, :, side:].any()
        print("%s: %d episode ends in %d steps x %d envs, %d cells read 7, %d read 8" % (case, ends, steps, n, sevens, eights))
        assert sevens > 0 and eights > 0 and ends >= (3 * n if auto else 1)
        assert env.core.faults() == 0 and twin.core.faults() == 0
    finally:
        env.close()
        twin.close()


def test_observe_after_a_step_is_the_steps_observation():
    from active_tracking_rl_amd.environment import VecEnv
    n = 5
    env = VecEnv(PZR, n, device=DEV, seed=2, occlusion=True, fov=90, map_memory=True, **ON)
    try:
        gen = torch.Generator(device=DEV)
        gen.manual_seed(3)
        acts = torch.randint(0, 4, (20, 2, n), device=DEV, generator=gen)
        env.reset()
        painted = 0
        for t in range(20):
            o, _, _, _ = env.step([acts[t, 0], acts[t, 1]])
            o = o.clone()
            tiles = _tiles(env._seen).copy()
            assert torch.equal(env.observe(), o) and np.array_equal(_tiles(env._seen), tiles), t
            assert torch.equal(env.observe(), o) and _tiles(env._seen).tobytes() == tiles.tobytes(), t
            painted += int(((o == 7) | (o == 8)).sum())
        assert painted > 0 and env.core.faults() == 0
    finally:
        env.close()


def test_clone_and_restore_repeat_a_continuation():
    """10 steps, clone_state(), 12 more steps recorded (episodes end in between), restore_state(): the tiles are the clone's, in
    the same tensor, and the same 12 actions give the same observations, rewards, done flags and tiles bit for bit. A masked
    restore puts back the masked envs' tiles only."""
    from active_tracking_rl_amd.environment import VecEnv
    n = 5
    env = VecEnv(PZR, n, device=DEV, seed=3, occlusion=True, map_memory="both", **ON)
    try:
        gen = torch.Generator(device=DEV)
        gen.manual_seed(11)
        acts = torch.randint(0, 4, (22, 2, n), device=DEV, generator=gen)
        i32 = lambda t: t.view(torch.int32)
        env.reset()
        for t in range(10):
            env.step([acts[t, 0], acts[t, 1]])
        state = env.clone_state()
        at_clone = i32(env._seen.clone())
        address = env._seen.data_ptr()
        assert (at_clone != 0).any() and state["seen"] is not env._seen

        def walk():
            out = []
            for t in range(10, 22):
                o, r, d, _ = env.step([acts[t, 0], acts[t, 1]])
                out.append((o.clone(), r.clone(), d.clone(), i32(env._seen.clone())))
            return out
        first = walk()
        assert sum(int(x[2].sum()) for x in first) > 0 and not torch.equal(i32(env._seen), at_clone)
        env.restore_state(state)
        assert torch.equal(i32(env._seen), at_clone) and env._seen.data_ptr() == address
        for a, b in zip(first, walk()):
            assert all(torch.equal(x, y) for x, y in zip(a, b))
        moved = i32(env._seen.clone())
        mask = torch.arange(n, device=DEV) % 3 == 0
        env.restore_state(state, mask=mask)
        assert torch.equal(i32(env._seen)[mask], at_clone[mask]) and torch.equal(i32(env._seen)[~mask], moved[~mask])
        assert not torch.equal(at_clone[~mask], moved[~mask]) and env._seen.data_ptr() == address
        assert env.core.faults() == 0
    finally:
        env.close()


def test_shard_state_round_trip(tmp_path):
    """64 envs, num_steps=5, through train.make_player and train.rollout. Player P: two rollouts, shard_state() — which holds the
    tiles as env_seen — saved and loaded as a file, a third rollout. A second player Q built the same way loads the file: the tiles
    land in its env's own tensor, and its next rollout's store and tiles equal P's third bit for bit."""
    from active_tracking_rl_amd.train import default_args, make_player, rollout

    def player():
        args = default_args(env=PZR, network="tat-maze-lstm", aux="reward", num_envs=64, num_steps=5, seed=23, occlusion=True,
                            map_memory=True)
        args.gpu_ids = [0]
        return make_player(args, torch.device(DEV))[0]
    P, Q = player(), player()
    try:
        assert P.env._memory_roles == 3 and Q.env._seen is not P.env._seen
        for _ in range(2):
            rollout(P, 5)
            P.clear_actions()
        torch.cuda.synchronize()
        d = P.shard_state()
        at_save = _tiles(P.env._seen).copy()
        assert d["env_seen"].dtype == torch.uint32 and not d["env_seen"].is_cuda and np.array_equal(_tiles(d["env_seen"]), at_save)
        assert at_save.any()
        path = str(tmp_path / "shard.pt")
        torch.save(d, path)
        rollout(P, 5)
        torch.cuda.synchronize()
        address = Q.env._seen.data_ptr()
        Q.load_shard_state(torch.load(path, weights_only=False))
        assert Q.env._seen.data_ptr() == address and np.array_equal(_tiles(Q.env._seen), at_save)
        rollout(Q, 5)
        torch.cuda.synchronize()
        for i, (x, y) in enumerate(zip(Q._buf, P._buf)):
            assert torch.equal(x, y), i
        assert np.array_equal(_tiles(Q.env._seen), _tiles(P.env._seen)) and not np.array_equal(_tiles(P.env._seen), at_save)
        assert ((P._buf[0] == 7) | (P._buf[0] == 8)).any()
        with pytest.raises(ValueError, match="saved seen tiles have shape"):
            Q.load_shard_state(dict(d, env_seen=d["env_seen"][:32]))
    finally:
        P.env.close()
        Q.env.close()


@pytest.mark.parametrize("rng", ["philox", "numpy"])
@pytest.mark.parametrize("env_id", [PZR, NAV], ids=["pzr", "nav"])
def test_gym_protocol_env_equals_its_twin(env_id, rng):
    """Track2DEnv(map_memory=True) under the reference's gym protocol, on the device generators and in the reference-exact mode
    (whose reset goes through t2d_inject and observe(), a path of its own), with a model-driven and with a scripted (Nav) target:
    two episodes of reset and 15 steps against a twin of the same seed and flags without memory — observations equal the spec of
    the twin's, rewards, done flags and distances are the twin's, every reset starts from empty tiles (a reset observation is
    the twin's: nothing is remembered yet)."""
    from active_tracking_rl_amd.environment import Track2DEnv
    env = Track2DEnv(env_id, device=DEV, seed=3, rng=rng, occlusion=True, fov=90, map_memory=True)
    twin = Track2DEnv(env_id, device=DEV, seed=3, rng=rng, occlusion=True, fov=90)
    try:
        roles = 3 if env_id == PZR else 1
        assert env.vec._memory_roles == roles
        host = _Host(twin.vec, roles)
        rs = np.random.RandomState(2)
        painted = 0
        for episode in range(2):
            o, p = env.reset(), twin.reset()
            assert o.dtype == p.dtype == np.float32 and o.shape == p.shape == (2, 1, 1, 13, 13)
            assert np.array_equal(o.reshape(1, 2, 13, 13), host.begin(p.reshape(1, 2, 13, 13))), (episode, "reset")
            assert np.array_equal(o, p) and np.array_equal(_tiles(env.vec._seen), host.tiles())
            for t in range(15):
                a = rs.randint(0, 4, 2)
                o, r, d, info = env.step(a)
                p, r2, d2, info2 = twin.step(a)
                want = host.step(p.reshape(1, 2, 13, 13), None)
                assert np.array_equal(o.reshape(1, 2, 13, 13), want), (episode, t)
                assert np.array_equal(_tiles(env.vec._seen), host.tiles()), (episode, t)
                assert np.array_equal(r, r2) and d == d2 and info["distance"] == info2["distance"]
                painted += int((o != p).sum())
                if d:
                    break
        assert painted > 0
    finally:
        env.close()
        twin.close()


def test_five_steps_captured_in_one_graph_replay_with_fresh_actions():
    """Five VecEnv.step calls on static action tensors inside one torch.cuda.graph, replayed three times with fresh actions
    copied in: all fifteen observations, with rewards, done flags and the tiles after each replay, equal the spec on a twin that
    takes the same fifteen steps eagerly. The tiles are state the replays carry."""
    from active_tracking_rl_amd.environment import VecEnv
    n, T, replays = 5, 5, 3
    kw = dict(occlusion=True, fov=90, **ON)
    env = VecEnv(PZR, n, device=DEV, seed=8, map_memory=True, **kw)
    twin = VecEnv(PZR, n, device=DEV, seed=8, **kw)
    try:
        host = _Host(twin, 3)
        raw = lambda o: o.cpu().numpy().reshape(n, 2, 13, 13)
        gen = torch.Generator(device=DEV)
        gen.manual_seed(12)
        fresh = torch.randint(0, 4, (replays + 1, T, 2, n), device=DEV, generator=gen)
        env.reset()
        host.begin(raw(twin.reset()))
        static = fresh[replays].clone()

        def five(e):
            out = [e.step([static[t, 0], static[t, 1]]) for t in range(T)]
            e.flush()
            return out

        def compare(got, k):
            """The twin takes the five steps one by one (its state is read after each), `got` is compared."""
            ends = painted = 0
            for t in range(T):
                p, r2, d2, _ = twin.step([static[t, 0], static[t, 1]])
                dh = d2.cpu().numpy()
                o, r, d, _ = got[t]
                want = host.step(raw(p), dh)
                assert np.array_equal(raw(o), want), (k, t)
                assert torch.equal(r, r2) and torch.equal(d, d2), (k, t)
                ends += int(dh.astype(bool).sum())
                painted += int((want >= 7).sum())
            twin.flush()
            assert np.array_equal(_tiles(env._seen), host.tiles()), k
            return ends, painted
        compare(five(env), "eager")        # (one eager pass first: code objects are loaded before the capture)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            outs = five(env)
        ends = painted = 0
        for k in range(replays):
            static.copy_(fresh[k])
            g.replay()
            torch.cuda.synchronize()
            e, p = compare(outs, k)
            ends, painted = ends + e, painted + p
        assert ends > 0 and painted > 0 and env.core.faults() == 0 and twin.core.faults() == 0
        del g
    finally:
        env.close()
        twin.close()


def _twin_walk(n, seed, actions, first):
    """A byte env with occlusion and without memory put into the state of the snapshot blob `first` and driven by `actions`
    [T, 2, N]: (obs u8 [T+1, N, 2, 13, 13], walls [T+1, N, 82, 82], pos [T+1, N, 2, 2], sides [T+1, N], rew [T, N, 2],
    done [T, N])."""
    from active_tracking_rl_amd.environment import VecEnv
    twin = VecEnv(PZR, n, device=DEV, seed=seed, obs_u8=True, occlusion=True)
    try:
        twin.reset()
        twin.core.snapshot().load_bytes(first).restore()
        raw = lambda o: o.cpu().numpy().reshape(n, 2, 13, 13)
        obs, walls, pos, sides, rew, done = [raw(twin.observe())], [], [], [], [], []

        def world():
            st = twin.core.get_state()
            walls.append(twin.core.get_maps() != 0)
            pos.append(st["pos"])
            sides.append(st["side"])
        world()
        for t in range(actions.shape[0]):
            o, r, d, _ = twin.step([actions[t, 0].contiguous(), actions[t, 1].contiguous()])
            obs.append(raw(o))
            world()
            rew.append(r.cpu().numpy())
            done.append(d.cpu().numpy())
        assert twin.core.faults() == 0
        return np.stack(obs), np.stack(walls), np.stack(pos), np.stack(sides), np.stack(rew), np.stack(done)
    finally:
        twin.close()


def _store_equals_the_spec(player, n, seed, blob, seen0, what):
    """The rollout store of `player` against its own twin: an occluded env without memory started from the snapshot `blob`, driven
    by the stored actions, remembered on the host from the sets the shard had before the rollout."""
    acts = player._cache.actions
    raw, walls, pos, sides, rew, done = _twin_walk(n, seed, acts, blob)
    model = sp.Model(n, 3)
    model.seen = np.array(seen0)
    want = [model.keep(raw[0], walls[0], pos[0], sides[0])]
    for t in range(acts.shape[0]):
        want.append(model.step(raw[t + 1], walls[t + 1], pos[t + 1], sides[t + 1], done[t]))
    obs, r, d = (b.cpu().numpy() for b in player._buf)
    assert obs.dtype == np.uint8 and np.array_equal(obs, np.stack(want)), what
    assert np.array_equal(r, rew) and np.array_equal(d, done), what
    assert np.array_equal(_tiles(player.env._seen), sp.pack(model.seen)), what
    assert (obs == 7).any() and (obs == 8).any() and (raw == 5).any()


@pytest.mark.parametrize("schedule", ["eager", "synchronous", "pipelined"])
def test_training_stores_what_the_players_see(schedule):
    """64 envs x 5 steps, tat-maze-lstm, occlusion and map memory: two iterations of the eager loop (rollout + optimize) and of
    each graphed schedule, with the memory launch inside the captured rollout. Every window of the second iteration's rollout store
    equals the spec applied to its own twin — an occluded env without memory put into the state the shard had before that
    iteration (a snapshot blob, and the tiles read at that moment) and driven by the iteration's stored actions; the env never
    takes the fused step; the bucket and the loss terms are finite and the env kernels flag no fault."""
    from active_tracking_rl_amd.train import GraphedIteration, PipelinedIteration, default_args, make_player, rollout
    n, T = 64, 5
    args = default_args(env=PZR, num_envs=n, num_steps=T, seed=2, network="tat-maze-lstm", aux="reward", train_mode=-1,
                        occlusion=True, map_memory=True)
    args.gpu_ids = [0]
    player, opt = make_player(args, torch.device(DEV), 0, 1)
    env = player.env
    try:
        assert env.map_memory == "both" and env._memory_roles == 3 and env.obs_u8 and env.occlusion

        def mark():
            torch.cuda.synchronize()
            seen = np.zeros((n, 2, S, S), bool)
            side = env.core.map_side
            seen[:, :, :side, :side] = env.seen_cells().cpu().numpy()
            return env.core.snapshot().save().to_bytes(), seen
        if schedule == "eager":
            optimize = lambda: player.optimize(None, opt, player.model, args.train_mode, torch.device(DEV))
            rollout(player, T)
            optimize()
            blob, seen0 = mark()
            rollout(player, T)
            torch.cuda.synchronize()
            last = player
            _store_equals_the_spec(last, n, args.seed, blob, seen0, schedule)
            stats = optimize()
        else:
            it = (GraphedIteration if schedule == "synchronous" else PipelinedIteration)(player, opt, args)
            it.run()
            it.finish()
            blob, seen0 = mark()
            stats = it.run()
            it.finish()
            torch.cuda.synchronize()
            last = it.player if schedule == "synchronous" else it.players[(it.i - 1) & 1]
            _store_equals_the_spec(last, n, args.seed, blob, seen0, schedule)
        torch.cuda.synchronize()
        assert not last.model.env_stepped and not last.model.env_step_fused_seen
        assert all(bool(torch.isfinite(s).all()) for s in stats)
        assert torch.isfinite(opt.bucket.flat).all() and torch.isfinite(opt.bucket.grad).all()
        assert env.core.faults() == 0
    finally:
        env.close()
