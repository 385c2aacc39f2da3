"""-m gpu: Rooms maps (include/track2d.h T2D_MAP_ROOMS; csrc/t2d_device.h gen_rooms) against the plain-Python rule of
tests/rooms_spec.py. Every comparison is for equality.

  (1) the maps of 9 envs over four episodes (in-launch auto-reset, both pre-generated slots) equal the spec's, cell for cell;
  (2) a Rooms env and a Block-id twin that runs a 'cycle' bank of the spec's maps give the same episode: observations, rewards,
      done flags — spawns, goals and Nav plans follow from the tile alone, on the path the oracle tests already pin;
  (3) a handle that mixes Block and Rooms envs: the Block envs are an all-Block handle's, the Rooms envs the spec's;
  (4) 'Full' observations are the spec map with 2 and 4 at the agents' cells;
  (5) the refusals: Rooms with an RPF target, numpy streams on a Rooms handle;
  (6) through the product: both captured training schedules, and `map_bank make`;
  (7) snapshots: the identity check takes map_type 3, a Rooms handle rewinds and a twin continues from the blob.

An episode's number is the device's own counter, get_state()['episode']: 1 for the episode a reset starts, then 2, 3, ... —
the number the bank rule (include/track2d_bank.h: (global env id + episode) mod K) uses too."""
import functools

import numpy as np
import pytest
import torch

import rooms_spec as rs
from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 1234567


@functools.lru_cache(maxsize=None)
def spec_map(seed, genv, episode, level):
    g = rs.rooms_map(seed, genv, episode, level)
    g.setflags(write=False)
    return g


def _handle(env_id, n, seed=SEED, base=0, max_steps=500, **kw):
    from active_tracking_rl_amd.vec_env import VecTrack2D
    return VecTrack2D(env_id, num_envs=n, device=DEV, seed=seed, env_id_base=base, max_episode_steps=max_steps, **kw)


def _actions(n, steps, seed=3):
    a = np.random.RandomState(seed).randint(0, 4, size=(steps, 2, n))
    return [(torch.as_tensor(a[t, 0], dtype=torch.int64, device=DEV), torch.as_tensor(a[t, 1], dtype=torch.int64, device=DEV))
            for t in range(steps)]


@pytest.mark.parametrize("level", [0, 1, 4, 15])
def test_maps_equal_the_spec_through_episode_turnover(level):
    """(1) 9 envs (odd; more than one workgroup's four waves) at global ids 4090 .. 4098, a 3-step TimeLimit: after the reset and
    after 3, 6 and 9 steps every env stands in the first state of its 1st .. 4th episode on the spec's map of that episode."""
    n, base = 9, 4090
    env = _handle("Track2D-RoomsPartialPZR-v%d" % level, n, base=base, max_steps=3)
    env.reset()
    acts = _actions(n, 9)
    for k in range(4):
        for t in range(3 * (k - 1), 3 * k) if k else ():
            _, _, done = env.step(*acts[t])
            assert bool(done.all()) == (t % 3 == 2) and bool(done.any()) == bool(done.all())
        st = env.get_state()
        assert (st["episode"] == 1 + k).all() and (st["t"] == 0).all() and (st["side"] == 82).all()
        maps = env.get_maps()
        for e in range(n):
            want = spec_map(SEED, base + e, 1 + k, level)
            assert np.array_equal(maps[e], want), (k, e)
            (tr, tg), goals = st["pos"][e], st["goals"][e]
            assert want[tr[0], tr[1]] == 0 and want[tg[0], tg[1]] == 0
            assert want[goals[0][0], goals[0][1]] == 0 and want[goals[1][0], goals[1][1]] == 0
    assert env.faults() == 0
    env.close()


@pytest.mark.parametrize("mode, level", [("PZR", 1), ("Nav", 0)])
@pytest.mark.parametrize("base", [0, 7, 4095])
def test_episode_equals_a_bank_twin(base, mode, level):
    """(2) One env, a 5-step TimeLimit, 20 steps of fixed random actions: the reset starts episode 1 and the 20th step returns the
    first observation of episode 5. The twin is a Block-id handle of the same seed and base with a 'cycle' bank in which index
    (genv + ep) mod K holds the spec's map of (genv, ep). K = 5, not 4: the five episodes whose observations are compared need
    five different bank members (with four, episode 5 would be served episode 1's map)."""
    K, steps = 5, 20
    rooms = _handle("Track2D-RoomsPartial%s-v%d" % (mode, level), 1, base=base, max_steps=5)
    twin = _handle("Track2D-BlockPartial%s-v0" % mode, 1, base=base, max_steps=5)
    bank = np.zeros((K, 82, 82), np.uint8)
    for ep in range(1, K + 1):
        bank[(base + ep) % K] = spec_map(SEED, base, ep, level)
    twin.attach_map_bank(bank, "cycle")
    oa, ob = rooms.reset(), twin.reset()
    assert torch.equal(oa, ob)
    ended = 0
    for t, (a0, a1) in enumerate(_actions(1, steps, seed=11 + base)):
        ra, rb = rooms.step(a0, a1), twin.step(a0, a1)
        for x, y, what in zip(ra, rb, ("obs", "rew", "done")):
            assert torch.equal(x, y), (t, what)
        ended += int(ra[2].sum())
        sa, sb = rooms.get_state(), twin.get_state()
        for key in ("pos", "goals", "c_far", "t", "episode", "d2", "side"):
            assert np.array_equal(sa[key], sb[key]), (t, key)
        assert np.array_equal(rooms.get_maps(), twin.get_maps()), t
        ta, tb = rooms.get_target(), twin.get_target()
        assert all(np.array_equal(ta[k], tb[k]) for k in ta), t
    assert ended == 4 and int(sa["episode"][0]) == 5              # (the TimeLimit: 11 far steps do not fit into 5)
    assert rooms.faults() == 0 and twin.faults() == 0
    rooms.close(); twin.close()


def test_mixed_block_and_rooms_handle():
    """(3) 8 envs alternating Block / Rooms at level 1."""
    from active_tracking_rl_amd import registry
    n, base = 8, 100
    mt = np.array([registry.MAP_CODE["Block"] if e % 2 == 0 else registry.MAP_CODE["Rooms"] for e in range(n)], np.uint8)
    mixed = _handle("Track2D-BlockPartialPZR-v1", n, base=base, map_type_per_env=mt)
    block = _handle("Track2D-BlockPartialPZR-v1", n, base=base)
    om, ob = mixed.reset(), block.reset()
    mm, mb = mixed.get_maps(), block.get_maps()
    blk = np.arange(0, n, 2)
    assert torch.equal(om[blk], ob[blk]) and np.array_equal(mm[blk], mb[blk])
    for e in range(1, n, 2):
        assert np.array_equal(mm[e], spec_map(SEED, base + e, 1, 1)), e
    assert (mixed.get_state()["side"] == 82).all()
    for t, (a0, a1) in enumerate(_actions(n, 10, seed=8)):
        rm, rb = mixed.step(a0, a1), block.step(a0, a1)
        for x, y in zip(rm, rb):
            assert torch.equal(x[blk], y[blk]), t
    assert np.array_equal(mixed.get_maps()[blk], block.get_maps()[blk])
    assert mixed.faults() == 0
    mixed.close(); block.close()


def test_full_observations():
    """(4) 2 envs of Track2D-RoomsFullPZR-v1: both planes of the reset observation are the spec map, 2 at the tracker's cell,
    4 at the target's (painted last)."""
    env = _handle("Track2D-RoomsFullPZR-v1", 2, base=31)
    obs = env.reset().cpu().numpy()
    st = env.get_state()
    assert obs.shape == (2, 2, 82, 82) and obs.dtype == np.float32
    for e in range(2):
        want = spec_map(SEED, 31 + e, 1, 1).astype(np.float32)
        (tr, tg) = st["pos"][e]
        want[tr[0], tr[1]] = 2.0
        want[tg[0], tg[1]] = 4.0
        assert np.array_equal(obs[e, 0], want) and np.array_equal(obs[e, 1], want)
    env.close()


def test_refusals():
    """(5) with the library's text."""
    from active_tracking_rl_amd import np_mode, registry
    from active_tracking_rl_amd.vec_env import T2DError
    with pytest.raises(T2DError, match=r"error -1: t2d_create: Rooms maps have no RPF patrol target \(env 0\)"):
        _handle(None, 2, map_type="Rooms", target_mode="RPF")
    modes = np.array([registry.TARGET_CODE["PZR"], registry.TARGET_CODE["RPF"]], np.uint8)
    with pytest.raises(T2DError, match=r"Rooms maps have no RPF patrol target \(env 1\)"):
        _handle(None, 2, map_type="Rooms", target_mode="PZR", target_mode_per_env=modes)
    with pytest.raises(T2DError, match=r"t2d_create: map_type 4"):
        _handle(None, 2, map_type="Block", target_mode="PZR", map_type_per_env=np.array([0, 4], np.uint8))
    env = _handle("Track2D-RoomsPartialPZR-v0", 2)
    with pytest.raises(np_mode.NpError, match="t2d_np_attach: the handle has Rooms maps"):
        np_mode.attach_device_streams(env, [1, 2])
    mixed = _handle("Track2D-BlockPartialPZR-v0", 2, map_type_per_env=np.array([0, 3], np.uint8))
    with pytest.raises(np_mode.NpError, match="t2d_np_attach: the handle has Rooms maps"):
        np_mode.attach_device_streams(mixed, [1, 2])
    for h in (env, mixed):                        # still working handles
        h.reset()
        h.step(*_actions(2, 1)[0])
        assert h.faults() == 0
        h.close()


def test_snapshot_identity_accepts_rooms_handles():
    """The snapshot's identity check (csrc/state_hip.hip: a hash over cfg) takes map_type 3: a Rooms handle rewinds to its own
    snapshot, a twin handle continues from the blob, and a Block handle of the same shape refuses it."""
    from active_tracking_rl_amd.vec_env import T2DError
    n, base, acts = 5, 40, _actions(5, 12, seed=4)
    env = _handle("Track2D-RoomsPartialPZR-v0", n, base=base, max_steps=4)
    env.reset()
    for a in acts[:2]:
        env.step(*a)
    snap = env.snapshot().save()
    st0, maps0 = env.get_state(), env.get_maps()
    outs = [env.step(*a) for a in acts[2:]]
    assert (env.get_state()["episode"] == 4).all()           # 12 steps of a 4-step TimeLimit
    snap.restore()
    st1 = env.get_state()
    assert all(np.array_equal(st0[k], st1[k]) for k in st0) and np.array_equal(maps0, env.get_maps())
    for a, want in zip(acts[2:], outs):
        assert all(torch.equal(x, y) for x, y in zip(env.step(*a), want))
    twin = _handle("Track2D-RoomsPartialPZR-v0", n, base=base, max_steps=4)
    twin.reset()
    twin.snapshot().load_bytes(snap.to_bytes()).restore()
    assert np.array_equal(maps0, twin.get_maps())
    for a, want in zip(acts[2:], outs):
        assert all(torch.equal(x, y) for x, y in zip(twin.step(*a), want))
    for e in range(n):
        assert np.array_equal(twin.get_maps()[e], spec_map(SEED, base + e, 4, 0)), e
    block = _handle("Track2D-BlockPartialPZR-v0", n, base=base, max_steps=4)
    block.reset()
    with pytest.raises(T2DError, match="the blob's cfg differs from the handle's"):
        block.snapshot().load_bytes(snap.to_bytes())
    assert env.faults() == 0 and twin.faults() == 0
    env.close(); twin.close(); block.close()


def _train(schedule):
    from active_tracking_rl_amd.train import GraphedIteration, PipelinedIteration, default_args, make_player
    args = default_args(env="Track2D-RoomsPartialPZR-v0", num_envs=64, num_steps=5, seed=3)
    player, opt = make_player(args, torch.device(DEV))
    try:
        it = (GraphedIteration if schedule == "synchronous" else PipelinedIteration)(player, opt, args)
        for _ in range(3):
            it.run()
        it.finish()
        torch.cuda.synchronize()
        agents = [player] if schedule == "synchronous" else it.players
        stores = [b.detach().clone() for a in agents for b in a._buf]
        core = player.env.core
        st = core.get_state()
        maps = core.get_maps()
        for e in range(0, 64, 9):
            assert np.array_equal(maps[e], spec_map(3, e, int(st["episode"][e]), 0)), e
        return opt.bucket.flat.detach().clone(), stores, core.faults()
    finally:
        player.env.close()


@pytest.mark.parametrize("schedule", ["synchronous", "pipelined"])
def test_training_on_rooms_maps(schedule):
    """(6) 64 envs x 5 steps of Track2D-RoomsPartialPZR-v0, 3 iterations under captured graphs: finite weights, no fault word,
    and two runs with one seed leave equal rollout stores (and weights)."""
    wa, sa, fa = _train(schedule)
    wb, sb, fb = _train(schedule)
    assert fa == 0 and fb == 0
    assert torch.isfinite(wa).all() and torch.equal(wa, wb)
    assert len(sa) == len(sb) >= 3 and all(torch.equal(x, y) for x, y in zip(sa, sb))
    assert all(torch.isfinite(x.float()).all() for x in sa)


def test_map_bank_make_on_a_rooms_id(tmp_path):
    """(6) `python -m active_tracking_rl_amd.map_bank make` turns generated floor plans into an editable .txt bank."""
    from active_tracking_rl_amd import map_bank
    out = str(tmp_path / "rooms.txt")
    assert map_bank.main(["make", "--env", "Track2D-RoomsPartialNav-v1", "--count", "3", "--seed", "5", "--out", out,
                          "--device", DEV]) == 0
    bank = map_bank.MapBank.load(out)
    assert bank.count == 3 and bank.side == 82
    for e in range(3):
        assert np.array_equal(bank.maps[e], spec_map(5, e, 1, 1)), e
