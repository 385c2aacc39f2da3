"""-m gpu: map banks (include/track2d_bank.h; csrc/track2d_hip.hip generate_episode, k_bank_index).

  (1) the selection rule: every env's map is bank[spec index] after the reset and after every step, through both pre-generated
      slots and several generator windows; map_index() says the same;
  (2) identity: an env whose bank map is the map the generator would have made gets the generator's episode, bit for bit
      (spawns, goals, target plans, observations, rewards, done flags) — k_gen, the Ram form, k_gen_nav; and a Nav handle above
      kGenNavMaxEnvs on the k_gen<NAV> form;
  (3) fixed spawn rows, and the sampler's invariants where there is none;
  (4) every refusal of t2d_map_bank_attach / t2d_map_bank_index, each leaving the handle usable;
  (5) the real paths: a captured training iteration, test.evaluate eager and graphed, VecEnv with occlusion and frame stacks;
  (6) a handle without a bank steps as it always did."""
import numpy as np
import pytest
import torch

import map_bank_spec as sp
from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BASE = 1000
PZR, RAM, NAV = "Track2D-BlockPartialPZR-v0", "Track2D-BlockPartialRam-v0", "Track2D-MazePartialNav-v0"


def _empty(side):
    m = np.ones((side, side), np.uint8)
    m[1:-1, 1:-1] = 0
    return m


def _corridor(side):
    """One corridor along row 40 with a short side arm: 80-odd free cells."""
    m = np.ones((side, side), np.uint8)
    m[40, 1:side - 1] = 0
    m[36:40, 17] = 0
    return m


def _pocket(side):
    """An empty room with a walled-off 3 x 3 pocket no path leads into."""
    m = _empty(side)
    m[9:14, 9:14] = 1
    m[10:13, 10:13] = 0
    return m


def _pillars(side):
    m = _empty(side)
    m[4:side - 4:6, 4:side - 4:5] = 1
    return m


def _blocks(side):
    m = _empty(side)
    m[20:30, 20:60] = 1
    m[50:52, 3:70] = 1
    return m


def hand_bank(count, side=82):
    makers = [_empty, _corridor, _pocket, _pillars, _blocks]
    return np.stack([makers[i](side) for i in range(count)])


def _handle(env_id, n, seed=11, base=BASE, max_steps=10, **kw):
    from active_tracking_rl_amd.vec_env import VecTrack2D
    return VecTrack2D(env_id, num_envs=n, device=DEV, seed=seed, env_id_base=base, max_episode_steps=max_steps, **kw)


def _actions(n, steps, seed=3):
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 4, size=(steps, 2, n))
    return [(torch.as_tensor(a[t, 0], dtype=torch.int64, device=DEV), torch.as_tensor(a[t, 1], dtype=torch.int64, device=DEV))
            for t in range(steps)]


def _check_maps(env, bank, select, seed, base=BASE):
    """Every env's map is the bank member the rule names for the episode it runs; map_index() names it too."""
    st = env.get_state()
    side = bank.shape[1]
    want = sp.indices(sp.SELECT[select], seed, base, st["episode"], bank.shape[0])
    maps = env.get_maps()
    assert np.array_equal(maps[:, :side, :side], bank[want])
    assert not maps[:, side:, :].any() and not maps[:, :, side:].any()
    assert np.array_equal(env.map_index().cpu().numpy(), want)
    return st, want


@pytest.mark.parametrize("select", ["cycle", "random"])
@pytest.mark.parametrize("n", [1, 5, 8])
@pytest.mark.parametrize("count", [1, 2, 3, 5])
def test_index_rule(count, n, select):
    """(1) reset + 45 steps with a 10-step TimeLimit: episodes switch in-launch at steps 10, 20, 30 and 40."""
    bank = hand_bank(count)
    env = _handle(PZR, n)
    assert env.map_bank_count == 0
    env.attach_map_bank(bank, select)
    assert env.map_bank_count == count
    env.reset()
    st, _ = _check_maps(env, bank, select, 11)
    assert (st["episode"] == 1).all()
    seen = set()
    for t, (a0, a1) in enumerate(_actions(n, 45)):
        _, _, done = env.step(a0, a1)
        st, idx = _check_maps(env, bank, select, 11)
        assert (st["episode"] == 1 + (t + 1) // 10).all() and bool(done.all()) == ((t + 1) % 10 == 0)
        seen.update(int(i) for i in idx)
    assert env.faults() == 0
    if select == "cycle":                      # (n + 4 consecutive residues over the five episodes: every map was served)
        assert seen == set(range(count))
    env.close()


def _record(env, n, steps, side, acts):
    """reset + `steps` steps: per step the observation, rewards and done flags, and at every step boundary the state."""
    rec = dict(obs=[env.reset().cpu().numpy()], rew=[], done=[], state=[], target=[], maps=[])

    def snap():
        rec["state"].append(env.get_state())
        rec["target"].append(env.get_target())
        rec["maps"].append(env.get_maps()[:, :side, :side])
    snap()
    for t in range(steps):
        obs, rew, done = env.step(*acts[t])
        rec["obs"].append(obs.cpu().numpy()); rec["rew"].append(rew.cpu().numpy()); rec["done"].append(done.cpu().numpy())
        snap()
    return rec


@pytest.mark.parametrize("env_id, n, side", [(PZR, 6, 82), (RAM, 6, 82), (NAV, 3, 81)])
def test_bank_map_equal_to_the_generated_map_gives_the_generated_episode(env_id, n, side):
    """(2) handle A generates; handle B (same arguments, same actions) runs a 6-map 'cycle' bank arranged so that in episode
    EP every env receives the map A generated for it. Throughout that episode B is A, bit for bit."""
    EP, K, steps = 3, 6, 32
    acts = _actions(n, steps, seed=5)
    a = _handle(env_id, n, seed=23)
    ra = _record(a, n, steps, side, acts)
    a.close()
    first = 10 * (EP - 1)                      # the step boundary at which episode EP stands in its first state
    assert (ra["state"][first]["episode"] == EP).all() and (ra["state"][first]["t"] == 0).all()
    assert all(d.all() == ((t + 1) % 10 == 0) and d.any() == d.all() for t, d in enumerate(ra["done"]))
    bank = np.stack([_empty(side)] * K)
    for e in range(n):
        bank[(BASE + e + EP) % K] = ra["maps"][first][e]
    b = _handle(env_id, n, seed=23)
    b.attach_map_bank(bank, "cycle")
    rb = _record(b, n, steps, side, acts)
    assert b.faults() == 0
    b.close()
    for k in range(first, first + 10):         # the boundaries of episode EP: its first state .. the state before its last step
        sa, sb = ra["state"][k], rb["state"][k]
        assert (sb["episode"] == EP).all()
        for key in ("pos", "goals", "c_far", "t", "d2", "side"):
            assert np.array_equal(sa[key], sb[key]), (k, key)
        for key in ("plan", "len", "cursor", "navgoal"):
            assert np.array_equal(ra["target"][k][key], rb["target"][k][key]), (k, key)
        assert np.array_equal(ra["maps"][k], rb["maps"][k])
        assert np.array_equal(ra["obs"][k], rb["obs"][k]), k                 # obs[k]: what the players see at boundary k
        assert np.array_equal(ra["rew"][k], rb["rew"][k]) and np.array_equal(ra["done"][k], rb["done"][k]), k
    # ... and B is not A elsewhere: the other episodes ran on other maps
    assert not np.array_equal(ra["maps"][0], rb["maps"][0])


def test_nav_above_the_workgroup_form_limit():
    """(2) 2052 Maze + Nav envs (above kGenNavMaxEnvs = 2048: the one-wave-per-episode generator with the Nav plans inside):
    reset + 12 steps; the index rule holds and every agent stands on a free cell of its bank map."""
    n, count = 2052, 5
    bank = hand_bank(count, 81)
    env = _handle(NAV, n, seed=7)
    env.attach_map_bank(bank, "random")
    env.reset()
    acts = _actions(n, 12, seed=9)
    for t in range(13):
        if t:
            env.step(*acts[t - 1])
        st = env.get_state()
        want = sp.indices(sp.RANDOM, 7, BASE, st["episode"], count)
        assert np.array_equal(env.map_index().cpu().numpy(), want)
        if t in (0, 9, 10, 12):
            assert np.array_equal(env.get_maps()[:, :81, :81], bank[want])
        assert (st["episode"] == (1 if t < 10 else 2)).all()
        m = bank[want]
        e = np.arange(n)
        assert not m[e, st["pos"][:, 0, 0], st["pos"][:, 0, 1]].any() and not m[e, st["pos"][:, 1, 0], st["pos"][:, 1, 1]].any()
        assert not m[e, st["goals"][:, 0, 0], st["goals"][:, 0, 1]].any() and not m[e, st["goals"][:, 1, 0], st["goals"][:, 1, 1]].any()
    assert set(int(i) for i in want) == set(range(count))
    assert env.faults() == 0
    env.close()


@pytest.mark.parametrize("env_id", [PZR, RAM])
def test_fixed_spawns(env_id):
    """(3) maps 0 and 2 carry a spawn row (map 2's is co-located), maps 1 and 3 sample as usual."""
    n, count = 8, 4
    bank = hand_bank(count)
    spawns = np.array([[5, 6, 70, 71], [-1, -1, -1, -1], [11, 11, 11, 11], [-1, -1, -1, -1]], np.int32)    # (11, 11): in the pocket
    from active_tracking_rl_amd.map_bank import MapBank
    env = _handle(env_id, n, seed=31)
    env.attach_map_bank(MapBank(bank, spawns), "cycle")
    env.reset()
    acts = _actions(n, 30, seed=2)
    fixed = sampled = 0
    for t in range(31):
        if t:
            env.step(*acts[t - 1])
        if t % 10:
            continue
        st = env.get_state()                   # every env stands in the first state of an episode
        assert (st["t"] == 0).all()
        idx = sp.indices(sp.CYCLE, 31, BASE, st["episode"], count)
        for e in range(n):
            m, (tr, tg), goals = bank[idx[e]], st["pos"][e], st["goals"][e]
            if (spawns[idx[e]] != -1).all():
                assert [int(v) for v in tr] + [int(v) for v in tg] == spawns[idx[e]].tolist()
                fixed += 1
            else:                              # sample_close_states: tracker on a free cell, target in the 2 x 2 block up-left of it
                assert m[tr[0], tr[1]] == 0 and m[tg[0], tg[1]] == 0
                assert 0 <= tr[0] - tg[0] <= 1 and 0 <= tr[1] - tg[1] <= 1
                sampled += 1
            g0, g1 = tuple(goals[0]), tuple(goals[1])
            assert m[g0] == 0 and m[g1] == 0 and g0 != g1 and tuple(tr) not in (g0, g1)
            assert st["d2"][e] == (tr[0] - tg[0]) ** 2 + (tr[1] - tg[1]) ** 2
    assert fixed >= 8 and sampled >= 8 and env.faults() == 0
    env.close()


def _refused(code, match, fn, *args):
    from active_tracking_rl_amd.vec_env import T2DError
    with pytest.raises(T2DError, match=r"\(%d\).*%s" % (code, match)):
        fn(*args)


def test_refusals_leave_the_handle_usable():
    """(4) T2D_ERR_INVALID (-1) and T2D_ERR_STATE (-4), straight at the C ABI."""
    import ctypes as C
    from active_tracking_rl_amd import map_bank, np_mode, registry
    L = map_bank.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    good = np.ascontiguousarray(hand_bank(3))
    env = _handle(PZR, 4)

    def attach(h, maps, spawns=None, count=None, side=None, select=0):
        maps = np.ascontiguousarray(maps, np.uint8)
        sp_ = None if spawns is None else ptr(np.ascontiguousarray(spawns, np.int32))
        keep.append((maps, spawns))
        return L.t2d_map_bank_attach(h, ptr(maps), sp_, maps.shape[0] if count is None else count,
                                     maps.shape[1] if side is None else side, select, None)
    keep = []
    _refused(-1, "null", L.t2d_map_bank_attach, None, ptr(good), None, 3, 82, 0, None)
    _refused(-1, "null", L.t2d_map_bank_attach, env.h, None, None, 3, 82, 0, None)
    for count in (0, -1, 65537):
        _refused(-1, "count", attach, env.h, good, None, count)
    for select in (-1, 2):
        _refused(-1, "select", attach, env.h, good, None, None, None, select)
    _refused(-1, "side 81", attach, env.h, hand_bank(3, 81))
    bad = good.copy(); bad[1, 7, 9] = 2
    _refused(-1, r"map 1: cell \(7, 9\) is 2", attach, env.h, bad)
    for r, c in ((0, 5), (81, 5), (5, 0), (5, 81)):
        bad = good.copy(); bad[2, r, c] = 0
        _refused(-1, r"map 2: border cell \(%d, %d\)" % (r, c), attach, env.h, bad)
    bad = good.copy(); bad[0] = 1; bad[0, 3, 3:5] = 0
    _refused(-1, "map 0: 2 free", attach, env.h, bad)
    bad[0, 3, 5] = 0                            # three free cells are enough (checked at the end: this bank attaches)
    three_free = bad
    none = [-1, -1, -1, -1]
    for row, why in (([5, 5, -1, -1], "neither all -1"), ([5, 5, 82, 5], "neither all -1"), ([-2, 5, 5, 5], "neither all -1"),
                     ([0, 0, 5, 5], "on a wall"), ([5, 5, 81, 81], "on a wall")):
        _refused(-1, "map 0: spawn row.*" + why, attach, env.h, good, [row, none, none])
    assert env.map_bank_count == 0
    # handles a bank cannot serve
    maze = _handle(NAV, 2)
    _refused(-1, "side 82", attach, maze.h, good)
    mixed = _handle(None, 2, map_type="Block", target_mode="PZR", map_type_per_env=np.array([0, 1], np.uint8))
    _refused(-1, "mixes sides", attach, mixed.h, good)
    _refused(-1, "mixes sides", attach, mixed.h, hand_bank(3, 81))
    rpf = _handle("Track2D-BlockPartialRPF-v0", 2)
    _refused(-1, "RPF", attach, rpf.h, good)
    ext = _handle(None, 2, map_type="Block", target_mode="PZR",
                  target_mode_per_env=np.array([registry.TARGET_CODE["PZR"], registry.TARGET_CODE["Ext"]], np.uint8))
    _refused(-1, "EXT", attach, ext.h, good)
    npy = _handle(PZR, 2)
    np_mode.attach_device_streams(npy, [1, 2])
    _refused(-1, "numpy streams", attach, npy.h, good)
    for h in (maze, mixed, rpf, ext, npy):
        assert h.map_bank_count == 0
        h.reset()                                # (still a working handle)
        h.close()
    # state
    idx = torch.zeros(4, dtype=torch.int32, device=DEV)
    _refused(-4, "no map bank", L.t2d_map_bank_index, env.h, C.c_void_p(idx.data_ptr()), None)
    _refused(-1, "null", L.t2d_map_bank_index, env.h, None, None)
    assert attach(env.h, three_free, [[3, 3, 3, 5], none, none]) == 0 and env.map_bank_count == 3
    _refused(-4, "already has", attach, env.h, good)
    _refused(-4, "t2d_reset first", L.t2d_map_bank_index, env.h, C.c_void_p(idx.data_ptr()), None)
    with pytest.raises(np_mode.NpError, match="map bank"):
        np_mode.attach_device_streams(env, [1, 2, 3, 4])
    env.reset()
    st = env.get_state()
    want = sp.indices(sp.CYCLE, 11, BASE, st["episode"], 3)
    assert np.array_equal(env.get_maps(), three_free[want]) and np.array_equal(env.map_index().cpu().numpy(), want)
    for e in np.nonzero(want == 0)[0]:
        assert st["pos"][e].reshape(-1).tolist() == [3, 3, 3, 5]
    a0, a1 = _actions(4, 1)[0]
    env.step(a0, a1)
    assert env.faults() == 0
    env.close()
    late = _handle(PZR, 2)
    late.reset()
    _refused(-4, "before the first", attach, late.h, good)
    late.step(*_actions(2, 1)[0])
    late.close()
    inj = _handle(PZR, 2, auto_reset=False)
    inj.inject(good[0], [5, 5, 6, 6], first=0)
    _refused(-4, "before the first", attach, inj.h, good)
    inj.close()


def test_captured_training_iteration_on_a_bank():
    """(5) GraphedIteration on 64 PZR envs with a 4-map bank, three replayed iterations: the generator launches inside the
    captured rollout hold the bank argument; afterwards every env's map is the bank member the rule names."""
    from active_tracking_rl_amd.map_bank import MapBank
    from active_tracking_rl_amd.train import GraphedIteration, default_args, make_player
    dev = torch.device(DEV)
    bank = MapBank(hand_bank(4))
    args = default_args(env=PZR, num_envs=64, seed=3, map_bank=bank, bank_select="random")
    player, opt = make_player(args, dev)
    core = player.env.core
    assert core.map_bank_count == 4
    it = GraphedIteration(player, opt, args)
    for _ in range(3):
        it.run()
    torch.cuda.synchronize()
    st = core.get_state()
    want = sp.indices(sp.RANDOM, 3, 0, st["episode"], 4)
    assert np.array_equal(core.get_maps(), bank.maps[want])
    assert np.array_equal(core.map_index().cpu().numpy(), want)
    assert core.faults() == 0
    assert torch.isfinite(opt.bucket.flat).all()
    player.env.close()


def test_evaluate_on_a_bank_eager_and_graphed():
    """(5) test.evaluate with --eval-map-bank: 8 episodes; info['map_index'] is (eval_env_id_base + e + episode) mod K with
    episode = 1, the first episode of every evaluation env. The eager round and the graphed one take the argmax of the same
    policy on the same episodes (the fixture policy's actor rows are scaled so that no near tie decides an action:
    tests/greedy_eval_spec.py), so lengths and returns are equal."""
    import greedy_eval_spec as gs
    from active_tracking_rl_amd.map_bank import MapBank
    from active_tracking_rl_amd.test import evaluate
    env_id = "Track2D-BlockPartialNav-v0"
    bank = MapBank(hand_bank(5))
    args = gs.fixture_args(env_id, 8, eval_map_bank=bank, map_bank=None, bank_select="random")
    model = gs.fixture_model(args, DEV)
    want = (gs.EVAL_BASE + np.arange(8) + 1) % 5
    out = {}
    for graphed in (False, True):
        info = {}
        rsum, length = evaluate(model, env_id, args, torch.device(DEV), 8, graphed=graphed, info=info)
        assert rsum.shape == (8, 2) and length.shape == (8,) and (length >= 1).all()
        assert np.array_equal(info["map_index"], want) and info["map_index"].dtype == np.int32
        out[graphed] = (rsum, length)
    assert np.array_equal(out[False][1], out[True][1]) and np.array_equal(out[False][0], out[True][0])


def test_vecenv_with_bank_occlusion_and_frame_stack():
    """(5) VecEnv(map_bank=..., occlusion=True, stack_frames=2) resets and steps; the maps are the bank's."""
    from active_tracking_rl_amd.environment import VecEnv
    bank = hand_bank(3)
    env = VecEnv(PZR, 6, device=DEV, seed=4, env_id_base=BASE, map_bank=bank, bank_select="cycle", occlusion=True, stack_frames=2,
                 max_episode_steps=10)
    obs = env.reset()
    assert tuple(obs.shape) == (6, 2, 2, 1, 13, 13) and env.map_bank.count == 3
    for a0, a1 in _actions(6, 12):
        obs, rew, done, _ = env.step([a0, a1])
        assert tuple(obs.shape) == (6, 2, 2, 1, 13, 13) and torch.isfinite(rew).all()
    st = env.core.get_state()
    want = sp.indices(sp.CYCLE, 4, BASE, st["episode"], 3)
    assert (st["episode"] == 2).all() and np.array_equal(env.core.get_maps(), bank[want])
    assert np.array_equal(env.map_index().cpu().numpy(), want) and env.core.faults() == 0
    env.close()


@pytest.mark.parametrize("env_id", [PZR, NAV])
def test_no_bank_no_change(env_id):
    """(6) a handle on which only t2d_map_bank_count was called steps bit-identically to one on which nothing was."""
    n = 6
    a, b = _handle(env_id, n, seed=17), _handle(env_id, n, seed=17)
    assert b.map_bank_count == 0
    oa, ob = a.reset(), b.reset()
    assert torch.equal(oa, ob)
    for a0, a1 in _actions(n, 25):
        ra, rb = a.step(a0, a1), b.step(a0, a1)
        assert b.map_bank_count == 0
        assert all(torch.equal(x, y) for x, y in zip(ra, rb))
    sa, sb = a.get_state(), b.get_state()
    assert all(np.array_equal(sa[k], sb[k]) for k in sa) and np.array_equal(a.get_maps(), b.get_maps())
    assert (sa["episode"] == 3).all()
    a.close(); b.close()
