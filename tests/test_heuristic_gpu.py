"""-m gpu: the heuristic players on the device (include/track2d_heuristic.h, csrc/heuristic_hip.hip k_heuristic) against the
specification (tests/heuristic_spec.py) fed with get_maps() and get_state() of the same handle. Every comparison is exact.

  (1) hand-made maps injected at sides 82 and 81; (2) generated episodes with in-launch restarts; (3) roles; (4) no side effect;
  (5) the call inside a replayed graph; (6) refusals; (7) Agent.action_test; (8) a derived property of a whole evaluation round;
  (9) the command lines."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import greedy_eval_spec as gs
import heuristic_spec as hs
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7


def _spec(env):
    st = env.get_state()
    return hs.batch(env.get_maps(), st["pos"], st["side"])


def _check(env, **kw):
    """One call for both roles against the spec for the handle's current state; returns (act, dist) as numpy."""
    want_act, want_dist = _spec(env)
    act, dist = env.heuristic_actions(**kw)
    act, dist = act.cpu().numpy(), dist.cpu().numpy()
    assert act.dtype == np.int64 and dist.dtype == np.int32
    bad = np.nonzero((act != want_act).any(1) | (dist != want_dist))[0]
    assert bad.size == 0, (bad[:8], act[bad[:8]], want_act[bad[:8]], dist[bad[:8]], want_dist[bad[:8]])
    return act, dist


# ---- (1) hand-made maps ----------------------------------------------------------------------------------------------
def _bordered(side):
    m = np.zeros((side, side), np.uint8)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 1
    return m


def _serpentine(side):
    """A wall on every other row with the gap alternating between the two ends: one path through every free cell."""
    m = _bordered(side)
    for k, r in enumerate(range(2, side - 2, 2)):
        m[r, 1:side - 1] = 1
        m[r, side - 2 if k % 2 == 0 else 1] = 0
    return m


def _walled(side):
    m = _bordered(side)
    m[:, 40] = 1
    return m


def _ell(side):
    """Walls everywhere but a one-wide L: row 5, columns 5 .. 20, and column 5, rows 5 .. 20."""
    m = np.ones((side, side), np.uint8)
    m[5, 5:21] = 0
    m[5:21, 5] = 0
    return m


def _plus(side):
    """Walls everywhere but row 40 and column 40 inside the border."""
    m = np.ones((side, side), np.uint8)
    m[40, 1:side - 1] = 0
    m[1:side - 1, 40] = 0
    return m


def _hand_cases(side):
    """(name, map, tracker, target, expected (pursuit, evade, dist) where it is typed by hand, else None)"""
    s2 = side - 2
    last = max(r for r in range(1, side - 1) if r % 2 == 1 and r <= s2)          # the serpentine's last free row
    cases = [
        ("rows 63/64", _bordered(side), (63, 10), (64, 10), (1, 1, 1)),
        ("rows 64/63, cols 31/32", _bordered(side), (66, 30), (60, 33), None),
        ("cols 63/64", _bordered(side), (10, 62), (12, 65), None),
        ("cols 32/31 on row 64", _bordered(side), (64, 32), (64, 31), (2, 0, 1)),
        ("corner 63/64 both ways", _bordered(side), (64, 64), (63, 63), (0, 0, 2)),
        ("serpentine", _serpentine(side), (1, 1), (last, 40), None),
        ("serpentine back", _serpentine(side), (last, 40), (1, 1), None),
        ("full-height wall", _walled(side), (10, 10), (10, 60), (0, 0, -1)),
        ("full-height wall, at the wall", _walled(side), (10, 39), (70, 41), (3, 2, -1)),
        ("co-located, open", _bordered(side), (20, 20), (20, 20), (0, 0, 0)),
        ("co-located, corridor corner", _ell(side), (5, 5), (5, 5), (0, 1, 0)),
        ("closed end of a corridor", _ell(side), (5, 10), (5, 20), (3, 0, 10)),
        ("closed end of the other arm", _ell(side), (10, 5), (20, 5), (1, 1, 10)),
        ("unique up", _plus(side), (40, 40), (30, 40), (0, 0, 10)),
        ("unique down", _plus(side), (40, 40), (50, 40), (1, 1, 10)),
        ("unique left", _plus(side), (40, 40), (40, 30), (2, 2, 10)),
        ("unique right", _plus(side), (40, 40), (40, 50), (3, 3, 10)),
        ("tie up / left", _bordered(side), (44, 44), (42, 42), (0, 0, 4)),
        ("tie down / right", _bordered(side), (42, 42), (44, 44), (1, 1, 4)),
        ("row side - 2", _bordered(side), (s2, 5), (s2, s2), (3, 0, s2 - 5)),
        ("column side - 2", _bordered(side), (5, s2), (s2, s2), (1, 2, s2 - 5)),
    ]
    return cases


@pytest.mark.parametrize("side", [82, 81])
def test_hand_made_maps(side):
    from active_tracking_rl_amd.vec_env import VecTrack2D
    n = 7
    env = VecTrack2D(num_envs=n, device=DEV, seed=2, auto_reset=False, map_type="Maze" if side == 81 else "Block",
                     target_mode="PZR")
    env.reset()
    cases = _hand_cases(side)
    long_paths = 0
    for lo in range(0, len(cases), n):
        group = [cases[min(lo + i, len(cases) - 1)] for i in range(n)]
        env.inject(np.stack([c[1] for c in group]), [c[2] + c[3] for c in group])
        st = env.get_state()
        assert (st["side"] == side).all() and np.array_equal(st["pos"].reshape(n, 4), np.array([c[2] + c[3] for c in group]))
        act, dist = _check(env)
        for i, c in enumerate(group):
            if c[4] is not None:
                assert (int(act[i, 0]), int(act[i, 1]), int(dist[i])) == c[4], c[0]
            if c[0].startswith("serpentine"):
                assert dist[i] > 1500, (c[0], dist[i])      # a level counter of 8 or 10 bits has wrapped by here
                long_paths += 1
    assert long_paths >= 2
    env.close()


# ---- (2) generated episodes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id", ["Track2D-BlockPartialPZR-v0", "Track2D-MazePartialNav-v0", "Track2D-EmptyPartialRam-v0"])
@pytest.mark.parametrize("n", [33, 1])
def test_generated_episodes(env_id, n):
    from active_tracking_rl_amd.vec_env import VecTrack2D
    env = VecTrack2D(env_id, num_envs=n, device=DEV, seed=3, auto_reset=True, max_episode_steps=5)
    env.reset()
    _check(env)
    g = torch.Generator().manual_seed(100 + n)
    restarts = 0
    for t in range(12):
        a = torch.randint(0, 4, (2, n), generator=g, dtype=torch.int64).to(DEV)
        _, _, done = env.step(a[0].contiguous(), a[1].contiguous())
        restarts += int(done.sum().item())
        _check(env)
    assert restarts >= 2 * n            # 12 steps of 5-step episodes: every env restarted inside a launch at least twice
    if "Maze" in env_id:
        assert (env.get_state()["side"] == 81).all()
    env.close()


# ---- (3) roles -----------------------------------------------------------------------------------------------------------
def test_roles_leave_the_other_column_alone():
    from active_tracking_rl_amd.vec_env import VecTrack2D
    n = 33
    env = VecTrack2D("Track2D-BlockPartialPZR-v0", num_envs=n, device=DEV, seed=4)
    env.reset()
    env.step(torch.zeros(n, dtype=torch.int64, device=DEV), torch.ones(n, dtype=torch.int64, device=DEV))
    want_act, want_dist = _spec(env)
    for roles, col in ((("pursuit",), 0), (("evade",), 1), ("pursuit", 0)):
        buf = torch.full((n, 2), SENTINEL, dtype=torch.int64, device=DEV)
        act, dist = env.heuristic_actions(roles, out=buf)                 # dist=None: a fresh tensor comes back
        assert act is buf and dist.dtype == torch.int32 and tuple(dist.shape) == (n,)
        assert np.array_equal(buf[:, col].cpu().numpy(), want_act[:, col]) and bool((buf[:, 1 - col] == SENTINEL).all())
        assert np.array_equal(dist.cpu().numpy(), want_dist)
    buf = torch.full((n, 2), SENTINEL, dtype=torch.int64, device=DEV)
    act, none = env.heuristic_actions(out=buf, dist=False)                # no distances at all (a null pointer in the ABI)
    assert none is None and np.array_equal(buf.cpu().numpy(), want_act)
    out = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    assert env.path_distance(out=out) is out and np.array_equal(out.cpu().numpy(), want_dist)
    assert np.array_equal(env.path_distance().cpu().numpy(), want_dist)
    with pytest.raises(ValueError, match="role"):
        env.heuristic_actions(("flee",))
    env.close()


# ---- (4) no side effect ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id", ["Track2D-BlockPartialPZR-v0", "Track2D-MazePartialNav-v0"])
def test_the_call_changes_nothing(env_id):
    from active_tracking_rl_amd.vec_env import VecTrack2D
    n = 33
    mk = lambda: VecTrack2D(env_id, num_envs=n, device=DEV, seed=6, max_episode_steps=3)
    env, twin = mk(), mk()
    assert torch.equal(env.reset(), twin.reset())
    snap = env.snapshot()
    before = snap.save().to_bytes()
    env.heuristic_actions()
    env.path_distance()
    assert snap.save().to_bytes() == before
    g = torch.Generator().manual_seed(9)
    for t in range(5):
        a = torch.randint(0, 4, (2, n), generator=g, dtype=torch.int64).to(DEV)
        env.heuristic_actions()
        got = env.step(a[0].contiguous(), a[1].contiguous())
        want = twin.step(a[0].contiguous(), a[1].contiguous())
        for x, y in zip(got, want):
            assert torch.equal(x, y), t
    env.close()
    twin.close()


# ---- (5) graph ---------------------------------------------------------------------------------------------------------
def test_the_call_replays_in_a_graph():
    from active_tracking_rl_amd.vec_env import VecTrack2D
    n = 33
    env = VecTrack2D("Track2D-BlockPartialPZR-v0", num_envs=n, device=DEV, seed=8, max_episode_steps=4)
    env.reset()
    act = torch.full((n, 2), SENTINEL, dtype=torch.int64, device=DEV)
    dist = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    env.heuristic_actions(out=act, dist=dist)                             # (the code object is loaded outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                         # one call = one launch, nothing beside it
        env.heuristic_actions(out=act, dist=dist)
    g = torch.Generator().manual_seed(10)
    for t in range(3):
        a = torch.randint(0, 4, (2, n), generator=g, dtype=torch.int64).to(DEV)
        env.step(a[0].contiguous(), a[1].contiguous())                    # eager, between the replays
        act.fill_(SENTINEL)
        dist.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        want_act, want_dist = _spec(env)
        assert np.array_equal(act.cpu().numpy(), want_act) and np.array_equal(dist.cpu().numpy(), want_dist), t
    del graph
    env.close()


# ---- (6) refusals ----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_next_call_working():
    from active_tracking_rl_amd.vec_env import T2DError, VecTrack2D, heuristic_lib
    n = 5
    moore = VecTrack2D("Track2D-BlockPartialPZR-v0", num_envs=n, device=DEV, seed=1, action_type="Moore")
    moore.reset()
    with pytest.raises(T2DError, match="Moore"):
        moore.heuristic_actions()
    moore.close()
    env = VecTrack2D("Track2D-BlockPartialPZR-v0", num_envs=n, device=DEV, seed=1)
    with pytest.raises(T2DError, match="t2d_reset"):
        env.heuristic_actions()                                           # before the first reset
    env.reset()
    _check(env)
    f = heuristic_lib().t2d_heuristic_actions
    act = torch.full((n + 1, 2), SENTINEL, dtype=torch.int64, device=DEV)
    for roles in (0, 4):
        with pytest.raises(T2DError, match="roles %d" % roles):
            f(env.h, roles, C.c_void_p(act.data_ptr()), None, env._stream())
    with pytest.raises(T2DError, match="8-byte aligned"):
        f(env.h, 3, C.c_void_p(act.data_ptr() + 4), None, env._stream())
    dist = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    with pytest.raises(T2DError, match="4-byte aligned"):
        f(env.h, 3, C.c_void_p(act.data_ptr()), C.c_void_p(dist.data_ptr() + 2), env._stream())
    with pytest.raises(T2DError, match="null act"):
        f(env.h, 3, None, None, env._stream())
    torch.cuda.synchronize()
    assert bool((act == SENTINEL).all())                                  # a refused call wrote nothing
    _check(env)
    env.close()


# ---- (7) Agent -------------------------------------------------------------------------------------------------------
class _Recorder(object):
    """A VecEnv whose step() keeps the actions it was given."""

    def __init__(self, env):
        self.env, self.sent = env, []

    def __getattr__(self, name):
        return getattr(self.env, name)

    def step(self, actions, out=None):
        self.sent.append([a.clone() for a in actions])
        return self.env.step(actions, out=out)


def _first_step(heuristic):
    from active_tracking_rl_amd.environment import VecEnv
    from active_tracking_rl_amd.player_util import Agent
    env_id = "Track2D-BlockPartialPZR-v0"
    args = gs.fixture_args(env_id, 8)
    model = gs.fixture_model(args, DEV).eval()
    env = _Recorder(VecEnv(env_id, 8, device=DEV, seed=1, env_id_base=gs.EVAL_BASE))
    player = Agent(model, env, args, None, torch.device(DEV))
    assert player.heuristic == (None, None)
    if heuristic is not None:
        player.heuristic = heuristic
    player.reset()
    want_act, _ = _spec(env.core)
    player.action_test()
    sent = [a.cpu().numpy() for a in env.sent[0]]
    env.close()
    return sent, want_act


def test_agent_replaces_one_column():
    twin, _ = _first_step(None)
    plain, _ = _first_step((None, None))
    assert len(plain) == 2 and all(np.array_equal(a, b) for a, b in zip(plain, twin))      # the default: the model's actions
    sent, want = _first_step(("pursuit", None))
    assert np.array_equal(sent[0], want[:, 0]) and np.array_equal(sent[1], twin[1])
    sent, want = _first_step((None, "evade"))
    assert np.array_equal(sent[0], twin[0]) and np.array_equal(sent[1], want[:, 1])
    sent, want = _first_step(("pursuit", "evade"))
    assert np.array_equal(sent[0], want[:, 0]) and np.array_equal(sent[1], want[:, 1])


# ---- (8) a whole round: derived, not measured -----------------------------------------------------------------------
def test_pursuit_keeps_the_nav_target_of_an_empty_map():
    """On an Empty map path distance is L1 distance. The target starts within the tracker's 2 x 2 neighbourhood
    (generators.py:82-94), so d0 <= 2. Both agents move at most one cell per step and pursuit removes one step of distance
    whenever d > 0, so d <= 2 at every step: the Euclidean distance is <= 2 <= 6, the far counter never starts and every episode
    runs to the 500-step limit, with a tracker reward of at least 1 - 2 * 2 / 6 = 1/3 per step."""
    from active_tracking_rl_amd.test import evaluate
    env_id = "Track2D-EmptyPartialNav-v0"
    args = gs.fixture_args(env_id, 8)
    rsum, length = evaluate(None, env_id, args, torch.device(DEV), episodes=8, heuristic_tracker="pursuit")
    print("lengths", length, "tracker returns", rsum[:, 0])
    assert length.shape == (8,) and (length == 500).all()
    assert (rsum[:, 0] >= 500.0 / 3.0 - 1e-3).all()
    rsum2, length2 = evaluate(None, env_id, args, torch.device(DEV), episodes=8, heuristic_tracker="pursuit")
    assert np.array_equal(rsum, rsum2) and np.array_equal(length, length2)


# ---- (9) command lines ----------------------------------------------------------------------------------------------
def test_gym_eval_runs_the_pursuit_tracker_without_a_checkpoint(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gym_eval.py"), "--env", "Track2D-EmptyPartialNav-v0", "--num-episodes", "4",
                        "--heuristic-tracker", "pursuit", "--log-dir", str(tmp_path) + "/"],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "R_mean:" in r.stderr and "EL_mean: 500.00" in r.stderr and "S_rate: 1.0" in r.stderr


def test_main_writes_the_heuristic_scalars(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--env", "Track2D-BlockPartialPZR-v0", "--num-envs", "8",
                        "--num-steps", "5", "--max-step", "1", "--test-every", "100", "--log-every", "0", "--no-graph", "--test-eps", "2",
                        "--eval-heuristic", "--log-dir", str(tmp_path)],
                       capture_output=True, text=True, cwd=ROOT, timeout=420)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = []
    for dirpath, _, files in os.walk(str(tmp_path)):
        if "scalars.jsonl" in files and os.path.basename(dirpath) == "Test":
            recs += [json.loads(ln) for ln in open(os.path.join(dirpath, "scalars.jsonl"))]
    tags = [r_["tag"] for r_ in recs]
    for tag in ("test/vs_evade/reward0", "test/vs_evade/eps_len", "test/vs_pursuit/reward1", "test/vs_pursuit/eps_len"):
        assert tags.count(tag) == 2, (tag, sorted(set(tags)))              # one record per episode of the one round
    assert tags.count("test/reward0") == 2 and tags.count("test/eps_len") == 2              # the round itself, as before
    assert "vs_evade: ave eps reward0" in r.stderr and "vs_pursuit: ave eps reward1" in r.stderr
