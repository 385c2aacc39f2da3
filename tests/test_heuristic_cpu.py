"""CPU-side checks of the heuristic players: the specification (tests/heuristic_spec.py) against an independent second
implementation and against hand-typed expectations, its properties, include/track2d_heuristic.h against the built library and
vec_env.HEURISTIC_PROTOTYPES, the new flags of gym_eval.py and main.py, and evaluate()'s refusal of a player without a policy."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import heuristic_spec as hs
from conftest import ROOT
from test_abi_cpu import _c_class, _py_class

BIG = 10 ** 6


def _relaxed_field(m, x):
    """D(x, .) as an int array by relaxation: sweeps of `free cell = min(itself, a neighbour + 1)` until nothing changes."""
    side = m.shape[0]
    free = m == 0
    d = np.full((side, side), BIG, np.int64)
    d[x] = 0
    if not free[x]:
        return d
    while True:
        p = np.pad(d, 1, constant_values=BIG)
        near = np.minimum(np.minimum(p[:-2, 1:-1], p[2:, 1:-1]), np.minimum(p[1:-1, :-2], p[1:-1, 2:])) + 1
        new = np.where(free, np.minimum(d, near), d)
        new[x] = 0
        if (new == d).all():
            return d
        d = new


def _second_players(m, t, g):
    """(pursuit, evade, dist) from relaxed fields and the header's wording, without heuristic_spec."""
    side = m.shape[0]
    wall = np.pad(m != 0, 1, constant_values=True)           # wall[r + 1, c + 1]; the rim is outside the square
    step = lambda x, a: (x[0] + ((-1, 1, 0, 0)[a]), x[1] + ((0, 0, -1, 1)[a]))
    is_wall = lambda x: bool(wall[x[0] + 1, x[1] + 1])
    at = lambda f, x: BIG if is_wall(x) else int(f[x])

    def hold(x):
        for a in range(4):
            if is_wall(step(x, a)):
                return a
        return 0
    to_g, from_t = _relaxed_field(m, g), _relaxed_field(m, t)
    d = 0 if t == g else at(from_t, g)
    p = e = None
    if 0 < d < BIG:
        p = next((a for a in range(4) if at(to_g, step(t, a)) == d - 1), None)
    if d < BIG:
        e = next((a for a in range(4) if at(from_t, step(g, a)) == d + 1), None)
    return (hold(t) if p is None else p), (hold(g) if e is None else e), (-1 if d >= BIG else d)


def _random_case(rng, side=9):
    m = (rng.random((side, side)) < 0.3).astype(np.uint8)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 1
    free = np.argwhere(m == 0)
    if len(free) < 2:
        m[1:3, 1:3] = 0
        free = np.argwhere(m == 0)
    t = tuple(int(v) for v in free[rng.integers(len(free))])
    g = t if rng.random() < 0.1 else tuple(int(v) for v in free[rng.integers(len(free))])
    return m, t, g


def test_spec_matches_the_relaxation_implementation_on_random_maps():
    rng = np.random.default_rng(20240607)
    unreachable = colocated = 0
    for _ in range(200):
        m, t, g = _random_case(rng)
        want = _second_players(m, t, g)
        assert hs.players(m, 9, t, g) == want, (m, t, g)
        assert (hs.pursuit(m, 9, t, g), hs.evade(m, 9, t, g), hs.dist_out(m, 9, t, g)) == want, (m, t, g)
        unreachable += want[2] < 0
        colocated += t == g
    assert unreachable > 5 and colocated > 5            # the draw covers both


def _grid(rows):
    return np.array([[1 if ch == "#" else 0 for ch in row] for row in rows], np.uint8)


OPEN = _grid(["#######",
              "#.....#",
              "#.....#",
              "#.....#",
              "#.....#",
              "#.....#",
              "#######"])


def test_hold_by_hand():
    assert hs.hold(OPEN, 7, (1, 3)) == 0            # a wall above
    assert hs.hold(OPEN, 7, (3, 5)) == 3            # a wall only to the right
    assert hs.hold(OPEN, 7, (3, 3)) == 0            # open space
    assert hs.hold(OPEN, 7, (5, 1)) == 1            # below and to the left: the first in order
    assert hs.hold(np.zeros((3, 3), np.uint8), 3, (1, 2)) == 3      # the square's edge is a wall


def test_players_by_hand():
    # a tie: the target is up and to the left; up (0) comes before left (2); the target flees down (1) before right (3)
    assert hs.players(OPEN, 7, (4, 4), (2, 2)) == (0, 0, 4)
    assert hs.pursuit(OPEN, 7, (4, 4), (2, 2)) == 0 and hs.dist_out(OPEN, 7, (4, 4), (2, 2)) == 4
    assert hs.evade(OPEN, 7, (2, 2), (4, 4)) == 1               # tracker up-left of the target: down and right both gain, down first
    assert hs.evade(OPEN, 7, (4, 4), (2, 2)) == 0               # tracker down-right of the target: up and left both gain, up first
    assert hs.pursuit(OPEN, 7, (2, 2), (4, 4)) == 1             # down before right
    # straight lines: each action as the only answer
    assert hs.pursuit(OPEN, 7, (3, 3), (1, 3)) == 0 and hs.pursuit(OPEN, 7, (3, 3), (5, 3)) == 1
    assert hs.pursuit(OPEN, 7, (3, 3), (3, 1)) == 2 and hs.pursuit(OPEN, 7, (3, 3), (3, 5)) == 3
    # co-located in the open: the tracker holds with 0 (all four free), the target leaves upwards (every neighbour is at d + 1)
    assert hs.players(OPEN, 7, (3, 3), (3, 3)) == (0, 0, 0)
    # co-located in a corner: up is a wall for both; the target's first FREE neighbour is down
    assert hs.players(OPEN, 7, (1, 1), (1, 1)) == (0, 1, 0)


CORRIDOR = _grid(["#######",
                  "#.....#",
                  "#####.#",
                  "#...#.#",
                  "#.#...#",
                  "#######"])


def test_dead_end_and_unreachable_by_hand():
    m = np.zeros((7, 7), np.uint8)
    m[:6, :7] = CORRIDOR
    m[6, :] = 1
    # the target at the closed end (1, 1) of the top corridor, the tracker in the corridor: no neighbour is farther, it holds with
    # the first wall-bound action (up)
    assert hs.players(m, 7, (1, 4), (1, 1)) == (2, 0, 3)
    # the target in the dead end (4, 1) behind (3, 1)-(3, 2)-(3, 3)-(4, 3)-(4, 4)-(4, 5)-(3, 5)-(2, 5)-(1, 5): 13 steps from
    # (1, 1), the first of them to the right; the target's only free neighbour (3, 1) is closer, so it holds: up is free, down is
    # the first wall
    assert hs.players(m, 7, (1, 1), (4, 1)) == (3, 1, 13)
    # an unreachable partner: a full wall between the two
    w = OPEN.copy()
    w[:, 3] = 1
    assert hs.players(w, 7, (2, 1), (2, 5)) == (2, 3, -1)       # both hold: the tracker's first wall is to the left, the target's to the right
    assert hs.players(w, 7, (1, 2), (5, 4)) == (0, 1, -1)       # tracker: wall above; target: up free, wall below
    assert hs.distance(w, 7, (2, 1), (2, 5)) == hs.INF


def test_spec_properties():
    rng = np.random.default_rng(7)
    moved = 0
    for _ in range(120):
        m, t, g = _random_case(rng)
        d = hs.distance(m, 9, t, g)
        assert d == hs.distance(m, 9, g, t)                                       # symmetric
        if 0 < d < hs.INF:                                                        # one pursuit move against a still target
            n = hs.dest(t, hs.pursuit(m, 9, t, g))
            assert not hs.is_wall(m, 9, n) and hs.distance(m, 9, n, g) == d - 1
            moved += 1
        a = hs.evade(m, 9, t, g)                                                  # one evade move against a still tracker
        n = hs.dest(g, a)
        if hs.is_wall(m, 9, n):
            n = g
        if d < hs.INF:
            assert hs.distance(m, 9, t, n) >= d
        else:
            assert n == g or hs.distance(m, 9, t, n) == hs.INF
    assert moved > 30


def _heuristic_functions():
    """{name: (class of the result, [class per parameter])} of every t2d_* function include/track2d_heuristic.h declares."""
    txt = open(os.path.join(ROOT, "include", "track2d_heuristic.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", txt).split("\n") if not ln.lstrip().startswith("#"))
    out = {}
    for m in re.finditer(r"([^;{}()]*?)\b(t2d_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", txt):
        params = [p.strip() for p in m.group(3).split(",")]
        assert m.group(2) not in out
        out[m.group(2)] = (_c_class(m.group(1)), [_c_class(re.sub(r"\w+$", "", p)) for p in params])
    return out


def test_heuristic_prototypes_match_the_header():
    from active_tracking_rl_amd import vec_env
    funcs = _heuristic_functions()
    assert sorted(funcs) == ["t2d_heuristic_actions"] == sorted(vec_env.HEURISTIC_PROTOTYPES)
    for name, (res, params) in funcs.items():
        restype, argtypes = vec_env.HEURISTIC_PROTOTYPES[name]
        assert _py_class(restype) == res, name
        assert len(argtypes) == len(params), name
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _py_class(a) == c, (name, i)
    txt = open(os.path.join(ROOT, "include", "track2d_heuristic.h")).read()
    assert re.search(r"#define\s+T2D_HEUR_PURSUIT\s+%d\b" % vec_env.HEUR_PURSUIT, txt)
    assert re.search(r"#define\s+T2D_HEUR_EVADE\s+%d\b" % vec_env.HEUR_EVADE, txt)
    assert vec_env.HEURISTIC_ROLES == {"pursuit": 1, "evade": 2}


def test_library_exports_every_function_of_the_heuristic_header():
    from active_tracking_rl_amd import build, vec_env
    build.build()
    assert os.path.join("..", "..", "include", "track2d_heuristic.h") in build.HEADERS
    assert "heuristic_hip.hip" in build.SOURCES and build.NO_SCRATCH_HEURISTIC == {"heuristic_hip.hip": "k_heuristic"}
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    for name in _heuristic_functions():
        assert hasattr(lib, name), name
    # the pinned headers gained nothing
    for pinned in ("track2d.h", "track2d_np.h", "atr_policy.h"):
        assert "t2d_heuristic" not in open(os.path.join(ROOT, "include", pinned)).read()


def test_heuristic_binding_refuses_without_a_device():
    """The null and range checks come before any device work, and the errcheck raises T2DError with the library's text."""
    from active_tracking_rl_amd import build, vec_env
    build.build()
    f = vec_env.heuristic_lib().t2d_heuristic_actions
    assert f.restype is ctypes.c_int and list(f.argtypes) == vec_env.HEURISTIC_PROTOTYPES["t2d_heuristic_actions"][1]
    with pytest.raises(vec_env.T2DError, match=r"^t2d_heuristic_actions failed \(-1\): .*null handle"):
        f(None, 3, None, None, None)


@pytest.mark.parametrize("script, flags", [("gym_eval.py", ("--heuristic-tracker {pursuit}", "--heuristic-target {evade}")),
                                           ("main.py", ("--eval-heuristic",))])
def test_parsers_list_the_heuristic_flags(script, flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in flags:
        assert flag in r.stdout, flag


def test_evaluate_without_a_model_needs_enough_heuristics():
    """Checked before an env is created: no device is needed to be told which player lacks a policy."""
    import torch
    from active_tracking_rl_amd.test import evaluate, heuristic_players
    dev = torch.device("cpu")
    with pytest.raises(ValueError, match="tracker has no policy"):
        evaluate(None, "Track2D-BlockPartialNav-v0", None, dev, 2)
    with pytest.raises(ValueError, match="tracker has no policy"):
        evaluate(None, "Track2D-BlockPartialPZR-v0", None, dev, 2, heuristic_target="evade")
    with pytest.raises(ValueError, match="target has no policy"):
        evaluate(None, "Track2D-BlockPartialPZR-v0", None, dev, 2, heuristic_tracker="pursuit")
    with pytest.raises(ValueError, match="heuristic tracker is 'pursuit'"):
        evaluate(None, "Track2D-BlockPartialNav-v0", None, dev, 2, heuristic_tracker="evade")
    assert heuristic_players(None, "Track2D-BlockPartialNav-v0", "pursuit", None) == ("pursuit", None)
    assert heuristic_players(None, "Track2D-BlockPartialPZR-v0", "pursuit", "evade") == ("pursuit", "evade")
    assert heuristic_players(object(), "Track2D-BlockPartialPZR-v0") == (None, None)
