"""The rule of include/atr_fov.h in plain numpy loops, one cell at a time, written from the header's text (not from the kernel and
not from csrc/atr_fov_rule.h): the reference of the field-of-view tests."""
import numpy as np

SIDE, WINDOW, CENTRE, NONE, HIDDEN, NEAR = 13, 169, 6, 255, 5, 1
MOVES = {0: (-1, 0), 1: (1, 0), 2: (0, -1), 3: (0, 1)}      # track_1v1.py:275-279, (ur, uc)
SLOPE = {90: 1, 180: 0, 270: -1}
APERTURES = (90, 180, 270, 360)
FACINGS = (0, 1, 2, 3, NONE)
VALUES = (0, 1, 2, 4, 5, 255)


def hidden_cells(facing, aperture, near=NEAR):
    """bool [13, 13]: the cells a player of this facing, aperture and near radius does not see."""
    assert aperture in APERTURES and 0 <= near <= 6
    out = np.zeros((SIDE, SIDE), bool)
    if facing == NONE or aperture == 360:
        return out
    ur, uc = MOVES[facing]
    s = SLOPE[aperture]
    for r in range(SIDE):
        for c in range(SIDE):
            dr, dc = r - CENTRE, c - CENTRE
            f = dr * ur + dc * uc
            l = abs(dr * uc - dc * ur)
            in_cone = f >= s * l
            is_near = max(abs(dr), abs(dc)) <= near
            out[r, c] = not in_cone and not is_near
    return out


def turn(facing, action=None, done=None):
    """The facing after a step: done (None = not given) first, then the action (None = not given), else unchanged."""
    if done is not None and done != 0:
        return NONE
    if action is not None and 0 <= action <= 3:
        return int(action)
    return facing


def turn_all(facing, actions=(None, None), done=None):
    """facing uint8 [N, P] -> the new facings: turn() per (env, player); actions: per player None or an [N] array."""
    f = np.array(facing, np.uint8)
    for e in range(f.shape[0]):
        for p in range(f.shape[1]):
            a = None if p >= len(actions) or actions[p] is None else int(actions[p][e])
            f[e, p] = turn(int(f[e, p]), a, None if done is None else int(done[e]))
    return f


def restrict(windows, facing, apertures=(90, 90), near=NEAR, hidden=HIDDEN):
    """A copy of windows [N, P, 13, 13] with every cell that player (e, p) of facing[e, p] does not see set to `hidden`."""
    w = np.asarray(windows)
    out = w.copy()
    f = np.asarray(facing)
    assert w.ndim == 4 and f.shape == w.shape[:2]
    masks = {}
    for e in range(w.shape[0]):
        for p in range(w.shape[1]):
            key = (int(f[e, p]) if int(f[e, p]) in MOVES else NONE, apertures[p])
            if key not in masks:
                masks[key] = hidden_cells(key[0], key[1], near)
            out[e, p][masks[key]] = hidden
    return out


def step(windows, facing, actions=(None, None), done=None, apertures=(90, 90), near=NEAR, hidden=HIDDEN):
    """One call of atr_fov_windows: (restricted windows, new facing)."""
    f = turn_all(facing, actions, done)
    return restrict(windows, f, apertures, near, hidden), f


def random_windows(n, p, seed, dtype=np.uint8):
    """[n, p, 13, 13] with cells drawn from VALUES."""
    rs = np.random.RandomState(seed)
    return np.array(VALUES, dtype)[rs.randint(0, len(VALUES), (n, p, SIDE, SIDE))]


def rot90_facing(facing):
    """The facing after the quarter turn of np.rot90 (counter-clockwise: up -> left -> down -> right -> up)."""
    return {0: 2, 2: 1, 1: 3, 3: 0, NONE: NONE}[facing]
