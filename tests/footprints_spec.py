"""The rule of include/atr_footprints.h in plain numpy loops, one entry and one cell at a time, written from the header's text (not
from the kernel and not from csrc/atr_footprint_rule.h): the reference of the footprint tests.

pos is int [N, 2, 2]: pos[e, p] = (r, c) of env e's player p (0 tracker, 1 target), as VecTrack2D.get_state()['pos'] hands it
out. A trail is uint16 [N, 2, K + 1]."""
import numpy as np

SIDE, WINDOW, CENTRE = 13, 169, 6
EMPTY, VALUE, MAX_K = 0xFFFF, 6, 63
PEEK, STEP, BEGIN = 0, 1, 2
VALUES = (0, 1, 2, 4, 5, 255)


def cell(r, c):
    return int(r) | int(c) << 8


def new_trail(n, k):
    return np.full((n, 2, k + 1), EMPTY, np.uint16)


def record(trail, pos, mode, done=None):
    """The trail after one recording call: a new array, `trail` is left alone."""
    s = np.array(trail, np.uint16)
    assert s.ndim == 3 and s.shape[1] == 2 and 1 <= s.shape[2] - 1 <= MAX_K and mode in (PEEK, STEP, BEGIN)
    if mode == PEEK:
        return s
    k = s.shape[2] - 1
    for e in range(s.shape[0]):
        for p in range(2):
            cur = cell(pos[e][p][0], pos[e][p][1])
            old = [int(x) for x in s[e, p]]
            if mode == BEGIN or (done is not None and int(done[e]) != 0):
                new = [cur] + [EMPTY] * k
            elif cur != old[0]:
                new = [cur] + old[:k]
            else:
                new = old
            s[e, p] = new
    return s


def paintable(trail, pos, roles):
    """bool [N, 2, 13, 13]: the window cells that hold a print the viewer could see — from the positions and the trail alone."""
    s = np.asarray(trail)
    out = np.zeros((s.shape[0], 2, SIDE, SIDE), bool)
    for e in range(s.shape[0]):
        for v in range(2):
            if not (roles >> v) & 1:
                continue
            vr, vc = int(pos[e][v][0]), int(pos[e][v][1])
            for j in range(1, s.shape[2]):
                pr = int(s[e, 1 - v, j])
                if pr == EMPTY:
                    continue
                dr, dc = (pr & 255) - vr, (pr >> 8) - vc
                if max(abs(dr), abs(dc)) <= CENTRE:
                    out[e, v, CENTRE + dr, CENTRE + dc] = True
    return out


def paint(windows, trail, pos, roles, value=VALUE):
    """A copy of windows [N, 2, 13, 13] with every paintable cell that reads exactly 0 set to `value`."""
    w = np.asarray(windows)
    assert w.ndim == 4 and w.shape[1:] == (2, SIDE, SIDE) and roles in (1, 2, 3) and 0 <= value <= 255
    out = w.copy()
    can = paintable(trail, pos, roles)
    for e, v, r, c in np.argwhere(can):           # (one cell at a time, over the paintable cells only)
        if w[e, v, r, c] == 0:
            out[e, v, r, c] = value
    return out


def call(windows, trail, pos, mode, done=None, roles=1, value=VALUE):
    """One call of atr_footprint_windows: (painted windows, new trail)."""
    s = record(trail, pos, mode, done)
    return paint(windows, s, pos, roles, value), s


def window_of(grid, r, c, other, me, you):
    """The 13 x 13 window of a player on (r, c) of a square 0 / 1 map `grid` as the env draws it: walls and the padding outside
    the map read 1, the viewer `me` at the centre, the other player (on `other`) as `you` where it is inside."""
    side = grid.shape[0]
    w = np.ones((SIDE, SIDE), np.uint8)
    for i in range(SIDE):
        for j in range(SIDE):
            rr, cc = r - CENTRE + i, c - CENTRE + j
            if 0 <= rr < side and 0 <= cc < side:
                w[i, j] = grid[rr, cc]
    dr, dc = other[0] - r, other[1] - c
    if max(abs(dr), abs(dc)) <= CENTRE:
        w[CENTRE + dr, CENTRE + dc] = you
    w[CENTRE, CENTRE] = me
    return w


def windows_of(grid, pos):
    """uint8 [N, 2, 13, 13] for pos [N, 2, 2] on one map: the tracker reads 2, the target 4."""
    pos = np.asarray(pos)
    return np.stack([np.stack([window_of(grid, pos[e, 0, 0], pos[e, 0, 1], pos[e, 1], 2, 4),
                               window_of(grid, pos[e, 1, 0], pos[e, 1, 1], pos[e, 0], 4, 2)]) for e in range(pos.shape[0])])


def random_windows(n, seed, dtype=np.uint8):
    """[n, 2, 13, 13] with cells drawn from VALUES."""
    rs = np.random.RandomState(seed)
    return np.array(VALUES, dtype)[rs.randint(0, len(VALUES), (n, 2, SIDE, SIDE))]


def random_trail(n, k, pos, seed, reach=9):
    """uint16 [n, 2, k + 1]: cells within `reach` of either player (inside and outside its window, duplicates likely), some
    EMPTY; entry 0 is the player's cell, another cell or EMPTY."""
    rs = np.random.RandomState(seed)
    pos = np.asarray(pos)
    s = new_trail(n, k)
    for e in range(n):
        for p in range(2):
            for j in range(k + 1):
                u = rs.randint(0, 10)
                if u == 0:
                    continue
                about = pos[e, rs.randint(0, 2)]
                r = min(255, max(0, int(about[0]) + rs.randint(-reach, reach + 1)))
                c = min(255, max(0, int(about[1]) + rs.randint(-reach, reach + 1)))
                s[e, p, j] = cell(r, c)
                if j == 0 and u < 5:
                    s[e, p, j] = cell(pos[e, p, 0], pos[e, p, 1])
                if j >= 2 and u == 1:
                    s[e, p, j] = s[e, p, j - 1]
    return s
