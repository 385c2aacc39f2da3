"""What the CPU and GPU tests of the sight statistics share: the rule of include/atr_sight.h written one sample at a time in plain
Python (a loop over the line cells, a deque breadth-first search) — independent of sight_stats.classify — and builders of
hand-made windows: a wall on each single line cell, walls everywhere but the line, an enclosed target, a serpentine corridor whose
only path is 64 steps long, and wall-free windows. Stores come from tracking_stats_spec.synthetic_store (walls at density 0.3)."""
from collections import deque

import numpy as np

from tracking_stats_spec import synthetic_store  # noqa: F401

WINDOW, CENTRE = 169, 84
BIN_OUT, BIN_TERMINAL, BIN_INCONSISTENT = 169, 170, 171
CLEAR, BLOCKED_CLASS, OUT_CLASS = 0, 1, 2
SEEN, BLOCKED, NOPATH, PATH, DETOUR, TRANS = 0, 169, 338, 507, 676, 761
OUT, TERMINAL, INCONSISTENT, SAMPLES, TABLE = 770, 771, 772, 773, 776
OFFSETS = [(dr, dc) for dr in range(-6, 7) for dc in range(-6, 7) if (dr, dc) != (0, 0)]          # the 168 of them
LONGEST_PATH = 64             # the length of the only path of longest_window(): stated here, found by the flood


def sgn(v):
    return (v > 0) - (v < 0)


def line(dr, dc):
    """The header's line cells, one k at a time."""
    m = max(abs(dr), abs(dc))
    cells = []
    for k in range(1, m):
        cells.append((6 + sgn(dr) * ((2 * k * abs(dr) + m) // (2 * m)), 6 + sgn(dc) * ((2 * k * abs(dc) + m) // (2 * m))))
    return cells


def bfs(window, dr, dc):
    """Length of a shortest 4-connected path over the cells != 1 of window [13, 13] from (6, 6) to (6 + dr, 6 + dc); 0: none."""
    goal = (6 + dr, 6 + dc)
    dist = {(6, 6): 0}
    todo = deque([(6, 6)])
    while todo:
        r, c = todo.popleft()
        if (r, c) == goal:
            return dist[(r, c)]
        for nr, nc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
            if 0 <= nr < 13 and 0 <= nc < 13 and (nr, nc) not in dist and window[nr][nc] != 1:
                dist[(nr, nc)] = dist[(r, c)] + 1
                todo.append((nr, nc))
    return 0


def sample_bin(w0, w1, r, done, flags):
    """The bin of one sample (the rule of include/atr_track_stats.h, restated in include/atr_sight.h)."""
    if done and not flags & 1:
        return BIN_TERMINAL
    four, two = np.flatnonzero(w0 == 4), np.flatnonzero(w1 == 2)
    ok = w0[CENTRE] == 2 and w1[CENTRE] == 4
    one = np.float32(r) == np.float32(1.0)
    if ok and one and len(four) == 0 and len(two) == 0:
        return CENTRE
    if ok and not one and len(four) == 1 and len(two) == 1 and two[0] == 168 - four[0]:
        return int(four[0])
    if ok and not one and len(four) == 0 and len(two) == 0:
        return BIN_OUT
    return BIN_INCONSISTENT


def sight_of(w0, bin_):
    """(class, P) of an in-view sample from the tracker's window [169]: P = 0 for no path, None for the co-located bin."""
    if bin_ == CENTRE:
        return CLEAR, None
    dr, dc = bin_ // 13 - 6, bin_ % 13 - 6
    win = np.asarray(w0).reshape(13, 13)
    blocked = any(win[r][c] == 1 for r, c in line(dr, dc))
    return (BLOCKED_CLASS if blocked else CLEAR), bfs(win.tolist(), dr, dc)


def loop_model(obs, rew, done, carry=None, flags=0, tab=None):
    """The header's per-env walk, one sample at a time. -> (tab int64 [776], carry int32 [N], classes [T, N] (-1: none),
    paths [T, N] (-1: not computed, 0: no path))."""
    obs, rew, done = np.asarray(obs), np.asarray(rew, np.float32), np.asarray(done)
    T, N = done.shape
    obs = obs.reshape(T + 1, N, 2, WINDOW)
    rew = rew.reshape(T, N, 2)
    tab = np.zeros(TABLE, np.int64) if tab is None else np.array(tab, np.int64)
    carry = np.full(N, -1, np.int32) if carry is None else np.array(carry, np.int32)
    classes, paths = np.full((T, N), -1, np.int32), np.full((T, N), -1, np.int32)
    for e in range(N):
        prev = int(carry[e]) if -1 <= carry[e] <= 2 else -1
        for t in range(T):
            b = sample_bin(obs[t + 1, e, 0], obs[t + 1, e, 1], rew[t, e, 0], done[t, e], flags)
            tab[SAMPLES] += 1
            cls = -1
            if b == BIN_TERMINAL:
                tab[TERMINAL] += 1
            elif b == BIN_INCONSISTENT:
                tab[INCONSISTENT] += 1
            elif b == BIN_OUT:
                tab[OUT] += 1
                cls = OUT_CLASS
            else:
                cls, p = sight_of(obs[t + 1, e, 0], b)
                tab[SEEN + b] += 1
                if cls == BLOCKED_CLASS:
                    tab[BLOCKED + b] += 1
                if p is not None:
                    paths[t, e] = p
                    if p == 0:
                        tab[NOPATH + b] += 1
                    else:
                        detour = p - abs(b // 13 - 6) - abs(b % 13 - 6)
                        assert detour >= 0 and detour % 2 == 0 and 1 <= p <= 168
                        tab[PATH + p] += 1
                        tab[DETOUR + detour // 2] += 1
            if cls >= 0 and prev >= 0:
                tab[TRANS + prev * 3 + cls] += 1
            prev = -1 if cls < 0 or done[t, e] else cls
            classes[t, e] = cls
        carry[e] = prev
    return tab, carry, classes, paths


def check_identities(tab, hist=None):
    """The table identities of a consistent table; hist: tracking_stats.classify's for the same store."""
    tab = np.asarray(tab, np.int64)
    seen, blocked, nopath = tab[SEEN:SEEN + 169], tab[BLOCKED:BLOCKED + 169], tab[NOPATH:NOPATH + 169]
    assert seen.sum() + tab[OUT] + tab[TERMINAL] + tab[INCONSISTENT] == tab[SAMPLES]
    assert tab[PATH:PATH + 169].sum() + nopath.sum() == seen.sum() - seen[CENTRE]
    assert tab[DETOUR:DETOUR + 85].sum() == tab[PATH:PATH + 169].sum() and tab[PATH] == 0
    for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        b = (dr + 6) * 13 + dc + 6
        assert blocked[b] == 0 and nopath[b] == 0
    assert (blocked <= seen).all() and (nopath <= seen).all() and blocked[CENTRE] == 0 and nopath[CENTRE] == 0
    assert tab[TRANS:TRANS + 9].sum() <= tab[SAMPLES] and not tab[774:].any()
    if hist is not None:
        assert np.array_equal(seen, np.asarray(hist)[:169])


def assert_equal(got, want, what=""):
    for name, g, w in zip(("tab", "carry"), got, want):
        g, w = np.asarray(g).astype(np.int64), np.asarray(w).astype(np.int64)
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:8].ravel().tolist())


# -- hand-made windows -------------------------------------------------------------------------------------------------
def pair(w0, dr, dc):
    """(obs u8 [2, 169], rew0) of an in-view sample whose tracker window is w0 [13, 13] (walls 0 / 1): the centres and the target
    written in, the target's own window wall-free."""
    w = np.zeros((2, 13, 13), np.uint8)
    w[0] = w0
    w[0, 6, 6], w[1, 6, 6] = 2, 4
    w[0, 6 + dr, 6 + dc], w[1, 6 - dr, 6 - dc] = 4, 2
    return w.reshape(2, WINDOW), np.float32(max(1.0 - 2.0 * float(np.hypot(dr, dc)) / 6.0, -1.0))


def wall_on_line_cell(dr, dc, k):
    w0 = np.zeros((13, 13), np.uint8)
    r, c = line(dr, dc)[k]
    w0[r, c] = 1
    return pair(w0, dr, dc)


def walls_off_the_line(dr, dc):
    w0 = np.ones((13, 13), np.uint8)
    for r, c in line(dr, dc):
        w0[r, c] = 0
    return pair(w0, dr, dc)


def enclosed(dr, dc):
    """The target's four neighbours are walls (where they are in the window and not the tracker's cell: |dr| + |dc| >= 2)."""
    assert abs(dr) + abs(dc) >= 2
    w0 = np.zeros((13, 13), np.uint8)
    for r, c in ((5 + dr, 6 + dc), (7 + dr, 6 + dc), (6 + dr, 5 + dc), (6 + dr, 7 + dc)):
        if 0 <= r < 13 and 0 <= c < 13:
            w0[r, c] = 1
    return pair(w0, dr, dc)


def longest_window():
    """A serpentine corridor one cell wide whose only path from the tracker to the target is 64 steps long. The even rows are
    free, every odd row is a wall with one gap: rows 7 and 11 at column 0, row 9 at column 12, rows 5 and 1 at column 12, row 3 at
    column 0; row 7 has a second gap at column 12, and (6, 7), right of the tracker, is a wall. The target sits at (0, 0). The
    path: (6, 6) left to (6, 0): 6; down through (7, 0) to (8, 0): 2; right to (8, 12): 12; up the right edge (7, 12), (6, 12),
    (5, 12), (4, 12): 4; left to (4, 0): 12; up to (2, 0): 2; right to (2, 12): 12; up to (0, 12): 2; left to (0, 0): 12 — 64 in
    all. Rows 9 .. 12 and the cells (6, 8) .. (6, 11) are dead ends. -> (obs [2, 169], rew0, dr, dc, P)."""
    w0 = np.zeros((13, 13), np.uint8)
    for r in range(1, 13, 2):
        w0[r, :] = 1
    for r, c in ((7, 0), (9, 12), (11, 0), (5, 12), (3, 0), (1, 12), (7, 12)):
        w0[r, c] = 0
    w0[6, 7] = 1
    obs, rew = pair(w0, -6, -6)
    return obs, rew, -6, -6, LONGEST_PATH


def store_of(samples):
    """A one-step store per sample: [(obs [2, 169], rew0)] -> obs u8 [2, S, 2, 13, 13], rew f32 [1, S, 2], done u8 [1, S]."""
    S = len(samples)
    obs = np.zeros((2, S, 2, WINDOW), np.uint8)
    rew = np.zeros((1, S, 2), np.float32)
    for i, (w, r) in enumerate(samples):
        obs[0, i] = obs[1, i] = w
        rew[0, i, 0] = r
    return obs.reshape(2, S, 2, 13, 13), rew, np.zeros((1, S), np.uint8)
