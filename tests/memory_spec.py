"""The rule of include/atr_memory.h in plain numpy loops, one cell at a time, over UNPACKED bool maps, written from the header's text
(not from the kernel and not from csrc/atr_memory_rule.h): the reference of the map-memory tests.

pos is int [N, 2, 2]: pos[e, p] = (r, c) of env e's player p (0 tracker, 1 target), as VecTrack2D.get_state()['pos'] hands it
out. seen is bool [N, 2, S, S] with S >= every env's side (cells outside an env's side x side square stay False); walls is
bool / 0-1 [N, S, S], the envs' maps; sides is int [N]."""
import numpy as np

SIDE, WINDOW, CENTRE = 13, 169, 6
TILE_WORDS, ROW_WORDS, MAX_SIDE = 256, 3, 82
HIDDEN, WALL, FREE = 5, 7, 8
KEEP, STEP, BEGIN = 0, 1, 2
VALUES = (0, 1, 2, 4, 5, 6)


def new_seen(n, s=MAX_SIDE):
    return np.zeros((n, 2, s, s), bool)


def clear(seen, mode, done=None, roles=3):
    """The seen sets after the clearing of one call: a new array."""
    s = np.array(seen, bool)
    assert mode in (KEEP, STEP, BEGIN) and roles in (1, 2, 3)
    for e in range(s.shape[0]):
        for p in range(2):
            if not (roles >> p) & 1:
                continue
            if mode == BEGIN or (mode == STEP and done is not None and int(done[e]) != 0):
                s[e, p] = False
    return s


def record(seen, windows, pos, sides, roles=3, hidden=HIDDEN):
    """The seen sets after the recording of one call: a new array."""
    s = np.array(seen, bool)
    w = np.asarray(windows)
    for e in range(s.shape[0]):
        for p in range(2):
            if not (roles >> p) & 1:
                continue
            pr, pc, side = int(pos[e][p][0]), int(pos[e][p][1]), int(sides[e])
            for wr in range(SIDE):
                for wc in range(SIDE):
                    r, c = pr - CENTRE + wr, pc - CENTRE + wc
                    if 0 <= r < side and 0 <= c < side and w[e, p, wr, wc] != hidden:
                        s[e, p, r, c] = True
    return s


def paint(windows, seen, walls, pos, sides, roles=3, hidden=HIDDEN, wall_value=WALL, free_value=FREE):
    """A copy of windows [N, 2, 13, 13] with every remembered hidden cell written as wall_value / free_value."""
    w = np.asarray(windows)
    assert w.ndim == 4 and w.shape[1:] == (2, SIDE, SIDE) and roles in (1, 2, 3)
    out = w.copy()
    for e in range(w.shape[0]):
        for p in range(2):
            if not (roles >> p) & 1:
                continue
            pr, pc, side = int(pos[e][p][0]), int(pos[e][p][1]), int(sides[e])
            for wr in range(SIDE):
                for wc in range(SIDE):
                    r, c = pr - CENTRE + wr, pc - CENTRE + wc
                    if w[e, p, wr, wc] == hidden and 0 <= r < side and 0 <= c < side and seen[e, p, r, c]:
                        out[e, p, wr, wc] = wall_value if walls[e][r, c] else free_value
    return out


def call(windows, seen, walls, pos, sides, mode, done=None, roles=3, hidden=HIDDEN, wall_value=WALL, free_value=FREE):
    """One call of atr_memory_windows: (painted windows, new seen sets)."""
    s = record(clear(seen, mode, done, roles), windows, pos, sides, roles, hidden)
    return paint(windows, s, walls, pos, sides, roles, hidden, wall_value, free_value), s


def pack(seen):
    """uint32 [N, 2, 256] of bool [N, 2, S, S]: row r is words 3 r .. 3 r + 2, column c is bit c & 31 of word c >> 5."""
    s = np.asarray(seen, bool)
    out = np.zeros((s.shape[0], 2, TILE_WORDS), np.uint32)
    for e, p, r, c in np.argwhere(s):
        out[e, p, ROW_WORDS * r + (c >> 5)] |= np.uint32(1 << (c & 31))
    return out


def unpack(tiles, s=MAX_SIDE):
    """bool [N, 2, s, s] of uint32 [N, 2, 256], and whether any bit lies outside the s x s square."""
    t = np.asarray(tiles, np.uint32)
    out = np.zeros((t.shape[0], 2, s, s), bool)
    stray = False
    for e in range(t.shape[0]):
        for p in range(2):
            for wd in np.flatnonzero(t[e, p]):
                for b in range(32):
                    if (int(t[e, p, wd]) >> b) & 1:
                        r, c = int(wd) // ROW_WORDS, 32 * (int(wd) % ROW_WORDS) + b
                        if r < s and c < s:
                            out[e, p, r, c] = True
                        else:
                            stray = True
    return out, stray


def place_row(mask, pc, side):
    """The three words of the map row that holds the 13-bit window-row mask of a player in column pc, one bit at a time."""
    words = [0, 0, 0]
    for wc in range(SIDE):
        c = pc - CENTRE + wc
        if (mask >> wc) & 1 and 0 <= c < side:
            words[c >> 5] |= 1 << (c & 31)
    return words


def place_table(side):
    """uint32 [side, 8192, 3]: place_row for every pc and every 13-bit mask — the same rule, one window column and one pc at a
    time, over all masks at once."""
    masks = np.arange(1 << SIDE, dtype=np.uint32)
    out = np.zeros((side, 1 << SIDE, ROW_WORDS), np.uint32)
    for pc in range(side):
        for wc in range(SIDE):
            c = pc - CENTRE + wc
            if 0 <= c < side:
                out[pc, :, c >> 5] |= ((masks >> np.uint32(wc)) & np.uint32(1)) << np.uint32(c & 31)
    return out


def row_bits(m0, m1, m2, wr):
    """The 13-bit mask of window row wr out of the 169-bit mask m0 | m1 << 64 | m2 << 128, by Python's big integers."""
    return ((m0 | m1 << 64 | m2 << 128) >> (SIDE * wr)) & ((1 << SIDE) - 1)


def random_windows(n, seed, dtype=np.uint8, values=VALUES):
    """[n, 2, 13, 13] with cells drawn from `values` (5 twice as likely as each of the others, so that plenty is hidden)."""
    rs = np.random.RandomState(seed)
    vals = np.array(tuple(values) + (HIDDEN,), dtype)
    return vals[rs.randint(0, len(vals), (n, 2, SIDE, SIDE))]


class Model(object):
    """The seen sets of N envs, step by step, from windows WITHOUT memory (a twin env's): begin() at a reset, step() behind every
    env step, keep() for an observe(). Each returns the windows as the env with memory shows them."""

    def __init__(self, n, roles):
        self.n, self.roles, self.seen = n, roles, new_seen(n)

    def _call(self, windows, walls, pos, sides, mode, done=None):
        out, self.seen = call(windows, self.seen, walls, pos, sides, mode, done, self.roles)
        return out

    def begin(self, windows, walls, pos, sides):
        return self._call(windows, walls, pos, sides, BEGIN)

    def step(self, windows, walls, pos, sides, done):
        return self._call(windows, walls, pos, sides, STEP, done)

    def keep(self, windows, walls, pos, sides):
        return self._call(windows, walls, pos, sides, KEEP)
