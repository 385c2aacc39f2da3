"""The Rooms map rule (include/track2d.h T2D_MAP_ROOMS) in plain Python: the specification the device generator
(csrc/t2d_device.h gen_rooms), the rule header (csrc/t2d_rooms_rule.h) and the host program (tests/rooms_host.cpp) are held to.

The map is 82 x 82, border = wall, interior rows / columns 1 .. 80. A region is a rectangle (r0, c0, r1, c1) of interior cells,
bounds inclusive; the root is (1, 1, 80, 80). Each region has ONE Philox4x32-10 block of its own,

    X, Y, Z, W = philox4x32_10(counter = (r0 | c0 << 7 | r1 << 14 | c1 << 21, episode, genv, 3), key = (seed & 0xffffffff, seed >> 32))

and pick(word, n) = (word * n) >> 32. Smallest room side m = 3 + 2 level, or at level 0 m = 5 + 2 pick(P.x, 4) with P the block
whose counter word 0 is 0xffffffff. With h, w the region's height and width:

  1. h <= 4m and w <= 4m and ((X >> 8) & 7) == 0: final;
  2. a horizontal wall (a row) if h > w, a vertical one if w > h, on a tie horizontal iff (X & 1) == 0;
  3. candidates = the even t with a0 + m <= t <= a1 - m along the split axis a0 .. a1; none: final; else t = candidates[pick(Y, count)];
  4. the wall is every cell of line t across the other extent b0 .. b1 (L = b1 - b0 + 1 cells);
  5. doors = the odd d in b0 .. b1; door 1 = doors[pick(Z, count)], and if L >= 32 door 2 = doors[pick(W, count)]; cleared after the wall;
  6. the two rectangles on either side of line t are split by the same rule.

Nothing here depends on the order regions are processed in: rooms_map(order='dfs') and rooms_map(order='bfs') agree."""
import numpy as np

SIDE = 82
ROOT = (1, 1, 80, 80)
STREAM_ROOMS = 3
MAX_REGIONS = 337
_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 on Python integers: counter four words, key two; returns four words."""
    c0, c1, c2, c3 = [int(x) & _M32 for x in counter]
    k0, k1 = [int(x) & _M32 for x in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def pick(word, n):
    return (word * n) >> 32


def region_words(seed, genv, episode, word0):
    return philox4x32_10((word0, episode, genv, STREAM_ROOMS), (seed & _M32, (seed >> 32) & _M32))


def min_side(seed, genv, episode, level):
    if level >= 1:
        return 3 + 2 * level
    return 5 + 2 * pick(region_words(seed, genv, episode, 0xFFFFFFFF)[0], 4)


def split(region, m, words):
    """None for a final region, else (horizontal, t, doors (one or two positions), (child, child))."""
    r0, c0, r1, c1 = region
    X, Y, Z, W = words
    h, w = r1 - r0 + 1, c1 - c0 + 1
    if h <= 4 * m and w <= 4 * m and ((X >> 8) & 7) == 0:
        return None
    horizontal = h > w or (h == w and (X & 1) == 0)
    (a0, a1), (b0, b1) = ((r0, r1), (c0, c1)) if horizontal else ((c0, c1), (r0, r1))
    cand = [t for t in range(a0 + m, a1 - m + 1) if t % 2 == 0]
    if not cand:
        return None
    t = cand[pick(Y, len(cand))]
    doors = [d for d in range(b0, b1 + 1) if d % 2 == 1]
    picked = [doors[pick(Z, len(doors))]]
    if b1 - b0 + 1 >= 32:
        picked.append(doors[pick(W, len(doors))])
    if horizontal:
        kids = ((r0, c0, t - 1, c1), (t + 1, c0, r1, c1))
    else:
        kids = ((r0, c0, r1, t - 1), (r0, t + 1, r1, c1))
    return horizontal, t, picked, kids


def rooms_map(seed, genv, episode, level, order="dfs", info=None):
    """The 82 x 82 uint8 map (1 = wall) of (seed, global env id, episode, level). info (a dict) receives m, the final rooms,
    the number of regions processed and the deepest the work list got."""
    m = min_side(seed, genv, episode, level)
    g = np.zeros((SIDE, SIDE), np.uint8)
    work, rooms, n, deepest = [ROOT], [], 0, 1
    while work:
        region = work.pop() if order == "dfs" else work.pop(0)
        n += 1
        r0, c0, r1, c1 = region
        s = split(region, m, region_words(seed, genv, episode, r0 | c0 << 7 | r1 << 14 | c1 << 21))
        if s is None:
            rooms.append(region)
            continue
        horizontal, t, doors, kids = s
        if horizontal:
            g[t, c0:c1 + 1] = 1
            for d in doors:
                g[t, d] = 0
        else:
            g[r0:r1 + 1, t] = 1
            for d in doors:
                g[d, t] = 0
        work.extend(kids)
        deepest = max(deepest, len(work))
    g[0, :] = g[-1, :] = 1
    g[:, 0] = g[:, -1] = 1
    if info is not None:
        info.update(m=m, rooms=rooms, regions=n, deepest=deepest)
    return g


def connected(g):
    """True if the free cells of g are one 4-connected set."""
    free = g == 0
    start = np.argwhere(free)
    if len(start) == 0:
        return False
    seen = np.zeros_like(free)
    stack = [tuple(start[0])]
    seen[stack[0]] = True
    while stack:
        r, c = stack.pop()
        for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
            if 0 <= rr < g.shape[0] and 0 <= cc < g.shape[1] and free[rr, cc] and not seen[rr, cc]:
                seen[rr, cc] = True
                stack.append((rr, cc))
    return bool((seen == free).all())
