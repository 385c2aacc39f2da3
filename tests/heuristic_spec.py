"""The heuristic players' specification (include/track2d_heuristic.h) in plain Python: breadth-first distance with a
collections.deque, the pursuit tracker, the evading target. No torch.

map[r][c] is 1 for a wall and 0 for a free cell; a cell outside the side x side square counts as a wall; agents are not
obstacles. Moves are the VonNeumann table: action 0 = (-1, 0), 1 = (+1, 0), 2 = (0, -1), 3 = (0, +1)."""
from collections import deque

import numpy as np

MOVES = ((-1, 0), (1, 0), (0, -1), (0, 1))
INF = 1 << 30


def is_wall(m, side, cell):
    r, c = cell
    return r < 0 or c < 0 or r >= side or c >= side or m[r][c] != 0


def dest(cell, a):
    return (cell[0] + MOVES[a][0], cell[1] + MOVES[a][1])


def distance(m, side, x, y):
    """D(x, y): 4-connected breadth-first distance over free cells, INF if y cannot be reached from x. D(x, x) = 0; for x != y a
    wall at either end means INF."""
    x, y = (int(x[0]), int(x[1])), (int(y[0]), int(y[1]))
    if x == y:
        return 0
    if is_wall(m, side, x) or is_wall(m, side, y):
        return INF
    seen = {x: 0}
    q = deque([x])
    while q:
        cur = q.popleft()
        for a in range(4):
            nxt = dest(cur, a)
            if nxt in seen or is_wall(m, side, nxt):
                continue
            seen[nxt] = seen[cur] + 1
            if nxt == y:
                return seen[nxt]
            q.append(nxt)
    return INF


def hold(m, side, x):
    """The first action whose destination is a wall (the env leaves the agent in place), 0 in open space."""
    x = (int(x[0]), int(x[1]))
    for a in range(4):
        if is_wall(m, side, dest(x, a)):
            return a
    return 0


def pursuit(m, side, t, g):
    """The tracker's action."""
    t, g = (int(t[0]), int(t[1])), (int(g[0]), int(g[1]))
    d = distance(m, side, t, g)
    if 0 < d < INF:
        for a in range(4):
            n = dest(t, a)
            if not is_wall(m, side, n) and distance(m, side, n, g) == d - 1:
                return a
    return hold(m, side, t)


def evade(m, side, t, g):
    """The target's action."""
    t, g = (int(t[0]), int(t[1])), (int(g[0]), int(g[1]))
    d = distance(m, side, t, g)
    if d < INF:
        for a in range(4):
            n = dest(g, a)
            if not is_wall(m, side, n) and distance(m, side, t, n) == d + 1:
                return a
    return hold(m, side, g)


def dist_out(m, side, t, g):
    d = distance(m, side, t, g)
    return -1 if d >= INF else d


def distances_from(m, side, x, cells):
    """{cell: D(x, cell)} for the listed cells with ONE flood from x, stopped once every listed cell that can be labelled is:
    what distance() gives cell by cell (tests/test_heuristic_cpu.py holds the two together)."""
    x = (int(x[0]), int(x[1]))
    out = {c: (0 if c == x else INF) for c in cells}
    if is_wall(m, side, x):
        return out
    want = set(c for c in cells if c != x and not is_wall(m, side, c))
    seen = {x: 0}
    q = deque([x])
    while q and want:
        cur = q.popleft()
        for a in range(4):
            nxt = dest(cur, a)
            if nxt in seen or is_wall(m, side, nxt):
                continue
            seen[nxt] = seen[cur] + 1
            if nxt in want:
                out[nxt] = seen[nxt]
                want.discard(nxt)
            q.append(nxt)
    return out


def players(m, side, t, g):
    """(pursuit action, evade action, dist) of one env: pursuit(), evade() and dist_out() from two floods instead of eleven —
    one from g for D(dest(t, a), g) = D(g, dest(t, a)) (D is symmetric: the grid's edges have no direction), one from t."""
    t, g = (int(t[0]), int(t[1])), (int(g[0]), int(g[1]))
    from_g = distances_from(m, side, g, [t] + [dest(t, a) for a in range(4)])
    from_t = distances_from(m, side, t, [g] + [dest(g, a) for a in range(4)])
    d = from_t[g]
    assert d == from_g[t]
    p = e = None
    if 0 < d < INF:
        p = next((a for a in range(4) if not is_wall(m, side, dest(t, a)) and from_g[dest(t, a)] == d - 1), None)
    if d < INF:
        e = next((a for a in range(4) if not is_wall(m, side, dest(g, a)) and from_t[dest(g, a)] == d + 1), None)
    return (hold(m, side, t) if p is None else p), (hold(m, side, g) if e is None else e), (-1 if d >= INF else d)


def batch(maps, pos, sides):
    """For maps u8 [N, 82, 82], pos [N, 2, 2] (tracker, target) and sides [N]: (act int64 [N, 2], dist int32 [N])."""
    n = len(sides)
    act, dist = np.zeros((n, 2), np.int64), np.zeros(n, np.int32)
    for e in range(n):
        side = int(sides[e])
        m = np.asarray(maps[e])[:side, :side]
        act[e, 0], act[e, 1], dist[e] = players(m, side, pos[e][0], pos[e][1])
    return act, dist
