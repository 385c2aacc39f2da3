"""The rule of include/atr_occlusion.h in plain numpy loops, one cell at a time, written from the header's text (not from the kernel,
which works on bit masks, and not from a product module): the reference of the occlusion tests."""
import numpy as np

SIDE, WINDOW, CENTRE, WALL, HIDDEN = 13, 169, 6, 1, 5
OFFSETS = [(dr, dc) for dr in range(-6, 7) for dc in range(-6, 7) if (dr, dc) != (0, 0)]


def sgn(x):
    return (x > 0) - (x < 0)


def line(dr, dc):
    """L(dr, dc): the offsets of the line's cells, both end cells excluded."""
    m = max(abs(dr), abs(dc))
    return [(sgn(dr) * ((2 * k * abs(dr) + m) // (2 * m)), sgn(dc) * ((2 * k * abs(dc) + m) // (2 * m))) for k in range(1, m)]


def near_line(dr, dc):
    """A(X) for X = (6 + dr, 6 + dc): window cells."""
    return [(CENTRE + r, CENTRE + c) for r, c in line(dr, dc)]


def far_line(dr, dc):
    """B(X) = X + L(-dr, -dc): window cells."""
    return [(CENTRE + dr + r, CENTRE + dc + c) for r, c in line(-dr, -dc)]


def hidden_cells(window):
    """bool [13, 13]: the HIDDEN cells of one window (any dtype; a wall is a cell equal to 1)."""
    w = np.asarray(window).reshape(SIDE, SIDE)
    out = np.zeros((SIDE, SIDE), bool)
    for dr, dc in OFFSETS:
        a = any(w[r, c] == WALL for r, c in near_line(dr, dc))
        b = any(w[r, c] == WALL for r, c in far_line(dr, dc))
        out[CENTRE + dr, CENTRE + dc] = a and b
    return out


_NEAR = _FAR = None


def _masks():
    """bool [169, 169] twice: per cell X (flat), its near and its far line as flat window masks — the loops above, tabulated once."""
    global _NEAR, _FAR
    if _NEAR is None:
        _NEAR, _FAR = np.zeros((WINDOW, WINDOW), bool), np.zeros((WINDOW, WINDOW), bool)
        for dr, dc in OFFSETS:
            x = (CENTRE + dr) * SIDE + CENTRE + dc
            for r, c in near_line(dr, dc):
                _NEAR[x, r * SIDE + c] = True
            for r, c in far_line(dr, dc):
                _FAR[x, r * SIDE + c] = True
    return _NEAR, _FAR


def occlude(windows, hidden=HIDDEN):
    """A copy of windows [..., 13, 13] (or [..., 169]) with every hidden cell set to `hidden`: the tabulated form of hidden_cells
    for many windows (test_occlusion_cpu holds the two to one another)."""
    w = np.asarray(windows)
    flat = w.reshape(-1, WINDOW)
    near, far = _masks()
    walls = (flat == WALL).astype(np.int32)
    hid = (walls @ near.T.astype(np.int32) > 0) & (walls @ far.T.astype(np.int32) > 0)
    out = flat.copy()
    out[hid] = hidden
    return out.reshape(w.shape)


def random_windows(n, density, seed, dtype=np.uint8):
    """[n, 13, 13] over {0, 1, 2, 4}: walls with probability `density`, a 2 in the centre, one 4 somewhere else."""
    rs = np.random.RandomState(seed)
    w = (rs.random_sample((n, SIDE, SIDE)) < density).astype(dtype)
    spot = rs.randint(0, WINDOW, n)
    w.reshape(n, WINDOW)[np.arange(n), spot] = 4
    w[:, CENTRE, CENTRE] = 2
    return w


def window_of(grid, r, c):
    """The 13 x 13 window of a map (2-D array) centred on (r, c), padded with 1 outside the map, as the env writes it."""
    grid = np.asarray(grid)
    out = np.ones((SIDE, SIDE), grid.dtype)
    for i in range(SIDE):
        for j in range(SIDE):
            y, x = r - CENTRE + i, c - CENTRE + j
            if 0 <= y < grid.shape[0] and 0 <= x < grid.shape[1]:
                out[i, j] = grid[y, x]
    return out
