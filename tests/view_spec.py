"""The player views' rule (include/atr_view.h) in numpy, twice: plain loops over one frame (frame_cells, frame_rgb) and array
form (view_cells, view_rgb). The tests hold the two against each other and the library against both."""
import numpy as np

SIDE, WIN, POB, WINDOW = 82, 13, 6, 169
UNKNOWN, OUTSIDE, HIDDEN = 15, 255, 5
BAND_HIDDEN, BAND_BEYOND = 16, 32
CELLS_H, CELLS_W, GAP, ZOOM = 82, 242, 2, 6
WIN_ROWS, WIN0_X0, WIN1_X0 = 78, 84, 164
KNOWN = (0, 1, 2, 4, 5, 6, 7, 8)
NONE = 255                                   # the facing of a player that looks all round (atr_fov.h)
# r | g << 8 | b << 16, as include/atr_view.h writes them
RGB = {0: 0xFFFFFF, 1: 0x000000, 2: 0xFF0000, 4: 0x0000FF, 5: 0x505050, 6: 0x00FFFF, 7: 0x303060, 8: 0xC0C0E8, 15: 0xFF00FF}
BACKGROUND = 0x808080


def channels(rgb):
    return (rgb & 255, (rgb >> 8) & 255, (rgb >> 16) & 255)


def code_rgb(code):
    """(r, g, b) of a code."""
    band, v = code >> 4, code & 15
    if band == 0 and v in RGB:
        return channels(RGB[v])
    if band == 1 and v in (0, 1, 2, 4):
        return tuple((c + 128) >> 1 for c in channels(RGB[v]))
    if band == 2 and v in (0, 1, 2, 4):
        return tuple((c + 384) >> 2 for c in channels(RGB[v]))
    return channels(BACKGROUND)


PALETTE = np.array([code_rgb(c) for c in range(256)], np.uint8)          # [256, 3]


def known(v):
    """The code of one window value (a Python or numpy scalar, int or float)."""
    for k in KNOWN:
        if v == k:
            return k
    return UNKNOWN


def heading_of(facing):
    return int(facing) if 0 <= int(facing) <= 3 else 0


def src_cell(h, cell):
    """atr_ego's cell map: the cell of the absolute window that cell `cell` of the window turned by heading h shows."""
    er, ec = cell // WIN - POB, cell % WIN - POB
    ur, uc = ((-1, 0), (1, 0), (0, -1), (0, 1))[h]
    return (POB + (-er * ur + ec * uc)) * WIN + POB + (-er * uc - ec * ur)


def truth(maze, side, pos, r, c):
    v = int(maze[r, c])
    if (r, c) == (int(pos[0][0]), int(pos[0][1])):
        v = 2
    if (r, c) == (int(pos[1][0]), int(pos[1][1])):
        v = 4
    return v


def frame_cells(maze, side, pos, windows, facing, turned, viewer):
    """Loops, one frame: maze [82, 82] (0 / 1), side, pos [2][2], windows [2, 13, 13] (any dtype), facing [2] or None.
    Returns (cells u8 [82, 82], windows u8 [2, 13, 13])."""
    wc = np.zeros((2, WINDOW), np.uint8)
    for p in range(2):
        flat = np.asarray(windows[p]).reshape(-1)
        for i in range(WINDOW):
            wc[p, i] = known(flat[i])
    w_abs = wc[viewer].copy()
    if (turned >> viewer) & 1:
        h = heading_of(facing[viewer])
        for i in range(WINDOW):
            w_abs[src_cell(h, i)] = wc[viewer, i]
    pr, pc = int(pos[viewer][0]), int(pos[viewer][1])
    cells = np.full((SIDE, SIDE), OUTSIDE, np.uint8)
    for r in range(min(int(side), SIDE)):
        for c in range(min(int(side), SIDE)):
            t = truth(maze, side, pos, r, c)
            dr, dc = r - pr, c - pc
            if abs(dr) > POB or abs(dc) > POB:
                cells[r, c] = BAND_BEYOND + t
            else:
                w = int(w_abs[(POB + dr) * WIN + POB + dc])
                cells[r, c] = BAND_HIDDEN + t if w == HIDDEN else w
    return cells, wc.reshape(2, WIN, WIN)


def frame_rgb(cells, windows, scale, pitch):
    """Loops, one frame: u8 [82 * scale, pitch] from the codes (pad bytes 0)."""
    out = np.zeros((CELLS_H * scale, pitch), np.uint8)
    for cy in range(CELLS_H):
        for cx in range(CELLS_W):
            code = OUTSIDE
            if cx < SIDE:
                code = int(cells[cy, cx])
            elif WIN0_X0 <= cx < WIN0_X0 + WIN_ROWS and cy < WIN_ROWS:
                code = int(windows[0, cy // ZOOM, (cx - WIN0_X0) // ZOOM])
            elif cx >= WIN1_X0 and cy < WIN_ROWS:
                code = int(windows[1, cy // ZOOM, (cx - WIN1_X0) // ZOOM])
            rgb = code_rgb(code)
            for sy in range(scale):
                for sx in range(scale):
                    x = 3 * (cx * scale + sx)
                    out[cy * scale + sy, x:x + 3] = rgb
    return out


# -- array form -------------------------------------------------------------------------------------------------------------------

def window_codes(windows):
    """u8 codes of windows of any shape and dtype."""
    w = np.asarray(windows)
    out = np.full(w.shape, UNKNOWN, np.uint8)
    for k in KNOWN:
        out[w == k] = k
    return out


_SRC = np.array([[src_cell(h, i) for i in range(WINDOW)] for h in range(4)])


def view_cells(maps, side, pos, windows, facing, turned, viewer):
    """Arrays: maps [F, 82, 82], side [F], pos [F, 2, 2], windows [F, 2, 13, 13], facing [F, 2] or None -> (cells u8 [F, 82, 82],
    windows u8 [F, 2, 13, 13]), frame by frame the inputs' rows."""
    maps, side, pos = np.asarray(maps), np.asarray(side).astype(np.int64), np.asarray(pos).astype(np.int64)
    f = maps.shape[0]
    wc = window_codes(windows).reshape(f, 2, WINDOW)
    w_abs = wc[:, viewer].copy()
    if (turned >> viewer) & 1:
        fac = np.asarray(facing)[:, viewer].astype(np.int64)
        h = np.where((fac >= 0) & (fac <= 3), fac, 0)
        w_abs = np.zeros_like(w_abs)
        np.put_along_axis(w_abs, _SRC[h], wc[:, viewer], axis=1)
    rr, cc = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
    rr, cc = rr[None], cc[None]
    t = maps.astype(np.int64).copy()
    ar = np.arange(f)
    t[ar, pos[:, 0, 0], pos[:, 0, 1]] = 2
    t[ar, pos[:, 1, 0], pos[:, 1, 1]] = 4
    dr, dc = rr - pos[:, viewer, 0, None, None], cc - pos[:, viewer, 1, None, None]
    inside = (np.abs(dr) <= POB) & (np.abs(dc) <= POB)
    idx = np.clip((POB + dr) * WIN + POB + dc, 0, WINDOW - 1)
    w = np.take_along_axis(w_abs, idx.reshape(f, -1), axis=1).reshape(f, SIDE, SIDE).astype(np.int64)
    cells = np.where(~inside, BAND_BEYOND + t, np.where(w == HIDDEN, BAND_HIDDEN + t, w))
    out_of_map = (rr >= side[:, None, None]) | (cc >= side[:, None, None])
    return np.where(out_of_map, OUTSIDE, cells).astype(np.uint8), wc.reshape(f, 2, WIN, WIN)


def canvas_codes(cells, windows):
    """u8 [F, 82, 242]: the code of every canvas cell."""
    f = cells.shape[0]
    canvas = np.full((f, CELLS_H, CELLS_W), OUTSIDE, np.uint8)
    canvas[:, :, :SIDE] = cells
    for p, x0 in ((0, WIN0_X0), (1, WIN1_X0)):
        canvas[:, :WIN_ROWS, x0:x0 + WIN_ROWS] = np.repeat(np.repeat(windows[:, p], ZOOM, axis=1), ZOOM, axis=2)
    return canvas


def view_rgb(cells, windows, scale, pitch):
    """Arrays: u8 [F, 82 * scale, pitch] from cells [F, 82, 82] and windows [F, 2, 13, 13] (pad bytes 0)."""
    img = PALETTE[canvas_codes(np.asarray(cells), np.asarray(windows))]                  # [F, 82, 242, 3]
    img = np.repeat(np.repeat(img, scale, axis=1), scale, axis=2).reshape(img.shape[0], CELLS_H * scale, -1)
    out = np.zeros((img.shape[0], CELLS_H * scale, pitch), np.uint8)
    out[:, :, :img.shape[2]] = img
    return out
