"""Host model of the episode traces and the renderer (include/track2d_trace.h): what the device must produce, computed from
(map, spawns, actions) alone in plain numpy. Reference: envs/gym-track2d/gym_track2d/envs/track_1v1.py:71-127 (step),
:160-164 (reset), :170-216 (render), :295-326 (the two observations).

Used by tests/test_traces_cpu.py (against the reference's own record, tests/golden/traces.npz) and tests/test_traces_gpu.py."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MOVES = {0: (-1, 0), 1: (1, 0), 2: (0, -1), 3: (0, 1)}
OUTSIDE = 255
CANVAS_H, CANVAS_W, WIN_X0, WIN_ZOOM, WIN = 82, 162, 84, 6, 13
BACKGROUND = (128, 128, 128)


def load_fixture():
    """The episodes of tests/golden/traces.npz as dicts, plus the palette {value: (r, g, b)}."""
    g = np.load(os.path.join(GOLDEN, "traces.npz"))
    eps = []
    for name in [str(n) for n in g["names"]]:
        p = name + "/"
        side = int(g[p + "side"])
        maze = np.unpackbits(g[p + "maze"])[: side * side].reshape(side, side).astype(np.uint8)
        ep = dict(name=name, env_id=str(g[p + "env_id"]), maze=maze, side=side)
        for k in ("init", "rel0", "cells0", "full0", "partial0", "actions", "done", "pos", "traces", "rel", "cells", "full", "partial"):
            ep[k] = g[p + k]
        eps.append(ep)
    palette = {int(v): tuple(int(x) for x in rgb) for v, rgb in zip(g["palette_values"], g["palette"])}
    return eps, palette, g["coverage"]


def step_state(maze, state, actions):
    """_next_state for both agents (VonNeumann): a move into a wall leaves the agent where it is."""
    out = []
    for (r, c), a in zip(state, actions):
        dr, dc = MOVES[int(a)]
        nr, nc = r + dr, c + dc
        out.append([r, c] if maze[nr][nc] == 1 else [nr, nc])
    return out


def positions(maze, init, actions):
    """[T + 1][2][2]: slot 0 the spawns, slot k both agents' cells after the k-th step — the device store's `pos`."""
    state = [[int(v) for v in init[0]], [int(v) for v in init[1]]]
    out = [state]
    for a in actions:
        state = step_state(maze, state, a)
        out.append(state)
    return out


def traces(pos, t):
    """info['traces'] after step t (t = 0: after reset): the TRACKER's spawn, then the TARGET's cell of every step."""
    return [list(pos[0][0])] + [list(pos[k][1]) for k in range(1, t + 1)]


def traces_relative(pos, t):
    """info['traces_relative'] after step t >= 1: per j, [s_i - s_j for i in 0, 1] on the CURRENT states (init_states aliases
    state); t = 0 (reset): the flat [s_i - s_0 for i in 0, 1]."""
    s = np.array(pos[t], np.int32)
    if t == 0:
        return [s[i] - s[0] for i in range(2)]
    return [[s[i] - s[j] for i in range(2)] for j in range(2)]


def full_obs(maze, state):
    obs = np.array(maze, np.uint8)
    obs[state[0][0], state[0][1]] = 2
    obs[state[1][0], state[1][1]] = 4          # the target wins when co-located
    return obs


def pad82(a):
    out = np.full((82, 82), OUTSIDE, np.uint8)
    out[: a.shape[0], : a.shape[1]] = a
    return out


def cells(maze, pos, t, trace=True):
    """u8 [82, 82]: the painted full observation render() draws after step t; OUTSIDE beyond the env's side."""
    obs = full_obs(maze, pos[t])
    if trace:
        for r, c in traces(pos, t)[:-1]:       # painted AFTER the agents; not the latest entry
            obs[r, c] = 6
    return pad82(obs)


def partial(maze, pos, t):
    """u8 [13, 13]: _get_partial_obs(0, 6) — the tracker's own cell is re-painted 2, out of the map is wall."""
    side = maze.shape[0]
    obs = full_obs(maze, pos[t])
    tr, tc = pos[t][0]
    obs[tr, tc] = 2
    out = np.ones((WIN, WIN), np.uint8)
    for i in range(WIN):
        for j in range(WIN):
            r, c = tr - 6 + i, tc - 6 + j
            if 0 <= r < side and 0 <= c < side:
                out[i, j] = obs[r, c]
    return out


def rgb(cells82, partial13, palette, scale):
    """u8 [82 * scale, 162 * scale, 3]: the fixed canvas of t2d_render_rgb from the cells, the window and the palette."""
    lut = np.zeros((256, 3), np.uint8)
    lut[:] = BACKGROUND
    for v, c in palette.items():
        lut[v] = c
    canvas = np.full((CANVAS_H, CANVAS_W), OUTSIDE, np.uint8)
    canvas[:, :82] = cells82
    canvas[: WIN * WIN_ZOOM, WIN_X0:] = np.kron(partial13, np.ones((WIN_ZOOM, WIN_ZOOM), np.uint8))
    img = lut[canvas]
    return np.repeat(np.repeat(img, scale, axis=0), scale, axis=1)


def decode_png(data):
    """Decode an 8-bit RGB, non-interlaced PNG by hand (zlib + the five row filters) -> u8 [H, W, 3]."""
    import struct
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    off, idat, hdr = 8, b"", None
    while off < len(data):
        n, kind = struct.unpack(">I4s", data[off:off + 8])
        body = data[off + 8:off + 8 + n]
        assert struct.unpack(">I", data[off + 8 + n:off + 12 + n])[0] == (zlib.crc32(kind + body) & 0xFFFFFFFF), kind
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        off += 12 + n
    w, h, depth, ctype, comp, flt, lace = hdr
    assert (depth, ctype, comp, flt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    out = np.zeros((h, 3 * w), np.uint8)
    for y in range(h):
        f, line = int(raw[y, 0]), raw[y, 1:].astype(np.int32)
        prev = out[y - 1].astype(np.int32) if y else np.zeros(3 * w, np.int32)
        if f == 0:
            out[y] = line
        elif f == 2:
            out[y] = (line + prev) & 255
        else:                                   # Sub / Average / Paeth run along the row
            cur = np.zeros(3 * w, np.int32)
            for x in range(3 * w):
                a = cur[x - 3] if x >= 3 else 0
                b = prev[x]
                c = prev[x - 3] if x >= 3 else 0
                if f == 1:
                    p = a
                elif f == 3:
                    p = (a + b) // 2
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[x] = (line[x] + p) & 255
            out[y] = cur
    return out.reshape(h, w, 3)
