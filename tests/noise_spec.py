"""Host model of sensor noise, as include/atr_noise.h states it (plain numpy, no project import; the Philox4x32-10 is
tests/draw_spec.py's, which reproduces the three Random123 known-answer vectors — KAT below).

Window p of env e is player p's view (0 tracker, 1 target); the centre is cell 84; the other player's value is O = 4 in window 0
and 2 in window 1. `roles` (1, 2, 3) says which windows are noisy: bit 0 the tracker's, bit 1 the target's. A window whose bit is
clear is neither read nor written and its clock does not move.

A probability is an integer threshold t in 0 .. ONE = 1 << 24; an event with 32-bit word w happens iff (w >> 8) < t.

Clock uint32 [N, 2]. ADVANCE: clock[e, p] += 1 (wrapping) and the draws use the new value. PEEK: the draws use the value as it
stands, nothing is stored.

Draws: Philox4x32-10, key (key & 0xFFFFFFFF, key >> 32), counter (global env id, clock, p, TAG ^ block), TAG = 0x4E5E0000.
Block 0: w0 decides the miss, w1 the ghost, the ghost's cell is g = (w2 * 169) >> 32. Block 1 + L, L = 0 .. 63: word j is the
flicker word of cell L + 64 j (j = 0, 1, 2; cells below 169).

Verdicts, all from the window as it reads before any store:
  1. flicker: a cell i != 84 reading exactly 0 or 1 whose flicker word passes `flicker` is written 1 - v;
  2. miss: if w0 passes `miss`, every cell i != 84 reading O is written 0;
  3. ghost: if w1 passes `ghost`, g != 84 and cell g read exactly 0, cell g is written O; there the ghost wins over a flicker.
Nothing else changes."""
import numpy as np

from draw_spec import philox4x32_10

WINDOW, SIDE, CENTRE = 169, 13, 84
ONE = 1 << 24
TAG = 0x4E5E0000
PEEK, ADVANCE = 0, 1
KEY_SALT = 0x6E6F6973655F7632
M64 = 2 ** 64 - 1

# Random123's known-answer vectors for philox4x32_10: (counter, key, output)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def key_of(seed):
    return (int(seed) & M64) ^ KEY_SALT


def threshold_of(p):
    return int(round(float(p) * ONE))


def other_value(p):
    return 2 if p else 4


def block(key, env, clock, p, blk):
    """The four uint32 words of block `blk` of window (global env id `env`, player p) at clock value `clock`; env, clock, p and
    blk may be arrays (broadcast)."""
    key = int(key) & M64
    c3 = np.asarray(blk).astype(np.uint64) ^ np.uint64(TAG)
    return philox4x32_10([env, clock, p, c3], [key & 0xFFFFFFFF, key >> 32])


def passes(w, t):
    return (np.asarray(w).astype(np.uint64) >> np.uint64(8)) < np.uint64(t)


def ghost_cell(w2):
    return ((np.asarray(w2).astype(np.uint64) * np.uint64(WINDOW)) >> np.uint64(32)).astype(np.int64)


def flicker_words(key, env, clock, p):
    """uint32 [..., 169]: the flicker word of every cell of the windows (env, clock, p) (arrays of one shape, or scalars)."""
    env, clock, p = np.broadcast_arrays(np.asarray(env), np.asarray(clock), np.asarray(p))
    w = block(key, env[..., None], clock[..., None], p[..., None], 1 + np.arange(64))        # four arrays [..., 64]
    return np.concatenate(w[:3], -1)[..., :WINDOW]          # (cell L + 64 j sits at index 64 j + L)


def apply_window(win, key, env, clock, p, thresholds):
    """One window in plain loops: `win` the 169 cells as they read, (env, clock, p) the counter the draws use. Returns the new
    169 cells."""
    flicker, miss, ghost = thresholds
    win = np.asarray(win).reshape(WINDOW)
    out = win.copy()
    O = other_value(p)
    w0, w1, w2, _ = [int(x) for x in block(key, env, clock, p, 0)]
    miss_hit, ghost_hit, g = (w0 >> 8) < miss, (w1 >> 8) < ghost, (w2 * WINDOW) >> 32
    for i in range(WINDOW):
        if i == CENTRE:
            continue
        v = win[i]
        fw = int(block(key, env, clock, p, 1 + (i & 63))[i >> 6])
        if ghost_hit and i == g and v == 0:
            out[i] = O
        elif (v == 0 or v == 1) and (fw >> 8) < flicker:
            out[i] = 1 - v
        elif v == O and miss_hit:
            out[i] = 0
    return out


def apply(windows, clock, key, thresholds, roles, mode, env_base=0):
    """All windows at once. windows [N, 2, 13, 13] (any integer or float dtype), clock uint32 [N, 2]. Returns (new windows, new
    clock); neither input is changed."""
    flicker, miss, ghost = thresholds
    windows = np.asarray(windows)
    n = windows.shape[0]
    assert windows.shape == (n, 2, SIDE, SIDE) and mode in (PEEK, ADVANCE) and roles in (1, 2, 3)
    clock = np.asarray(clock, np.uint32).reshape(n, 2)
    noisy = np.array([(roles >> p) & 1 for p in (0, 1)], bool)[None, :].repeat(n, 0)          # [N, 2]
    used = (clock.astype(np.uint64) + np.uint64(1 if mode == ADVANCE else 0)).astype(np.uint32)          # (wraps)
    new_clock = np.where(noisy, used, clock).astype(np.uint32)
    env = (np.uint64(env_base) + np.arange(n, dtype=np.uint64))[:, None].repeat(2, 1) & np.uint64(0xFFFFFFFF)
    p = np.arange(2)[None, :].repeat(n, 0)
    win = windows.reshape(n, 2, WINDOW)
    b0 = block(key, env, used, p, 0)
    miss_hit, ghost_hit, g = passes(b0[0], miss), passes(b0[1], ghost), ghost_cell(b0[2])          # [N, 2]
    fw = flicker_words(key, env, used, p)                                                        # [N, 2, 169]
    cells = np.arange(WINDOW)[None, None, :]
    off = cells != CENTRE
    O = np.array([4, 2])[None, :, None]
    is_ghost = ghost_hit[..., None] & (cells == g[..., None]) & (win == 0) & off
    is_flick = ((win == 0) | (win == 1)) & passes(fw, flicker) & off & ~is_ghost
    is_miss = (win == O) & miss_hit[..., None] & off
    out = win.copy()
    out[is_flick] = (1 - win)[is_flick]
    out[is_miss] = 0
    out = np.where(is_ghost, O.astype(win.dtype), out)
    out = np.where(noisy[..., None], out, win)
    return out.reshape(windows.shape).astype(windows.dtype), new_clock
