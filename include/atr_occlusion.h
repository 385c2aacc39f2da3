/*
 * atr_occlusion.h — C ABI of the occluded observations in libtrack2d_hip.so: walls hide what is behind them. A 13 x 13 window as
 * the env writes it shows everything inside it, through any number of walls; atr_occlude_windows rewrites windows so that every cell
 * whose line of sight from the window's centre is blocked by a wall holds an "unseen" value instead. It is a pass over stored
 * windows in a launch of its own (the env step is untouched), on both players' windows alike.
 *
 * The RULE. A window is 13 x 13 cells, cell (r, c) at index r * 13 + c, centre (6, 6). A wall is a cell equal to 1 (1.0f in a float
 * window); the padding the env writes outside the map is 1 and blocks like a wall. Every other value (0, 2, 4, 5, 255, ...) is free.
 *
 *   For an offset (dr, dc), L(dr, dc) is the LINE of include/atr_sight.h: with m = max(|dr|, |dc|), for k = 1 .. m-1 the offsets
 *   (sgn(dr) * ((2 k |dr| + m) / (2 m)), sgn(dc) * ((2 k |dc| + m) / (2 m))), integer division; both end cells are excluded.
 *
 *   For the cell X = (6 + dr, 6 + dc) two lines are tested:
 *     the near line  A(X) = (6, 6) + L(dr, dc)       (the line of the sight statistics: drawn from the centre)
 *     the far line   B(X) = X + L(-dr, -dc)          (the same rule drawn from the other end)
 *   X is HIDDEN if and only if A(X) holds a wall AND B(X) holds a wall. A hidden cell is written as the value `hidden` (default
 *   ATR_OCCLUDE_HIDDEN = 5: the reference's colour table, track_1v1.py:66, has seven entries 0 .. 6, of which a 1-v-1 env uses 0, 1,
 *   2 and 4). Every other cell is copied unchanged.
 *
 *   What follows:
 *     - the centre and all cells with m <= 1 have no line cell and are never hidden;
 *     - a wall whose lines are clear stays 1: the face of a wall is seen;
 *     - both lines lie inside the window, so the output is a pure function of the window's 169 cells (of "cell == 1" for the
 *       verdicts, of the cell itself for what is copied);
 *     - SYMMETRY: the two lines drawn between tracker T and target G are the same two sets of map cells whichever player looks
 *       (T's near line is G's far line and the other way round), so the tracker sees the target if and only if the target sees
 *       the tracker. The near line alone would not do: for 56 of the 168 offsets the two lines differ at a rounding tie. On an
 *       occluded store a target in range but hidden therefore has no cell 4 in window 0 AND no cell 2 in window 1: the bin of
 *       include/atr_track_stats.h / atr_sight.h is OUT, never INCONSISTENT.
 *
 * atr_occlude_windows — n_env * n_win windows, window (e, p) at ELEMENT e * se + p * sp of both src and dst (uint8 when is_u8 != 0,
 *   else float32), its 169 cells contiguous. dst == src (in place) is allowed: a wavefront reads its whole window before it writes
 *   any of it, and no lane stores outside its own window (byte windows start at any alignment; the dwords they share with their
 *   neighbours are read whole and written by byte). In place only the hidden cells are stored. The windows of dst must not overlap
 *   one another (strides below 169 elements): the call does not check it.
 *
 * Both pointers are device pointers; `stream` is a hipStream_t. The call enqueues ONE launch (capturable in a hipGraph; no
 * allocation, no atomics, no synchronisation) and returns 0 or a T2D_ERR_* code of include/track2d.h, with the text in
 * t2d_last_error(). Refused with T2D_ERR_INVALID before any device is touched: a null pointer, n_env <= 0 or n_win <= 0, more than
 * ATR_OCCLUDE_MAX_WINDOWS windows, a negative stride, hidden outside 0 .. 255, float windows not 4-byte aligned, src != dst whose
 * byte ranges overlap.
 */
#ifndef ATR_OCCLUSION_H
#define ATR_OCCLUSION_H

#include "track2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ATR_OCCLUDE_WINDOW 169              /* cells of a 13 x 13 window */
#define ATR_OCCLUDE_SIDE 13
#define ATR_OCCLUDE_CENTRE 6                /* row and column of the window's centre */
#define ATR_OCCLUDE_WALL 1                  /* the one value that blocks */
#define ATR_OCCLUDE_HIDDEN 5                /* the default `hidden` value */
#define ATR_OCCLUDE_MAX_WINDOWS 2147483647  /* n_env * n_win per call */

int atr_occlude_windows(const void *src, void *dst, int is_u8, long long n_env, long long n_win, long long se, long long sp,
                        int hidden, void *stream);

#ifdef __cplusplus
}
#endif

#endif
