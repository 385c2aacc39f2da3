/*
 * atr_fov.h — C ABI of facing and field of view in libtrack2d_hip.so: a player sees only a cone ahead. A 13 x 13 window as the env
 * writes it shows everything round the player, all the time; atr_fov_windows keeps one FACING byte per player, turns it with the
 * step's actions, and rewrites every window cell outside the player's cone as an "unseen" value. Like the occluded observations
 * (atr_occlusion.h) it is a pass over stored windows in a launch of its own (the env step is untouched). Unlike them it has state
 * (the facing bytes, which the caller owns) and it is not symmetric between the two players: the target behind the tracker sees a
 * tracker that does not see it.
 *
 * The RULE (csrc/atr_fov_rule.h holds it once, for host and device).
 *
 *   Geometry. A window is 13 x 13 cells, cell (r, c) at index r * 13 + c, centre (6, 6); the cell's offset is
 *   (dr, dc) = (r - 6, c - 6).
 *
 *   Facing. One byte per player. The values 0 .. 3 are the four VonNeumann moves of the reference (track_1v1.py:275-279) as
 *   (ur, uc): 0 = (-1, 0), 1 = (+1, 0), 2 = (0, -1), 3 = (0, +1). ATR_FOV_NONE = 255 means "looks all round". (Any other value is
 *   not a facing; the kernel treats it as NONE.)
 *
 *   Forward and lateral components. With facing (ur, uc): f = dr * ur + dc * uc and l = |dr * uc - dc * ur|.
 *
 *   Aperture. A cell is IN THE CONE if and only if f >= s * l, where the aperture sets s:
 *       90   s =  1   the quadrant ahead, diagonals included
 *       180  s =  0   the half plane ahead
 *       270  s = -1   all but the quadrant behind (whose diagonals stay visible)
 *       360  —        this player is not restricted: its windows are never touched (neither read nor written, in place or not)
 *
 *   Near radius. `near` (0 .. 6) keeps the cells with max(|dr|, |dc|) <= near always visible: a player feels what it touches.
 *
 *   Hidden value. A cell that is neither in the cone nor near is written as `hidden` (default ATR_FOV_HIDDEN = 5, the value of
 *   atr_occlusion.h; 0 .. 255). Every other cell is copied unchanged. Facing NONE leaves the window unchanged.
 *
 *   What follows:
 *     - the centre has f = l = 0 and is in every cone: it is never hidden;
 *     - hidden cells per window at near = 1: 115 / 75 / 35 for 90 / 180 / 270; at near = 0: 120 / 78 / 36;
 *     - the hidden sets nest: 270 inside 180 inside 90;
 *     - rotating a window by a quarter turn, and the facing with it, rotates the output;
 *     - the rule does not look at the window's cells: which cells are hidden depends on (facing, aperture, near) alone.
 *
 *   Turning. For player p of env e in one call, in this order:
 *     1. if `done` is given and done[e] != 0, the facing becomes NONE (with the env's in-launch auto-reset the stored window is the
 *        new episode's first, and it is seen all round);
 *     2. else, if player p's action array is given and its action a holds 0 <= a <= 3, the facing becomes a (a move that a wall
 *        blocks still turns the player);
 *     3. else the facing stays.
 *   The window is then restricted with the UPDATED facing. A new episode started by the caller (reset) starts from NONE: the
 *   caller fills the bytes, no launch is needed.
 *
 *   Order with occlusion. Occlusion runs first, then this pass: occlusion's verdicts read "cell == 1", and a 5 written by this
 *   pass would stop being a wall.
 *
 * atr_fov_windows — n_env * n_win windows (n_win 1 or 2), window (e, p) at ELEMENT e * se + p * sp of both src and dst (uint8 when
 *   is_u8 != 0, else float32), its 169 cells contiguous; facing byte (e, p) at facing[e * n_win + p], read and written. a0 / a1 are
 *   player 0's / player 1's actions, one per env, of type act_dtype (T2D_ACT_* of track2d.h), NULL = that player does not turn (a1
 *   is not looked at when n_win is 1); done is one byte per env, NULL = no episode turnover in this call. aperture0 / aperture1
 *   belong to player 0 / 1.
 *
 *   One wavefront owns window (e, p) and its facing byte: it computes the new facing, one lane stores it, and no other wavefront
 *   touches that byte. dst == src (in place) is allowed: only the hidden cells are stored, each by its own lane, a byte window's
 *   cells by byte, so that no lane writes outside its own window at any alignment; since the stored value does not depend on the
 *   window, an in-place call reads no window at all. With dst != src a wavefront reads its window whole before it writes any of
 *   it, and every cell of dst is written (except for a player of aperture 360). The windows of dst must not overlap one another
 *   (strides below 169 elements): the call does not check it.
 *
 * All pointers are device pointers; `stream` is a hipStream_t. The call enqueues ONE launch (capturable in a hipGraph; no
 * allocation, no atomics, no synchronisation) and returns 0 or a T2D_ERR_* code of include/track2d.h, with the text in
 * t2d_last_error(). Refused with T2D_ERR_INVALID before any device is touched: a null src / dst / facing, n_env <= 0 or n_win <= 0,
 * n_win > 2, more than ATR_FOV_MAX_WINDOWS windows, an aperture outside {90, 180, 270, 360}, near outside 0 .. 6, hidden outside
 * 0 .. 255, an act_dtype that is no T2D_ACT_* while an action pointer is given, a negative stride, float windows not 4-byte aligned,
 * src != dst whose byte ranges overlap.
 */
#ifndef ATR_FOV_H
#define ATR_FOV_H

#include "track2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ATR_FOV_WINDOW 169              /* cells of a 13 x 13 window */
#define ATR_FOV_SIDE 13
#define ATR_FOV_CENTRE 6                /* row and column of the window's centre */
#define ATR_FOV_NONE 255                /* the facing of a player that looks all round */
#define ATR_FOV_HIDDEN 5                /* the default `hidden` value (ATR_OCCLUDE_HIDDEN) */
#define ATR_FOV_NEAR 1                  /* the default `near` radius */
#define ATR_FOV_MAX_NEAR 6
#define ATR_FOV_MAX_WINDOWS 2147483647  /* n_env * n_win per call */

int atr_fov_windows(const void *src, void *dst, int is_u8, long long n_env, int n_win, long long se, long long sp,
                    unsigned char *facing, const void *a0, const void *a1, int act_dtype, const unsigned char *done,
                    int aperture0, int aperture1, int near, int hidden, void *stream);

#ifdef __cplusplus
}
#endif

#endif
