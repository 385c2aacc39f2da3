/*
 * atr_view.h — C ABI of the player views in libtrack2d_hip.so: draw the 13 x 13 windows the players were actually handed, and
 * project one player's window back onto the map. The renderer of track2d_trace.h rebuilds the tracker's window from the map tile,
 * so it cannot show what the passes over stored windows (atr_occlusion.h, atr_fov.h, atr_footprints.h, atr_memory.h, atr_noise.h,
 * atr_ego.h) made of it: a hidden cell, a print, a remembered wall, a ghost, a turned window. This one reads the windows
 * themselves. It needs no trace store, changes nothing in the env and knows none of those passes' rules.
 *
 * The RULE (csrc/atr_view_rule.h holds its arithmetic once, for host and device).
 *
 *   Inputs. The handle's current map tile, side and both positions. The 2 N windows as the players were given them, window
 *   (e, p) at ELEMENT e * se + p * sp of obs (uint8 when is_u8 != 0, else float32), its 169 cells contiguous. Optionally the
 *   facing bytes, u8 [N][2] (the byte of atr_fov.h). `turned`, 0 .. 3: bit p is set when window p was turned by the egocentric
 *   pass (atr_ego.h).
 *
 *   Known values. A window cell is known when it reads exactly one of 0, 1, 2, 4, 5, 6, 7, 8 (in a float window it must equal
 *   that integer exactly). Anything else — 3, 9, 255, 0.5, a NaN — is ATR_VIEW_UNKNOWN = 15.
 *
 *   Truth. T(r, c) is the map bit, then 2 on the tracker's cell, then 4 on the target's (the target wins when co-located): the
 *   renderer's painted cell without the trace.
 *
 *   The viewer's absolute window. `viewer` is 0 (tracker) or 1 (target). If bit `viewer` of `turned` is set, the given window E
 *   is un-turned with h = the heading of facing[e][viewer] (0 .. 3 is itself, anything else looks up: 0):
 *   W[src_cell(h, cell)] = E[cell] for all 169 cells, src_cell of atr_ego.h — a rotation, hence a bijection. Otherwise W = E.
 *
 *   The map panel's code of map cell (r, c), the viewer standing at (pr, pc):
 *     r >= side or c >= side                                    255 (ATR_VIEW_OUTSIDE)
 *     (r - pr, c - pc) outside [-6, 6] x [-6, 6]                32 + T     outside the window: the truth
 *     else w = W[(6 + r - pr) * 13 + 6 + c - pc] is 5           16 + T     hidden: the truth
 *     w one of 0, 1, 2, 4, 6, 7, 8                              w          what the player was told, lies and prints included
 *     w unknown                                                 15
 *   A code is band * 16 + value: band 0 is what the viewer was shown, bands 1 and 2 are what is really there where the viewer was
 *   shown nothing.
 *
 *   The window panels. Both windows as given (a turned window stays turned: that is what the policy saw), each cell a known value
 *   or 15.
 *
 *   Colours (the ATR_VIEW_RGB_* macros, r | g << 8 | b << 16). Band 0 and the window panels use the colour of the value; 0, 1, 2,
 *   4 and 6 are the renderer's. Band 1 is, per channel, (c + 128) >> 1 of T's colour and band 2 is (c + 384) >> 2. Code 255,
 *   anything that is no code, and every canvas cell in no panel: ATR_VIEW_RGB_BACKGROUND.
 *
 *   The canvas: ATR_VIEW_CELLS_H = 82 rows of ATR_VIEW_CELLS_W = 242 cells. Map panel columns 0 .. 81; a 2-cell gap; the
 *   tracker's window at 6 canvas cells per window cell, columns 84 .. 161, rows 0 .. 77; a 2-cell gap; the target's window,
 *   columns 164 .. 241. RGB is `scale` pixels per canvas cell (1 .. ATR_VIEW_MAX_SCALE), 3 bytes per pixel; rows are pitch_bytes
 *   apart (a multiple of 16, at least 726 * scale), frames 82 * scale * pitch_bytes apart; row bytes past 726 * scale are
 *   written 0.
 *
 * atr_view_cells — frame k is env env_ids[k]: cells u8 [count][82][82] (the map panel's codes; 4-byte aligned) and / or windows
 *   u8 [count][2][169] (the window panels' codes). Either may be NULL, not both.
 * atr_view_rgb — frame k is env env_ids[k], rgb 16-byte aligned.
 *
 * All pointers but h are device pointers; `stream` is a hipStream_t. env_ids are int32, may repeat and come in any order; an id
 * outside [0, N) is clamped into it and bit 5 of the handle's fault word (T2D_FAULT_RENDER_ID of track2d_trace.h) is set. Each
 * call enqueues ONE launch (capturable in a hipGraph; no allocation, no synchronisation, no atomics but that fault bit) and
 * returns 0 or a T2D_ERR_* code of include/track2d.h, with the text in t2d_last_error(). Refused with T2D_ERR_INVALID before the
 * handle is looked at, in this order: a null obs; a null env_ids; both outputs null (cells) / a null rgb; count outside
 * 1 .. 65535; viewer outside 0 .. 1; turned outside 0 .. 3; turned != 0 with a null facing; a negative stride; float windows not
 * 4-byte aligned; cells not 4-byte aligned (cells) / scale outside 1 .. 8, then a pitch that is no multiple of 16 or below
 * 726 * scale, then rgb not 16-byte aligned (rgb); a null h. Refused after that, from the handle's state: a handle that was never
 * reset (all envs), a handle with whole-map ('Full') observations.
 */
#ifndef ATR_VIEW_H
#define ATR_VIEW_H

#include "track2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ATR_VIEW_UNKNOWN 15             /* a window cell that reads no known value */
#define ATR_VIEW_OUTSIDE 255            /* a map cell outside the env's own side x side map */
#define ATR_VIEW_HIDDEN 5               /* the window value of a cell the player was shown nothing of */
#define ATR_VIEW_BAND_HIDDEN 16         /* code 16 + T: hidden in the viewer's window, the truth */
#define ATR_VIEW_BAND_BEYOND 32         /* code 32 + T: outside the viewer's window, the truth */
#define ATR_VIEW_CELLS_H 82             /* canvas, in cells */
#define ATR_VIEW_CELLS_W 242            /* 82 + 2 + 13 * 6 + 2 + 13 * 6 */
#define ATR_VIEW_WINDOW 169
#define ATR_VIEW_MAX_SCALE 8

#define ATR_VIEW_RGB_FREE 0xFFFFFF      /* value 0 */
#define ATR_VIEW_RGB_WALL 0x000000      /* value 1 */
#define ATR_VIEW_RGB_TRACKER 0xFF0000   /* value 2 */
#define ATR_VIEW_RGB_TARGET 0x0000FF    /* value 4 */
#define ATR_VIEW_RGB_UNSEEN 0x505050    /* value 5 (window panels only) */
#define ATR_VIEW_RGB_PRINT 0x00FFFF     /* value 6 */
#define ATR_VIEW_RGB_MEM_WALL 0x303060  /* value 7: a remembered wall */
#define ATR_VIEW_RGB_MEM_FREE 0xC0C0E8  /* value 8: remembered free */
#define ATR_VIEW_RGB_UNKNOWN 0xFF00FF   /* value 15 */
#define ATR_VIEW_RGB_BACKGROUND 0x808080

int atr_view_cells(t2d_handle *h, const void *obs, int is_u8, long long se, long long sp, const unsigned char *facing, int turned,
                   const int *env_ids, int count, int viewer, unsigned char *cells, unsigned char *windows, void *stream);
int atr_view_rgb(t2d_handle *h, const void *obs, int is_u8, long long se, long long sp, const unsigned char *facing, int turned,
                 const int *env_ids, int count, int viewer, int scale, unsigned char *rgb, int pitch_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
