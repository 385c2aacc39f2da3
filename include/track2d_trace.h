/*
 * track2d_trace.h — episode traces and the device renderer of libtrack2d_hip.so: the part of the gym protocol the
 * step/reset ABI (track2d.h) leaves out. Reference (G/ = envs/gym-track2d/gym_track2d/):
 *   info['traces'] / info['traces_relative']   G/envs/track_1v1.py:90-93,120-123,160-164
 *   Track1v1Env.render()                       G/envs/track_1v1.py:170-216
 *
 * The reference keeps a Python list per env and draws a matplotlib figure that needs a display. Here a per-env position
 * record lives on the device, kept by ONE small launch per step (t2d_trace_append), and a HIP rasteriser turns (map tile,
 * positions, record) into cell images (the parity surface) or RGB frames. Nothing here runs unless it is called: the step
 * kernels do not know about the record.
 *
 * Conventions are those of track2d.h (status codes, t2d_last_error, "dev" / "host" pointers, `stream`).
 *
 * The store (owned by the handle, freed by t2d_destroy):
 *   pos     i16 [N][capacity + 1][2 agents][r, c]   slot 0: both spawns; slot k >= 1: both agents' cells after the
 *                                                   episode's k-th step (the same cell again after a wall bump)
 *   len     i32 [N]                                 slots written
 *   closed  u8  [N]                                 the episode has ended: no append writes the env until a begin names it
 *   dropped u32 [N]                                 appends refused because the env's slots were full
 * info['traces'] of the reference is [pos[0][tracker]] + [pos[k][target] for k >= 1]: its first entry is the TRACKER's
 * spawn (track_1v1.py:163), every later one the TARGET's cell (:120).
 *
 * Only for handles created with auto_reset = 0. With auto_reset = 1 a terminal step has already replaced the env's state
 * with the next episode's spawn when it returns, so the last cell of an episode cannot be recorded from outside the step
 * kernels; t2d_trace_attach refuses such a handle.
 *
 * Bad env ids: env_ids lives on the device, and the render calls do not synchronise. A listed id outside [0, N) is
 * CLAMPED into range by the kernel (the frame shows env 0 or N - 1) and bit 5 of the handle's sticky fault word
 * (t2d_get_faults, T2D_FAULT_RENDER_ID) is set. A caller that holds the ids on the host checks them there (the Python
 * binding does). Every other bad argument is refused by the return code before anything is launched.
 */
#ifndef TRACK2D_TRACE_H
#define TRACK2D_TRACE_H

#include <stdint.h>

#include "track2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define T2D_RENDER_TRACE 1            /* flags bit 0: paint the trace (value 6); without it nothing is painted 6 */
#define T2D_FAULT_RENDER_ID 32u       /* fault word bit 5: a render call listed an env id outside [0, N) */
#define T2D_RENDER_CELLS_H 82         /* canvas, in cells: the map panel (T2D_MAX_SIDE wide), a 2-cell gap, the tracker's */
#define T2D_RENDER_CELLS_W 162        /* window at 6 canvas cells per window cell: 82 + 2 + 13 * 6 */
#define T2D_RENDER_MAX_SCALE 8
#define T2D_RENDER_OUTSIDE 255        /* render_cells: a cell outside the env's own side x side map */

/* Allocate the store for `capacity` steps per episode (capacity in [1, 65535]; a second attach replaces the store).
 * Refused on an auto_reset = 1 handle (see above). Synchronises. */
int t2d_trace_attach(t2d_handle *h, int capacity, void *stream);

/* Track1v1Env.reset()'s `traces = [init_states[0]]` (track_1v1.py:160-164). Call after t2d_reset / t2d_inject: for every
 * env whose mask byte is non-zero (mask_dev == NULL: all) slot 0 takes both current positions, len = 1, closed = 0,
 * dropped = 0. One launch, no synchronisation. */
int t2d_trace_begin(t2d_handle *h, const uint8_t *mask_dev_or_null, void *stream);

/* Track1v1Env.step()'s `traces.append(state[1])` (track_1v1.py:120). Call after a step with its done bytes [N]: every open
 * env with room writes both current positions to slot `len` and increments len; an env whose slots are full writes
 * nothing and counts a drop; then closed |= done. One launch; neither allocates nor synchronises (capturable). */
int t2d_trace_append(t2d_handle *h, const uint8_t *done_dev, void *stream);

/* Read back envs [first, first + count): pos_host i16 [count][capacity + 1][2][2], len_host i32 [count], dropped_host
 * u32 [count]; any may be NULL. Slots at and beyond len are unspecified. Synchronises. */
int t2d_trace_get(t2d_handle *h, int first, int count, int16_t *pos_host, int32_t *len_host, uint32_t *dropped_host,
                  void *stream);

/* The cells render() would draw, for env env_ids[i], i < count (ids may repeat, in any order):
 *   cells_dev   u8 [count][82][82]: _get_full_obs() (map 0 / 1, then the tracker's cell 2, then the target's 4: the target
 *               wins when co-located), then — with T2D_RENDER_TRACE — every cell of traces[:-1] set to 6, AFTER the agents
 *               (track_1v1.py:177-182, with the cell indexing the line intends); T2D_RENDER_OUTSIDE beyond the env's side.
 *               May be NULL. 4-byte aligned.
 *   partial_dev u8 [count][13][13]: _get_partial_obs(0, 6), the tracker's window, never painted 6; out of the map -> 1.
 *               May be NULL.
 * One launch; neither allocates nor synchronises (capturable). */
int t2d_render_cells(t2d_handle *h, const int32_t *env_ids_dev, int count, int flags, uint8_t *cells_dev,
                     uint8_t *partial_dev, void *stream);

/* One RGB frame per listed env: 82 * scale rows of 162 * scale pixels, 3 bytes each, rows pitch_bytes apart, frames
 * 82 * scale * pitch_bytes apart. Left: the painted map of t2d_render_cells at `scale` pixels per cell; a 2-cell gap;
 * right, top-aligned: the tracker's window at 6 * scale pixels per cell. Colours: the reference's ListedColormap
 * (track_1v1.py:66-68) for the values 0, 1, 2, 4, 6; everything that is in neither panel (the gap, below the window, cells
 * outside the env's side) is (128, 128, 128). The bytes of a row past 486 * scale are written as 0.
 * scale in [1, T2D_RENDER_MAX_SCALE]; pitch_bytes a multiple of 16, >= 486 * scale; rgb_dev 16-byte aligned.
 * One launch; neither allocates nor synchronises (capturable). */
int t2d_render_rgb(t2d_handle *h, const int32_t *env_ids_dev, int count, int scale, int flags, uint8_t *rgb_dev,
                   int pitch_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
