/*
 * atr_memory.h — C ABI of map memory in libtrack2d_hip.so: a cell of a player's 13 x 13 window that reads "unseen" (5: behind a
 * wall, atr_occlusion.h; outside the cone, atr_fov.h) shows whether the map has a wall there, if the player has ever seen that
 * cell in this episode. It is the "explored map" of partially observable navigation envs, for the static world only. Like the
 * passes before it this is a pass over stored windows in a launch of its own (the env step is untouched). Like the footprints it
 * has state, the seen tiles, which the caller owns.
 *
 * The RULE (csrc/atr_memory_rule.h holds the arithmetic once, for host and device).
 *
 *   State. `seen` is uint32 [N][2][ATR_MEMORY_TILE_WORDS = 256], contiguous: one bit-packed tile per (env e, player p; 0 tracker,
 *   1 target) in exactly the layout of the handle's map tiles: row r is words 3 r .. 3 r + 2, column c is bit c & 31 of word
 *   c >> 5. Bit (r, c) set: player p has had map cell (r, c) in its window, not hidden, since its tile was last cleared. Bits
 *   outside the side x side square are always 0 (words 3 side .. 255 too).
 *
 *   Inputs from the handle: the `pos` word, tracker (pos & 255, pos >> 8 & 255), target (pos >> 16 & 255, pos >> 24), as
 *   (pr, pc); side = cnt >> 24; the env's current map tile maps[e]. The windows handed in must be the ones the handle's last
 *   launch wrote, after the occlusion, field-of-view and footprint passes; that is the caller's business, as the stream order is.
 *
 *   `roles` (1, 2 or 3) names the players the call is about: bit p set means player p. Nothing of a player outside `roles` is
 *   read or written: not its window, not its tile — its tile is not cleared either.
 *
 *   Clearing, for every player in `roles`, by `mode`:
 *     ATR_MEMORY_KEEP (0)    nothing is cleared.
 *     ATR_MEMORY_STEP (1)    where `done` is given and done[e] != 0 the tiles of env e become all zero (with the env's in-launch
 *                            auto-reset the map, the positions and the window are already the new episode's).
 *     ATR_MEMORY_BEGIN (2)   every env is cleared; `done` is not looked at.
 *
 *   Recording, after clearing, in every mode, for player p in `roles` standing on map cell (pr, pc). Window cell (wr, wc) stands
 *   for map cell (r, c) = (pr - 6 + wr, pc - 6 + wc). If 0 <= r, c < side and the window cell is NOT EQUAL to `hidden` (default
 *   ATR_MEMORY_HIDDEN = 5), bit (r, c) of tile (e, p) is set. The centre counts as a recorded cell like any other. Recording is
 *   idempotent: a KEEP call on an unchanged window changes nothing.
 *
 *   Painting, after recording. A window cell that EQUALS `hidden`, whose map cell is inside the square and whose seen bit is set,
 *   is written as `wall_value` (default ATR_MEMORY_WALL = 7) if the map tile has the bit set, else as `free_value` (default
 *   ATR_MEMORY_FREE = 8). Nothing else is written; the call is in place only.
 *
 *   What follows:
 *     - players are never remembered: a hidden cell that holds the other player reads 7 or 8 like any other remembered cell (the
 *       map tile holds walls only), and so do footprints;
 *     - a cell outside the map square stays 5; a cell that was never seen stays 5;
 *     - a cell that is visible now is never changed; a call on a window this pass has already painted changes nothing either: a
 *       painted cell differs from `hidden`, so it is recorded, but its bit was set already (that is why it was painted), and no
 *       cell that could be painted still reads `hidden`;
 *     - each player's memory is fed only by its own window;
 *     - 7 and 8 are values no window holds otherwise (0, 1, 2, 4 from the env, 5 from occlusion / field of view, 6 footprints).
 *
 *   Order. Occlusion, field of view, footprints, this pass, then the egocentric turn (atr_ego.h): memory works in the map frame
 *   and must see the final 5s; the turn moves 7s and 8s like any value.
 *
 * atr_memory_windows — the windows of handle h (N is the handle's), window (e, p) at ELEMENT e * se + p * sp of obs (uint8 when
 *   is_u8 != 0, else float32), its 169 cells contiguous; done is one byte per env or NULL.
 *
 *   One wavefront owns window (e, p) and seen tile (e, p): no two wavefronts ever share a byte they write. Within the wavefront
 *   every word of the tile has exactly one lane that may store it, the clear included, and the paint reads seen and wall bits from
 *   the wavefront's own staging, never from global memory this launch wrote. A byte window's cells are stored by byte, so that no
 *   lane writes outside its own window at any alignment. A wavefront that finds its env's side outside 1 .. 82 or its player outside
 *   the square (no live episode has either) returns without reading or writing a window or a tile.
 *
 * All pointers but h are device pointers; `stream` is a hipStream_t. The call enqueues ONE launch (capturable in a hipGraph; no
 * allocation, no atomics, no synchronisation) and returns 0 or a T2D_ERR_* code of include/track2d.h, with the text in
 * t2d_last_error(). Refused with T2D_ERR_INVALID before the handle is looked at, in this order: a null obs or seen; roles outside
 * 1 .. 3; mode outside 0 .. 2; hidden, wall_value or free_value outside 0 .. 255; wall_value or free_value equal to hidden; a
 * negative stride; float windows not 4-byte aligned; seen not 16-byte aligned; a null h. Refused after that, from the handle's
 * state: a handle that was never reset (all envs), a handle with whole-map ('Full') observations. A handle with the Moore action
 * table is fine: the rule never looks at an action.
 */
#ifndef ATR_MEMORY_H
#define ATR_MEMORY_H

#include "track2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ATR_MEMORY_WINDOW 169           /* cells of a 13 x 13 window */
#define ATR_MEMORY_SIDE 13
#define ATR_MEMORY_CENTRE 6             /* row and column of the window's centre */
#define ATR_MEMORY_TILE_WORDS 256       /* uint32 words of a seen tile (the handle's map tile) */
#define ATR_MEMORY_ROW_WORDS 3          /* words of a tile row */
#define ATR_MEMORY_MAX_SIDE 82          /* the largest map side a tile holds */
#define ATR_MEMORY_HIDDEN 5             /* the default `hidden`: what occlusion and the field of view write */
#define ATR_MEMORY_WALL 7               /* the default `wall_value` */
#define ATR_MEMORY_FREE 8               /* the default `free_value` */
#define ATR_MEMORY_KEEP 0
#define ATR_MEMORY_STEP 1
#define ATR_MEMORY_BEGIN 2

int atr_memory_windows(t2d_handle *h, void *obs, int is_u8, long long se, long long sp, unsigned int *seen, int roles, int mode,
                       const unsigned char *done, int hidden, int wall_value, int free_value, void *stream);

#ifdef __cplusplus
}
#endif

#endif
