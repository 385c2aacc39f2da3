/*
 * atr_footprints.h — C ABI of footprints in libtrack2d_hip.so: each player leaves a trail on the last K cells it stepped off, and
 * the other player's 13 x 13 window shows them. The reference names the cue — its observation space runs to 6, and its colour table
 * gives 6 to the trace of visited cells (track_1v1.py:66, painted only by render(), :181-182) — but no observation of it ever holds
 * a 6. Like the occluded observations (atr_occlusion.h) and the field of view (atr_fov.h) this is a pass over stored windows in a
 * launch of its own (the env step is untouched). Like the field of view it has state, the trail, which the caller owns.
 *
 * The RULE (csrc/atr_footprint_rule.h holds it once, for host and device).
 *
 *   State. `trail` is uint16 [N][2][K + 1], contiguous, 1 <= K <= ATR_FOOTPRINT_MAX_K = 63. Entry (e, p, j) is a map cell
 *   r | c << 8 of env e's player p (0 tracker, 1 target), or ATR_FOOTPRINT_EMPTY = 0xFFFF. Entry 0 is the cell the player stood on
 *   at the last recording call; it is never painted. Entries 1 .. K are its prints, newest first.
 *
 *   Positions come from the handle, not from the windows: the `pos` word of the handle's state, tracker
 *   (pos & 255, pos >> 8 & 255), target (pos >> 16 & 255, pos >> 24), as (r, c). The windows handed in must be the ones the
 *   handle's last launch wrote; that is the caller's business, as the stream order is.
 *
 *   Recording, for player p of env e with `cur` its current cell and s its trail row, by `mode`:
 *     ATR_FOOTPRINT_PEEK (0)   the state is not touched.
 *     ATR_FOOTPRINT_STEP (1)   if `done` is given and done[e] != 0: s' = [cur, EMPTY, ..., EMPTY] (with the env's in-launch
 *                              auto-reset `cur` is the new episode's spawn: a new episode starts with no prints);
 *                              else if cur != s[0]: s' = [cur, s[0], ..., s[K - 1]] (the oldest print drops; an EMPTY s[0] needs
 *                              no case of its own: an EMPTY shifts in);
 *                              else (a wall bump, a stay) s' = s: a player that does not move leaves no new print, and its old
 *                              ones do not age.
 *     ATR_FOOTPRINT_BEGIN (2)  every env is treated as if done[e] != 0; `done` is not looked at.
 *
 *   Painting, after recording and with the updated state, in every mode. Window v of env e is painted if and only if `roles`
 *   (1, 2 or 3) has bit v set: bit 0 paints the tracker's window with the target's prints, bit 1 the target's window with the
 *   tracker's prints. For each entry j = 1 .. K of the OTHER player that is not EMPTY: (dr, dc) = print - viewer's cell; if
 *   max(|dr|, |dc|) <= 6 the window cell is (6 + dr) * 13 + 6 + dc, and if that cell READS EXACTLY 0 (0.0f in a float window) it
 *   is written as `value` (default ATR_FOOTPRINT_VALUE = 6; 0 .. 255). Nothing else is read or written; the call is in place only.
 *
 *   What follows, in windows as the env (and the passes before this one) writes them:
 *     - the centre holds the viewer and is never painted; a wall (1) is never painted; a cell holding the other player (2 / 4)
 *       is never painted, for example a target that walked back onto its own print; a cell that occlusion or the field of view
 *       wrote as 5 is never painted; the padding outside the map (1) is never painted;
 *     - a print outside the window is not seen; two prints on one cell write the same value twice;
 *     - which cells CAN be painted depends on the positions and the trail alone; which cells ARE painted also depends on the
 *       window reading 0.
 *
 *   Order. Occlusion first, then field of view, then this pass.
 *
 * atr_footprint_windows — the 2 N windows of handle h (N is the handle's), window (e, p) at ELEMENT e * se + p * sp of obs (uint8
 *   when is_u8 != 0, else float32), its 169 cells contiguous; done is one byte per env or NULL.
 *
 *   One wavefront owns trail row (e, p) and is the only writer of window (e, 1 - p): no two wavefronts ever share a byte they
 *   write. The wavefront loads its whole row before it stores any of it, and stores only the entries that changed. A byte
 *   window's cells are stored by byte, so that no lane writes outside its own window at any alignment.
 *
 * All pointers but h are device pointers; `stream` is a hipStream_t. The call enqueues ONE launch (capturable in a hipGraph; no
 * allocation, no atomics, no synchronisation) and returns 0 or a T2D_ERR_* code of include/track2d.h, with the text in
 * t2d_last_error(). Refused with T2D_ERR_INVALID before the handle is looked at, in this order: a null obs or trail; k outside
 * 1 .. 63; roles outside 1 .. 3; mode outside 0 .. 2; value outside 0 .. 255; a negative stride; float windows not 4-byte aligned;
 * a trail not 2-byte aligned; a null h. Refused after that, from the handle's state: a handle that was never reset (all envs), a
 * handle with whole-map ('Full') observations. A handle with the Moore action table is fine: the rule never looks at an action.
 */
#ifndef ATR_FOOTPRINTS_H
#define ATR_FOOTPRINTS_H

#include "track2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ATR_FOOTPRINT_WINDOW 169        /* cells of a 13 x 13 window */
#define ATR_FOOTPRINT_SIDE 13
#define ATR_FOOTPRINT_CENTRE 6          /* row and column of the window's centre */
#define ATR_FOOTPRINT_EMPTY 65535       /* 0xFFFF: a trail entry that holds no cell */
#define ATR_FOOTPRINT_VALUE 6           /* the default `value` (the reference's trace colour index) */
#define ATR_FOOTPRINT_MAX_K 63
#define ATR_FOOTPRINT_PEEK 0
#define ATR_FOOTPRINT_STEP 1
#define ATR_FOOTPRINT_BEGIN 2

int atr_footprint_windows(t2d_handle *h, void *obs, int is_u8, long long se, long long sp, unsigned short *trail, int k, int roles,
                          int mode, const unsigned char *done, int value, void *stream);

#ifdef __cplusplus
}
#endif

#endif
