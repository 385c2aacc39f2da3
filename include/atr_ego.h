/*
 * atr_ego.h — C ABI of the egocentric view in libtrack2d_hip.so: a player's 13 x 13 window turns with the player, so that it always
 * looks up, and its four actions mean forward / back / left / right. The windows as the env writes them are drawn north-up and the
 * four actions are compass moves; the field of view (atr_fov.h) already gives every player a facing byte. This rule reads that
 * byte as a HEADING: atr_ego_actions turns the policy's relative actions into the env's absolute ones before the step, and
 * atr_ego_windows turns the stored windows after it. Both are launches of their own (the env step is untouched).
 *
 * The RULE (csrc/atr_ego_rule.h holds it once, for host and device).
 *
 *   Heading. The heading is the facing byte of atr_fov.h, with the same values: 0 = (-1, 0), 1 = (+1, 0), 2 = (0, -1),
 *   3 = (0, +1) as (ur, uc), and ATR_FOV_NONE = 255. NONE, and any value that is no facing, counts as heading 0 (up): a new
 *   episode is drawn north-up with compass moves until its player has moved. The byte turns by the rule of atr_fov.h ("Turning"),
 *   unchanged: done gives NONE; otherwise an ABSOLUTE action in 0 .. 3 becomes the heading (a move that a wall blocks still turns
 *   the player); otherwise the heading stays.
 *
 *   Relative actions. A policy action k in 0 .. 3 means 0 = forward, 1 = back, 2 = left, 3 = right. The env is stepped with
 *   ABS[heading][k]:
 *       heading 0 (up)      0 1 2 3
 *       heading 1 (down)    1 0 3 2
 *       heading 2 (left)    2 3 1 0
 *       heading 3 (right)   3 2 0 1
 *   An action outside 0 .. 3 passes through unchanged. At heading 0 / NONE relative equals absolute. Every row is a permutation;
 *   REL[heading][abs] is its inverse. ABS[h][0] = h, and ABS[h][1] is the opposite move.
 *
 *   View. The egocentric window E of an absolute window W (cell (r, c) at index r * 13 + c, centre (6, 6)) under heading
 *   (ur, uc): for the ego offset (er, ec) = (r - 6, c - 6),
 *       E[r][c] = W[6 + dr][6 + dc]   with   (dr, dc) = (-er * ur + ec * uc, -er * uc - ec * ur).
 *   Heading 0 is the identity, heading 1 a half turn (numpy's rot90(W, 2)), heading 2 rot90(W, 3), heading 3 rot90(W, 1). The
 *   cell at the ego offset of relative action k — (-1, 0), (+1, 0), (0, -1), (0, +1) — is the cell ABS[heading][k] moves
 *   towards. Values are moved, never changed: occlusion's and the field of view's 5s and the footprints' 6s turn with the rest.
 *
 *   Order within a step.
 *     1. Relative actions become absolute, read with the heading the step starts from (atr_ego_actions).
 *     2. The env step runs, on the absolute actions.
 *     3. Occlusion, field of view and footprints run, all in the absolute frame and with the absolute actions.
 *     4. The heading turns, once only: the field-of-view pass does it where it is on, otherwise atr_ego_windows does (it is
 *        given the absolute actions and the done flags exactly then).
 *     5. The window is turned with the UPDATED heading (atr_ego_windows).
 *
 *   What the policy side keeps. Everything the policy side keeps is the RELATIVE action: the rollout store's actions, the
 *   learner's log-probabilities, the tracker-action embedding of the tat-* networks. The absolute action exists between
 *   atr_ego_actions and the passes of the same step, in buffers the env owns.
 *
 * atr_ego_actions — for every env e and player p (0 the tracker, 1 the target): abs_p[e] = ABS[heading(facing[e * 2 + p])][rel_p[e]]
 *   where bit p of `roles` is set (bit 0 the tracker, bit 1 the target), else abs_p[e] = rel_p[e]. The facing bytes are always two
 *   per env, as the env keeps them, and are only read. rel1 / abs1 may both be NULL (a scripted target takes no action): that
 *   player is skipped. abs_p == rel_p (in place) is allowed; any other overlap among the four arrays is refused. The arrays hold
 *   n_env values of type act_dtype (T2D_ACT_* of track2d.h). One lane per (env, player).
 *
 * atr_ego_windows — n_env * n_win windows (n_win 1 or 2), window (e, p) at ELEMENT e * se + p * sp of both src and dst (uint8 when
 *   is_u8 != 0, else float32), its 169 cells contiguous; facing byte (e, p) at facing[e * n_win + p], read and written. a0 / a1
 *   are player 0's / player 1's ABSOLUTE actions, one per env, of type act_dtype, NULL = that player does not turn in this call
 *   (a1 is not looked at when n_win is 1); done is one byte per env, NULL = no episode turnover in this call. A player whose bit
 *   of `roles` is clear is neither turned, read nor written.
 *
 *   One wavefront owns window (e, p) and its facing byte: it computes the new facing, lane 0 stores it, and no other wavefront
 *   addresses that byte. It then loads its 169 cells, parks them in its own slot of LDS, reads them back permuted and stores them;
 *   the stores depend on the LDS reads and those on the LDS writes of every loaded cell, so the whole window has been read
 *   before any of it is written. dst == src (in place) is therefore allowed, and with heading 0 / NONE an in-place wavefront ends
 *   after the turn with nothing read or written. A byte window's cells are stored by byte: no lane writes outside its own window
 *   at any alignment. With dst != src every cell of dst of a player in `roles` is written. The windows of dst must not overlap
 *   one another (strides below 169 elements): the call does not check it.
 *
 * All pointers are device pointers; `stream` is a hipStream_t. Each call enqueues ONE launch (capturable in a hipGraph; no
 * allocation, no atomics, no synchronisation) and returns 0 or a T2D_ERR_* code of include/track2d.h, with the text in
 * t2d_last_error(). Refused with T2D_ERR_INVALID before any device is touched — both: a null facing, n_env <= 0, roles outside
 * 1 .. 3, an act_dtype that is no T2D_ACT_* while an action pointer is given; atr_ego_actions: a null rel0 / abs0, rel1 and abs1
 * not both NULL or both given, more than ATR_EGO_MAX_WINDOWS / 2 envs, arrays that overlap other than abs_p == rel_p;
 * atr_ego_windows: a null src / dst, n_win <= 0 or > 2, more than ATR_EGO_MAX_WINDOWS windows, a negative stride, float windows
 * not 4-byte aligned, src != dst whose byte ranges overlap.
 */
#ifndef ATR_EGO_H
#define ATR_EGO_H

#include "atr_fov.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ATR_EGO_WINDOW 169              /* cells of a 13 x 13 window (ATR_FOV_WINDOW) */
#define ATR_EGO_SIDE 13
#define ATR_EGO_CENTRE 6                /* row and column of the window's centre */
#define ATR_EGO_FORWARD 0               /* the relative actions */
#define ATR_EGO_BACK 1
#define ATR_EGO_LEFT 2
#define ATR_EGO_RIGHT 3
#define ATR_EGO_TRACKER 1               /* the bits of `roles` */
#define ATR_EGO_TARGET 2
#define ATR_EGO_MAX_WINDOWS 2147483647  /* n_env * n_win per call */

int atr_ego_actions(const unsigned char *facing, const void *rel0, const void *rel1, void *abs0, void *abs1, int act_dtype,
                    long long n_env, int roles, void *stream);

int atr_ego_windows(const void *src, void *dst, int is_u8, long long n_env, int n_win, long long se, long long sp,
                    unsigned char *facing, const void *a0, const void *a1, int act_dtype, const unsigned char *done, int roles,
                    void *stream);

#ifdef __cplusplus
}
#endif

#endif
