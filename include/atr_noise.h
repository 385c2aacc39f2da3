/*
 * atr_noise.h — C ABI of sensor noise in libtrack2d_hip.so: a player's 13 x 13 window flickers, misses the other player and shows
 * false detections. The passes before this one (atr_occlusion.h, atr_fov.h, atr_footprints.h, atr_memory.h) are deterministic and
 * truthful: a cell that is visible is always right. The reference has nothing that makes a single observation wrong (its --inv
 * swaps whole frames). Like the others this is a pass over stored windows in a launch of its own (the env step is untouched), and
 * like them it has state the caller owns, a per-window clock. Its result is a draw, but a pure function of (key, global env id,
 * per-window clock, player): it can be held bit for bit against a host model (tests/noise_spec.py).
 *
 * The RULE (csrc/atr_noise_rule.h holds its arithmetic once, for host and device).
 *
 *   Windows, values and roles. Window p of env e is player p's view (0 tracker, 1 target). The centre is cell ATR_NOISE_CENTRE =
 *   84. The other player's value is O = 4 in window 0 and O = 2 in window 1. `roles` (1, 2 or 3) says which windows are noisy, as
 *   in atr_footprints.h: bit 0 the tracker's window, bit 1 the target's. A window whose bit is clear is neither read nor written,
 *   and its clock does not move.
 *
 *   Probabilities. Each is an integer threshold t in 0 .. ATR_NOISE_ONE = 1 << 24. An event with 32-bit draw word w happens if and
 *   only if (w >> 8) < t: 0 is never, ATR_NOISE_ONE is always. (Python converts with t = round(p * 2**24), p in [0, 1].)
 *
 *   Clock. `clock` is uint32 [N][2], contiguous, the caller's. Entry (e, p) belongs to window (e, p) alone.
 *     ATR_NOISE_ADVANCE (1)   clock[e][p] += 1 (wrapping), and the draws use the new value.
 *     ATR_NOISE_PEEK (0)      the draws use the value as it stands and nothing is stored to the clock: a second look at the same
 *                             state shows the same noisy window again.
 *   An in-launch auto-reset needs no case: the clock runs on across episodes, and the pass takes no `done`.
 *
 *   Draws. Philox4x32-10 with key words (key & 0xFFFFFFFF, key >> 32) of the 64-bit `key` argument and counter words
 *     c0 = the handle's global env id (its env_id_base + e), c1 = clock, c2 = p, c3 = ATR_NOISE_TAG ^ block  (ATR_NOISE_TAG =
 *     0x4E5E0000).
 *   Block 0 is the window's draws: output word w0 decides the miss, w1 decides the ghost, the ghost's cell is
 *   g = (w2 * 169) >> 32 as a 64-bit product (0 .. 168); w3 is unused. Block 1 + L, L = 0 .. 63, gives the flicker word of cell
 *   L + 64 j as word j, for j = 0, 1, 2 and cells below 169; word 3 is unused.
 *
 *   Verdicts, with the three thresholds `flicker`, `miss` and `ghost`. All verdicts come from the window as it reads BEFORE any
 *   store of this call.
 *     1. Flicker. A cell i != 84 reading exactly 0 or 1 (0.0f / 1.0f in a float window) whose flicker word passes `flicker` is
 *        written as 1 - v.
 *     2. Miss. If w0 passes `miss`, every cell i != 84 reading O is written 0.
 *     3. Ghost. If w1 passes `ghost`, and g != 84, and cell g read exactly 0, cell g is written O. On that cell the ghost wins
 *        over a flicker.
 *   Nothing else is read or written: the centre is never touched, nor is a 5, 6, 7 or 8, nor any other value. A window under
 *   occlusion can show a ghost only where the player can see. A cell whose verdict leaves it unchanged is not stored.
 *
 *   Order. After occlusion, field of view, footprints and map memory, ahead of the egocentric turn. Map memory's record and paint
 *   therefore read noise-free visibility: the noise applies to what the sensor reports, and memory's 7s and 8s stay true.
 *
 *   What follows:
 *     - with all three thresholds 0 the call changes no window byte; ADVANCE still advances the clock;
 *     - the env's dynamics, rewards and `done` are unchanged: the pass reads no env state but the handle's env_id_base;
 *     - the result does not depend on how envs are sharded: one handle of 8 envs at base 0 and two handles of 4 at bases 0 and 4
 *       draw the same words.
 *
 * atr_noise_windows — the 2 N windows of handle h (N is the handle's), window (e, p) at ELEMENT e * se + p * sp of obs (uint8 when
 *   is_u8 != 0, else float32), its 169 cells contiguous.
 *
 *   One wavefront owns window (e, p) and clock entry (e, p): no two wavefronts ever share a byte they write. The wavefront loads
 *   its whole window and its clock entry before it stores any of either. A byte window's cells are stored by byte, so that no
 *   lane writes outside its own window at any alignment.
 *
 * All pointers but h are device pointers; `stream` is a hipStream_t. The call enqueues ONE launch (capturable in a hipGraph; no
 * allocation, no atomics, no synchronisation) and returns 0 or a T2D_ERR_* code of include/track2d.h, with the text in
 * t2d_last_error(). Refused with T2D_ERR_INVALID before the handle is looked at, in this order: a null obs or clock; a threshold
 * outside 0 .. 1 << 24 (flicker, miss, ghost in that order); roles outside 1 .. 3; mode outside 0 .. 1; a negative stride; float
 * windows not 4-byte aligned; a clock not 4-byte aligned; a null h. Refused after that, from the handle's state: a handle that was
 * never reset (all envs), a handle with whole-map ('Full') observations.
 */
#ifndef ATR_NOISE_H
#define ATR_NOISE_H

#include "track2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ATR_NOISE_WINDOW 169            /* cells of a 13 x 13 window */
#define ATR_NOISE_CENTRE 84             /* the window's centre cell: the viewer */
#define ATR_NOISE_ONE 16777216          /* 1 << 24: the threshold of probability 1 */
#define ATR_NOISE_TAG 1314783232        /* 0x4E5E0000: counter word 3 is this ^ block */
#define ATR_NOISE_PEEK 0
#define ATR_NOISE_ADVANCE 1

int atr_noise_windows(t2d_handle *h, void *obs, int is_u8, long long se, long long sp, unsigned int *clock, unsigned long long key,
                      int flicker, int miss, int ghost, int roles, int mode, void *stream);

#ifdef __cplusplus
}
#endif

#endif
