/*
 * track2d_bank_prio.h — prioritized map replay on a map bank (csrc/track2d_hip.hip): the maps of an attached bank
 * (track2d_bank.h) are drawn from a weight table, and the handle keeps a per-map account of the episodes that end on them.
 *
 * Prioritized Level Replay (Jiang et al., 2021) serves hard and stale levels more often. The device side of it is three
 * things, all on the handle: a weighted draw inside the generator pass, a per-map account of finished episodes, and the
 * table between them. The rule that turns accounts into weights lives with the caller (active_tracking_rl_amd/map_priority.py
 * states one on tensors): weights arrive as a float32 device array and nothing here goes through the host.
 *
 * The table. For weights w[K]: a weight that is NaN, infinite, zero or negative counts as 0; w_max is the largest remaining
 * weight; S = floor((2^31 - 1) / K).
 *     q_i = 0                                                              if w_i counts as 0
 *     q_i = max(1, floor(((double)w_i / (double)w_max) * (double)S))       otherwise
 * (the division, then the multiplication, each rounded to float64; no fused multiply-add). If every q_i is 0, every q_i = 1.
 * cum[i] = q_0 + ... + q_i in integers; the total cum[K - 1] lies in 1 .. 2^31 - 1. Maximum and integer sums do not depend
 * on the order of a reduction: a host model restates the table bit for bit (tests/map_priority_spec.py).
 *
 * The draw. For the episode `ep` of global env `genv` (track2d_bank.h's names):
 *     r   = Stream(k0, k1, ep, genv, STREAM_MAP, ctr = 0).bounded(cum[K - 1] - 1)
 *     idx = the number of i with cum[i] <= r
 * so map i is drawn with probability q_i / cum[K - 1] and a map with q_i = 0 never. K = 1 draws nothing. The generator wave
 * stores idx into an index ring, chosen[ep & 7][e], and fetches the tile; everything after the fetch is what track2d_bank.h
 * describes, draw for draw (spawn word, SPAWN and TARGET streams). The generator runs at most two episodes ahead of the
 * running one, so the ring entries of episodes episode[e] - 5 .. episode[e] are intact. Slots generated before a change of
 * the table keep their choice.
 *
 * The accounts. stat[K][5] int64 = {episodes, steps, episodes of at least success_len steps, sum of llrint(R0 * 65536),
 * sum of llrint(R1 * 65536)} with R0 / R1 the float32 returns of tracker and target accumulated in step order, and one
 * `unattributed` counter. Integer sums: a host model restates them exactly, whatever the order of the atomic adds.
 *
 * Snapshots (track2d_state.h) do not hold the ring, the table or the accounts, and the index of an episode is no longer a
 * function of its number: t2d_snapshot_save / _restore / _import refuse a prioritised handle with T2D_ERR_STATE.
 *
 * Conventions as in track2d.h (status codes, t2d_last_error, `stream` = hipStream_t as void *).
 */
#ifndef TRACK2D_BANK_PRIO_H
#define TRACK2D_BANK_PRIO_H

#include <stdint.h>

#include "track2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define T2D_PRIO_RING 8         /* episodes of the index ring */
#define T2D_PRIO_FIELDS 5       /* int64 per map of the accounts */
#define T2D_PRIO_KEEP 5         /* an env's episodes older than episode[e] - T2D_PRIO_KEEP are not attributed */

/* After t2d_map_bank_attach (either select) and before the first reset: from now on the handle ignores `select` and draws
 * from the table. Allocates, owned by the handle and freed by t2d_destroy: cum[K] u32 (the uniform table q_i = 1), the ring
 * chosen[8][N] i32 (-1), the accounts (0) and the carry of t2d_bank_prio_score (0); initialised on `stream`, synchronises.
 * t2d_map_bank_index on such a handle reads chosen[episode[e] & 7][e].
 * T2D_ERR_INVALID: null handle. T2D_ERR_STATE: no bank attached, after the first t2d_reset / t2d_inject, or called twice. */
int t2d_bank_prio_enable(t2d_handle *h, void *stream);

/* w_dev [K] float32 (device) -> cum, by the rule above. One launch of one workgroup on `stream` (behind the handle's forked
 * generator launches, if any): no allocation, no synchronisation, capturable.
 * T2D_ERR_INVALID: null argument. T2D_ERR_STATE: the handle has no priorities (t2d_bank_prio_enable). */
int t2d_bank_prio_set_weights(t2d_handle *h, const float *w_dev, void *stream);

/* Account for the T steps the handle has just taken: rew [T][N][2] float32 and done [T][N] u8 read in place through element
 * strides (rew_st / rew_sn / rew_sp: step, env, player; done_st / done_sn), as in atr_stats.h. Call it after those T steps
 * and before any further step or reset of the handle. One launch, one thread per env, capturable. Per env: d = the number of
 * done flags, ep_end = episode[e]; the episode running at step 0 has number ep_end - d. The steps are walked in order with the
 * handle's own carry (run_ret [N][2] float32, run_len [N] — episodes that span calls continue; a t2d_reset of every env
 * zeroes it). At each done flag the episode's map is m = chosen[ep & 7][e] and stat[m] receives, by integer atomic adds,
 * {1, L, L >= success_len, llrint((double)R0 * 65536.0), llrint((double)R1 * 65536.0)}.
 * Not attributed (they add 1 to `unattributed` and nothing to any map): an env's episodes older than ep_end - 5 when it ends
 * more than 5 in one call, and an episode whose ring entry is not a map index.
 * T2D_ERR_INVALID: null argument, T < 1, a negative stride. T2D_ERR_STATE: no priorities, or before the first reset. */
int t2d_bank_prio_score(t2d_handle *h, const float *rew, long long rew_st, long long rew_sn, long long rew_sp,
                        const unsigned char *done, long long done_st, long long done_sn, int T, int success_len, void *stream);

/* out_dev [K * 5 + 1] int64 (device) = the accounts, map-major, then `unattributed`; the handle's copy is zeroed by the same
 * launch. In stream order between two t2d_bank_prio_score calls nothing is lost and nothing counted twice. Capturable.
 * T2D_ERR_INVALID: null argument. T2D_ERR_STATE: no priorities. */
int t2d_bank_prio_drain(t2d_handle *h, long long *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif
