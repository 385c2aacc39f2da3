/*
 * atr_stats.h — C ABI of the training-episode statistics in libtrack2d_hip.so: returns and lengths of the episodes that END
 * during training rollouts, kept on the device and advanced once per rollout from the step rewards and done flags the rollout
 * has stored. The reference's worker does this on the host, one env at a time (train.py:63-88: `reward_sum += player.reward`,
 * written as train/reward_<j> and zeroed on `done`); its evaluation script turns finished episodes into mean / std of return
 * and length and a success rate (gym_eval.py:110-125: `eps_len >= 500` is a success).
 *
 * atr_episode_stats — one thread per env. Per env e, for t = 0 .. T-1 in order:
 *
 *     run_ret[e][p] = run_ret[e][p] + rew[t][e][p]        (float32, p = 0, 1, step order)
 *     run_len[e]   += 1
 *     if done[t][e]:
 *         fin[e] += {1, R0, R1, R0*R0, R1*R1, L, L*L, L >= success_len}
 *         run_ret[e] = 0;  run_len[e] = 0
 *
 *   R0 and R1 are the float32 run_ret values promoted to float64, L is run_len. fin is float64 [N, 8]: counts are exact and
 *   sums do not lose small returns; every product is rounded to float64 before it is added (no fused multiply-add). rew and
 *   done are addressed through ELEMENT strides, so a rollout store [T, N, 2] / [T, N], a slice of a larger store and a stacked
 *   list all fit without a copy. Consecutive lanes read consecutive envs of a step's row. No atomics, no barriers, no
 *   cross-lane traffic. The episode that is still running when the call ends stays in run_ret / run_len: the next call
 *   continues it, so T steps in one call equal any split into consecutive calls.
 *
 * atr_episode_stats_drain — totals[8] = sum over e of fin[e] in float64, and fin zeroed, in ONE launch: in stream order between
 *   two atr_episode_stats calls, so no episode is lost or counted twice between a sum and a separate zeroing. run_ret / run_len
 *   are not touched. The summation order is fixed (ATR_STATS_DRAIN_LANES = 32 row lanes, one workgroup):
 *
 *     part[r][k] = 0.0;  for i = 0, 1, 2, ... while r + 32 i < N:  part[r][k] = part[r][k] + fin[r + 32 i][k]    (r = 0 .. 31)
 *     totals[k]  = 0.0;  for r = 0 .. 31:                          totals[k]  = totals[k]  + part[r][k]
 *
 *   A host model that adds in this order restates totals bit for bit (episode_stats.drain_model).
 *
 * All pointers are device pointers; `stream` is a hipStream_t. Both calls only enqueue one launch (capturable in a hipGraph).
 * Both return 0 or a T2D_ERR_* code of include/track2d.h, with the text in t2d_last_error(). Refused with T2D_ERR_INVALID before
 * any device is touched: a null pointer, N <= 0, T <= 0, fin or totals not 8-byte aligned, run_ret / run_len / rew not 4-byte
 * aligned.
 */
#ifndef ATR_STATS_H
#define ATR_STATS_H

#include "track2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ATR_STATS_FIELDS 8        /* count, R0, R1, R0^2, R1^2, L, L^2, successes */
#define ATR_STATS_DRAIN_LANES 32  /* row lanes of the drain's fixed summation order */

/* rew float32, element (t, e, p) at rew[t * rew_st + e * rew_sn + p * rew_sp]; done uint8 (non-zero = the episode ended with this
 * step), element (t, e) at done[t * done_st + e * done_sn]; run_ret float32 [N,2], run_len int32 [N], fin float64 [N,8],
 * contiguous. Strides are in elements and must be >= 0. */
int atr_episode_stats(const float *rew, long long rew_st, long long rew_sn, long long rew_sp, const unsigned char *done,
                      long long done_st, long long done_sn, float *run_ret, int *run_len, double *fin, int T, int N,
                      int success_len, void *stream);

/* fin float64 [N,8] (read, then zeroed), totals float64 [8] (written) */
int atr_episode_stats_drain(double *fin, double *totals, int N, void *stream);

#ifdef __cplusplus
}
#endif

#endif
