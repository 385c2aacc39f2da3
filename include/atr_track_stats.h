/*
 * atr_track_stats.h — C ABI of the tracking statistics in libtrack2d_hip.so: where the target sits relative to the tracker
 * (a 13 x 13 heat map of the offset target - tracker, plus out of view / co-located), and which action each player takes from
 * each offset, counted on the device for all N envs of a shard with one launch per rollout over what the rollout has already
 * stored: both players' 13 x 13 windows, the step rewards, the done flags and the actions. The reference can only get these
 * figures on the host, one env at a time, from info['traces'].
 *
 * What the windows say (track_1v1.py:297-313; the reward: track_1v1.py:96-100). The tracker's window shows the byte 4 at cell
 * (6 + dr, 6 + dc) exactly when the target is at offset (dr, dc), |dr|, |dc| <= 6, and not on the tracker's own cell; the
 * target's window then shows the byte 2 at the mirrored cell (6 - dr, 6 - dc). Two agents on one cell do not see each other:
 * the tracker's centre is 2 and the target's centre is 4 either way, so "no 4 in the window" alone cannot tell a co-located
 * target from one out of view. The tracker's reward can: r_track = 1 - 2 d / 6 is 1.0f exactly for d = 0 and for no other
 * distance. A fresh episode's first state has no reward in the store, which is why it is never classified.
 *
 * atr_track_stats — the post-step state of env e at step t is sample (t, e), t = 0 .. T-1: its windows are obs[t+1][e][0 | 1]
 *   (obs has T+1 slots, slot 0 is not classified), its reward is rew[t][e][0], its flag is done[t][e]. Per env, in step order:
 *
 *     b = carry[e]                                          (the bin of the state the step's actions were taken from, or -1)
 *     if done[t][e] and flags bit 0 is clear:               (auto-reset store: the stored observation is the NEXT episode's)
 *         bin = TERMINAL;  carry[e] = -1
 *     else:
 *         n4, i4 = number and index of the cells == 4 in window 0;   n2, i2 = the same for cells == 2 in window 1
 *         c0, c1 = the centre cells (index 84) of window 0 and window 1;   r = rew[t][e][0]
 *         c0 == 2, c1 == 4, r == 1.0f, n4 == 0, n2 == 0                            bin = 84          (co-located)
 *         c0 == 2, c1 == 4, r != 1.0f, n4 == 1, n2 == 1, i2 == 168 - i4            bin = i4          ((dr+6) * 13 + (dc+6))
 *         c0 == 2, c1 == 4, r != 1.0f, n4 == 0, n2 == 0                            bin = OUT
 *         anything else                                                            bin = INCONSISTENT
 *         carry[e] = -1 if bin == INCONSISTENT or done[t][e] (flags bit 0 set: the handle does not auto-reset, the observation
 *                    is the terminal state's own and the next state comes from a reset), else bin
 *     hist[bin] += 1;  hist[SAMPLES] += 1
 *     if act and b >= 0, for p = 0, 1:  a = act[t][e][p];  0 <= a < n_actions: act_hist[p][b][a] += 1, else hist[INCONSISTENT] += 1
 *
 *   The action taken from a state belongs to that state's bin, so act[0] pairs with the previous call's last state: T steps in
 *   one call equal any split into consecutive calls, counter for counter. A carry outside [-1, OUT] is read as -1. float32
 *   observations are compared with 2.0f and 4.0f. Every tensor is addressed through ELEMENT strides (>= 0): the rollout store, a
 *   slice of a larger store and a stacked list all fit without a copy; only a window's 169 cells must be contiguous. One
 *   wavefront per env; counters are added in LDS per workgroup and flushed with one 64-bit integer atomic add per non-zero
 *   counter, so the totals do not depend on the execution order. No env reads another env's data; N is any positive number.
 *
 * atr_track_stats_drain — out_hist = hist, out_act_hist = act_hist, and both tables zeroed, in ONE launch: in stream order
 *   between two atr_track_stats calls, so no sample is lost or counted twice. carry is not touched.
 *
 * All pointers are device pointers; `stream` is a hipStream_t. Both calls only enqueue one launch (capturable in a hipGraph).
 * Both return 0 or a T2D_ERR_* code of include/track2d.h, with the text in t2d_last_error(). Refused with T2D_ERR_INVALID before
 * any device is touched: a null pointer (act alone may be null), N <= 0, T <= 0 or T > ATR_TRACK_MAX_T, n_actions outside
 * [1, ATR_TRACK_MAX_ACTIONS], flags other than bit 0, a negative stride, hist / act_hist / act / out_* not 8-byte aligned,
 * carry / rew / float32 obs not 4-byte aligned.
 */
#ifndef ATR_TRACK_STATS_H
#define ATR_TRACK_STATS_H

#include "track2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ATR_TRACK_WINDOW 169        /* cells of a 13 x 13 window; bins 0 .. 168 = (dr + 6) * 13 + (dc + 6) */
#define ATR_TRACK_CENTRE 84         /* the window's centre cell; as a bin: co-located */
#define ATR_TRACK_OUT 169           /* target out of the tracker's view */
#define ATR_TRACK_TERMINAL 170      /* done step of an auto-reset store: the episode's last state is not in the store */
#define ATR_TRACK_INCONSISTENT 171  /* windows / reward that no state produces, or an action outside [0, n_actions) */
#define ATR_TRACK_SAMPLES 172       /* every sample, whatever its bin */
#define ATR_TRACK_HIST 176          /* length of hist (173 .. 175 stay zero) */
#define ATR_TRACK_ACT_ROWS 170      /* act_hist rows per player: bins 0 .. 168 and OUT */
#define ATR_TRACK_MAX_ACTIONS 8     /* act_hist columns (Moore: 8 actions, VonNeumann: the first 4) */
#define ATR_TRACK_MAX_T 1048576     /* steps per call (the per-workgroup counters are 32-bit) */
#define ATR_TRACK_NO_AUTO_RESET 1   /* flags bit 0: done steps hold the terminal state's own observation */

/* obs: uint8 (obs_is_u8 != 0) or float32, window p of env e in slot s at obs[s * obs_st + e * obs_se + p * obs_sp], its 169
 * cells contiguous, s = 0 .. T; rew float32, element (t, e, p) at rew[t * rew_st + e * rew_se + p * rew_sp]; done uint8, element
 * (t, e) at done[t * done_st + e * done_se]; act int64 or null, element (t, e, p) at act[t * act_st + e * act_se + p * act_sp];
 * carry int32 [N]; hist uint64 [ATR_TRACK_HIST]; act_hist uint64 [2][ATR_TRACK_ACT_ROWS][ATR_TRACK_MAX_ACTIONS]. */
int atr_track_stats(const void *obs, int obs_is_u8, long long obs_st, long long obs_se, long long obs_sp, const float *rew,
                    long long rew_st, long long rew_se, long long rew_sp, const unsigned char *done, long long done_st,
                    long long done_se, const long long *act, long long act_st, long long act_se, long long act_sp, int *carry,
                    unsigned long long *hist, unsigned long long *act_hist, int T, int N, int n_actions, int flags, void *stream);

/* hist / act_hist (read, then zeroed); out_hist uint64 [ATR_TRACK_HIST], out_act_hist uint64 [2][170][8] (written) */
int atr_track_stats_drain(unsigned long long *hist, unsigned long long *act_hist, unsigned long long *out_hist,
                          unsigned long long *out_act_hist, void *stream);

#ifdef __cplusplus
}
#endif

#endif
