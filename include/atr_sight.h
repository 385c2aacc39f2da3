/*
 * atr_sight.h — C ABI of the sight statistics in libtrack2d_hip.so: does the target use the obstacles? For every stored step of
 * all N envs of a shard, with one launch per rollout over what the rollout has already stored (both players' 13 x 13 windows, the
 * step rewards, the done flags): is the tracker's line of sight to the target clear or blocked by a wall, how long is the shortest
 * way round that the tracker can see, and how often is sight lost to a wall rather than to range, and regained. The offset counts of
 * include/atr_track_stats.h put a target three cells away in the open and one three cells away behind a wall into the same bin.
 *
 * atr_sight_stats — the post-step state of env e at step t is sample (t, e), t = 0 .. T-1: its windows are obs[t+1][e][0 | 1]
 *   (obs has T+1 slots, slot 0 is not classified), its reward is rew[t][e][0], its flag is done[t][e]. Its BIN is the bin of
 *   atr_track_stats, by the same rule (the kernel recomputes it; the two features share no state):
 *
 *     if done[t][e] and flags bit 0 is clear:               (auto-reset store: the stored observation is the NEXT episode's)
 *         bin = TERMINAL
 *     else:
 *         n4, i4 = number and index of the cells == 4 in window 0;   n2, i2 = the same for cells == 2 in window 1
 *         c0, c1 = the centre cells (index 84) of window 0 and window 1;   r = rew[t][e][0]
 *         c0 == 2, c1 == 4, r == 1.0f, n4 == 0, n2 == 0                            bin = 84          (co-located)
 *         c0 == 2, c1 == 4, r != 1.0f, n4 == 1, n2 == 1, i2 == 168 - i4            bin = i4          ((dr+6) * 13 + (dc+6))
 *         c0 == 2, c1 == 4, r != 1.0f, n4 == 0, n2 == 0                            bin = OUT
 *         anything else                                                            bin = INCONSISTENT
 *
 *   The sight CLASS of a classified sample (bin 0 .. 168 or OUT; TERMINAL and INCONSISTENT samples have none):
 *     OUT (2)      the bin is OUT
 *     CLEAR (0)    the bin is the centre (co-located), or no line cell of window 0 is a wall
 *     BLOCKED (1)  the target is at offset (dr, dc) != (0, 0) and at least one line cell of window 0 is a wall
 *   A wall is a cell equal to 1 (1.0f in a float store); everything else (0, 2, 4) is free. The padding the env writes outside
 *   the map is 1: it blocks like a wall.
 *
 *   The LINE runs from the tracker's centre (6, 6) to the target, end cells excluded. With m = max(|dr|, |dc|), for k = 1 .. m-1
 *   the line cell is (6 + sgn(dr) * ((2 k |dr| + m) / (2 m)), 6 + sgn(dc) * ((2 k |dc| + m) / (2 m))), integer division (the
 *   minor coordinate rounded half away from the tracker's row / column). Adjacent and diagonal-adjacent targets (m = 1) have no
 *   line cell and are always CLEAR; a diagonal line passes between two wall corners, as the Moore table's moves do. The rule is
 *   the TRACKER's line: it is not symmetric under swapping the ends (for 56 of the 168 offsets the line drawn from the target's
 *   end differs at a rounding tie).
 *
 *   The WINDOW PATH of an in-view sample that is not co-located: P = the length of a shortest 4-connected path over free cells of
 *   window 0 from (6, 6) to (6 + dr, 6 + dc), found by a breadth-first flood that stops at the level that reaches the target or
 *   when it stops growing (then the sample is NOPATH). 1 <= P <= 168, and the detour P - |dr| - |dc| is even and >= 0. The true
 *   shortest path may leave the window, so P is an UPPER BOUND on the map's path distance: "the way round that the tracker can
 *   see", not the map distance.
 *
 *   Per env, in step order (prev = carry[e], read as -1 when outside [-1, 2]):
 *     tab[SAMPLES] += 1;  tab[OUT | TERMINAL | INCONSISTENT] += 1 for such a bin
 *     bin 0 .. 168: tab[SEEN + bin] += 1;  class BLOCKED: tab[BLOCKED + bin] += 1
 *       bin != 84: no path: tab[NOPATH + bin] += 1, else tab[PATH + P] += 1 and tab[DETOUR + (P - |dr| - |dc|) / 2] += 1
 *     the sample has a class and prev >= 0: tab[TRANS + prev * 3 + class] += 1
 *     carry[e] = -1 after TERMINAL or INCONSISTENT, -1 after a done step with flags bit 0 set (the handle does not auto-reset:
 *                the next state comes from a reset), else the sample's class
 *   T steps in one call equal any split into consecutive calls, counter for counter. Every tensor is addressed through ELEMENT
 *   strides (>= 0): the rollout store, a slice of a larger store and a stacked list all fit without a copy; only a window's 169
 *   cells must be contiguous. One wavefront per env; counters are added in LDS per workgroup (32-bit, hence ATR_SIGHT_MAX_T) and
 *   flushed with one 64-bit integer atomic add per non-zero counter, so the totals do not depend on the execution order. No env
 *   reads another env's data; N is any positive number.
 *
 * atr_sight_stats_drain — out_tab = tab, and tab zeroed, in ONE launch: in stream order between two atr_sight_stats calls, so no
 *   sample is lost or counted twice. carry is not touched.
 *
 * All pointers are device pointers; `stream` is a hipStream_t. Both calls only enqueue one launch (capturable in a hipGraph).
 * Both return 0 or a T2D_ERR_* code of include/track2d.h, with the text in t2d_last_error(). Refused with T2D_ERR_INVALID before
 * any device is touched: a null pointer, N <= 0, T <= 0 or T > ATR_SIGHT_MAX_T, flags other than bit 0, a negative stride,
 * tab / out_tab not 8-byte aligned, carry / rew / float32 obs not 4-byte aligned.
 */
#ifndef ATR_SIGHT_H
#define ATR_SIGHT_H

#include "track2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ATR_SIGHT_WINDOW 169        /* cells of a 13 x 13 window; bins 0 .. 168 = (dr + 6) * 13 + (dc + 6) */
#define ATR_SIGHT_CENTRE 84         /* the window's centre cell; as a bin: co-located */
#define ATR_SIGHT_BIN_OUT 169       /* bins as in atr_track_stats: target out of the tracker's view */
#define ATR_SIGHT_BIN_TERMINAL 170
#define ATR_SIGHT_BIN_INCONSISTENT 171
#define ATR_SIGHT_CLEAR 0           /* sight classes (carry values; -1: none) */
#define ATR_SIGHT_BLOCKED_CLASS 1
#define ATR_SIGHT_OUT_CLASS 2
#define ATR_SIGHT_MAX_PATH 168      /* the longest window path, and the bound of the flood's levels */
/* segments of tab, one after another */
#define ATR_SIGHT_SEEN 0            /* [169] samples per in-view bin (84: co-located) */
#define ATR_SIGHT_BLOCKED 169       /* [169] of those, class BLOCKED (the centre and the m = 1 bins stay 0) */
#define ATR_SIGHT_NOPATH 338        /* [169] of those, no path inside the window */
#define ATR_SIGHT_PATH 507          /* [169] index P (entry 0 stays 0) */
#define ATR_SIGHT_DETOUR 676        /* [85] index (P - |dr| - |dc|) / 2 */
#define ATR_SIGHT_TRANS 761         /* [9] prev * 3 + cur */
#define ATR_SIGHT_OUT 770           /* target out of the tracker's view */
#define ATR_SIGHT_TERMINAL 771      /* done step of an auto-reset store: the episode's last state is not in the store */
#define ATR_SIGHT_INCONSISTENT 772  /* windows / reward that no state produces */
#define ATR_SIGHT_SAMPLES 773       /* every sample, whatever its bin */
#define ATR_SIGHT_TABLE 776         /* length of tab (774, 775 stay zero) */
#define ATR_SIGHT_MAX_T 1048576     /* steps per call (the per-workgroup counters are 32-bit) */
#define ATR_SIGHT_NO_AUTO_RESET 1   /* flags bit 0: done steps hold the terminal state's own observation */

/* obs: uint8 (obs_is_u8 != 0) or float32, window p of env e in slot s at obs[s * obs_st + e * obs_se + p * obs_sp], its 169
 * cells contiguous, s = 0 .. T; rew float32, element (t, e, p) at rew[t * rew_st + e * rew_se + p * rew_sp]; done uint8, element
 * (t, e) at done[t * done_st + e * done_se]; carry int32 [N]; tab uint64 [ATR_SIGHT_TABLE]. */
int atr_sight_stats(const void *obs, int obs_is_u8, long long obs_st, long long obs_se, long long obs_sp, const float *rew,
                    long long rew_st, long long rew_se, long long rew_sp, const unsigned char *done, long long done_st,
                    long long done_se, int *carry, unsigned long long *tab, int T, int N, int flags, void *stream);

/* tab (read, then zeroed); out_tab uint64 [ATR_SIGHT_TABLE] (written) */
int atr_sight_stats_drain(unsigned long long *tab, unsigned long long *out_tab, void *stream);

#ifdef __cplusplus
}
#endif

#endif
