// tracking_stats_hip.hip — where the target sits relative to the tracker and what both players do about it, counted on the
// device from the rollout store (C ABI, the classification and the table layout in full: include/atr_track_stats.h).
//
//   k_track_stats         one wavefront per env, four envs per 256-thread workgroup. A lane holds one aligned dword (four cells)
//                         of each byte window, or cells l, l + 64 and l + 128 of a float window; the compares go through
//                         __ballot, so the counts (popcount), the index of the single 4 / 2 (find-first-set) and the centre cells
//                         (one __shfl) are wave-uniform. The bin of a sample does not depend on the carry, so the steps are taken
//                         kChunk at a time: all loads of a chunk are issued before the first compare (lane k fetches step k's
//                         reward, flag and actions), then the carry walks the chunk's bins in step order and lane 0 adds into the
//                         workgroup's LDS counters. At the end every non-zero LDS counter goes out as ONE 64-bit integer atomic
//                         add: the totals are sums of integers, the same in any execution order.
//   k_track_stats_drain   copies both tables out and zeroes them, one workgroup.
//
// Cost model: 4096 envs x 20 steps x 2 windows x 169 B = 27.7 MB read per rollout (u8), 3.5 us of HBM time; the launch is bound
// by the number of load instructions and their latency, not by bytes (DESIGN.md section 5 "Tracking statistics": byte-wide
// loads, three per window, took 47 us; a 16-wave workgroup form with a quarter of the global atomics took 62 us).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/atr_track_stats.h"

namespace atr {

constexpr int kTrackWaves = 4;                                       // envs per workgroup (one wave each)
constexpr int kTrackBlock = 64 * kTrackWaves;
constexpr int kChunk = 10;                                           // steps whose loads are in flight together
constexpr int kActCounters = 2 * ATR_TRACK_ACT_ROWS * ATR_TRACK_MAX_ACTIONS;        // 2720
constexpr int kCounters = ATR_TRACK_HIST + kActCounters;             // 2896 LDS counters (11.3 KB)
constexpr int kTailLanes = ATR_TRACK_WINDOW - 128;                   // 41 lanes hold a third cell

struct TrackArgs {
    const void *obs;
    long long obs_st, obs_se, obs_sp;
    const float *rew;
    long long rew_st, rew_se;
    const uint8_t *done;
    long long done_st, done_se;
    const long long *act;
    long long act_st, act_se, act_sp;
    int *carry;
    unsigned long long *hist, *act_hist;
    int T, N, n_actions, flags;
};

// What one lane holds of a window. Bytes: ONE aligned dword of the 43 or 44 that cover the window's 169 bytes (a window starts at
// any byte address — 169 is odd — so the dwords are taken from the aligned address below it and `mis` bytes are skipped; an
// aligned dword that holds a byte of the window lies in the window's own page). Floats: cells l, l + 64, l + 128.
template <typename ObsT> struct WinRegs;
template <> struct WinRegs<uint8_t> {
    uint32_t v;
    int mis;
};
template <> struct WinRegs<float> {
    float v[3];
};

__device__ inline void load_window(const uint8_t *w, int lane, WinRegs<uint8_t> &o)
{
    const int mis = (int)((uintptr_t)w & 3u);
    o.mis = mis;
    o.v = lane * 4 < mis + ATR_TRACK_WINDOW ? ((const uint32_t *)(w - mis))[lane] : 0u;
}

__device__ inline void load_window(const float *w, int lane, WinRegs<float> &o)
{
    o.v[0] = w[lane];
    o.v[1] = w[lane + 64];
    o.v[2] = lane < kTailLanes ? w[lane + 128] : 0.0f;
}

struct Found {
    int n, idx;        // how many cells hold the value, and the index of one of them (THE one when n == 1)
};

__device__ inline Found find_cells(const WinRegs<uint8_t> &r, int lane, unsigned val)
{
    Found f = {0, 0};
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int c = lane * 4 + b - r.mis;
        const unsigned long long m = __ballot(c >= 0 && c < ATR_TRACK_WINDOW && ((r.v >> (8 * b)) & 255u) == val);
        f.n += __popcll(m);
        if (m) f.idx = (__ffsll((long long)m) - 1) * 4 + b - r.mis;
    }
    return f;
}

__device__ inline Found find_cells(const WinRegs<float> &r, int lane, unsigned val)
{
    Found f = {0, 0};
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const unsigned long long m = __ballot(r.v[j] == (float)val);        // (lanes without a third cell hold 0)
        f.n += __popcll(m);
        if (m) f.idx = 64 * j + __ffsll((long long)m) - 1;
    }
    return f;
}

__device__ inline bool centre_is(const WinRegs<uint8_t> &r, unsigned val)
{
    const int p = ATR_TRACK_CENTRE + r.mis;
    return ((__shfl(r.v, p >> 2) >> (8 * (p & 3))) & 255u) == val;
}

__device__ inline bool centre_is(const WinRegs<float> &r, unsigned val)
{
    return __shfl(r.v[1], ATR_TRACK_CENTRE - 64) == (float)val;
}

// The bin of one sample (wave-uniform): four = the 4s of window 0, two = the 2s of window 1, c0 = window 0's centre is 2,
// c1 = window 1's centre is 4, r = the tracker's reward.
__device__ inline int sample_bin(Found four, Found two, bool c0, bool c1, float r)
{
    if (!c0 || !c1) return ATR_TRACK_INCONSISTENT;
    if (r == 1.0f) return four.n == 0 && two.n == 0 ? ATR_TRACK_CENTRE : ATR_TRACK_INCONSISTENT;
    if (four.n == 0 && two.n == 0) return ATR_TRACK_OUT;
    if (four.n == 1 && two.n == 1 && two.idx == ATR_TRACK_WINDOW - 1 - four.idx) return four.idx;
    return ATR_TRACK_INCONSISTENT;
}

template <typename ObsT>
__global__ __launch_bounds__(kTrackBlock) void k_track_stats(TrackArgs a)
{
    __shared__ unsigned cnt[kCounters];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_cnt = a.act ? kCounters : ATR_TRACK_HIST;
    for (int i = tid; i < n_cnt; i += kTrackBlock) cnt[i] = 0u;
    __syncthreads();
    const long long e = (long long)blockIdx.x * kTrackWaves + wave;
    if (e < a.N) {        // (wave-uniform)
        const ObsT *obs = (const ObsT *)a.obs + e * a.obs_se;
        const float *rew = a.rew + e * a.rew_se;
        const uint8_t *done = a.done + e * a.done_se;
        const long long *act = a.act ? a.act + e * a.act_se : nullptr;
        int carry = a.carry[e];
        if (carry < -1 || carry > ATR_TRACK_OUT) carry = -1;
        unsigned samples = 0u;
        for (int t0 = 0; t0 < a.T; t0 += kChunk) {
            // lane k < kChunk fetches step t0 + k's reward, flag and actions (an action outside [0, n_actions) becomes -1);
            // every lane fetches its part of the chunk's windows. A step past the end reads the last step again: unused.
            const long long ts = min((long long)t0 + (lane < kChunk ? lane : 0), (long long)a.T - 1);
            const float r_l = rew[ts * a.rew_st];
            const int d_l = done[ts * a.done_st];
            int a0_l = -1, a1_l = -1;
            if (act) {
                const long long v0 = act[ts * a.act_st], v1 = act[ts * a.act_st + a.act_sp];
                a0_l = v0 >= 0 && v0 < a.n_actions ? (int)v0 : -1;
                a1_l = v1 >= 0 && v1 < a.n_actions ? (int)v1 : -1;
            }
            WinRegs<ObsT> x[kChunk], y[kChunk];
#pragma unroll
            for (int k = 0; k < kChunk; k++) {
                const long long t = min((long long)t0 + k, (long long)a.T - 1);
                const ObsT *w0 = obs + (t + 1) * a.obs_st;
                load_window(w0, lane, x[k]);
                load_window(w0 + a.obs_sp, lane, y[k]);
            }
#pragma unroll
            for (int k = 0; k < kChunk; k++) {
                if (t0 + k >= a.T) continue;        // (no break: the loop must unroll fully, x / y stay in registers)
                const Found four = find_cells(x[k], lane, 4u), two = find_cells(y[k], lane, 2u);
                const bool c0 = centre_is(x[k], 2u), c1 = centre_is(y[k], 4u);
                const float r = __shfl(r_l, k);
                const int d = __shfl(d_l, k);
                const int before = carry;
                int bin;
                if (d && !(a.flags & ATR_TRACK_NO_AUTO_RESET)) {
                    bin = ATR_TRACK_TERMINAL;
                    carry = -1;
                } else {
                    bin = sample_bin(four, two, c0, c1, r);
                    carry = (bin == ATR_TRACK_INCONSISTENT || d) ? -1 : bin;
                }
                samples += 1u;
                const int av[2] = {__shfl(a0_l, k), __shfl(a1_l, k)};
                if (lane == 0) {
                    atomicAdd(&cnt[bin], 1u);
                    if (act && before >= 0) {
#pragma unroll
                        for (int p = 0; p < 2; p++) {
                            if (av[p] >= 0)
                                atomicAdd(&cnt[ATR_TRACK_HIST + (p * ATR_TRACK_ACT_ROWS + before) * ATR_TRACK_MAX_ACTIONS + av[p]], 1u);
                            else
                                atomicAdd(&cnt[ATR_TRACK_INCONSISTENT], 1u);
                        }
                    }
                }
            }
        }
        if (lane == 0) {
            atomicAdd(&cnt[ATR_TRACK_SAMPLES], samples);
            a.carry[e] = carry;
        }
    }
    __syncthreads();
    for (int i = tid; i < n_cnt; i += kTrackBlock) {
        const unsigned c = cnt[i];
        if (c) atomicAdd(i < ATR_TRACK_HIST ? a.hist + i : a.act_hist + (i - ATR_TRACK_HIST), (unsigned long long)c);
    }
}

__global__ __launch_bounds__(256) void k_track_stats_drain(unsigned long long *__restrict__ hist, unsigned long long *__restrict__ act_hist,
                                                           unsigned long long *__restrict__ out_hist,
                                                           unsigned long long *__restrict__ out_act_hist)
{
    for (int i = threadIdx.x; i < kCounters; i += 256) {
        unsigned long long *src = i < ATR_TRACK_HIST ? hist + i : act_hist + (i - ATR_TRACK_HIST);
        unsigned long long *dst = i < ATR_TRACK_HIST ? out_hist + i : out_act_hist + (i - ATR_TRACK_HIST);
        *dst = *src;
        *src = 0ull;
    }
}

// (as csrc/episode_stats_hip.hip: the refusals put their text into the calling thread's t2d_last_error() buffer)
static int track_refuse(int code, const char *fmt, ...)
{
    char *buf = const_cast<char *>(t2d_last_error());
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, 256, fmt, ap);
    va_end(ap);
    return code;
}

static int track_launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : track_refuse(T2D_ERR_HIP, "%s: launch failed: %s", what, hipGetErrorString(e));
}

}  // namespace atr

using namespace atr;

extern "C" int atr_track_stats(const void *obs, int obs_is_u8, long long obs_st, long long obs_se, long long obs_sp, const float *rew,
                               long long rew_st, long long rew_se, long long rew_sp, const unsigned char *done, long long done_st,
                               long long done_se, const long long *act, long long act_st, long long act_se, long long act_sp,
                               int *carry, unsigned long long *hist, unsigned long long *act_hist, int T, int N, int n_actions,
                               int flags, void *stream)
{
    if (!obs || !rew || !done || !carry || !hist || !act_hist)
        return track_refuse(T2D_ERR_INVALID, "atr_track_stats: null pointer (obs %p rew %p done %p carry %p hist %p act_hist %p)", obs,
                            (const void *)rew, (const void *)done, (void *)carry, (void *)hist, (void *)act_hist);
    if (N <= 0 || T <= 0) return track_refuse(T2D_ERR_INVALID, "atr_track_stats: needs N > 0 and T > 0 (N %d, T %d)", N, T);
    if (T > ATR_TRACK_MAX_T) return track_refuse(T2D_ERR_INVALID, "atr_track_stats: T %d above %d steps per call", T, ATR_TRACK_MAX_T);
    if (n_actions < 1 || n_actions > ATR_TRACK_MAX_ACTIONS)
        return track_refuse(T2D_ERR_INVALID, "atr_track_stats: n_actions %d outside [1, %d]", n_actions, ATR_TRACK_MAX_ACTIONS);
    if (flags & ~ATR_TRACK_NO_AUTO_RESET) return track_refuse(T2D_ERR_INVALID, "atr_track_stats: unknown flags 0x%x", flags);
    if (obs_st < 0 || obs_se < 0 || obs_sp < 0 || rew_st < 0 || rew_se < 0 || rew_sp < 0 || done_st < 0 || done_se < 0 || act_st < 0 ||
        act_se < 0 || act_sp < 0)
        return track_refuse(T2D_ERR_INVALID, "atr_track_stats: negative element stride");
    if (((uintptr_t)hist | (uintptr_t)act_hist | (uintptr_t)act) & 7u)
        return track_refuse(T2D_ERR_INVALID, "atr_track_stats: hist %p / act_hist %p / act %p not 8-byte aligned", (void *)hist,
                            (void *)act_hist, (const void *)act);
    if ((((uintptr_t)carry | (uintptr_t)rew) & 3u) || (!obs_is_u8 && ((uintptr_t)obs & 3u)))
        return track_refuse(T2D_ERR_INVALID, "atr_track_stats: carry / rew / float32 obs not 4-byte aligned");
    (void)rew_sp;        // (only player 0's reward is read: element p = 0)
    TrackArgs a;
    a.obs = obs;
    a.obs_st = obs_st, a.obs_se = obs_se, a.obs_sp = obs_sp;
    a.rew = rew;
    a.rew_st = rew_st, a.rew_se = rew_se;
    a.done = (const uint8_t *)done;
    a.done_st = done_st, a.done_se = done_se;
    a.act = act;
    a.act_st = act_st, a.act_se = act_se, a.act_sp = act_sp;
    a.carry = carry, a.hist = hist, a.act_hist = act_hist;
    a.T = T, a.N = N, a.n_actions = n_actions, a.flags = flags;
    const dim3 grid((unsigned)((N + kTrackWaves - 1) / kTrackWaves)), block(kTrackBlock);
    if (obs_is_u8)
        hipLaunchKernelGGL(k_track_stats<uint8_t>, grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_track_stats<float>, grid, block, 0, (hipStream_t)stream, a);
    return track_launched("atr_track_stats");
}

extern "C" int atr_track_stats_drain(unsigned long long *hist, unsigned long long *act_hist, unsigned long long *out_hist,
                                     unsigned long long *out_act_hist, void *stream)
{
    if (!hist || !act_hist || !out_hist || !out_act_hist)
        return track_refuse(T2D_ERR_INVALID, "atr_track_stats_drain: null pointer (hist %p act_hist %p out_hist %p out_act_hist %p)",
                            (void *)hist, (void *)act_hist, (void *)out_hist, (void *)out_act_hist);
    if (((uintptr_t)hist | (uintptr_t)act_hist | (uintptr_t)out_hist | (uintptr_t)out_act_hist) & 7u)
        return track_refuse(T2D_ERR_INVALID, "atr_track_stats_drain: a table is not 8-byte aligned");
    hipLaunchKernelGGL(k_track_stats_drain, dim3(1), dim3(256), 0, (hipStream_t)stream, hist, act_hist, out_hist, out_act_hist);
    return track_launched("atr_track_stats_drain");
}
