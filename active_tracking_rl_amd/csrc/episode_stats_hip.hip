// episode_stats_hip.hip — returns and lengths of the episodes that end during TRAINING rollouts, kept on the device (C ABI
// and the accounting in full: include/atr_stats.h). The reference's worker adds `player.reward` to `reward_sum` per env step on
// the host and writes it when the episode ends (train.py:63-88); a replayed rollout graph cannot read the host per step, so the
// accounts advance in one launch per rollout over the step rewards [T, N, 2] and done flags [T, N] the rollout already stored.
//
//   k_episode_stats         one thread per env: walks the T steps in order, float32 running return per player and running
//                           length; on a done flag the finished episode goes into the env's float64 row fin[e][8]
//                           = {count, R0, R1, R0^2, R1^2, L, L^2, L >= success_len} and the running accounts restart.
//   k_episode_stats_drain   totals[8] = sum over envs of fin in a fixed order, fin zeroed by the same launch.
//
// Cost model: 4096 envs x 20 steps x 9 B = 0.7 MB read per rollout, one dependent float add per step: a launch of a few
// microseconds whose time is its latency. 64-thread workgroups (one wave each) spread a 4096-env shard over 64 CUs; lane i of
// a wave reads env base + i of a step's row, so a wave's loads of one step are 512 B (rewards) and 64 B (flags) of consecutive
// addresses. The loads of a step do not depend on the accounts, so the unrolled loop keeps several steps' loads in flight.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/atr_stats.h"

namespace atr {

constexpr int kStatsBlock = 64;
constexpr int kDrainBlock = ATR_STATS_DRAIN_LANES * ATR_STATS_FIELDS;        // 256: thread j = (row lane j / 8, field j % 8)

__global__ __launch_bounds__(kStatsBlock) void k_episode_stats(const float *__restrict__ rew, long long rew_st, long long rew_sn,
                                                               long long rew_sp, const uint8_t *__restrict__ done,
                                                               long long done_st, long long done_sn, float *__restrict__ run_ret,
                                                               int *__restrict__ run_len, double *__restrict__ fin, int T, int N,
                                                               int success_len)
{
    const int e = blockIdx.x * kStatsBlock + threadIdx.x;
    if (e >= N) return;
    float r0 = run_ret[2 * e], r1 = run_ret[2 * e + 1];
    int len = run_len[e];
    const float *re = rew + (long long)e * rew_sn;
    const uint8_t *de = done + (long long)e * done_sn;
    double *f = fin + (long long)e * ATR_STATS_FIELDS;
#pragma unroll 4
    for (int t = 0; t < T; t++) {
        const float a0 = re[t * rew_st], a1 = re[t * rew_st + rew_sp];
        const uint8_t d = de[t * done_st];
        r0 = r0 + a0;
        r1 = r1 + a1;
        len += 1;
        if (d) {        // (rare; the env's own row: nobody else writes it)
            const double R0 = (double)r0, R1 = (double)r1, L = (double)len;
            f[0] = f[0] + 1.0;
            f[1] = f[1] + R0;
            f[2] = f[2] + R1;
            f[3] = f[3] + R0 * R0;
            f[4] = f[4] + R1 * R1;
            f[5] = f[5] + L;
            f[6] = f[6] + L * L;
            f[7] = f[7] + (len >= success_len ? 1.0 : 0.0);
            r0 = 0.0f;
            r1 = 0.0f;
            len = 0;
        }
    }
    run_ret[2 * e] = r0;
    run_ret[2 * e + 1] = r1;
    run_len[e] = len;
}

// One workgroup of 256 threads: thread j owns field k = j % 8 of row lane r = j / 8 and adds the rows r, r + 32, r + 64, ... in
// that order (a wave reads 64 consecutive doubles per pass: rows 8 w .. 8 w + 7 of the pass), zeroing each as it goes; the 32
// partial rows meet in LDS and threads 0 .. 7 add them in lane order. The order is the one include/atr_stats.h states. A drain
// is one launch per log record, not per iteration: at 4096 envs it reads and zeroes 256 KB.
__global__ __launch_bounds__(kDrainBlock) void k_episode_stats_drain(double *__restrict__ fin, double *__restrict__ totals, int N)
{
    __shared__ double part[kDrainBlock];
    const int j = threadIdx.x, r = j / ATR_STATS_FIELDS, k = j % ATR_STATS_FIELDS;
    double s = 0.0;
    for (long long row = r; row < N; row += ATR_STATS_DRAIN_LANES) {
        double *p = fin + row * ATR_STATS_FIELDS + k;
        s = s + *p;
        *p = 0.0;
    }
    part[j] = s;
    __syncthreads();
    if (j < ATR_STATS_FIELDS) {
        double tot = 0.0;
        for (int q = 0; q < ATR_STATS_DRAIN_LANES; q++) tot = tot + part[q * ATR_STATS_FIELDS + j];
        totals[j] = tot;
    }
}

// t2d_last_error() hands out the calling thread's message buffer of the library (csrc/track2d_hip.hip: 512 chars); the
// refusals of this file put their text there, as the header promises, and stay well inside it.
static int refuse(int code, const char *fmt, ...)
{
    char *buf = const_cast<char *>(t2d_last_error());
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, 256, fmt, ap);
    va_end(ap);
    return code;
}

static int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : refuse(T2D_ERR_HIP, "%s: launch failed: %s", what, hipGetErrorString(e));
}

}  // namespace atr

using namespace atr;

extern "C" int atr_episode_stats(const float *rew, long long rew_st, long long rew_sn, long long rew_sp, const unsigned char *done,
                                 long long done_st, long long done_sn, float *run_ret, int *run_len, double *fin, int T, int N,
                                 int success_len, void *stream)
{
    if (!rew || !done || !run_ret || !run_len || !fin)
        return refuse(T2D_ERR_INVALID, "atr_episode_stats: null pointer (rew %p done %p run_ret %p run_len %p fin %p)", (const void *)rew,
                      (const void *)done, (void *)run_ret, (void *)run_len, (void *)fin);
    if (N <= 0 || T <= 0) return refuse(T2D_ERR_INVALID, "atr_episode_stats: needs N > 0 and T > 0 (N %d, T %d)", N, T);
    if (rew_st < 0 || rew_sn < 0 || rew_sp < 0 || done_st < 0 || done_sn < 0)
        return refuse(T2D_ERR_INVALID, "atr_episode_stats: negative element stride");
    if ((uintptr_t)fin & 7u) return refuse(T2D_ERR_INVALID, "atr_episode_stats: fin %p is not 8-byte aligned", (void *)fin);
    if (((uintptr_t)rew | (uintptr_t)run_ret | (uintptr_t)run_len) & 3u)
        return refuse(T2D_ERR_INVALID, "atr_episode_stats: rew / run_ret / run_len not 4-byte aligned");
    hipLaunchKernelGGL(k_episode_stats, dim3((unsigned)((N + kStatsBlock - 1) / kStatsBlock)), dim3(kStatsBlock), 0,
                       (hipStream_t)stream, rew, rew_st, rew_sn, rew_sp, (const uint8_t *)done, done_st, done_sn, run_ret, run_len,
                       fin, T, N, success_len);
    return launched("atr_episode_stats");
}

extern "C" int atr_episode_stats_drain(double *fin, double *totals, int N, void *stream)
{
    if (!fin || !totals)
        return refuse(T2D_ERR_INVALID, "atr_episode_stats_drain: null pointer (fin %p totals %p)", (void *)fin, (void *)totals);
    if (N <= 0) return refuse(T2D_ERR_INVALID, "atr_episode_stats_drain: needs N > 0 (N %d)", N);
    if (((uintptr_t)fin | (uintptr_t)totals) & 7u)
        return refuse(T2D_ERR_INVALID, "atr_episode_stats_drain: fin %p / totals %p not 8-byte aligned", (void *)fin, (void *)totals);
    hipLaunchKernelGGL(k_episode_stats_drain, dim3(1), dim3(kDrainBlock), 0, (hipStream_t)stream, fin, totals, N);
    return launched("atr_episode_stats_drain");
}
