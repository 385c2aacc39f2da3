// occlusion_hip.hip — occluded observations: every cell of a 13 x 13 window whose line of sight from the centre is blocked by a wall
// is rewritten as an "unseen" value (C ABI and the rule in full: include/atr_occlusion.h).
//
//   k_occlude             one wavefront per window, four windows per 256-thread workgroup (the shape of k_sight_stats, csrc/
//                         sight_stats_hip.hip). A byte window is fetched as the aligned dwords that cover it, one per lane, and one
//                         __shfl per cell hands lane l the bytes of cells l, l + 64, l + 128; a float window is fetched as those
//                         cells directly. From there both kinds are one code: three __ballot of "cell == 1" are the window's
//                         bitboard (bit c & 63 of word c >> 6 is cell c: no flood runs here, so the rows need no stride of their
//                         own and the ballots are the board), a lane tests its cells' two line masks (a constant table in the same
//                         layout, near line and far line per cell) against it and stores each cell on its own: a byte store per cell
//                         of a byte window, so that no lane ever writes a byte of another window, whatever the window's alignment.
//                         The ballots need every lane's cells: a wave has read its whole window before it stores any of it, which
//                         is what makes dst == src safe. In place only the hidden cells are stored.
//
// Cost model: 4096 envs x 2 windows x 169 B = 1.4 MB read and, out of place, as much written per step (u8; four times that for
// floats); per lane 3 loads of 48 table bytes (8 KB in all, cache resident). The launch is launch-bound at that size. DESIGN.md
// section 5 "Occluded observations".
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/atr_occlusion.h"

namespace atr_occ {

typedef unsigned long long u64;

constexpr int kOccWaves = 4;                                         // windows per workgroup (one wave each)
constexpr int kOccBlock = 64 * kOccWaves;
constexpr int kOccTail = ATR_OCCLUDE_WINDOW - 128;                   // 41 lanes hold a third cell

struct OccArgs {
    const void *src;
    void *dst;
    long long n_win, total, se, sp;
    int hidden;
};

// Per cell X: words 0 .. 2 the near line A(X), words 3 .. 5 the far line B(X) (include/atr_occlusion.h "The RULE"); cell c is bit
// c & 63 of word c >> 6.
struct OccTable {
    u64 m[ATR_OCCLUDE_WINDOW][6];
};

constexpr OccTable make_occ_table()
{
    OccTable t = {};
    for (int x = 0; x < ATR_OCCLUDE_WINDOW; x++) {
        const int dr = x / 13 - 6, dc = x % 13 - 6;
        const int ar = dr < 0 ? -dr : dr, ac = dc < 0 ? -dc : dc, m = ar > ac ? ar : ac;
        const int sr = dr < 0 ? -1 : 1, sc = dc < 0 ? -1 : 1;
        for (int k = 1; k < m; k++) {
            const int lr = (2 * k * ar + m) / (2 * m), lc = (2 * k * ac + m) / (2 * m);
            const int a = (6 + sr * lr) * 13 + 6 + sc * lc;                  // (6, 6) + L(dr, dc)
            const int b = (6 + dr - sr * lr) * 13 + 6 + dc - sc * lc;        // X + L(-dr, -dc)
            t.m[x][a >> 6] |= 1ull << (a & 63);
            t.m[x][3 + (b >> 6)] |= 1ull << (b & 63);
        }
    }
    return t;
}

__device__ const OccTable kOccLines = make_occ_table();

// Cells lane, lane + 64, lane + 128 of a window (0 past the window's end). Bytes: every lane fetches ONE aligned dword of the 43 that
// cover the window's 169 bytes, from the aligned address below the window (an aligned dword that holds a byte of the window lies in
// the window's own page), and the cells come out of the lanes that hold them.
__device__ inline void occ_fetch(const uint8_t *w, int lane, unsigned v[3])
{
    const int mis = (int)((uintptr_t)w & 3u);
    const uint32_t d = lane * 4 < mis + ATR_OCCLUDE_WINDOW ? ((const uint32_t *)(w - mis))[lane] : 0u;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int p = 64 * i + lane + mis;                                   // (p >> 2 <= 48: a lane of this wave)
        const unsigned b = (__shfl(d, p >> 2) >> (8 * (p & 3))) & 255u;
        v[i] = 64 * i + lane < ATR_OCCLUDE_WINDOW ? b : 0u;
    }
}

__device__ inline void occ_fetch(const float *w, int lane, float v[3])
{
    v[0] = w[lane];
    v[1] = w[lane + 64];
    v[2] = lane < kOccTail ? w[lane + 128] : 0.0f;
}

template <typename ObsT, typename RegT>
__global__ __launch_bounds__(kOccBlock) void k_occlude(OccArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long win = (long long)blockIdx.x * kOccWaves + wave;
    if (win >= a.total) return;        // (wave-uniform)
    const long long e = win / a.n_win, p = win - e * a.n_win;
    const long long off = e * a.se + p * a.sp;
    const ObsT *src = (const ObsT *)a.src + off;
    ObsT *dst = (ObsT *)a.dst + off;
    const bool in_place = a.src == a.dst;
    RegT v[3];
    occ_fetch(src, lane, v);
    u64 wall[3];
#pragma unroll
    for (int i = 0; i < 3; i++) wall[i] = __ballot(v[i] == (RegT)ATR_OCCLUDE_WALL);      // (cells past the end hold 0)
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int c = 64 * i + lane;
        if (c < ATR_OCCLUDE_WINDOW) {
            const u64 *ln = kOccLines.m[c];
            const bool near_ = ((wall[0] & ln[0]) | (wall[1] & ln[1]) | (wall[2] & ln[2])) != 0ull;
            const bool far_ = ((wall[0] & ln[3]) | (wall[1] & ln[4]) | (wall[2] & ln[5])) != 0ull;
            const bool hid = near_ && far_;
            if (hid || !in_place) dst[c] = hid ? (ObsT)a.hidden : (ObsT)v[i];
        }
    }
}

// (as csrc/sight_stats_hip.hip: the refusals put their text into the calling thread's t2d_last_error() buffer)
static int occ_refuse(int code, const char *fmt, ...)
{
    char *buf = const_cast<char *>(t2d_last_error());
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, 256, fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace atr_occ

using namespace atr_occ;

extern "C" int atr_occlude_windows(const void *src, void *dst, int is_u8, long long n_env, long long n_win, long long se, long long sp,
                                   int hidden, void *stream)
{
    if (!src || !dst) return occ_refuse(T2D_ERR_INVALID, "atr_occlude_windows: null pointer (src %p dst %p)", src, dst);
    if (n_env <= 0 || n_win <= 0)
        return occ_refuse(T2D_ERR_INVALID, "atr_occlude_windows: needs n_env > 0 and n_win > 0 (n_env %lld, n_win %lld)", n_env, n_win);
    if (n_env > ATR_OCCLUDE_MAX_WINDOWS / n_win)
        return occ_refuse(T2D_ERR_INVALID, "atr_occlude_windows: %lld x %lld windows above %d per call", n_env, n_win,
                          ATR_OCCLUDE_MAX_WINDOWS);
    if (se < 0 || sp < 0) return occ_refuse(T2D_ERR_INVALID, "atr_occlude_windows: negative element stride (se %lld, sp %lld)", se, sp);
    if (hidden < 0 || hidden > 255) return occ_refuse(T2D_ERR_INVALID, "atr_occlude_windows: hidden %d outside 0 .. 255", hidden);
    if (!is_u8 && (((uintptr_t)src | (uintptr_t)dst) & 3u))
        return occ_refuse(T2D_ERR_INVALID, "atr_occlude_windows: float32 windows not 4-byte aligned (src %p dst %p)", src, dst);
    if (src != dst) {
        // the bytes from the first window's first cell to the last window's last cell, of either side
        const unsigned __int128 cells = (unsigned __int128)(n_env - 1) * (unsigned long long)se +
                                        (unsigned __int128)(n_win - 1) * (unsigned long long)sp + ATR_OCCLUDE_WINDOW;
        const unsigned __int128 bytes = cells * (is_u8 ? 1u : 4u);
        const unsigned __int128 s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
        if (s0 < d0 + bytes && d0 < s0 + bytes)
            return occ_refuse(T2D_ERR_INVALID, "atr_occlude_windows: src %p and dst %p differ and their byte ranges overlap", src, dst);
    }
    OccArgs a;
    a.src = src, a.dst = dst;
    a.n_win = n_win, a.total = n_env * n_win, a.se = se, a.sp = sp;
    a.hidden = hidden;
    const dim3 grid((unsigned)((a.total + kOccWaves - 1) / kOccWaves)), block(kOccBlock);
    if (is_u8)
        hipLaunchKernelGGL((k_occlude<uint8_t, unsigned>), grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((k_occlude<float, float>), grid, block, 0, (hipStream_t)stream, a);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : occ_refuse(T2D_ERR_HIP, "atr_occlude_windows: launch failed: %s", hipGetErrorString(err));
}
