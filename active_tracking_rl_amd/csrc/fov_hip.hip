// fov_hip.hip — facing and field of view: every player keeps a facing byte that turns with its actions, and every cell of its
// 13 x 13 window outside the cone ahead is rewritten as an "unseen" value (C ABI and the rule in full: include/atr_fov.h; the
// predicate and the turn rule themselves: atr_fov_rule.h).
//
//   k_fov                 one wavefront per window (e, p), four windows per 256-thread workgroup (the shape of k_occlude, csrc/
//                         occlusion_hip.hip). Every lane of the wave works out the player's new facing from the same three bytes /
//                         words (facing, done[e], the player's action), so the result is wave-uniform without a broadcast; lane 0
//                         stores it, and no other wave ever addresses that byte. Lane l then owns cells l, l + 64, l + 128. Which
//                         of them are hidden is arithmetic on (facing, aperture, near) alone — no table, no ballot, and no look at
//                         the window — so an IN-PLACE call reads no window: it stores `hidden` into the hidden cells, a byte store
//                         per cell of a byte window, so that no lane ever writes a byte of another window, whatever the window's
//                         alignment. OUT OF PLACE a lane loads its three cells first (the wave has read its whole window before it
//                         stores any of it) and stores all three, hidden or copied. A wave whose player has aperture 360, and in
//                         place one whose facing is NONE, ends after the turn.
//
// Cost model: in place at 90 degrees 115 of 169 cells stored per window and nothing read: 4096 envs x 2 windows x 115 B = 0.9 MB of
// byte stores per step (u8; four times that for floats), plus 3 small loads and one byte store per wave for the turn. The launch is
// launch-bound at that size. DESIGN.md section 3 "Field of view".
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/atr_fov.h"
#include "atr_fov_rule.h"

static_assert(atr_fov::kNone == ATR_FOV_NONE && atr_fov::kSide == ATR_FOV_SIDE && atr_fov::kCentre == ATR_FOV_CENTRE &&
              atr_fov::kMaxNear == ATR_FOV_MAX_NEAR && ATR_FOV_SIDE * ATR_FOV_SIDE == ATR_FOV_WINDOW,
              "atr_fov_rule.h and include/atr_fov.h state one rule");

namespace atr_fov {

constexpr int kFovWaves = 4;                                         // windows per workgroup (one wave each)
constexpr int kFovBlock = 64 * kFovWaves;

struct FovArgs {
    const void *src;
    void *dst;
    long long total, se, sp;
    unsigned char *facing;
    const void *act0, *act1;
    const unsigned char *done;
    int n_win, act_dtype, aperture0, aperture1, near, hidden;
};

__device__ inline long long fov_action(const void *a, int dtype, long long e)
{
    return dtype == T2D_ACT_U8 ? (long long)((const uint8_t *)a)[e]
         : dtype == T2D_ACT_I32 ? (long long)((const int32_t *)a)[e] : ((const long long *)a)[e];
}

template <typename ObsT>
__global__ __launch_bounds__(kFovBlock) void k_fov(FovArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long win = (long long)blockIdx.x * kFovWaves + wave;
    if (win >= a.total) return;        // (wave-uniform)
    const long long e = win / a.n_win;
    const int p = (int)(win - e * a.n_win);
    // the turn: every lane computes it from the same addresses, lane 0 stores it
    const void *act = p ? a.act1 : a.act0;
    const int old = a.facing[win];
    const int facing = turn(old, a.done != nullptr, a.done ? (int)a.done[e] : 0, act != nullptr, act ? fov_action(act, a.act_dtype, e) : 0);
    if (lane == 0 && facing != old) a.facing[win] = (unsigned char)facing;
    const int aperture = p ? a.aperture1 : a.aperture0;
    if (aperture == 360) return;       // not restricted: the window is neither read nor written
    const bool in_place = a.src == a.dst;
    if (in_place && (facing < 0 || facing > 3)) return;      // looks all round: nothing to store
    const long long off = e * a.se + (long long)p * a.sp;
    const ObsT *src = (const ObsT *)a.src + off;
    ObsT *dst = (ObsT *)a.dst + off;
    ObsT v[3] = {};
    if (!in_place) {
#pragma unroll
        for (int i = 0; i < 3; i++)
            if (64 * i + lane < ATR_FOV_WINDOW) v[i] = src[64 * i + lane];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int c = 64 * i + lane;
        if (c < ATR_FOV_WINDOW) {
            const bool hid = !visible(facing, aperture, a.near, c / ATR_FOV_SIDE, c % ATR_FOV_SIDE);
            if (hid || !in_place) dst[c] = hid ? (ObsT)a.hidden : v[i];
        }
    }
}

// (as csrc/occlusion_hip.hip: the refusals put their text into the calling thread's t2d_last_error() buffer)
static int fov_refuse(int code, const char *fmt, ...)
{
    char *buf = const_cast<char *>(t2d_last_error());
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, 256, fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace atr_fov

using namespace atr_fov;

extern "C" int atr_fov_windows(const void *src, void *dst, int is_u8, long long n_env, int n_win, long long se, long long sp,
                               unsigned char *facing, const void *a0, const void *a1, int act_dtype, const unsigned char *done,
                               int aperture0, int aperture1, int near, int hidden, void *stream)
{
    if (!src || !dst || !facing)
        return fov_refuse(T2D_ERR_INVALID, "atr_fov_windows: null pointer (src %p dst %p facing %p)", src, dst, (void *)facing);
    if (n_env <= 0 || n_win <= 0)
        return fov_refuse(T2D_ERR_INVALID, "atr_fov_windows: needs n_env > 0 and n_win > 0 (n_env %lld, n_win %d)", n_env, n_win);
    if (n_win > 2) return fov_refuse(T2D_ERR_INVALID, "atr_fov_windows: n_win %d above the 2 players of an env", n_win);
    if (n_env > ATR_FOV_MAX_WINDOWS / n_win)
        return fov_refuse(T2D_ERR_INVALID, "atr_fov_windows: %lld x %d windows above %d per call", n_env, n_win, ATR_FOV_MAX_WINDOWS);
    if (!aperture_ok(aperture0) || !aperture_ok(aperture1))
        return fov_refuse(T2D_ERR_INVALID, "atr_fov_windows: aperture (%d, %d) outside {90, 180, 270, 360}", aperture0, aperture1);
    if (near < 0 || near > ATR_FOV_MAX_NEAR) return fov_refuse(T2D_ERR_INVALID, "atr_fov_windows: near %d outside 0 .. 6", near);
    if (hidden < 0 || hidden > 255) return fov_refuse(T2D_ERR_INVALID, "atr_fov_windows: hidden %d outside 0 .. 255", hidden);
    if ((a0 || a1) && act_dtype != T2D_ACT_U8 && act_dtype != T2D_ACT_I32 && act_dtype != T2D_ACT_I64)
        return fov_refuse(T2D_ERR_INVALID, "atr_fov_windows: act_dtype %d is no T2D_ACT_* value", act_dtype);
    if (se < 0 || sp < 0) return fov_refuse(T2D_ERR_INVALID, "atr_fov_windows: negative element stride (se %lld, sp %lld)", se, sp);
    if (!is_u8 && (((uintptr_t)src | (uintptr_t)dst) & 3u))
        return fov_refuse(T2D_ERR_INVALID, "atr_fov_windows: float32 windows not 4-byte aligned (src %p dst %p)", src, dst);
    if (src != dst) {
        // the bytes from the first window's first cell to the last window's last cell, of either side
        const unsigned __int128 cells = (unsigned __int128)(n_env - 1) * (unsigned long long)se +
                                        (unsigned __int128)(n_win - 1) * (unsigned long long)sp + ATR_FOV_WINDOW;
        const unsigned __int128 bytes = cells * (is_u8 ? 1u : 4u);
        const unsigned __int128 s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
        if (s0 < d0 + bytes && d0 < s0 + bytes)
            return fov_refuse(T2D_ERR_INVALID, "atr_fov_windows: src %p and dst %p differ and their byte ranges overlap", src, dst);
    }
    FovArgs a;
    a.src = src, a.dst = dst;
    a.total = n_env * n_win, a.se = se, a.sp = sp;
    a.facing = facing;
    a.act0 = a0, a.act1 = n_win > 1 ? a1 : nullptr;
    a.done = done;
    a.n_win = n_win, a.act_dtype = act_dtype;
    a.aperture0 = aperture0, a.aperture1 = aperture1;
    a.near = near, a.hidden = hidden;
    const dim3 grid((unsigned)((a.total + kFovWaves - 1) / kFovWaves)), block(kFovBlock);
    if (is_u8)
        hipLaunchKernelGGL((k_fov<uint8_t>), grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((k_fov<float>), grid, block, 0, (hipStream_t)stream, a);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : fov_refuse(T2D_ERR_HIP, "atr_fov_windows: launch failed: %s", hipGetErrorString(err));
}
