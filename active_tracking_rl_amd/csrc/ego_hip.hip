// ego_hip.hip — the egocentric view: a player's 13 x 13 window turns with the player so that it always looks up, and its four
// actions mean forward / back / left / right (C ABI and the rule in full: include/atr_ego.h; the two tables and the cell map
// themselves: atr_ego_rule.h; the heading is the facing byte of the field of view and turns by atr_fov::turn, atr_fov_rule.h).
//
//   k_ego_actions         one lane per (env, player): it reads the player's facing byte and its relative action and writes
//                         ABS[heading][rel] (a player outside `roles`: the action as it is). The table is one 32-bit constant, two
//                         bits per entry: no memory behind it. It only reads the facing bytes.
//
//   k_ego                 one wavefront per window (e, p), four windows per 256-thread workgroup (the shape of k_fov, csrc/
//                         fov_hip.hip). Every lane of the wave works out the player's new facing from the same three bytes / words
//                         (facing, done[e], the player's absolute action), so the result is wave-uniform without a broadcast; lane 0
//                         stores it, and no other wave ever addresses that byte. Lane l then owns cells l, l + 64, l + 128. Unlike
//                         the field of view's, this pass MOVES every cell, so an in-place call cannot store as it goes: the wave
//                         loads its 169 cells coalesced, parks them in its own 169-element slot of LDS, reads them back permuted
//                         (cell c of the output is cell src_cell(heading, c) of the input) and stores coalesced. Every global store
//                         takes its value from an LDS read, and the LDS reads follow the LDS writes of all three loaded cells of
//                         every lane (a wavefront-scope fence and a wave barrier: DS operations of one wave execute in order), so
//                         every load of the wave has returned before any store is issued — by data dependence, not by the order of
//                         statements. The four waves of a workgroup share nothing: there is no workgroup barrier, and a wave that
//                         returns early (past the last window, a player outside `roles`, in place with heading 0 / NONE: nothing to
//                         move) leaves nobody waiting. A byte window's cells are stored by byte, so that no lane ever writes a byte
//                         of another window, whatever the window's alignment.
//
// Cost model: in place 169 B read and 169 B written per turned byte window (four times that for floats), nothing for a window of
// heading 0 / NONE: at most 4096 envs x 2 windows x 338 B = 2.8 MB per step for bytes, 11 MB for floats, plus 3 small loads and one
// byte store per wave for the turn; 4 x 169 x 4 B = 2.7 KB of LDS per workgroup. The launch is launch-bound at that size, like its
// neighbours. DESIGN.md section 3 "Egocentric view".
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/atr_ego.h"
#include "atr_ego_rule.h"
#include "atr_fov_rule.h"

static_assert(atr_ego::kSide == ATR_EGO_SIDE && atr_ego::kCentre == ATR_EGO_CENTRE && atr_ego::kWindow == ATR_EGO_WINDOW &&
              ATR_EGO_WINDOW == ATR_FOV_WINDOW && atr_fov::kNone == ATR_FOV_NONE,
              "atr_ego_rule.h, include/atr_ego.h and include/atr_fov.h state one rule");
static_assert(atr_ego::abs_of(0, ATR_EGO_FORWARD) == 0 && atr_ego::abs_of(1, ATR_EGO_FORWARD) == 1 &&
              atr_ego::abs_of(2, ATR_EGO_LEFT) == 1 && atr_ego::abs_of(3, ATR_EGO_RIGHT) == 1 && atr_ego::rel_of(2, 1) == ATR_EGO_LEFT,
              "the packed tables read as include/atr_ego.h states them");

namespace atr_ego {

constexpr int kEgoWaves = 4;                                         // windows per workgroup (one wave each)
constexpr int kEgoBlock = 64 * kEgoWaves;
constexpr int kActBlock = 256;

struct EgoArgs {
    const void *src;
    void *dst;
    long long total, se, sp;
    unsigned char *facing;
    const void *act0, *act1;
    const unsigned char *done;
    int n_win, act_dtype, roles;
};

struct EgoActArgs {
    const unsigned char *facing;
    const void *rel0, *rel1;
    void *abs0, *abs1;
    long long n_env;
    int act_dtype, roles;
};

__device__ inline long long ego_action(const void *a, int dtype, long long e)
{
    return dtype == T2D_ACT_U8 ? (long long)((const uint8_t *)a)[e]
         : dtype == T2D_ACT_I32 ? (long long)((const int32_t *)a)[e] : ((const long long *)a)[e];
}

__global__ __launch_bounds__(kActBlock) void k_ego_actions(EgoActArgs a)
{
    const long long i = (long long)blockIdx.x * kActBlock + threadIdx.x;       // lane i: env i / 2, player i % 2
    if (i >= 2 * a.n_env) return;
    const long long e = i >> 1;
    const int p = (int)(i & 1);
    const void *rel = p ? a.rel1 : a.rel0;
    void *out = p ? a.abs1 : a.abs0;
    if (rel == nullptr) return;                    // (a scripted target takes no action)
    long long k = ego_action(rel, a.act_dtype, e);
    if ((a.roles >> p) & 1) k = abs_of(heading_of((int)a.facing[i]), k);
    if (a.act_dtype == T2D_ACT_U8) ((uint8_t *)out)[e] = (uint8_t)k;
    else if (a.act_dtype == T2D_ACT_I32) ((int32_t *)out)[e] = (int32_t)k;
    else ((long long *)out)[e] = k;
}

template <typename ObsT>
__global__ __launch_bounds__(kEgoBlock) void k_ego(EgoArgs a)
{
    __shared__ ObsT park[kEgoWaves][ATR_EGO_WINDOW];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long win = (long long)blockIdx.x * kEgoWaves + wave;
    if (win >= a.total) return;        // (wave-uniform)
    const long long e = win / a.n_win;
    const int p = (int)(win - e * a.n_win);
    if (!((a.roles >> p) & 1)) return; // not this rule's player: neither turned, read nor written
    // the turn: every lane computes it from the same addresses, lane 0 stores it
    const void *act = p ? a.act1 : a.act0;
    const int old = a.facing[win];
    const int facing = atr_fov::turn(old, a.done != nullptr, a.done ? (int)a.done[e] : 0, act != nullptr,
                                     act ? ego_action(act, a.act_dtype, e) : 0);
    if (lane == 0 && facing != old) a.facing[win] = (unsigned char)facing;
    const int heading = heading_of(facing);
    if (a.src == a.dst && heading == 0) return;               // looks up already: nothing moves
    const long long off = e * a.se + (long long)p * a.sp;
    const ObsT *src = (const ObsT *)a.src + off;
    ObsT *dst = (ObsT *)a.dst + off;
    ObsT *slot = park[wave];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int c = 64 * i + lane;
        if (c < ATR_EGO_WINDOW) slot[c] = src[c];
    }
    // (DS operations of one wave execute in order; this keeps the compiler from moving them and lets other lanes' cells be read)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int c = 64 * i + lane;
        if (c < ATR_EGO_WINDOW) dst[c] = slot[src_cell(heading, c)];
    }
}

// (as csrc/fov_hip.hip: the refusals put their text into the calling thread's t2d_last_error() buffer)
static int ego_refuse(int code, const char *fmt, ...)
{
    char *buf = const_cast<char *>(t2d_last_error());
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, 256, fmt, ap);
    va_end(ap);
    return code;
}

static bool act_dtype_ok(int d) { return d == T2D_ACT_U8 || d == T2D_ACT_I32 || d == T2D_ACT_I64; }

// do the n-element arrays at x and y (elements of `size` bytes) share a byte? (same_ok: not where they are one array)
static bool ego_clash(const void *x, const void *y, long long n, int size, bool same_ok)
{
    if (!x || !y || (same_ok && x == y)) return false;
    const unsigned __int128 bytes = (unsigned __int128)n * (unsigned)size, x0 = (uintptr_t)x, y0 = (uintptr_t)y;
    return x0 < y0 + bytes && y0 < x0 + bytes;
}

}  // namespace atr_ego

using namespace atr_ego;

extern "C" int atr_ego_actions(const unsigned char *facing, const void *rel0, const void *rel1, void *abs0, void *abs1,
                               int act_dtype, long long n_env, int roles, void *stream)
{
    if (!facing || !rel0 || !abs0)
        return ego_refuse(T2D_ERR_INVALID, "atr_ego_actions: null pointer (facing %p rel0 %p abs0 %p)", (const void *)facing, rel0, abs0);
    if ((rel1 == nullptr) != (abs1 == nullptr))
        return ego_refuse(T2D_ERR_INVALID, "atr_ego_actions: rel1 %p and abs1 %p must both be NULL or both be given", rel1, abs1);
    if (n_env <= 0) return ego_refuse(T2D_ERR_INVALID, "atr_ego_actions: needs n_env > 0 (n_env %lld)", n_env);
    if (n_env > ATR_EGO_MAX_WINDOWS / 2)
        return ego_refuse(T2D_ERR_INVALID, "atr_ego_actions: %lld envs x 2 players above %d per call", n_env, ATR_EGO_MAX_WINDOWS);
    if (roles < 1 || roles > 3) return ego_refuse(T2D_ERR_INVALID, "atr_ego_actions: roles %d outside 1 .. 3", roles);
    if (!act_dtype_ok(act_dtype)) return ego_refuse(T2D_ERR_INVALID, "atr_ego_actions: act_dtype %d is no T2D_ACT_* value", act_dtype);
    const int size = act_dtype == T2D_ACT_U8 ? 1 : act_dtype == T2D_ACT_I32 ? 4 : 8;
    if (ego_clash(abs0, rel0, n_env, size, true) || ego_clash(abs1, rel1, n_env, size, true) ||
        ego_clash(abs0, rel1, n_env, size, false) || ego_clash(abs1, rel0, n_env, size, false) ||
        ego_clash(abs0, abs1, n_env, size, false))
        return ego_refuse(T2D_ERR_INVALID, "atr_ego_actions: the action arrays overlap other than abs_p == rel_p (rel %p %p abs %p %p)",
                          rel0, rel1, abs0, abs1);
    EgoActArgs a;
    a.facing = facing;
    a.rel0 = rel0, a.rel1 = rel1, a.abs0 = abs0, a.abs1 = abs1;
    a.n_env = n_env, a.act_dtype = act_dtype, a.roles = roles;
    const dim3 grid((unsigned)((2 * n_env + kActBlock - 1) / kActBlock)), block(kActBlock);
    hipLaunchKernelGGL(k_ego_actions, grid, block, 0, (hipStream_t)stream, a);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : ego_refuse(T2D_ERR_HIP, "atr_ego_actions: launch failed: %s", hipGetErrorString(err));
}

extern "C" int atr_ego_windows(const void *src, void *dst, int is_u8, long long n_env, int n_win, long long se, long long sp,
                               unsigned char *facing, const void *a0, const void *a1, int act_dtype, const unsigned char *done,
                               int roles, void *stream)
{
    if (!src || !dst || !facing)
        return ego_refuse(T2D_ERR_INVALID, "atr_ego_windows: null pointer (src %p dst %p facing %p)", src, dst, (void *)facing);
    if (n_env <= 0 || n_win <= 0)
        return ego_refuse(T2D_ERR_INVALID, "atr_ego_windows: needs n_env > 0 and n_win > 0 (n_env %lld, n_win %d)", n_env, n_win);
    if (n_win > 2) return ego_refuse(T2D_ERR_INVALID, "atr_ego_windows: n_win %d above the 2 players of an env", n_win);
    if (n_env > ATR_EGO_MAX_WINDOWS / n_win)
        return ego_refuse(T2D_ERR_INVALID, "atr_ego_windows: %lld x %d windows above %d per call", n_env, n_win, ATR_EGO_MAX_WINDOWS);
    if (roles < 1 || roles > 3) return ego_refuse(T2D_ERR_INVALID, "atr_ego_windows: roles %d outside 1 .. 3", roles);
    if ((a0 || a1) && !act_dtype_ok(act_dtype))
        return ego_refuse(T2D_ERR_INVALID, "atr_ego_windows: act_dtype %d is no T2D_ACT_* value", act_dtype);
    if (se < 0 || sp < 0) return ego_refuse(T2D_ERR_INVALID, "atr_ego_windows: negative element stride (se %lld, sp %lld)", se, sp);
    if (!is_u8 && (((uintptr_t)src | (uintptr_t)dst) & 3u))
        return ego_refuse(T2D_ERR_INVALID, "atr_ego_windows: float32 windows not 4-byte aligned (src %p dst %p)", src, dst);
    if (src != dst) {
        // the bytes from the first window's first cell to the last window's last cell, of either side
        const unsigned __int128 cells = (unsigned __int128)(n_env - 1) * (unsigned long long)se +
                                        (unsigned __int128)(n_win - 1) * (unsigned long long)sp + ATR_EGO_WINDOW;
        const unsigned __int128 bytes = cells * (is_u8 ? 1u : 4u);
        const unsigned __int128 s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
        if (s0 < d0 + bytes && d0 < s0 + bytes)
            return ego_refuse(T2D_ERR_INVALID, "atr_ego_windows: src %p and dst %p differ and their byte ranges overlap", src, dst);
    }
    EgoArgs a;
    a.src = src, a.dst = dst;
    a.total = n_env * n_win, a.se = se, a.sp = sp;
    a.facing = facing;
    a.act0 = a0, a.act1 = n_win > 1 ? a1 : nullptr;
    a.done = done;
    a.n_win = n_win, a.act_dtype = act_dtype, a.roles = roles;
    const dim3 grid((unsigned)((a.total + kEgoWaves - 1) / kEgoWaves)), block(kEgoBlock);
    if (is_u8)
        hipLaunchKernelGGL((k_ego<uint8_t>), grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((k_ego<float>), grid, block, 0, (hipStream_t)stream, a);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : ego_refuse(T2D_ERR_HIP, "atr_ego_windows: launch failed: %s", hipGetErrorString(err));
}
