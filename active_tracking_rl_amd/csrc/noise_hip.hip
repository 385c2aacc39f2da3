// noise_hip.hip — sensor noise: a player's 13 x 13 window flickers, misses the other player and shows false detections, each a
// draw that is a pure function of (key, global env id, per-window clock, player) (C ABI and the rule in full: include/atr_noise.h;
// the draw blocks and the verdict on a cell themselves: atr_noise_rule.h).
//
//   k_noise               one wavefront per (env e, window p), four per 256-thread workgroup (the shape of k_footprints,
//                         csrc/footprints_hip.hip). The wave owns window (e, p) and clock entry (e, p): no two waves ever share a
//                         byte they write. A wave whose role bit is clear returns before any load. Lane L loads cells L, L + 64
//                         and L + 128 (the last only below 169) and the clock entry — one address in every lane, so the clock
//                         is wave-uniform without a broadcast — before any store. It computes Philox block 0 (the window's miss
//                         and ghost: the same in every lane) and block 1 + L (its own cells' flicker words), then applies the
//                         verdict to its own cells and stores only those that change: a byte store per cell of a byte window, so
//                         that no lane writes outside its own window at any alignment. Lane 0 stores the advanced clock. No LDS,
//                         no cross-lane traffic.
//
// Cost model: per wave 169 cells and one clock word read, 20 Philox rounds per lane, at most 169 cells and one word stored;
// 4096 envs x 2 waves. Measured at that size (profiles/noise.txt): 6.0 - 6.6 us per launch next to 5.0 / 5.5 us for k_fov — a
// launch plus the Philox rounds. DESIGN.md section 3 "Sensor noise".
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/atr_noise.h"
#include "atr_noise_rule.h"
#include "t2d_state_view.h"

static_assert(atr_noise::kWindow == ATR_NOISE_WINDOW && atr_noise::kCentre == ATR_NOISE_CENTRE && atr_noise::kOne == ATR_NOISE_ONE &&
              atr_noise::kTag == ATR_NOISE_TAG && atr_noise::kPeek == ATR_NOISE_PEEK && atr_noise::kAdvance == ATR_NOISE_ADVANCE &&
              ATR_NOISE_WINDOW > 128 && ATR_NOISE_WINDOW <= 192,
              "atr_noise_rule.h and include/atr_noise.h state one rule, and a window is three cells per lane of one wavefront");

namespace atr_noise {

constexpr int kNzWaves = 4;                                          // (env, window) pairs per workgroup (one wave each)
constexpr int kNzBlock = 64 * kNzWaves;

struct NoiseArgs {
    void *obs;
    long long se, sp;
    uint32_t *clock;
    unsigned long long key;
    uint32_t env_base;
    int n, flicker, miss, ghost, roles, mode;
};

template <typename ObsT>
__device__ __forceinline__ int reads_of(ObsT v, int other)
{
    return v == (ObsT)0 ? kZero : v == (ObsT)1 ? kWall : v == (ObsT)other ? kOther : kElse;
}

template <typename ObsT>
__global__ __launch_bounds__(kNzBlock) void k_noise(NoiseArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long w = (long long)blockIdx.x * kNzWaves + wave;
    if (w >= 2ll * a.n) return;                        // (wave-uniform)
    const long long e = w >> 1;
    const int p = (int)(w & 1);
    if (((a.roles >> p) & 1) == 0) return;             // (wave-uniform: before any load)
    ObsT *win = (ObsT *)a.obs + e * a.se + (long long)p * a.sp;
    const int other = other_value(p);
    // every load of the wave: its three cells and the clock entry
    const bool third = lane + 128 < kWindow;
    const int r0 = reads_of(win[lane], other), r1 = reads_of(win[lane + 64], other);
    const int r2 = third ? reads_of(win[lane + 128], other) : kElse;
    const uint32_t clk = __builtin_amdgcn_readfirstlane(a.clock[w]) + (a.mode == kAdvance ? 1u : 0u);
    const uint32_t env = a.env_base + (uint32_t)e;
    uint32_t b0[4], bl[4];
    draw_block(a.key, env, clk, p, 0u, b0);
    draw_block(a.key, env, clk, p, flicker_block(lane), bl);
    const bool miss_hit = passes(b0[0], a.miss), ghost_hit = passes(b0[1], a.ghost);
    const int g = ghost_cell(b0[2]);
    const int v0 = verdict(lane, r0, p, bl[0], a.flicker, miss_hit, ghost_hit, g);
    const int v1 = verdict(lane + 64, r1, p, bl[1], a.flicker, miss_hit, ghost_hit, g);
    const int v2 = third ? verdict(lane + 128, r2, p, bl[2], a.flicker, miss_hit, ghost_hit, g) : kKeep;
    if (v0 != kKeep) win[lane] = (ObsT)v0;
    if (v1 != kKeep) win[lane + 64] = (ObsT)v1;
    if (v2 != kKeep) win[lane + 128] = (ObsT)v2;
    if (lane == 0 && a.mode == kAdvance) a.clock[w] = clk;
}

// (as csrc/footprints_hip.hip: the refusals put their text into the calling thread's t2d_last_error() buffer)
static int nz_refuse(int code, const char *fmt, ...)
{
    char *buf = const_cast<char *>(t2d_last_error());
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, 256, fmt, ap);
    va_end(ap);
    return code;
}

struct NzDeviceScope {
    int prev = -1;
    bool changed = false;
    explicit NzDeviceScope(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = (hipSetDevice(dev) == hipSuccess);
    }
    ~NzDeviceScope()
    {
        if (changed) (void)hipSetDevice(prev);
    }
};

}  // namespace atr_noise

using namespace atr_noise;

extern "C" int atr_noise_windows(t2d_handle *h, void *obs, int is_u8, long long se, long long sp, unsigned int *clock,
                                 unsigned long long key, int flicker, int miss, int ghost, int roles, int mode, void *stream)
{
    if (!obs || !clock) return nz_refuse(T2D_ERR_INVALID, "atr_noise_windows: null pointer (obs %p clock %p)", obs, (void *)clock);
    if (flicker < 0 || flicker > ATR_NOISE_ONE)
        return nz_refuse(T2D_ERR_INVALID, "atr_noise_windows: flicker threshold %d outside 0 .. 16777216", flicker);
    if (miss < 0 || miss > ATR_NOISE_ONE)
        return nz_refuse(T2D_ERR_INVALID, "atr_noise_windows: miss threshold %d outside 0 .. 16777216", miss);
    if (ghost < 0 || ghost > ATR_NOISE_ONE)
        return nz_refuse(T2D_ERR_INVALID, "atr_noise_windows: ghost threshold %d outside 0 .. 16777216", ghost);
    if (roles < 1 || roles > 3) return nz_refuse(T2D_ERR_INVALID, "atr_noise_windows: roles %d outside 1 .. 3", roles);
    if (mode < ATR_NOISE_PEEK || mode > ATR_NOISE_ADVANCE)
        return nz_refuse(T2D_ERR_INVALID, "atr_noise_windows: mode %d outside 0 .. 1", mode);
    if (se < 0 || sp < 0)
        return nz_refuse(T2D_ERR_INVALID, "atr_noise_windows: negative element stride (se %lld, sp %lld)", se, sp);
    if (!is_u8 && ((uintptr_t)obs & 3u))
        return nz_refuse(T2D_ERR_INVALID, "atr_noise_windows: float32 windows not 4-byte aligned (obs %p)", obs);
    if ((uintptr_t)clock & 3u)
        return nz_refuse(T2D_ERR_INVALID, "atr_noise_windows: clock %p is not 4-byte aligned", (void *)clock);
    if (!h) return nz_refuse(T2D_ERR_INVALID, "atr_noise_windows: null handle");
    t2d_state_view v;
    const int rc = t2d_state_view_get(h, &v);
    if (rc) return rc;
    if (!v.ready) return nz_refuse(T2D_ERR_INVALID, "atr_noise_windows: call t2d_reset (all envs) first");
    if (v.obs_full)
        return nz_refuse(T2D_ERR_INVALID, "atr_noise_windows: the handle observes the whole map (the rule is stated for the "
                                          "13 x 13 windows of 'Partial' observations)");
    NzDeviceScope guard(v.device);
    NoiseArgs a;
    a.obs = obs, a.se = se, a.sp = sp;
    a.clock = clock;
    a.key = key;
    a.env_base = v.env_base;
    a.n = v.n, a.flicker = flicker, a.miss = miss, a.ghost = ghost, a.roles = roles, a.mode = mode;
    const dim3 grid((unsigned)((2ll * v.n + kNzWaves - 1) / kNzWaves)), block(kNzBlock);
    if (is_u8)
        hipLaunchKernelGGL((k_noise<uint8_t>), grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((k_noise<float>), grid, block, 0, (hipStream_t)stream, a);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : nz_refuse(T2D_ERR_HIP, "atr_noise_windows: launch failed: %s", hipGetErrorString(err));
}
