// footprints_hip.hip — footprints: every player keeps a trail of the last K cells it stepped off, and the other player's 13 x 13
// window shows the prints it could see as free cells (C ABI and the rule in full: include/atr_footprints.h; the recording rule and
// the paint predicate themselves: atr_footprint_rule.h).
//
//   k_footprints          one wavefront per (env e, player p), four per 256-thread workgroup (the shape of k_fov, csrc/fov_hip.hip).
//                         The wave owns trail row (e, p) and is the only writer of window (e, 1 - p): no two waves ever share a
//                         byte they write. Lane j <= K loads entry j — the wave has loaded its whole row before it stores any of
//                         it — and takes entry j - 1 from the lane below with one cross-lane move. The position word and done[e]
//                         are the same addresses in every lane, so what the call does to the row is wave-uniform without a
//                         broadcast of its own. A lane stores only an entry that changed. To paint, lane j in 1 .. K works out
//                         its print's window cell from the two positions, loads that one cell and stores `value` if it read 0: a
//                         byte store per cell of a byte window, so that no lane writes outside its own window at any alignment.
//                         Two prints on one cell store the same value twice.
//
// Cost model: per wave at most 128 B of trail read, K one-cell loads and at most K one-cell stores; 4096 envs x 2 waves. The launch
// is launch-bound at that size, as k_fov and k_occlude are. DESIGN.md section 3 "Footprints".
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/atr_footprints.h"
#include "atr_footprint_rule.h"
#include "t2d_state_view.h"

static_assert(atr_footprint::kEmpty == ATR_FOOTPRINT_EMPTY && atr_footprint::kSide == ATR_FOOTPRINT_SIDE &&
              atr_footprint::kCentre == ATR_FOOTPRINT_CENTRE && atr_footprint::kWindow == ATR_FOOTPRINT_WINDOW &&
              atr_footprint::kMaxK == ATR_FOOTPRINT_MAX_K && atr_footprint::kValue == ATR_FOOTPRINT_VALUE &&
              atr_footprint::kPeek == ATR_FOOTPRINT_PEEK && atr_footprint::kStep == ATR_FOOTPRINT_STEP &&
              atr_footprint::kBegin == ATR_FOOTPRINT_BEGIN && ATR_FOOTPRINT_MAX_K + 1 <= 64,
              "atr_footprint_rule.h and include/atr_footprints.h state one rule, and a row fits one wavefront");

namespace atr_footprint {

constexpr int kFpWaves = 4;                                          // (env, player) pairs per workgroup (one wave each)
constexpr int kFpBlock = 64 * kFpWaves;
constexpr int kArrPos = 1;                                           // row of t2d::kStateArray
static_assert(t2d::kStateArray[kArrPos].words == 1 && t2d::kStateArray[kArrPos].planes == 1, "pos sits where this file reads it");

struct FpArgs {
    void *obs;
    long long se, sp;
    unsigned short *trail;
    const uint32_t *pos;                 // the handle's [N] positions (r0 | c0 << 8 | r1 << 16 | c1 << 24)
    const unsigned char *done;
    int n, k, roles, mode, value;
};

template <typename ObsT>
__global__ __launch_bounds__(kFpBlock) void k_footprints(FpArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long w = (long long)blockIdx.x * kFpWaves + wave;
    if (w >= 2ll * a.n) return;        // (wave-uniform)
    const long long e = w >> 1;
    const int p = (int)(w & 1);
    const uint32_t pos = a.pos[e];
    const int cur = cell_of(pos, p), viewer = cell_of(pos, 1 - p);
    // the record: the whole row is loaded before any of it is stored
    unsigned short *row = a.trail + (e * 2 + p) * (long long)(a.k + 1);
    const int own = lane <= a.k ? (int)row[lane] : kEmpty;
    const int prev = __shfl_up(own, 1);
    const int s0 = __builtin_amdgcn_readfirstlane(own);
    const int kind = record_kind(a.mode, a.done != nullptr, a.done ? (int)a.done[e] : 0, cur, s0);
    const int now = record_entry(kind, lane, cur, own, prev);
    if (lane <= a.k && now != own) row[lane] = (unsigned short)now;
    // the paint: this player's prints into the other player's window
    if (((a.roles >> (1 - p)) & 1) == 0) return;       // (wave-uniform)
    if (lane >= 1 && lane <= a.k) {
        const int cell = paint_cell(now, viewer);
        if (cell >= 0) {
            ObsT *win = (ObsT *)a.obs + e * a.se + (long long)(1 - p) * a.sp;
            if (win[cell] == (ObsT)0) win[cell] = (ObsT)a.value;
        }
    }
}

// (as csrc/fov_hip.hip: the refusals put their text into the calling thread's t2d_last_error() buffer)
static int fp_refuse(int code, const char *fmt, ...)
{
    char *buf = const_cast<char *>(t2d_last_error());
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, 256, fmt, ap);
    va_end(ap);
    return code;
}

struct FpDeviceScope {
    int prev = -1;
    bool changed = false;
    explicit FpDeviceScope(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = (hipSetDevice(dev) == hipSuccess);
    }
    ~FpDeviceScope()
    {
        if (changed) (void)hipSetDevice(prev);
    }
};

}  // namespace atr_footprint

using namespace atr_footprint;

extern "C" int atr_footprint_windows(t2d_handle *h, void *obs, int is_u8, long long se, long long sp, unsigned short *trail, int k,
                                     int roles, int mode, const unsigned char *done, int value, void *stream)
{
    if (!obs || !trail)
        return fp_refuse(T2D_ERR_INVALID, "atr_footprint_windows: null pointer (obs %p trail %p)", obs, (void *)trail);
    if (k < 1 || k > ATR_FOOTPRINT_MAX_K) return fp_refuse(T2D_ERR_INVALID, "atr_footprint_windows: k %d outside 1 .. 63", k);
    if (roles < 1 || roles > 3) return fp_refuse(T2D_ERR_INVALID, "atr_footprint_windows: roles %d outside 1 .. 3", roles);
    if (mode < ATR_FOOTPRINT_PEEK || mode > ATR_FOOTPRINT_BEGIN)
        return fp_refuse(T2D_ERR_INVALID, "atr_footprint_windows: mode %d outside 0 .. 2", mode);
    if (value < 0 || value > 255) return fp_refuse(T2D_ERR_INVALID, "atr_footprint_windows: value %d outside 0 .. 255", value);
    if (se < 0 || sp < 0)
        return fp_refuse(T2D_ERR_INVALID, "atr_footprint_windows: negative element stride (se %lld, sp %lld)", se, sp);
    if (!is_u8 && ((uintptr_t)obs & 3u))
        return fp_refuse(T2D_ERR_INVALID, "atr_footprint_windows: float32 windows not 4-byte aligned (obs %p)", obs);
    if ((uintptr_t)trail & 1u)
        return fp_refuse(T2D_ERR_INVALID, "atr_footprint_windows: trail %p is not 2-byte aligned", (void *)trail);
    if (!h) return fp_refuse(T2D_ERR_INVALID, "atr_footprint_windows: null handle");
    t2d_state_view v;
    const int rc = t2d_state_view_get(h, &v);
    if (rc) return rc;
    if (!v.ready) return fp_refuse(T2D_ERR_INVALID, "atr_footprint_windows: call t2d_reset (all envs) first");
    if (v.obs_full)
        return fp_refuse(T2D_ERR_INVALID, "atr_footprint_windows: the handle observes the whole map (the rule is stated for the "
                                          "13 x 13 windows of 'Partial' observations)");
    FpDeviceScope guard(v.device);
    FpArgs a;
    a.obs = obs, a.se = se, a.sp = sp;
    a.trail = trail;
    a.pos = v.arr[kArrPos];
    a.done = done;
    a.n = v.n, a.k = k, a.roles = roles, a.mode = mode, a.value = value;
    const dim3 grid((unsigned)((2ll * v.n + kFpWaves - 1) / kFpWaves)), block(kFpBlock);
    if (is_u8)
        hipLaunchKernelGGL((k_footprints<uint8_t>), grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((k_footprints<float>), grid, block, 0, (hipStream_t)stream, a);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : fp_refuse(T2D_ERR_HIP, "atr_footprint_windows: launch failed: %s", hipGetErrorString(err));
}
