// view_hip.hip — the player views (include/atr_view.h; the rule's arithmetic: atr_view_rule.h): the 13 x 13 windows the players
// were handed, drawn as given, and one player's window projected back onto the map.
//
//   k_view_cells   one 256-thread workgroup per frame: the map panel's 82 x 82 codes and / or both windows' 2 x 169 codes;
//   k_view_rgb     one workgroup per (frame, band of kBandRows cell rows): the same codes, coloured, streamed out as whole
//                  16-byte vectors along the pixel rows (the structure of csrc/render_hip.hip's k_render_rgb).
// Both stage in LDS the env's 1 KiB map tile, the two windows as codes (338 bytes, loaded through the strides, floats converted
// by the exact-integer test) and the viewer's un-turned window (169 bytes, scattered through atr_ego::src_cell — a bijection, so
// no two lanes write one byte; the LDS stores are whole-byte stores). Then ONE device function, map_cell_code(), answers "code
// of map cell (r, c)" and ONE, atr_view::code_rgb(), "colour of a code" for both kernels: the RGB frame cannot disagree with
// the cells the tests pin.
//
// The handle (csrc/track2d_hip.hip) is reached through t2d_trace_view_get (the arrays and the fault word; it needs no trace
// store) and t2d_state_view_get (ready, obs_full); the step kernels know nothing of this file.
//
// Cost model: per frame 1 KiB + 338 window elements read; k_view_cells stores 6724 + 338 bytes, k_view_rgb 82 * scale rows of
// pitch bytes (238 KiB at scale 4): a launch plus a store stream, 242 / 162 of the renderer's bytes. DESIGN.md section 3
// "Player views".
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/atr_view.h"
#include "../../include/track2d_trace.h"
#include "atr_view_rule.h"
#include "t2d_device.h"
#include "t2d_state_view.h"
#include "t2d_trace_view.h"

static_assert(atr_view::kSide == T2D_MAX_SIDE && atr_view::kWin == T2D_WIN && atr_view::kPob == T2D_POB &&
              atr_view::kWindow == ATR_VIEW_WINDOW && atr_view::kUnknown == ATR_VIEW_UNKNOWN && atr_view::kOutside == ATR_VIEW_OUTSIDE &&
              atr_view::kHidden == ATR_VIEW_HIDDEN && atr_view::kBandHidden == ATR_VIEW_BAND_HIDDEN &&
              atr_view::kBandBeyond == ATR_VIEW_BAND_BEYOND && atr_view::kCanvasH == ATR_VIEW_CELLS_H &&
              atr_view::kCanvasW == ATR_VIEW_CELLS_W && atr_view::kWindow == atr_ego::kWindow,
              "atr_view_rule.h and include/atr_view.h state one rule");
static_assert(atr_view::kRgbFree == ATR_VIEW_RGB_FREE && atr_view::kRgbWall == ATR_VIEW_RGB_WALL &&
              atr_view::kRgbTracker == ATR_VIEW_RGB_TRACKER && atr_view::kRgbTarget == ATR_VIEW_RGB_TARGET &&
              atr_view::kRgbUnseen == ATR_VIEW_RGB_UNSEEN && atr_view::kRgbPrint == ATR_VIEW_RGB_PRINT &&
              atr_view::kRgbMemWall == ATR_VIEW_RGB_MEM_WALL && atr_view::kRgbMemFree == ATR_VIEW_RGB_MEM_FREE &&
              atr_view::kRgbUnknown == ATR_VIEW_RGB_UNKNOWN && atr_view::kRgbBackground == ATR_VIEW_RGB_BACKGROUND,
              "atr_view_rule.h and include/atr_view.h state one palette");

namespace atr_view {

constexpr int kBandRows = 2;                          // cell rows per k_view_rgb workgroup
constexpr int kViewThreads = 256;
constexpr int kCellsPerFrame = kSide * kSide;         // 6724 = 4 * 1681
static_assert(kCellsPerFrame % 4 == 0 && t2d::kTileWords == 4 * 64, "a frame's cells are whole words; 64 lanes stage the tile");

struct ViewArgs {
    const uint32_t *maps, *pos, *cnt;
    uint32_t *faults;
    const void *obs;
    long long se, sp;
    const uint8_t *facing;
    const int32_t *ids;
    int n, turned, viewer;
};

// what every thread of a view workgroup knows about its env
struct Frame {
    int side, tr, tc, gr, gc, pr, pc;
};

// Stage the env's tile, both windows as codes and the viewer's absolute window in LDS (whole workgroup; ends with a barrier).
template <typename ObsT>
__device__ __forceinline__ Frame frame_setup(const ViewArgs &a, int frame, uint32_t *tile, uint8_t *wcode, uint8_t *wabs)
{
    const int tid = threadIdx.x;
    int id = a.ids[frame];
    if (id < 0 || id >= a.n) {
        if (tid == 0) atomicOr(a.faults, T2D_FAULT_RENDER_ID);
        id = id < 0 ? 0 : a.n - 1;
    }
    Frame f;
    const uint32_t p = a.pos[id];
    f.side = min((int)(a.cnt[id] >> 24), kSide);
    f.tr = (int)(p & 0xffu); f.tc = (int)((p >> 8) & 0xffu); f.gr = (int)((p >> 16) & 0xffu); f.gc = (int)(p >> 24);
    f.pr = a.viewer ? f.gr : f.tr; f.pc = a.viewer ? f.gc : f.tc;
    if (tid < 64) reinterpret_cast<uint4 *>(tile)[tid] = reinterpret_cast<const uint4 *>(a.maps + (size_t)id * t2d::kTileWords)[tid];
    const bool turned = ((a.turned >> a.viewer) & 1) != 0;                 // (facing may be null when no window was turned)
    const int heading = turned ? atr_ego::heading_of((int)a.facing[(size_t)id * 2 + (size_t)a.viewer]) : 0;
    const ObsT *base = static_cast<const ObsT *>(a.obs) + (long long)id * a.se;
    for (int i = tid; i < 2 * kWindow; i += kViewThreads) {
        const int pl = i >= kWindow ? 1 : 0, cell = i - pl * kWindow;
        const int code = known(base[(long long)pl * a.sp + cell]);
        wcode[i] = (uint8_t)code;
        if (pl == a.viewer) wabs[unturn_cell(turned, heading, cell)] = (uint8_t)code;
    }
    __syncthreads();
    return f;
}

// the code of map cell (r, c), r, c in [0, 82)
__device__ __forceinline__ uint32_t map_cell_code(const Frame &f, const uint32_t *tile, const uint8_t *wabs, int r, int c)
{
    if (r >= f.side || c >= f.side) return (uint32_t)kOutside;
    const int t = truth((int)t2d::tile_bit(tile, r, c), r == f.tr && c == f.tc, r == f.gr && c == f.gc);
    const int dr = r - f.pr, dc = c - f.pc;
    const bool inside = in_window(dr, dc);
    return (uint32_t)map_code(t, inside, inside ? (int)wabs[window_index(dr, dc)] : 0);
}

template <typename ObsT>
__global__ __launch_bounds__(kViewThreads) void k_view_cells(ViewArgs a, uint8_t *cells, uint8_t *windows)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[t2d::kTileWords];
    __shared__ uint8_t wcode[2 * kWindow];
    __shared__ uint8_t wabs[kWindow];
    const int frame = blockIdx.x, tid = threadIdx.x;
    const Frame f = frame_setup<ObsT>(a, frame, tile, wcode, wabs);
    if (cells != nullptr) {
        uint32_t *out = reinterpret_cast<uint32_t *>(cells + (size_t)frame * kCellsPerFrame);
        for (int w = tid; w < kCellsPerFrame / 4; w += kViewThreads) {
            uint32_t word = 0u;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int i = 4 * w + j, r = i / kSide, c = i - r * kSide;
                word |= map_cell_code(f, tile, wabs, r, c) << (8 * j);
            }
            out[w] = word;
        }
    }
    if (windows != nullptr)
        for (int i = tid; i < 2 * kWindow; i += kViewThreads) windows[(size_t)frame * (2 * kWindow) + i] = wcode[i];
}

// grid (bands, frames). Per band: the colour of each of the 242 canvas cells of its kBandRows cell rows goes to LDS; a thread
// then builds each of its 16-byte vectors of a pixel row ONCE (all `scale` pixel rows of a cell row are the same bytes) and
// stores it `scale` times. A wave's 64 lanes write 1 KiB of consecutive bytes of one row.
template <typename ObsT>
__global__ __launch_bounds__(kViewThreads) void k_view_rgb(ViewArgs a, uint8_t *rgb, int scale, int pitch)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[t2d::kTileWords];
    __shared__ uint8_t wcode[2 * kWindow];
    __shared__ uint8_t wabs[kWindow];
    __shared__ uint32_t crow[kBandRows][kCanvasW];
    const int frame = blockIdx.y, tid = threadIdx.x, row0 = blockIdx.x * kBandRows;
    const Frame f = frame_setup<ObsT>(a, frame, tile, wcode, wabs);
    for (int i = tid; i < kBandRows * kCanvasW; i += kViewThreads) {
        const int b = i / kCanvasW, x = i - b * kCanvasW, cy = row0 + b;
        uint32_t v = (uint32_t)kOutside;
        if (cy < kCanvasH) {
            if (x < kSide) v = map_cell_code(f, tile, wabs, cy, x);
            else if (cy < kWinRows && x >= kWin0X0 && x < kWin0X0 + kWinRows) v = wcode[(cy / kZoom) * kWin + (x - kWin0X0) / kZoom];
            else if (cy < kWinRows && x >= kWin1X0) v = wcode[kWindow + (cy / kZoom) * kWin + (x - kWin1X0) / kZoom];
        }
        crow[b][x] = code_rgb((int)v);
    }
    __syncthreads();
    const int nvec = pitch >> 4, valid = 3 * kCanvasW * scale;     // bytes of a row that belong to pixels
    const size_t frame_base = (size_t)frame * (size_t)(kCanvasH * scale) * (size_t)pitch;
    for (int b = 0; b < kBandRows; b++) {
        const int cy = row0 + b;
        if (cy >= kCanvasH) break;
        for (int v = tid; v < nvec; v += kViewThreads) {
            const int byte0 = v * 16;
            int px = byte0 / 3, ch = byte0 - 3 * px;               // pixel and channel of the vector's first byte
            int cx = min(px / scale, kCanvasW - 1), sub = px - (px / scale) * scale;   // its canvas cell, the pixel's place in it
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 16; j++) {
                if (byte0 + j < valid) w[j >> 2] |= ((crow[b][cx] >> (8 * ch)) & 0xffu) << (8 * (j & 3));
                if (++ch == 3) {
                    ch = 0;
                    if (++sub == scale) { sub = 0; cx = min(cx + 1, kCanvasW - 1); }
                }
            }
            const uint4 q = make_uint4(w[0], w[1], w[2], w[3]);
            uint8_t *dst = rgb + frame_base + (size_t)(cy * scale) * (size_t)pitch + (size_t)byte0;
            for (int s = 0; s < scale; s++) *reinterpret_cast<uint4 *>(dst + (size_t)s * (size_t)pitch) = q;
        }
    }
}

// (as csrc/noise_hip.hip: the refusals put their text into the calling thread's t2d_last_error() buffer)
static int vw_refuse(int code, const char *fmt, ...)
{
    char *buf = const_cast<char *>(t2d_last_error());
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, 256, fmt, ap);
    va_end(ap);
    return code;
}

struct VwDeviceScope {
    int prev = -1;
    bool changed = false;
    explicit VwDeviceScope(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = (hipSetDevice(dev) == hipSuccess);
    }
    ~VwDeviceScope()
    {
        if (changed) (void)hipSetDevice(prev);
    }
};

// the refusals both entry points share, in the header's order: check_inputs, check_shape, then each entry point's own output
// checks, then open_handle; 0 = go on
static int check_inputs(const char *who, const void *obs, const int *env_ids, bool no_output)
{
    if (!obs) return vw_refuse(T2D_ERR_INVALID, "%s: null obs", who);
    if (!env_ids) return vw_refuse(T2D_ERR_INVALID, "%s: null env_ids", who);
    if (no_output) return vw_refuse(T2D_ERR_INVALID, "%s: null output buffer", who);
    return 0;
}

static int check_shape(const char *who, const void *obs, int is_u8, long long se, long long sp, const unsigned char *facing, int turned,
                       int count, int viewer)
{
    if (count < 1 || count > 65535) return vw_refuse(T2D_ERR_INVALID, "%s: count %d outside [1, 65535]", who, count);
    if (viewer < 0 || viewer > 1) return vw_refuse(T2D_ERR_INVALID, "%s: viewer %d outside 0 .. 1", who, viewer);
    if (turned < 0 || turned > 3) return vw_refuse(T2D_ERR_INVALID, "%s: turned %d outside 0 .. 3", who, turned);
    if (turned != 0 && !facing) return vw_refuse(T2D_ERR_INVALID, "%s: turned %d needs the facing bytes (null facing)", who, turned);
    if (se < 0 || sp < 0) return vw_refuse(T2D_ERR_INVALID, "%s: negative element stride (se %lld, sp %lld)", who, se, sp);
    if (!is_u8 && ((uintptr_t)obs & 3u)) return vw_refuse(T2D_ERR_INVALID, "%s: float32 windows not 4-byte aligned (obs %p)", who, obs);
    return 0;
}

// the handle's arrays, or a refusal from its state
static int open_handle(const char *who, t2d_handle *h, const void *obs, long long se, long long sp, const unsigned char *facing,
                       int turned, const int *env_ids, int viewer, ViewArgs &a, int &device)
{
    if (!h) return vw_refuse(T2D_ERR_INVALID, "%s: null handle", who);
    t2d_state_view sv;
    int rc = t2d_state_view_get(h, &sv);
    if (rc) return rc;
    if (!sv.ready) return vw_refuse(T2D_ERR_INVALID, "%s: call t2d_reset (all envs) first", who);
    if (sv.obs_full)
        return vw_refuse(T2D_ERR_INVALID, "%s: the handle observes the whole map (the rule is stated for the 13 x 13 windows of "
                                          "'Partial' observations)", who);
    t2d_trace_view tv;
    rc = t2d_trace_view_get(h, &tv);
    if (rc) return rc;
    a.maps = tv.maps; a.pos = tv.pos; a.cnt = tv.cnt; a.faults = tv.faults;
    a.obs = obs; a.se = se; a.sp = sp; a.facing = facing; a.ids = env_ids;
    a.n = tv.n; a.turned = turned; a.viewer = viewer;
    device = tv.device;
    return 0;
}

static int vw_launched(const char *who)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : vw_refuse(T2D_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
}

}  // namespace atr_view

using namespace atr_view;

extern "C" int atr_view_cells(t2d_handle *h, const void *obs, int is_u8, long long se, long long sp, const unsigned char *facing,
                              int turned, const int *env_ids, int count, int viewer, unsigned char *cells, unsigned char *windows,
                              void *stream)
{
    const char *who = "atr_view_cells";
    int rc = check_inputs(who, obs, env_ids, !cells && !windows);
    if (rc) return rc;
    rc = check_shape(who, obs, is_u8, se, sp, facing, turned, count, viewer);
    if (rc) return rc;
    if ((uintptr_t)cells & 3u) return vw_refuse(T2D_ERR_INVALID, "%s: cells buffer %p is not 4-byte aligned", who, (void *)cells);
    ViewArgs a;
    int device = 0;
    rc = open_handle(who, h, obs, se, sp, facing, turned, env_ids, viewer, a, device);
    if (rc) return rc;
    VwDeviceScope guard(device);
    const dim3 grid((unsigned)count), block(kViewThreads);
    if (is_u8)
        hipLaunchKernelGGL((k_view_cells<uint8_t>), grid, block, 0, (hipStream_t)stream, a, cells, windows);
    else
        hipLaunchKernelGGL((k_view_cells<float>), grid, block, 0, (hipStream_t)stream, a, cells, windows);
    return vw_launched(who);
}

extern "C" int atr_view_rgb(t2d_handle *h, const void *obs, int is_u8, long long se, long long sp, const unsigned char *facing,
                            int turned, const int *env_ids, int count, int viewer, int scale, unsigned char *rgb, int pitch_bytes,
                            void *stream)
{
    const char *who = "atr_view_rgb";
    int rc = check_inputs(who, obs, env_ids, !rgb);
    if (rc) return rc;
    rc = check_shape(who, obs, is_u8, se, sp, facing, turned, count, viewer);
    if (rc) return rc;
    if (scale < 1 || scale > ATR_VIEW_MAX_SCALE)
        return vw_refuse(T2D_ERR_INVALID, "%s: scale %d outside [1, %d]", who, scale, ATR_VIEW_MAX_SCALE);
    if (pitch_bytes < 3 * kCanvasW * scale || (pitch_bytes & 15) != 0)
        return vw_refuse(T2D_ERR_INVALID, "%s: pitch %d must be a multiple of 16 and at least %d (726 x scale)", who, pitch_bytes,
                         3 * kCanvasW * scale);
    if ((uintptr_t)rgb & 15u) return vw_refuse(T2D_ERR_INVALID, "%s: frame buffer %p is not 16-byte aligned", who, (void *)rgb);
    ViewArgs a;
    int device = 0;
    rc = open_handle(who, h, obs, se, sp, facing, turned, env_ids, viewer, a, device);
    if (rc) return rc;
    VwDeviceScope guard(device);
    const dim3 grid((unsigned)((kCanvasH + kBandRows - 1) / kBandRows), (unsigned)count), block(kViewThreads);
    if (is_u8)
        hipLaunchKernelGGL((k_view_rgb<uint8_t>), grid, block, 0, (hipStream_t)stream, a, rgb, scale, pitch_bytes);
    else
        hipLaunchKernelGGL((k_view_rgb<float>), grid, block, 0, (hipStream_t)stream, a, rgb, scale, pitch_bytes);
    return vw_launched(who);
}
