// render_hip.hip — episode traces and the device renderer (include/track2d_trace.h) of the batched Track2D environment.
//
//   k_trace_begin / k_trace_append   one thread per env, one 8-byte slot (both agents' cells) per env and step;
//   k_render_cells                   one 256-thread workgroup per frame: the painted 82 x 82 cell image + the tracker's window;
//   k_render_rgb                     one workgroup per (frame, band of kBandRows cell rows): the same cells, coloured, streamed
//                                    out as whole 16-byte vectors along the pixel rows.
// Both render kernels stage the env's 1 KiB map tile in LDS, scatter the trace (<= capacity entries) into an 82-row bit mask
// in LDS with atomic-or and then ask ONE device function, painted_cell(), for every cell: the RGB frame cannot disagree
// with the cells the tests pin. Reference: G/envs/track_1v1.py:170-216 (render), :295-326 (the two observations).
//
// The handle (csrc/track2d_hip.hip) is reached through t2d_trace_view_get alone; the step kernels know nothing of this file.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <new>

#include "../../include/track2d_trace.h"
#include "t2d_device.h"
#include "t2d_trace_view.h"

namespace t2d {

constexpr int kSide = T2D_MAX_SIDE;                  // 82
constexpr int kCanvasW = T2D_RENDER_CELLS_W;         // 162 canvas cells
constexpr int kGap = 2, kWinZoom = 6;                // window panel: canvas cells [84, 162), 6 per window cell
constexpr int kWinX0 = kSide + kGap, kWinRows = T2D_WIN * kWinZoom;   // 84, 78
constexpr int kBandRows = 2;                         // cell rows per k_render_rgb workgroup
constexpr int kRenderThreads = 256;
// cmap(norm(v)) of the reference's ListedColormap / BoundaryNorm (track_1v1.py:66-68) for the values that occur, as
// r | g << 8 | b << 16: the record in tests/golden/traces.npz ('palette') is the authority, the tests compare against it
constexpr uint32_t kRgbFree = 0xffffffu, kRgbWall = 0x000000u, kRgbTracker = 0xff0000u, kRgbTarget = 0x0000ffu,
                   kRgbTrace = 0x00ffffu, kRgbBackground = 0x808080u;

struct TraceStore {
    int16_t *pos;        // [N][cap + 1][2][2]
    int32_t *len;        // [N]
    uint8_t *closed;     // [N]
    uint32_t *dropped;   // [N]
    int cap, n, device;
};

struct RenderArgs {
    const uint32_t *maps, *pos, *cnt;
    uint32_t *faults;
    const int16_t *tpos;
    const int32_t *tlen;
    const int32_t *ids;
    int n, cap, flags;
};

// one slot = both agents' cells = four i16 = one 8-byte store
__device__ __forceinline__ void slot_write(int16_t *tpos, int cap, int e, int k, uint32_t p)
{
    const uint32_t lo = (p & 0xffu) | (((p >> 8) & 0xffu) << 16), hi = ((p >> 16) & 0xffu) | ((p >> 24) << 16);
    reinterpret_cast<uint2 *>(tpos)[(size_t)e * (size_t)(cap + 1) + (size_t)k] = make_uint2(lo, hi);
}

__global__ __launch_bounds__(256) void k_trace_begin(const uint32_t *__restrict__ pos, const uint8_t *__restrict__ mask, int16_t *tpos,
                                                     int32_t *tlen, uint8_t *closed, uint32_t *dropped, int cap, int n)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n || (mask != nullptr && mask[e] == 0)) return;
    slot_write(tpos, cap, e, 0, pos[e]);
    tlen[e] = 1;
    closed[e] = 0;
    dropped[e] = 0u;
}

__global__ __launch_bounds__(256) void k_trace_append(const uint32_t *__restrict__ pos, const uint8_t *__restrict__ done, int16_t *tpos,
                                                      int32_t *tlen, uint8_t *closed, uint32_t *dropped, int cap, int n)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n || closed[e] != 0) return;
    const int l = tlen[e];
    if (l >= 1 && l <= cap) {            // (l == 0: never begun — nothing to append to)
        slot_write(tpos, cap, e, l, pos[e]);
        tlen[e] = l + 1;
    } else if (l > cap) {
        dropped[e] += 1u;
    }
    if (done[e] != 0) closed[e] = 1;
}

// ---- the frame: what every thread of a render workgroup knows about its env ------------------------------------------
struct Frame {
    int env, side, tr, tc, gr, gc, len;
    bool paint;
};

// Stage the env's tile and the trace bit mask in LDS (whole workgroup; ends with a barrier).
// traces[:-1] = the tracker's spawn (slot 0) and the target's cell of slots 1 .. len - 2 (track_1v1.py:120,163,182).
__device__ __forceinline__ Frame frame_setup(const RenderArgs &a, int frame, uint32_t *tile, uint32_t *tbits)
{
    const int tid = threadIdx.x;
    int id = a.ids[frame];
    if (id < 0 || id >= a.n) {
        if (tid == 0) atomicOr(a.faults, T2D_FAULT_RENDER_ID);
        id = id < 0 ? 0 : a.n - 1;
    }
    Frame f;
    f.env = id;
    const uint32_t p = a.pos[id];
    f.side = min((int)(a.cnt[id] >> 24), kSide);      // 0 before the env's first episode: every cell is then outside
    f.tr = (int)(p & 0xffu); f.tc = (int)((p >> 8) & 0xffu); f.gr = (int)((p >> 16) & 0xffu); f.gc = (int)(p >> 24);
    f.paint = (a.flags & T2D_RENDER_TRACE) != 0;
    f.len = f.paint ? min(a.tlen[id], a.cap + 1) : 0;
    if (tid < 64) reinterpret_cast<uint4 *>(tile)[tid] = reinterpret_cast<const uint4 *>(a.maps + (size_t)id * kTileWords)[tid];
    tbits[tid] = 0u;                                   // kRenderThreads == kTileWords words
    __syncthreads();
    const int16_t *tp = a.tpos + (size_t)id * (size_t)(a.cap + 1) * 4;
    for (int k = tid; k < f.len - 1; k += kRenderThreads) {
        const int o = k * 4 + (k == 0 ? 0 : 2);
        const int r = tp[o], c = tp[o + 1];
        if ((unsigned)r < (unsigned)f.side && (unsigned)c < (unsigned)f.side)
            atomicOr(&tbits[r * kRowWords + (c >> 5)], 1u << (c & 31));
    }
    __syncthreads();
    return f;
}

// render()'s painted full observation at (r, c), r, c in [0, 82): map, then 2, then 4, then 6 (track_1v1.py:177-182,295-307)
__device__ __forceinline__ uint32_t painted_cell(const Frame &f, const uint32_t *tile, const uint32_t *tbits, int r, int c)
{
    if (r >= f.side || c >= f.side) return T2D_RENDER_OUTSIDE;
    uint32_t v = tile_bit(tile, r, c);
    if (r == f.tr && c == f.tc) v = 2u;
    if (r == f.gr && c == f.gc) v = 4u;
    if (f.paint && tile_bit(tbits, r, c)) v = 6u;
    return v;
}

// _get_partial_obs(0, 6) at window cell (i, j) (track_1v1.py:309-326): the full observation with the tracker's own cell
// re-painted 2 (it wins there even when co-located), padded with walls; never painted 6
__device__ __forceinline__ uint32_t window_cell(const Frame &f, const uint32_t *tile, int i, int j)
{
    const int r = f.tr - T2D_POB + i, c = f.tc - T2D_POB + j;
    if (i == T2D_POB && j == T2D_POB) return 2u;
    if (r < 0 || c < 0 || r >= f.side || c >= f.side) return 1u;
    if (r == f.gr && c == f.gc) return 4u;
    return tile_bit(tile, r, c);
}

__device__ __forceinline__ uint32_t cell_rgb(uint32_t v)
{
    return v == 0u ? kRgbFree : v == 1u ? kRgbWall : v == 2u ? kRgbTracker : v == 4u ? kRgbTarget : v == 6u ? kRgbTrace : kRgbBackground;
}

__global__ __launch_bounds__(kRenderThreads) void k_render_cells(RenderArgs a, uint8_t *cells, uint8_t *partial)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[kTileWords];
    __shared__ uint32_t tbits[kTileWords];
    const int frame = blockIdx.x, tid = threadIdx.x;
    const Frame f = frame_setup(a, frame, tile, tbits);
    if (cells != nullptr) {
        uint32_t *out = reinterpret_cast<uint32_t *>(cells + (size_t)frame * (kSide * kSide));   // 6724 = 4 * 1681 bytes per frame
        for (int w = tid; w < kSide * kSide / 4; w += kRenderThreads) {
            uint32_t word = 0u;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int i = 4 * w + j, r = i / kSide, c = i - r * kSide;
                word |= painted_cell(f, tile, tbits, r, c) << (8 * j);
            }
            out[w] = word;
        }
    }
    if (partial != nullptr && tid < T2D_WIN * T2D_WIN)
        partial[(size_t)frame * (T2D_WIN * T2D_WIN) + tid] = (uint8_t)window_cell(f, tile, tid / T2D_WIN, tid % T2D_WIN);
}

// grid (bands, frames). Per band: the colour of each of the 162 canvas cells of its kBandRows cell rows goes to LDS; a thread
// then builds each of its 16-byte vectors of a pixel row ONCE (all `scale` pixel rows of a cell row are the same bytes) and
// stores it `scale` times. A wave's 64 lanes write 1 KiB of consecutive bytes of one row.
__global__ __launch_bounds__(kRenderThreads) void k_render_rgb(RenderArgs a, uint8_t *rgb, int scale, int pitch)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[kTileWords];
    __shared__ uint32_t tbits[kTileWords];
    __shared__ uint32_t crow[kBandRows][kCanvasW];
    const int frame = blockIdx.y, tid = threadIdx.x, row0 = blockIdx.x * kBandRows;
    const Frame f = frame_setup(a, frame, tile, tbits);
    for (int i = tid; i < kBandRows * kCanvasW; i += kRenderThreads) {
        const int b = i / kCanvasW, x = i - b * kCanvasW, cy = row0 + b;
        uint32_t v = T2D_RENDER_OUTSIDE;
        if (cy < kSide) {
            if (x < kSide) v = painted_cell(f, tile, tbits, cy, x);
            else if (x >= kWinX0 && cy < kWinRows) v = window_cell(f, tile, cy / kWinZoom, (x - kWinX0) / kWinZoom);
        }
        crow[b][x] = cell_rgb(v);
    }
    __syncthreads();
    const int nvec = pitch >> 4, valid = 3 * kCanvasW * scale;     // bytes of a row that belong to pixels
    const size_t frame_base = (size_t)frame * (size_t)(kSide * scale) * (size_t)pitch;
    for (int b = 0; b < kBandRows; b++) {
        const int cy = row0 + b;
        if (cy >= kSide) break;
        for (int v = tid; v < nvec; v += kRenderThreads) {
            const int byte0 = v * 16;
            int px = byte0 / 3, ch = byte0 - 3 * px;               // pixel and channel of the vector's first byte
            int cx = px / scale, sub = px - cx * scale;            // canvas cell of that pixel and the pixel's place in it
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

// t2d_last_error() hands out the calling thread's message buffer of the library (csrc/track2d_hip.hip: 512 chars)
static int refuse(int code, const char *fmt, ...)
{
    char *buf = const_cast<char *>(t2d_last_error());
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, 256, fmt, ap);
    va_end(ap);
    return code;
}

#define TRACE_HIP_TRY(expr)                                                                                \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess) return refuse(T2D_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));   \
    } while (0)

struct DeviceScope {
    int prev = -1;
    bool changed = false;
    explicit DeviceScope(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceScope()
    {
        if (changed) (void)hipSetDevice(prev);
    }
};

static void store_free(void *p)
{
    TraceStore *s = static_cast<TraceStore *>(p);
    if (!s) return;
    for (void *d : {(void *)s->pos, (void *)s->len, (void *)s->closed, (void *)s->dropped})
        if (d) (void)hipFree(d);
    delete s;
}

// the handle's view and its store, or a refusal
static int open_store(t2d_handle *h, const char *who, t2d_trace_view &v, TraceStore *&s)
{
    if (!h) return refuse(T2D_ERR_INVALID, "%s: null handle", who);
    int rc = t2d_trace_view_get(h, &v);
    if (rc) return rc;
    s = static_cast<TraceStore *>(*v.store);
    if (!s) return refuse(T2D_ERR_STATE, "%s: the handle has no trace store (call t2d_trace_attach first)", who);
    return T2D_OK;
}

static int launched(const char *who)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? T2D_OK : refuse(T2D_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
}

static RenderArgs render_args(const t2d_trace_view &v, const TraceStore *s, const int32_t *ids, int flags)
{
    RenderArgs a;
    a.maps = v.maps; a.pos = v.pos; a.cnt = v.cnt; a.faults = v.faults;
    a.tpos = s->pos; a.tlen = s->len; a.ids = ids;
    a.n = v.n; a.cap = s->cap; a.flags = flags;
    return a;
}

}  // namespace t2d

using namespace t2d;

extern "C" int t2d_trace_attach(t2d_handle *h, int capacity, void *stream)
{
    if (!h) return refuse(T2D_ERR_INVALID, "t2d_trace_attach: null handle");
    t2d_trace_view v;
    int rc = t2d_trace_view_get(h, &v);
    if (rc) return rc;
    if (v.auto_reset)
        return refuse(T2D_ERR_STATE, "t2d_trace_attach: the handle restarts finished envs inside the step launch (auto_reset = 1), "
                                     "so an episode's last cell cannot be recorded: create it with auto_reset = 0");
    if (capacity < 1 || capacity > 65535) return refuse(T2D_ERR_INVALID, "t2d_trace_attach: capacity %d outside [1, 65535]", capacity);
    DeviceScope guard(v.device);
    hipStream_t st = (hipStream_t)stream;
    TRACE_HIP_TRY(hipStreamSynchronize(st));          // a launch that reads the store being replaced may still be in flight
    TraceStore *s = new (std::nothrow) TraceStore();
    if (!s) return refuse(T2D_ERR_INVALID, "t2d_trace_attach: out of host memory");
    s->pos = nullptr; s->len = nullptr; s->closed = nullptr; s->dropped = nullptr;
    s->cap = capacity; s->n = v.n; s->device = v.device;
    const size_t n = (size_t)v.n, pb = n * (size_t)(capacity + 1) * 4 * sizeof(int16_t);
    hipError_t err = hipMalloc((void **)&s->pos, pb);
    if (err == hipSuccess) err = hipMalloc((void **)&s->len, n * sizeof(int32_t));
    if (err == hipSuccess) err = hipMalloc((void **)&s->closed, n);
    if (err == hipSuccess) err = hipMalloc((void **)&s->dropped, n * sizeof(uint32_t));
    if (err == hipSuccess) err = hipMemsetAsync(s->pos, 0, pb, st);
    if (err == hipSuccess) err = hipMemsetAsync(s->len, 0, n * sizeof(int32_t), st);
    if (err == hipSuccess) err = hipMemsetAsync(s->closed, 1, n, st);       // closed until a begin names the env
    if (err == hipSuccess) err = hipMemsetAsync(s->dropped, 0, n * sizeof(uint32_t), st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err != hipSuccess) {
        store_free(s);
        return refuse(T2D_ERR_HIP, "t2d_trace_attach: device allocation failed: %s", hipGetErrorString(err));
    }
    if (*v.store) (*v.store_free)(*v.store);
    *v.store = s;
    *v.store_free = store_free;
    return T2D_OK;
}

extern "C" int t2d_trace_begin(t2d_handle *h, const uint8_t *mask_dev_or_null, void *stream)
{
    t2d_trace_view v;
    TraceStore *s = nullptr;
    int rc = open_store(h, "t2d_trace_begin", v, s);
    if (rc) return rc;
    DeviceScope guard(v.device);
    hipLaunchKernelGGL(k_trace_begin, dim3((unsigned)((v.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v.pos, mask_dev_or_null,
                       s->pos, s->len, s->closed, s->dropped, s->cap, v.n);
    return launched("t2d_trace_begin");
}

extern "C" int t2d_trace_append(t2d_handle *h, const uint8_t *done_dev, void *stream)
{
    t2d_trace_view v;
    TraceStore *s = nullptr;
    int rc = open_store(h, "t2d_trace_append", v, s);
    if (rc) return rc;
    if (!done_dev) return refuse(T2D_ERR_INVALID, "t2d_trace_append: null done buffer");
    DeviceScope guard(v.device);
    hipLaunchKernelGGL(k_trace_append, dim3((unsigned)((v.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v.pos, done_dev, s->pos,
                       s->len, s->closed, s->dropped, s->cap, v.n);
    return launched("t2d_trace_append");
}

extern "C" int t2d_trace_get(t2d_handle *h, int first, int count, int16_t *pos_host, int32_t *len_host, uint32_t *dropped_host,
                             void *stream)
{
    t2d_trace_view v;
    TraceStore *s = nullptr;
    int rc = open_store(h, "t2d_trace_get", v, s);
    if (rc) return rc;
    if (first < 0 || count < 0 || first > v.n || count > v.n - first)
        return refuse(T2D_ERR_INVALID, "t2d_trace_get: env range [%d, %d + %d) outside [0, %d)", first, first, count, v.n);
    if (count == 0) return T2D_OK;
    DeviceScope guard(v.device);
    hipStream_t st = (hipStream_t)stream;
    const size_t slot = (size_t)(s->cap + 1) * 4;
    if (pos_host)
        TRACE_HIP_TRY(hipMemcpyAsync(pos_host, s->pos + (size_t)first * slot, (size_t)count * slot * sizeof(int16_t), hipMemcpyDeviceToHost, st));
    if (len_host) TRACE_HIP_TRY(hipMemcpyAsync(len_host, s->len + first, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (dropped_host)
        TRACE_HIP_TRY(hipMemcpyAsync(dropped_host, s->dropped + first, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    TRACE_HIP_TRY(hipStreamSynchronize(st));
    return T2D_OK;
}

extern "C" int t2d_render_cells(t2d_handle *h, const int32_t *env_ids_dev, int count, int flags, uint8_t *cells_dev,
                                uint8_t *partial_dev, void *stream)
{
    t2d_trace_view v;
    TraceStore *s = nullptr;
    int rc = open_store(h, "t2d_render_cells", v, s);
    if (rc) return rc;
    if (count <= 0 || count > 65535) return refuse(T2D_ERR_INVALID, "t2d_render_cells: count %d outside [1, 65535]", count);
    if (!env_ids_dev || (!cells_dev && !partial_dev)) return refuse(T2D_ERR_INVALID, "t2d_render_cells: null buffer");
    if (((uintptr_t)cells_dev & 3u) != 0u) return refuse(T2D_ERR_INVALID, "t2d_render_cells: cells buffer %p is not 4-byte aligned", (void *)cells_dev);
    DeviceScope guard(v.device);
    hipLaunchKernelGGL(k_render_cells, dim3((unsigned)count), dim3(kRenderThreads), 0, (hipStream_t)stream,
                       render_args(v, s, env_ids_dev, flags), cells_dev, partial_dev);
    return launched("t2d_render_cells");
}

extern "C" int t2d_render_rgb(t2d_handle *h, const int32_t *env_ids_dev, int count, int scale, int flags, uint8_t *rgb_dev,
                              int pitch_bytes, void *stream)
{
    t2d_trace_view v;
    TraceStore *s = nullptr;
    int rc = open_store(h, "t2d_render_rgb", v, s);
    if (rc) return rc;
    if (scale < 1 || scale > T2D_RENDER_MAX_SCALE)
        return refuse(T2D_ERR_INVALID, "t2d_render_rgb: scale %d outside [1, %d]", scale, T2D_RENDER_MAX_SCALE);
    if (pitch_bytes < 3 * kCanvasW * scale || (pitch_bytes & 15) != 0)
        return refuse(T2D_ERR_INVALID, "t2d_render_rgb: pitch %d must be a multiple of 16 and at least %d (486 x scale)", pitch_bytes,
                      3 * kCanvasW * scale);
    if (count <= 0 || count > 65535) return refuse(T2D_ERR_INVALID, "t2d_render_rgb: count %d outside [1, 65535]", count);
    if (!env_ids_dev || !rgb_dev) return refuse(T2D_ERR_INVALID, "t2d_render_rgb: null buffer");
    if (((uintptr_t)rgb_dev & 15u) != 0u) return refuse(T2D_ERR_INVALID, "t2d_render_rgb: frame buffer %p is not 16-byte aligned", (void *)rgb_dev);
    DeviceScope guard(v.device);
    hipLaunchKernelGGL(k_render_rgb, dim3((unsigned)((kSide + kBandRows - 1) / kBandRows), (unsigned)count), dim3(kRenderThreads), 0,
                       (hipStream_t)stream, render_args(v, s, env_ids_dev, flags), rgb_dev, scale, pitch_bytes);
    return launched("t2d_render_rgb");
}
