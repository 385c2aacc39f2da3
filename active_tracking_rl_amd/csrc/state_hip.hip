// state_hip.hip — env shard snapshots (include/track2d_state.h): a second set of a handle's state arrays, one kernel that
// moves the masked envs' rows between the two, and the host blob. Reaches the handle only through t2d_state_view.h.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "../../include/track2d_state.h"
#include "t2d_state_view.h"

namespace t2d {

constexpr int kCopyWaves = 4;        // 256-thread workgroups, one wavefront per env

struct StateCopyArgs {
    uint32_t *handle[kStateArrays];  // the handle's arrays (null: not allocated, on both sides)
    uint32_t *snap[kStateArrays];    // the snapshot's
    const uint8_t *mask;             // [N] or null
    int n, to_handle;                // to_handle != 0: snapshot -> handle (restore), else handle -> snapshot (save)
};

constexpr int word_lanes(int upto)   // lanes taken by the word-per-env arrays before array `upto`: one per (array, plane)
{
    int j = 0;
    for (int i = 0; i < upto; i++)
        if (kStateArray[i].words == 1) j += kStateArray[i].planes;
    return j;
}
static_assert(word_lanes(kStateArrays) <= 64, "one lane per word-per-env array and plane");

constexpr bool widths_ok()
{
    for (int i = 0; i < kStateArrays; i++)
        if (kStateArray[i].words != 1 && (kStateArray[i].words % 4 != 0 || (kStateArray[i].words > 256 && kStateArray[i].words % 256 != 0)))
            return false;
    return true;
}
static_assert(widths_ok(), "tiles and planes move as whole 16-byte pieces, a wave-wide row of them at a time");

// Array I of the table, env e. A word-per-env array: lane word_lanes(I) + k is given plane k's addresses (the move itself
// happens once, after every array has handed out its lanes). A tile or plane: W / 4 16-byte pieces, contiguous across the wave,
// all loads of a row issued before its stores.
template <int I>
__device__ __forceinline__ void move_array(const StateCopyArgs &p, int e, int lane, const uint32_t *&wsrc, uint32_t *&wdst)
{
    constexpr int W = kStateArray[I].words, K = kStateArray[I].planes;
    const uint32_t *src = p.to_handle ? p.snap[I] : p.handle[I];
    uint32_t *dst = p.to_handle ? p.handle[I] : p.snap[I];
    if (src == nullptr || dst == nullptr) return;      // (uniform: kernel arguments)
    if constexpr (W == 1) {
        constexpr int j0 = word_lanes(I);
#pragma unroll
        for (int k = 0; k < K; k++)
            if (lane == j0 + k) {
                wsrc = src + ((size_t)k * p.n + e);
                wdst = dst + ((size_t)k * p.n + e);
            }
    } else {
        constexpr int Q = W / 4;                       // 16-byte pieces per row
#pragma unroll
        for (int k = 0; k < K; k++) {
            const size_t row = ((size_t)k * p.n + e) * W;
            const uint4 *s4 = reinterpret_cast<const uint4 *>(src + row);
            uint4 *d4 = reinterpret_cast<uint4 *>(dst + row);
            if constexpr (Q >= 64) {
                static_assert(Q / 64 <= 3, "a row is at most three wave-wide pieces");
                uint4 v0 = s4[lane], v1, v2;            // (named registers: an indexed array went to scratch memory)
                if constexpr (Q / 64 > 1) v1 = s4[64 + lane];
                if constexpr (Q / 64 > 2) v2 = s4[128 + lane];
                d4[lane] = v0;
                if constexpr (Q / 64 > 1) d4[64 + lane] = v1;
                if constexpr (Q / 64 > 2) d4[128 + lane] = v2;
            } else if (lane < Q) {
                d4[lane] = s4[lane];
            }
        }
    }
}

template <int... I>
__device__ __forceinline__ void move_all(const StateCopyArgs &p, int e, int lane, const uint32_t *&wsrc, uint32_t *&wdst,
                                         std::integer_sequence<int, I...>)
{
    (move_array<I>(p, e, lane, wsrc, wdst), ...);
}

// One wavefront per env: every state array of the masked envs, handle -> snapshot or back, in one launch.
__global__ __launch_bounds__(64 * kCopyWaves) void k_state_copy(StateCopyArgs p)
{
    const int lane = (int)(threadIdx.x & 63u);
    const int e = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kCopyWaves + (threadIdx.x >> 6)));
    if (e >= p.n) return;
    if (p.mask != nullptr && p.mask[e] == 0) return;
    const uint32_t *wsrc = nullptr;
    uint32_t *wdst = nullptr;
    move_all(p, e, lane, wsrc, wdst, std::make_integer_sequence<int, kStateArrays>{});
    if (wsrc != nullptr) *wdst = *wsrc;
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

#define STATE_HIP_TRY(expr)                                                                                \
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

// the fields a blob is compared by (the blob header's, track2d_state.h)
struct SnapIdent {
    uint32_t n, env_base;
    uint64_t seed;
    int32_t max_steps, auto_reset;
    uint32_t obs_type, action_type;
    uint64_t cfg_hash;
    uint32_t sections;
};

static const char *first_difference(const SnapIdent &a, const SnapIdent &b)
{
    if (a.n != b.n) return "num_envs";
    if (a.env_base != b.env_base) return "env_id_base";
    if (a.seed != b.seed) return "seed";
    if (a.max_steps != b.max_steps) return "max_episode_steps";
    if (a.auto_reset != b.auto_reset) return "auto_reset";
    if (a.obs_type != b.obs_type) return "obs_type";
    if (a.action_type != b.action_type) return "action_type";
    if (a.cfg_hash != b.cfg_hash) return "cfg";
    if (a.sections != b.sections) return "sections";
    return nullptr;
}

static void put32(uint8_t *p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i)); }
static void put64(uint8_t *p, uint64_t v) { for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i)); }
static uint32_t get32(const uint8_t *p) { uint32_t v = 0; for (int i = 0; i < 4; i++) v |= (uint32_t)p[i] << (8 * i); return v; }
static uint64_t get64(const uint8_t *p) { uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i); return v; }

static const char kMagic[8] = {'T', '2', 'D', 'S', 'N', 'A', 'P', '\0'};

}  // namespace t2d

using namespace t2d;

struct t2d_snapshot {
    t2d_handle *owner;
    int device;
    SnapIdent id;
    uint32_t random_step;
    bool valid;                         // a full save or an import has filled every row
    bool prio;                          // the owner was a prioritised handle when the snapshot was created (refused from then on)
    uint32_t *arr[kStateArrays];
    long long payload;                  // bytes
};

static size_t array_bytes(int i, uint32_t n)
{
    return (size_t)kStateArray[i].planes * n * (size_t)kStateArray[i].words * sizeof(uint32_t);
}

// the handle's view, or the refusal every entry point shares
static int open_handle(t2d_handle *h, const char *who, t2d_state_view &v)
{
    if (!h) return refuse(T2D_ERR_INVALID, "%s: null handle", who);
    int rc = t2d_state_view_get(h, &v);
    if (rc) return rc;
    if (v.np_attached)
        return refuse(T2D_ERR_INVALID, "%s: the handle has numpy-legacy streams attached (t2d_np_attach): their state is not part "
                                       "of a snapshot", who);
    if (v.trace_attached)
        return refuse(T2D_ERR_INVALID, "%s: the handle has a trace store attached (t2d_trace_attach): the episode record is not "
                                       "part of a snapshot", who);
    return T2D_OK;
}

extern "C" int t2d_snapshot_destroy(t2d_snapshot *s)
{
    if (!s) return T2D_OK;
    DeviceScope guard(s->device);
    for (uint32_t *p : s->arr)
        if (p) (void)hipFree(p);
    delete s;
    return T2D_OK;
}

extern "C" int t2d_snapshot_create(t2d_handle *h, t2d_snapshot **out)
{
    if (!out) return refuse(T2D_ERR_INVALID, "t2d_snapshot_create: null argument");
    t2d_state_view v;
    int rc = open_handle(h, "t2d_snapshot_create", v);
    if (rc) return rc;
    DeviceScope guard(v.device);
    t2d_snapshot *s = new (std::nothrow) t2d_snapshot();
    if (!s) return refuse(T2D_ERR_INVALID, "t2d_snapshot_create: out of host memory");
    s->owner = h; s->device = v.device; s->random_step = 0; s->valid = false; s->payload = 0;
    s->prio = v.prio_enabled != 0;
    for (uint32_t *&p : s->arr) p = nullptr;
    s->id.n = (uint32_t)v.n; s->id.env_base = v.env_base; s->id.seed = (uint64_t)v.k0 | ((uint64_t)v.k1 << 32);
    s->id.max_steps = v.max_steps; s->id.auto_reset = v.auto_reset;
    s->id.obs_type = v.obs_full ? T2D_OBS_FULL : T2D_OBS_PARTIAL;
    s->id.action_type = v.amask == 7 ? T2D_ACTIONS_MOORE : T2D_ACTIONS_VONNEUMANN;
    s->id.sections = (v.arr[kStateCore] ? T2D_SNAPSHOT_SECTION_NAV : 0u) | (v.arr[kStateCore + kStateNav] ? T2D_SNAPSHOT_SECTION_RING : 0u);
    std::vector<uint32_t> cfg((size_t)v.n);
    hipError_t err = hipMemcpy(cfg.data(), v.cfg, cfg.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
    uint64_t hash = 0xcbf29ce484222325ull;          // FNV-1a 64 over the words' bytes in memory order
    for (uint32_t w : cfg)
        for (int b = 0; b < 4; b++) hash = (hash ^ ((w >> (8 * b)) & 0xffu)) * 0x100000001b3ull;
    s->id.cfg_hash = hash;
    for (int i = 0; i < kStateArrays && err == hipSuccess; i++) {
        if (!v.arr[i]) continue;
        err = hipMalloc((void **)&s->arr[i], array_bytes(i, s->id.n));
        s->payload += (long long)array_bytes(i, s->id.n);
    }
    if (err != hipSuccess) {
        t2d_snapshot_destroy(s);
        return refuse(T2D_ERR_HIP, "t2d_snapshot_create: device allocation failed: %s", hipGetErrorString(err));
    }
    *out = s;
    return T2D_OK;
}

// flush, then one k_state_copy launch
static int copy_state(t2d_handle *h, const t2d_state_view &v, const t2d_snapshot *s, const uint8_t *mask_dev, int to_handle,
                      hipStream_t st, const char *who)
{
    int rc = t2d_flush(h, (void *)st);
    if (rc) return rc;
    StateCopyArgs a;
    for (int i = 0; i < kStateArrays; i++) { a.handle[i] = v.arr[i]; a.snap[i] = s->arr[i]; }
    a.mask = mask_dev; a.n = v.n; a.to_handle = to_handle;
    hipLaunchKernelGGL(k_state_copy, dim3((unsigned)((v.n + kCopyWaves - 1) / kCopyWaves)), dim3(64 * kCopyWaves), 0, st, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? T2D_OK : refuse(T2D_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
}

static int open_pair(t2d_handle *h, const t2d_snapshot *s, const char *who, t2d_state_view &v)
{
    if (!s) return refuse(T2D_ERR_INVALID, "%s: null snapshot", who);
    int rc = open_handle(h, who, v);
    if (rc) return rc;
    if (s->owner != h) return refuse(T2D_ERR_INVALID, "%s: the snapshot was created for another handle", who);
    // prioritized map replay (include/track2d_bank_prio.h): an episode's bank index is what the table drew when the slot was
    // generated, kept in a ring beside the table and the accounts, none of which a snapshot holds
    if (v.prio_enabled)
        return refuse(T2D_ERR_STATE, "%s: the handle draws its maps from a priority table (t2d_bank_prio_enable): the index ring, "
                                     "the table and the accounts are not part of a snapshot, so the handle cannot be rewound", who);
    if (!v.ready) return refuse(T2D_ERR_STATE, "%s: call t2d_reset (all envs) first", who);
    return T2D_OK;
}

extern "C" int t2d_snapshot_save(t2d_handle *h, t2d_snapshot *s, const uint8_t *mask_dev, void *stream)
{
    t2d_state_view v;
    int rc = open_pair(h, s, "t2d_snapshot_save", v);
    if (rc) return rc;
    if (mask_dev != nullptr && !s->valid)
        return refuse(T2D_ERR_STATE, "t2d_snapshot_save: the first save into a snapshot must cover every env (mask == NULL)");
    DeviceScope guard(v.device);
    if ((rc = copy_state(h, v, s, mask_dev, 0, (hipStream_t)stream, "t2d_snapshot_save"))) return rc;
    if (mask_dev == nullptr) { s->random_step = *v.random_step; s->valid = true; }
    return T2D_OK;
}

extern "C" int t2d_snapshot_restore(t2d_handle *h, const t2d_snapshot *s, const uint8_t *mask_dev, void *stream)
{
    t2d_state_view v;
    int rc = open_pair(h, s, "t2d_snapshot_restore", v);
    if (rc) return rc;
    if (!s->valid) return refuse(T2D_ERR_STATE, "t2d_snapshot_restore: the snapshot holds nothing yet (save or import first)");
    DeviceScope guard(v.device);
    if ((rc = copy_state(h, v, s, mask_dev, 1, (hipStream_t)stream, "t2d_snapshot_restore"))) return rc;
    if (mask_dev == nullptr) *v.random_step = s->random_step;
    return T2D_OK;
}

extern "C" long long t2d_snapshot_bytes(const t2d_snapshot *s)
{
    return s ? (long long)T2D_SNAPSHOT_HEADER_BYTES + s->payload : (long long)T2D_ERR_INVALID;
}

extern "C" int t2d_snapshot_export(const t2d_snapshot *s, void *blob_host, long long bytes, void *stream)
{
    if (!s || !blob_host) return refuse(T2D_ERR_INVALID, "t2d_snapshot_export: null argument");
    if (bytes != t2d_snapshot_bytes(s))
        return refuse(T2D_ERR_INVALID, "t2d_snapshot_export: size %lld, the blob takes %lld bytes", bytes, t2d_snapshot_bytes(s));
    if (!s->valid) return refuse(T2D_ERR_STATE, "t2d_snapshot_export: the snapshot holds nothing yet (save or import first)");
    DeviceScope guard(s->device);
    hipStream_t st = (hipStream_t)stream;
    uint8_t *b = static_cast<uint8_t *>(blob_host);
    std::memset(b, 0, T2D_SNAPSHOT_HEADER_BYTES);
    std::memcpy(b, kMagic, 8);
    put32(b + 8, T2D_SNAPSHOT_VERSION); put32(b + 12, T2D_SNAPSHOT_HEADER_BYTES);
    put32(b + 16, s->id.n); put32(b + 20, s->id.env_base); put64(b + 24, s->id.seed);
    put32(b + 32, (uint32_t)s->id.max_steps); put32(b + 36, (uint32_t)s->id.auto_reset);
    put32(b + 40, s->id.obs_type); put32(b + 44, s->id.action_type); put64(b + 48, s->id.cfg_hash);
    put32(b + 56, s->id.sections); put32(b + 60, s->random_step); put64(b + 64, (uint64_t)s->payload);
    size_t off = T2D_SNAPSHOT_HEADER_BYTES;
    for (int i = 0; i < kStateArrays; i++) {
        if (!s->arr[i]) continue;
        STATE_HIP_TRY(hipMemcpyAsync(b + off, s->arr[i], array_bytes(i, s->id.n), hipMemcpyDeviceToHost, st));
        off += array_bytes(i, s->id.n);
    }
    STATE_HIP_TRY(hipStreamSynchronize(st));
    return T2D_OK;
}

extern "C" int t2d_snapshot_import(t2d_snapshot *s, const void *blob_host, long long bytes, void *stream)
{
    if (!s || !blob_host) return refuse(T2D_ERR_INVALID, "t2d_snapshot_import: null argument");
    if (s->prio)
        return refuse(T2D_ERR_STATE, "t2d_snapshot_import: the snapshot belongs to a handle that draws its maps from a priority table "
                                     "(t2d_bank_prio_enable): the index ring, the table and the accounts are not part of a snapshot");
    if (bytes < (long long)T2D_SNAPSHOT_HEADER_BYTES)
        return refuse(T2D_ERR_INVALID, "t2d_snapshot_import: size %lld is shorter than the %d-byte header", bytes, T2D_SNAPSHOT_HEADER_BYTES);
    const uint8_t *b = static_cast<const uint8_t *>(blob_host);
    if (std::memcmp(b, kMagic, 8) != 0) return refuse(T2D_ERR_INVALID, "t2d_snapshot_import: wrong magic (not a snapshot blob)");
    if (get32(b + 8) != T2D_SNAPSHOT_VERSION)
        return refuse(T2D_ERR_INVALID, "t2d_snapshot_import: format version %u, this library reads %d", get32(b + 8), T2D_SNAPSHOT_VERSION);
    if (get32(b + 12) != T2D_SNAPSHOT_HEADER_BYTES)
        return refuse(T2D_ERR_INVALID, "t2d_snapshot_import: header size %u, expected %d", get32(b + 12), T2D_SNAPSHOT_HEADER_BYTES);
    SnapIdent id;
    id.n = get32(b + 16); id.env_base = get32(b + 20); id.seed = get64(b + 24);
    id.max_steps = (int32_t)get32(b + 32); id.auto_reset = (int32_t)get32(b + 36);
    id.obs_type = get32(b + 40); id.action_type = get32(b + 44); id.cfg_hash = get64(b + 48); id.sections = get32(b + 56);
    if (const char *field = first_difference(id, s->id))
        return refuse(T2D_ERR_INVALID, "t2d_snapshot_import: the blob's %s differs from the handle's", field);
    if (get64(b + 64) != (uint64_t)s->payload || bytes != t2d_snapshot_bytes(s))
        return refuse(T2D_ERR_INVALID, "t2d_snapshot_import: size %lld with a payload field of %llu, the blob takes %lld bytes", bytes,
                      (unsigned long long)get64(b + 64), t2d_snapshot_bytes(s));
    DeviceScope guard(s->device);
    hipStream_t st = (hipStream_t)stream;
    s->valid = false;
    size_t off = T2D_SNAPSHOT_HEADER_BYTES;
    for (int i = 0; i < kStateArrays; i++) {
        if (!s->arr[i]) continue;
        STATE_HIP_TRY(hipMemcpyAsync(s->arr[i], b + off, array_bytes(i, s->id.n), hipMemcpyHostToDevice, st));
        off += array_bytes(i, s->id.n);
    }
    STATE_HIP_TRY(hipStreamSynchronize(st));
    s->random_step = get32(b + 60);
    s->valid = true;
    return T2D_OK;
}
