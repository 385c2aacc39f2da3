// memory_hip.hip — map memory: a hidden cell of a player's 13 x 13 window shows whether the map has a wall there, if the player
// has seen that cell in this episode (C ABI and the rule in full: include/atr_memory.h; the bit arithmetic itself:
// atr_memory_rule.h).
//
//   k_memory              one wavefront per (env e, player p), four per 256-thread workgroup (the shape of k_fov, csrc/fov_hip.hip).
//                         The wave owns window (e, p) and seen tile (e, p): no two waves ever share a byte they write. A wave whose
//                         player is not in `roles` returns at once. Lane l owns window cells l, l + 64, l + 128 and, of the tile,
//                         words 4 l .. 4 l + 3 as ONE 16-byte load and at most one 16-byte store: the whole KiB in one coalesced
//                         access, and every word of the tile has exactly one lane that may store it, the clear path included (a
//                         clearing wave's lanes take zero in place of the load and always store; the others store only where a
//                         word changed). Three ballots of `cell != hidden` give the 169-bit visible mask in scalar registers, so
//                         each lane cuts the window rows of its own four words out of it (row_slice) and places them (place_word)
//                         without a cross-lane move. To paint, the wave parks the updated tile and the 13 map rows of the window
//                         (39 consecutive words of maps[e], read only) in its own slot of LDS and every lane looks up the two
//                         bits of its hidden cells there: the paint never re-reads global memory this launch wrote (a
//                         wavefront-scope fence and a wave barrier between the LDS writes and reads, as in ego_hip.hip). The four
//                         waves of a workgroup share nothing: there is no workgroup barrier, and a wave that returns early leaves
//                         nobody waiting. A byte window's cells are stored by byte, so that no lane ever writes a byte of another
//                         window, whatever the window's alignment. No atomics.
//
// Whole tile or narrow access: the 13 rows a window can touch are 39 consecutive words, so a narrow form would move 156 B of the seen
// tile where this one moves 1 KiB. It would also need a second ownership of the tile's words for the clear (which has to reach all
// 246 of them), i.e. two storing lanes per word unless the two forms become separate wave-uniform paths. The map tile, which is only
// read, IS read narrow. For the seen tile the whole-tile form is kept: one path, one owner per word, 8 MB of 16-byte coalesced reads
// at 4096 envs x 2, far below what makes the launch anything but launch-bound (profiles/memory.txt).
//
// Cost model: per wave 169 cells + 1 KiB of seen tile + 156 B of map tile read; at most 1 KiB of tile and the painted cells written.
// 4 x (256 + 40) x 4 B = 4.6 KB of LDS per workgroup. DESIGN.md section 3 "Map memory".
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/atr_memory.h"
#include "atr_memory_rule.h"
#include "t2d_device.h"
#include "t2d_state_view.h"

static_assert(atr_memory::kSide == ATR_MEMORY_SIDE && atr_memory::kCentre == ATR_MEMORY_CENTRE &&
              atr_memory::kWindow == ATR_MEMORY_WINDOW && atr_memory::kHidden == ATR_MEMORY_HIDDEN &&
              atr_memory::kWall == ATR_MEMORY_WALL && atr_memory::kFree == ATR_MEMORY_FREE &&
              atr_memory::kKeep == ATR_MEMORY_KEEP && atr_memory::kStep == ATR_MEMORY_STEP &&
              atr_memory::kBegin == ATR_MEMORY_BEGIN && atr_memory::kMaxSide == ATR_MEMORY_MAX_SIDE,
              "atr_memory_rule.h and include/atr_memory.h state one rule");
static_assert(atr_memory::kTileWords == t2d::kTileWords && atr_memory::kRowWords == t2d::kRowWords &&
              ATR_MEMORY_TILE_WORDS == t2d::kTileWords && ATR_MEMORY_ROW_WORDS == t2d::kRowWords &&
              atr_memory::kMaxSide * atr_memory::kRowWords <= atr_memory::kTileWords && atr_memory::kTileWords == 64 * 4,
              "a seen tile has the layout of the handle's map tiles (t2d_device.h), and a wavefront holds it as one uint4 per lane");

namespace atr_memory {

constexpr int kMemWaves = 4;                                         // (env, player) pairs per workgroup (one wave each)
constexpr int kMemBlock = 64 * kMemWaves;
constexpr int kMapWords = kSide * kRowWords;                         // the 13 map rows under a window: 39 words
constexpr int kSlotWords = kTileWords + 40;                          // the seen tile, then the map rows (padded to 16 bytes)
constexpr int kArrMaps = 0, kArrPos = 1, kArrCnt = 3;                // rows of t2d::kStateArray
static_assert(t2d::kStateArray[kArrMaps].words == kTileWords && t2d::kStateArray[kArrPos].words == 1 &&
              t2d::kStateArray[kArrCnt].words == 1, "maps, pos and cnt sit where this file reads them");
static_assert(kMapWords <= 64 && kMapWords <= kSlotWords - kTileWords, "one lane per staged map word");

struct MemArgs {
    void *obs;
    long long se, sp;
    uint32_t *seen;
    const uint32_t *maps, *pos, *cnt;    // the handle's [N][256] tiles, [N] positions, [N] counters (side << 24)
    const unsigned char *done;
    int n, roles, mode, hidden, wall_value, free_value;
};

template <typename ObsT>
__global__ __launch_bounds__(kMemBlock) void k_memory(MemArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t stage[kMemWaves][kSlotWords];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long w = (long long)blockIdx.x * kMemWaves + wave;
    if (w >= 2ll * a.n) return;        // (wave-uniform)
    const long long e = w >> 1;
    const int p = (int)(w & 1);
    if (!((a.roles >> p) & 1)) return; // not this call's player: neither read nor written
    const uint32_t pos = a.pos[e];
    const int side = (int)(a.cnt[e] >> 24), pr = row_of(pos, p), pc = col_of(pos, p);
    // (every position of a live episode lies inside its square and a tile holds sides up to 82; anything else is not looked at)
    if (side < 1 || side > kMaxSide || pr >= side || pc >= side) return;
    ObsT *win = (ObsT *)a.obs + e * a.se + (long long)p * a.sp;
    const ObsT hidden = (ObsT)a.hidden;
    // the window: three cells per lane, and the wave's visible mask
    bool hid[3];
    uint64_t vis[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int c = 64 * i + lane;
        const bool in = c < kWindow;
        const ObsT v = in ? win[c] : hidden;
        hid[i] = in && v == hidden;
        vis[i] = __ballot(in && v != hidden);
    }
    // the tile: clear, record; lane l is the one owner of words 4 l .. 4 l + 3
    const bool clear = clears(a.mode, a.done != nullptr, a.done ? (int)a.done[e] : 0);       // (wave-uniform)
    uint4 *tile = reinterpret_cast<uint4 *>(a.seen + (e * 2 + p) * (long long)kTileWords);
    uint4 old = make_uint4(0u, 0u, 0u, 0u);
    if (!clear) old = tile[lane];
    uint32_t add[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int wd = 4 * lane + j, r = wd / kRowWords, k = wd - r * kRowWords, wr = r - (pr - kCentre);
        const bool on = wr >= 0 && wr < kSide && r < side;
        add[j] = on ? place_word(row_slice(vis[0], vis[1], vis[2], on ? wr : 0), pc, side, k) : 0u;
    }
    const uint4 now = make_uint4(old.x | add[0], old.y | add[1], old.z | add[2], old.w | add[3]);
    if (clear || now.x != old.x || now.y != old.y || now.z != old.z || now.w != old.w) tile[lane] = now;
    // the paint: the updated tile and the window's map rows go through the wave's own LDS slot
    uint32_t *slot = stage[wave];
    reinterpret_cast<uint4 *>(slot)[lane] = now;
    if (lane < kMapWords) {
        const int r = pr - kCentre + lane / kRowWords;
        slot[kTileWords + lane] = (r >= 0 && r < side) ? a.maps[e * kTileWords + r * kRowWords + lane % kRowWords] : 0u;
    }
    // (DS operations of one wave execute in order; this keeps the compiler from moving them and lets other lanes' words be read)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int c = 64 * i + lane;
        if (!hid[i]) continue;
        const int wr = c / kSide, wc = c - wr * kSide, r = pr - kCentre + wr, col = pc - kCentre + wc;
        const bool inside = r >= 0 && col >= 0 && r < side && col < side;
        if (!inside) continue;
        const uint32_t bit = 1u << (col & 31);
        const bool seen = (slot[r * kRowWords + (col >> 5)] & bit) != 0u;
        const bool wall = (slot[kTileWords + wr * kRowWords + (col >> 5)] & bit) != 0u;
        const int verdict = paint_verdict(true, true, seen, wall, a.wall_value, a.free_value);
        if (verdict != kLeave) win[c] = (ObsT)verdict;
    }
}

// (as csrc/fov_hip.hip: the refusals put their text into the calling thread's t2d_last_error() buffer)
static int mem_refuse(int code, const char *fmt, ...)
{
    char *buf = const_cast<char *>(t2d_last_error());
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, 256, fmt, ap);
    va_end(ap);
    return code;
}

struct MemDeviceScope {
    int prev = -1;
    bool changed = false;
    explicit MemDeviceScope(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = (hipSetDevice(dev) == hipSuccess);
    }
    ~MemDeviceScope()
    {
        if (changed) (void)hipSetDevice(prev);
    }
};

}  // namespace atr_memory

using namespace atr_memory;

extern "C" int atr_memory_windows(t2d_handle *h, void *obs, int is_u8, long long se, long long sp, unsigned int *seen, int roles,
                                  int mode, const unsigned char *done, int hidden, int wall_value, int free_value, void *stream)
{
    if (!obs || !seen) return mem_refuse(T2D_ERR_INVALID, "atr_memory_windows: null pointer (obs %p seen %p)", obs, (void *)seen);
    if (roles < 1 || roles > 3) return mem_refuse(T2D_ERR_INVALID, "atr_memory_windows: roles %d outside 1 .. 3", roles);
    if (mode < ATR_MEMORY_KEEP || mode > ATR_MEMORY_BEGIN)
        return mem_refuse(T2D_ERR_INVALID, "atr_memory_windows: mode %d outside 0 .. 2", mode);
    if (hidden < 0 || hidden > 255 || wall_value < 0 || wall_value > 255 || free_value < 0 || free_value > 255)
        return mem_refuse(T2D_ERR_INVALID, "atr_memory_windows: value outside 0 .. 255 (hidden %d, wall_value %d, free_value %d)",
                          hidden, wall_value, free_value);
    if (wall_value == hidden || free_value == hidden)
        return mem_refuse(T2D_ERR_INVALID, "atr_memory_windows: wall_value %d / free_value %d equal to hidden %d (a painted cell "
                                           "would read as unseen)", wall_value, free_value, hidden);
    if (se < 0 || sp < 0)
        return mem_refuse(T2D_ERR_INVALID, "atr_memory_windows: negative element stride (se %lld, sp %lld)", se, sp);
    if (!is_u8 && ((uintptr_t)obs & 3u))
        return mem_refuse(T2D_ERR_INVALID, "atr_memory_windows: float32 windows not 4-byte aligned (obs %p)", obs);
    if ((uintptr_t)seen & 15u)
        return mem_refuse(T2D_ERR_INVALID, "atr_memory_windows: seen %p is not 16-byte aligned", (void *)seen);
    if (!h) return mem_refuse(T2D_ERR_INVALID, "atr_memory_windows: null handle");
    t2d_state_view v;
    const int rc = t2d_state_view_get(h, &v);
    if (rc) return rc;
    if (!v.ready) return mem_refuse(T2D_ERR_INVALID, "atr_memory_windows: call t2d_reset (all envs) first");
    if (v.obs_full)
        return mem_refuse(T2D_ERR_INVALID, "atr_memory_windows: the handle observes the whole map (the rule is stated for the "
                                           "13 x 13 windows of 'Partial' observations)");
    MemDeviceScope guard(v.device);
    MemArgs a;
    a.obs = obs, a.se = se, a.sp = sp;
    a.seen = seen;
    a.maps = v.arr[kArrMaps], a.pos = v.arr[kArrPos], a.cnt = v.arr[kArrCnt];
    a.done = done;
    a.n = v.n, a.roles = roles, a.mode = mode, a.hidden = hidden, a.wall_value = wall_value, a.free_value = free_value;
    const dim3 grid((unsigned)((2ll * v.n + kMemWaves - 1) / kMemWaves)), block(kMemBlock);
    if (is_u8)
        hipLaunchKernelGGL((k_memory<uint8_t>), grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((k_memory<float>), grid, block, 0, (hipStream_t)stream, a);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : mem_refuse(T2D_ERR_HIP, "atr_memory_windows: launch failed: %s", hipGetErrorString(err));
}
