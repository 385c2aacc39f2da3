// heuristic_hip.hip — the heuristic players (include/track2d_heuristic.h): shortest-path distance between tracker and target, the
// pursuit tracker and the evading target of every env of a handle in one launch, one wavefront per (env, role). Reaches the
// handle's maps / pos / cnt arrays through t2d_state_view.h and writes none of them.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "../../include/track2d_heuristic.h"
#include "t2d_device.h"
#include "t2d_state_view.h"

namespace t2d {

constexpr int kHeurWaves = 4;        // 256-thread workgroups, one wavefront per (env, role)
constexpr int kArrMaps = 0, kArrPos = 1, kArrCnt = 3;    // rows of kStateArray
static_assert(kStateArray[kArrMaps].words == kTileWords && kStateArray[kArrPos].words == 1 && kStateArray[kArrCnt].words == 1,
              "maps, pos and cnt sit where this file reads them");

struct HeurArgs {
    const uint32_t *maps, *pos, *cnt;   // the handle's [N][256] tiles, [N] positions (r0 | c0 << 8 | r1 << 16 | c1 << 24), [N] counters (side << 24)
    long long *act;                     // [N][2]
    int *dist;                          // [N] or null
    int n, roles;
};

// wave-uniform (r, c): is the cell a wall? Outside the side x side square: yes.
__device__ __forceinline__ bool cell_wall(const uint32_t *tile, int side, int r, int c)
{
    const bool inside = r >= 0 && c >= 0 && r < side && c < side;
    return !inside || tile_bit(tile, inside ? r : 0, inside ? c : 0) != 0u;
}

// the first action whose destination is a wall (the env leaves the agent in place), 0 in open space
__device__ __forceinline__ int hold_action(const uint32_t *tile, int side, int r, int c)
{
    const bool w0 = cell_wall(tile, side, r - 1, c), w1 = cell_wall(tile, side, r + 1, c);
    const bool w2 = cell_wall(tile, side, r, c - 1), w3 = cell_wall(tile, side, r, c + 1);
    return w0 ? 0 : (w1 ? 1 : (w2 ? 2 : (w3 ? 3 : 0)));
}

// wave-uniform (r, c): the bit of a row set, 0 outside the square
__device__ __forceinline__ uint32_t rowbits_at(const RowBits &a, const RowBits &b, int side, int r, int c)
{
    const bool inside = r >= 0 && c >= 0 && r < side && c < side;
    const uint32_t bit = rowbits_get(a, b, inside ? r : 0, inside ? c : 0);
    return inside ? bit : 0u;
}

// this lane's bit of cell (r, c) in a row set (non-zero in the owning lane only)
__device__ __forceinline__ uint32_t own_bit(const RowBits &a, const RowBits &b, int lane, int r, int c)
{
    uint32_t hit = 0u;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        if (j == (c >> 5) && r < 64 && lane == r) hit = a.w[j] & (1u << (c & 31));
        if (j == (c >> 5) && r >= 64 && lane == r - 64) hit = b.w[j] & (1u << (c & 31));
    }
    return hit;
}

// The evading target's flood: rooted at the tracker's cell (tr, tc), it runs until the level that reaches the target's cell
// (gr, gc) — that level is d — and then exactly one level more. frA / frB come back as that last frontier: the cells at distance
// d + 1 from the tracker, the only ones that can hold a neighbour of the target farther away than the target itself. Returns d,
// -1 if the target is never reached (frA / frB then mean nothing). No direction planes: the register rows of bfs_dir_field's
// level without them, the same wave-uniform skip of rows >= 64.
__device__ __forceinline__ int evade_flood(const uint32_t *tile, int side, int lane, int tr, int tc, int gr, int gc, RowBits &frA,
                                           RowBits &frB)
{
    RowBits freeA, freeB, visA, visB;
    const uint32_t m2 = valid_mask_w2(side);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const uint32_t vm = j == 2 ? m2 : 0xffffffffu;
        freeA.w[j] = (lane < side) ? (~tile[lane * kRowWords + j] & vm) : 0u;
        freeB.w[j] = (lane + 64 < side) ? (~tile[(lane + 64) * kRowWords + j] & vm) : 0u;
        frA.w[j] = 0u; frB.w[j] = 0u;
    }
    {   // seed the frontier with the tracker's cell (a tracker on a wall — RPF — reaches nothing)
        const uint32_t bit = 1u << (tc & 31);
        const int j = tc >> 5;
#pragma unroll
        for (int q = 0; q < 3; q++) {
            if (q == j && tr < 64 && lane == tr) frA.w[q] = bit & freeA.w[q];
            if (q == j && tr >= 64 && lane == tr - 64) frB.w[q] = bit & freeB.w[q];
        }
    }
    visA = frA; visB = frB;
    int level = 0, d = (tr == gr && tc == gc) ? 0 : -1;
    bool last = d >= 0;                       // the level about to run is the one past d
    for (;;) {
        const bool actB = __ballot((frB.w[0] | frB.w[1] | frB.w[2]) != 0u || (lane == 63 && (frA.w[0] | frA.w[1] | frA.w[2]) != 0u)) != 0ull;
        RowBits upA, dnA, upB, dnB;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const uint32_t a_prev = from_prev_lane(frA.w[j]);
            const uint32_t a_next = from_next_lane(frA.w[j]);
            upA.w[j] = lane == 0 ? 0u : a_prev;
            dnA.w[j] = a_next;
            upB.w[j] = 0u; dnB.w[j] = 0u;
        }
        if (actB) {
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const uint32_t b_prev = from_prev_lane(frB.w[j]);
                const uint32_t b_next = from_next_lane(frB.w[j]);
                const uint32_t a_last = __builtin_amdgcn_readlane(frA.w[j], 63);  // row 63
                const uint32_t b_first = __builtin_amdgcn_readlane(frB.w[j], 0);  // row 64
                if (lane == 63) dnA.w[j] = b_first;
                upB.w[j] = lane == 0 ? a_last : b_prev;
                dnB.w[j] = lane == 63 ? 0u : b_next;
            }
        }
        const RowBits lfA = row_shl1(frA), rtA = row_shr1(frA);
        uint32_t any = 0u;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const uint32_t nw = (upA.w[j] | dnA.w[j] | lfA.w[j] | rtA.w[j]) & freeA.w[j] & ~visA.w[j];
            visA.w[j] |= nw; frA.w[j] = nw; any |= nw;
        }
        if (actB) {
            const RowBits lfB = row_shl1(frB), rtB = row_shr1(frB);
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const uint32_t nw = (upB.w[j] | dnB.w[j] | lfB.w[j] | rtB.w[j]) & freeB.w[j] & ~visB.w[j];
                visB.w[j] |= nw; frB.w[j] = nw; any |= nw;
            }
        }
        level++;
        if (last) break;                      // frA / frB: the cells at distance d + 1
        if (__ballot(own_bit(frA, frB, lane, gr, gc) != 0u) != 0ull) { d = level; last = true; continue; }
        if (__ballot(any != 0u) == 0ull) break;
    }
    return d;
}

// One wavefront per (env, role). Wave w of the grid: both roles asked for — env w / 2, role w % 2; one role — env w.
__global__ __launch_bounds__(64 * kHeurWaves) void k_heuristic(HeurArgs p)
{
    const int lane = (int)(threadIdx.x & 63u);
    const int w = uni((int)(blockIdx.x * kHeurWaves + (threadIdx.x >> 6)));
    const bool both = p.roles == (T2D_HEUR_PURSUIT | T2D_HEUR_EVADE);
    const int e = both ? w >> 1 : w;
    if (e >= p.n) return;
    const bool evade = both ? (w & 1) != 0 : p.roles == T2D_HEUR_EVADE;
    const uint32_t *tile = p.maps + (size_t)e * kTileWords;
    const uint32_t pos = uni(p.pos[e]);
    const int side = (int)(uni(p.cnt[e]) >> 24);
    const int tr = (int)(pos & 0xffu), tc = (int)((pos >> 8) & 0xffu);
    const int gr = (int)((pos >> 16) & 0xffu), gc = (int)(pos >> 24);
    const bool writes_dist = p.dist != nullptr && (evade ? (p.roles & T2D_HEUR_PURSUIT) == 0 : true);
    int action = 0, d = -1;
    // (a tile is laid out for sides 65 .. 82 and every position of a live episode lies inside its square; anything else — a
    // handle whose arrays were never filled — gets the answer of an env with no path rather than a shift or a row out of range)
    const bool sane = side > 64 && side <= 82 && tr < side && tc < side && gr < side && gc < side;
    if (sane && !evade) {
        const bool same = tr == gr && tc == gc;
        NavField f;
        if (same) d = 0;
        else if (!cell_wall(tile, side, gr, gc)) d = bfs_dir_field(tile, side, lane, gr, gc, f, false, tr, tc);
        if (d > 0) action = (int)(rowbits_get(f.d0A, f.d0B, tr, tc) | (rowbits_get(f.d1A, f.d1B, tr, tc) << 1));
        else action = hold_action(tile, side, tr, tc);
    } else if (sane) {
        RowBits frA, frB;
        d = evade_flood(tile, side, lane, tr, tc, gr, gc, frA, frB);
        action = -1;
        if (d >= 0) {
            const uint32_t n0 = rowbits_at(frA, frB, side, gr - 1, gc), n1 = rowbits_at(frA, frB, side, gr + 1, gc);
            const uint32_t n2 = rowbits_at(frA, frB, side, gr, gc - 1), n3 = rowbits_at(frA, frB, side, gr, gc + 1);
            action = n0 ? 0 : (n1 ? 1 : (n2 ? 2 : (n3 ? 3 : -1)));
        }
        if (action < 0) action = hold_action(tile, side, gr, gc);
    }
    if (lane == 0) {
        p.act[(size_t)e * 2 + (evade ? 1 : 0)] = (long long)action;
        if (writes_dist) p.dist[e] = d;
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

}  // namespace t2d

using namespace t2d;

extern "C" int t2d_heuristic_actions(t2d_handle *h, int roles, long long *act_dev, int *dist_dev, void *stream)
{
    if (!h) return refuse(T2D_ERR_INVALID, "t2d_heuristic_actions: null handle");
    if (!act_dev) return refuse(T2D_ERR_INVALID, "t2d_heuristic_actions: null act");
    if (roles < 1 || roles > (T2D_HEUR_PURSUIT | T2D_HEUR_EVADE))
        return refuse(T2D_ERR_INVALID, "t2d_heuristic_actions: roles %d, expected T2D_HEUR_PURSUIT (1), T2D_HEUR_EVADE (2) or both (3)", roles);
    if (((uintptr_t)act_dev & 7u) != 0) return refuse(T2D_ERR_INVALID, "t2d_heuristic_actions: act is not 8-byte aligned");
    if (((uintptr_t)dist_dev & 3u) != 0) return refuse(T2D_ERR_INVALID, "t2d_heuristic_actions: dist is not 4-byte aligned");
    t2d_state_view v;
    int rc = t2d_state_view_get(h, &v);
    if (rc) return rc;
    if (v.amask == 7)
        return refuse(T2D_ERR_INVALID, "t2d_heuristic_actions: the handle has the Moore action table (the players are defined for "
                                       "the four VonNeumann moves)");
    if (!v.ready) return refuse(T2D_ERR_INVALID, "t2d_heuristic_actions: call t2d_reset (all envs) first");
    DeviceScope guard(v.device);
    HeurArgs a;
    a.maps = v.arr[kArrMaps]; a.pos = v.arr[kArrPos]; a.cnt = v.arr[kArrCnt];
    a.act = act_dev; a.dist = dist_dev; a.n = v.n; a.roles = roles;
    const long long waves = (long long)v.n * (roles == (T2D_HEUR_PURSUIT | T2D_HEUR_EVADE) ? 2 : 1);
    hipLaunchKernelGGL(k_heuristic, dim3((unsigned)((waves + kHeurWaves - 1) / kHeurWaves)), dim3(64 * kHeurWaves), 0,
                       (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? T2D_OK : refuse(T2D_ERR_HIP, "t2d_heuristic_actions: launch failed: %s", hipGetErrorString(e));
}
