// sight_stats_hip.hip — line of sight, window path and loss / recovery of sight between tracker and target, counted on the device
// from the rollout store (C ABI, the rule and the table layout in full: include/atr_sight.h).
//
//   k_sight_stats         one wavefront per env, four envs per 256-thread workgroup; the front end is k_track_stats' (csrc/
//                         tracking_stats_hip.hip): a lane holds one aligned dword of each byte window (or cells l, l + 64, l + 128 of
//                         a float window), the compares go through __ballot, and kSightChunk steps have their loads in flight
//                         together. New here: the ballots of "cell == 1" are turned into the window's BITBOARD — 13 rows at a
//                         16-bit stride in four 64-bit words, columns 13 .. 15 never free — by four more ballots (lane j asks for
//                         the cell that bit j of each word stands for), and step k's bin and bitboard are handed to LANE k. After
//                         the chunk's front end lanes 0 .. kSightChunk-1 each own one sample: they test the line mask of their bin
//                         (a constant table in the same layout), flood their bitboard in registers (shifts and ANDs; the loop ends
//                         at the level that reaches the target, when the frontier stops growing, and at 168 levels at the latest)
//                         and add into the workgroup's LDS counters. The class a sample leaves behind goes to the next lane by one
//                         __shfl_up, so the transitions need no walk in step order. At the end every non-zero LDS counter goes out
//                         as ONE 64-bit integer atomic add: the totals are sums of integers, the same in any execution order.
//   k_sight_drain         copies the table out and zeroes it, one workgroup.
//
// Cost model: 4096 envs x 20 steps x 2 windows x 169 B = 27.7 MB read per rollout (u8), as k_track_stats; on top per sample about
// 60 vector instructions for the bitboard, and per chunk the floods of its samples side by side: (levels of the chunk's longest
// path) x about 70 instructions. DESIGN.md section 5 "Sight statistics".
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/atr_sight.h"

namespace atr {

typedef unsigned long long u64;

constexpr int kSightWaves = 4;                                       // envs per workgroup (one wave each)
constexpr int kSightBlock = 64 * kSightWaves;
constexpr int kSightChunk = 10;                                      // steps whose loads are in flight together, one lane each after
constexpr int kSightTail = ATR_SIGHT_WINDOW - 128;                   // 41 lanes hold a third cell of a float window
constexpr u64 kRows4 = 0x1fff1fff1fff1fffull;                        // columns 0 .. 12 of four rows
constexpr int kCentreWord = 1, kCentreBit = 2 * 16 + 6;              // cell (6, 6): row 6 = word 1, row 2 of it

struct SightArgs {
    const void *obs;
    long long obs_st, obs_se, obs_sp;
    const float *rew;
    long long rew_st, rew_se;
    const uint8_t *done;
    long long done_st, done_se;
    int *carry;
    u64 *tab;
    int T, N, flags;
};

// A window as bit rows: cell (r, c) is bit (r & 3) * 16 + c of w[r >> 2].
struct Board {
    u64 w[4];
};

// The line cells of every bin (include/atr_sight.h "The LINE"), as a Board per bin.
struct LineTable {
    u64 m[ATR_SIGHT_WINDOW][4];
};

constexpr LineTable make_lines()
{
    LineTable t = {};
    for (int bin = 0; bin < ATR_SIGHT_WINDOW; bin++) {
        const int dr = bin / 13 - 6, dc = bin % 13 - 6;
        const int ar = dr < 0 ? -dr : dr, ac = dc < 0 ? -dc : dc, m = ar > ac ? ar : ac;
        const int sr = dr < 0 ? -1 : 1, sc = dc < 0 ? -1 : 1;
        for (int k = 1; k < m; k++) {
            const int r = 6 + sr * ((2 * k * ar + m) / (2 * m)), c = 6 + sc * ((2 * k * ac + m) / (2 * m));
            t.m[bin][r >> 2] |= 1ull << ((r & 3) * 16 + c);
        }
    }
    return t;
}

__device__ const LineTable kLines = make_lines();

// What one lane holds of a window (as csrc/tracking_stats_hip.hip). Bytes: ONE aligned dword of the 43 or 44 that cover the
// window's 169 bytes, taken from the aligned address below the window, `mis` bytes skipped (an aligned dword that holds a byte of
// the window lies in the window's own page). Floats: cells l, l + 64, l + 128.
template <typename ObsT> struct SightRegs;
template <> struct SightRegs<uint8_t> {
    uint32_t v;
    int mis;
};
template <> struct SightRegs<float> {
    float v[3];
};

__device__ inline void sight_load(const uint8_t *w, int lane, SightRegs<uint8_t> &o)
{
    const int mis = (int)((uintptr_t)w & 3u);
    o.mis = mis;
    o.v = lane * 4 < mis + ATR_SIGHT_WINDOW ? ((const uint32_t *)(w - mis))[lane] : 0u;
}

__device__ inline void sight_load(const float *w, int lane, SightRegs<float> &o)
{
    o.v[0] = w[lane];
    o.v[1] = w[lane + 64];
    o.v[2] = lane < kSightTail ? w[lane + 128] : 0.0f;
}

// The cells of a window that hold `val`, one bit per cell (wave-uniform). Bytes: bit l of m[b] is cell 4 l + b - mis (bits outside
// the window are 0); floats: bit l of m[j] is cell 64 j + l, m[3] = 0.
struct CellBits {
    u64 m[4];
    int mis;
};

__device__ inline CellBits cells_equal(const SightRegs<uint8_t> &r, int lane, unsigned val)
{
    CellBits o;
    o.mis = r.mis;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int c = lane * 4 + b - r.mis;
        o.m[b] = __ballot(c >= 0 && c < ATR_SIGHT_WINDOW && ((r.v >> (8 * b)) & 255u) == val);
    }
    return o;
}

__device__ inline CellBits cells_equal(const SightRegs<float> &r, int lane, unsigned val)
{
    CellBits o;
    o.mis = 0;
#pragma unroll
    for (int j = 0; j < 3; j++) o.m[j] = __ballot(r.v[j] == (float)val);        // (lanes without a third cell hold 0)
    o.m[3] = 0ull;
    return o;
}

template <typename ObsT> __device__ inline int cell_count(const CellBits &b)
{
    return __popcll(b.m[0]) + __popcll(b.m[1]) + __popcll(b.m[2]) + __popcll(b.m[3]);
}

// The index of a cell whose bit is set (THE cell when there is one).
template <typename ObsT> __device__ inline int cell_index(const CellBits &b);
template <> __device__ inline int cell_index<uint8_t>(const CellBits &b)
{
    int idx = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (b.m[j]) idx = (__ffsll((long long)b.m[j]) - 1) * 4 + j - b.mis;
    return idx;
}
template <> __device__ inline int cell_index<float>(const CellBits &b)
{
    int idx = 0;
#pragma unroll
    for (int j = 0; j < 3; j++)
        if (b.m[j]) idx = 64 * j + __ffsll((long long)b.m[j]) - 1;
    return idx;
}

// Is the bit of cell c (0 <= c < 169, any value per lane) set?
template <typename ObsT> __device__ inline bool cell_bit(const CellBits &b, int c);
template <> __device__ inline bool cell_bit<uint8_t>(const CellBits &b, int c)
{
    const int p = c + b.mis, s = p & 3;
    const u64 m = s == 0 ? b.m[0] : s == 1 ? b.m[1] : s == 2 ? b.m[2] : b.m[3];
    return (m >> (p >> 2)) & 1ull;
}
template <> __device__ inline bool cell_bit<float>(const CellBits &b, int c)
{
    const int s = c >> 6;
    const u64 m = s == 0 ? b.m[0] : s == 1 ? b.m[1] : b.m[2];
    return (m >> (c & 63)) & 1ull;
}

__device__ inline bool sight_centre_is(const SightRegs<uint8_t> &r, unsigned val)
{
    const int p = ATR_SIGHT_CENTRE + r.mis;
    return ((__shfl(r.v, p >> 2) >> (8 * (p & 3))) & 255u) == val;
}

__device__ inline bool sight_centre_is(const SightRegs<float> &r, unsigned val)
{
    return __shfl(r.v[1], ATR_SIGHT_CENTRE - 64) == (float)val;
}

// One level of the flood: the cells of `r`, their 4-neighbours, and of those the free ones.
__device__ inline Board grow(const Board &r, const Board &free_)
{
    Board n;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        u64 x = r.w[i] | (r.w[i] << 1) | (r.w[i] >> 1) | (r.w[i] << 16) | (r.w[i] >> 16);
        if (i > 0) x |= r.w[i - 1] >> 48;
        if (i < 3) x |= r.w[i + 1] << 48;
        n.w[i] = x & free_.w[i];
    }
    return n;
}

template <typename ObsT>
__global__ __launch_bounds__(kSightBlock) void k_sight_stats(SightArgs a)
{
    __shared__ unsigned cnt[ATR_SIGHT_TABLE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < ATR_SIGHT_TABLE; i += kSightBlock) cnt[i] = 0u;
    __syncthreads();
    const long long e = (long long)blockIdx.x * kSightWaves + wave;
    if (e < a.N) {        // (wave-uniform)
        const ObsT *obs = (const ObsT *)a.obs + e * a.obs_se;
        const float *rew = a.rew + e * a.rew_se;
        const uint8_t *done = a.done + e * a.done_se;
        int carry = a.carry[e];
        if (carry < -1 || carry > ATR_SIGHT_OUT_CLASS) carry = -1;
        // the cell that bit `lane` of each bitboard word stands for (-1: a padding column, or a row below the window)
        int cell_of[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int r = 4 * i + (lane >> 4), c = lane & 15;
            cell_of[i] = r < 13 && c < 13 ? r * 13 + c : -1;
        }
        for (int t0 = 0; t0 < a.T; t0 += kSightChunk) {
            // lane k < kSightChunk fetches step t0 + k's reward and flag; every lane fetches its part of the chunk's windows. A
            // step past the end reads the last step again: unused.
            const long long ts = min((long long)t0 + (lane < kSightChunk ? lane : 0), (long long)a.T - 1);
            const float r_l = rew[ts * a.rew_st];
            const int d_l = done[ts * a.done_st];
            SightRegs<ObsT> x[kSightChunk], y[kSightChunk];
#pragma unroll
            for (int k = 0; k < kSightChunk; k++) {
                const long long t = min((long long)t0 + k, (long long)a.T - 1);
                const ObsT *w0 = obs + (t + 1) * a.obs_st;
                sight_load(w0, lane, x[k]);
                sight_load(w0 + a.obs_sp, lane, y[k]);
            }
            // front end, wave-uniform per step; lane k keeps step k's bin and walls
            int bin = -1;        // (-1: this lane owns no sample of the chunk)
            Board walls = {{0ull, 0ull, 0ull, 0ull}};
#pragma unroll
            for (int k = 0; k < kSightChunk; k++) {
                if (t0 + k >= a.T) continue;        // (no break: the loop must unroll fully, x / y stay in registers)
                const CellBits four = cells_equal(x[k], lane, 4u), two = cells_equal(y[k], lane, 2u);
                const CellBits wall = cells_equal(x[k], lane, 1u);
                const bool c0 = sight_centre_is(x[k], 2u), c1 = sight_centre_is(y[k], 4u);
                const float r = __shfl(r_l, k);
                const int d = __shfl(d_l, k);
                const int n4 = cell_count<ObsT>(four), n2 = cell_count<ObsT>(two);
                const int i4 = cell_index<ObsT>(four), i2 = cell_index<ObsT>(two);
                int b;
                if (d && !(a.flags & ATR_SIGHT_NO_AUTO_RESET)) b = ATR_SIGHT_BIN_TERMINAL;
                else if (!c0 || !c1) b = ATR_SIGHT_BIN_INCONSISTENT;
                else if (r == 1.0f) b = n4 == 0 && n2 == 0 ? ATR_SIGHT_CENTRE : ATR_SIGHT_BIN_INCONSISTENT;
                else if (n4 == 0 && n2 == 0) b = ATR_SIGHT_BIN_OUT;
                else if (n4 == 1 && n2 == 1 && i2 == ATR_SIGHT_WINDOW - 1 - i4) b = i4;
                else b = ATR_SIGHT_BIN_INCONSISTENT;
                Board wb;
#pragma unroll
                for (int i = 0; i < 4; i++) wb.w[i] = __ballot(cell_of[i] >= 0 && cell_bit<ObsT>(wall, max(cell_of[i], 0)));
                if (lane == k) {
                    bin = b;
                    walls = wb;
                }
            }
            // back end: lane k owns sample t0 + k
            const int d_mine = d_l;                                  // (lane k fetched step t0 + k's flag itself)
            int cls = -1;                                            // the sample's class (-1: none)
            if (bin == ATR_SIGHT_BIN_OUT) cls = ATR_SIGHT_OUT_CLASS;
            else if (bin == ATR_SIGHT_CENTRE) cls = ATR_SIGHT_CLEAR;
            else if (bin >= 0 && bin < ATR_SIGHT_WINDOW) {
                const u64 *ln = kLines.m[bin];
                const bool blocked = ((walls.w[0] & ln[0]) | (walls.w[1] & ln[1]) | (walls.w[2] & ln[2]) | (walls.w[3] & ln[3])) != 0ull;
                cls = blocked ? ATR_SIGHT_BLOCKED_CLASS : ATR_SIGHT_CLEAR;
                // the flood, from the centre towards the target's cell
                const int tr = bin / 13, tc = bin - tr * 13, tw = tr >> 2;
                const u64 tbit = 1ull << ((tr & 3) * 16 + tc);
                Board target;
#pragma unroll
                for (int i = 0; i < 4; i++) target.w[i] = i == tw ? tbit : 0ull;
                Board free_ = {{~walls.w[0] & kRows4, ~walls.w[1] & kRows4, ~walls.w[2] & kRows4, ~walls.w[3] & 0x1fffull}};
                Board reach = {{0ull, 0ull, 0ull, 0ull}};
                reach.w[kCentreWord] = 1ull << kCentreBit;
                int path = 0;                                        // (0: no path)
                for (int level = 1; level <= ATR_SIGHT_MAX_PATH; level++) {
                    const Board next = grow(reach, free_);
                    const u64 hit = (next.w[0] & target.w[0]) | (next.w[1] & target.w[1]) | (next.w[2] & target.w[2]) | (next.w[3] & target.w[3]);
                    const u64 grown = (next.w[0] ^ reach.w[0]) | (next.w[1] ^ reach.w[1]) | (next.w[2] ^ reach.w[2]) | (next.w[3] ^ reach.w[3]);
                    reach = next;
                    if (hit) {
                        path = level;
                        break;
                    }
                    if (!grown) break;
                }
                const int dr = tr - 6, dc = tc - 6;
                atomicAdd(&cnt[ATR_SIGHT_SEEN + bin], 1u);
                if (blocked) atomicAdd(&cnt[ATR_SIGHT_BLOCKED + bin], 1u);
                if (path == 0) {
                    atomicAdd(&cnt[ATR_SIGHT_NOPATH + bin], 1u);
                } else {
                    atomicAdd(&cnt[ATR_SIGHT_PATH + path], 1u);
                    atomicAdd(&cnt[ATR_SIGHT_DETOUR + ((path - abs(dr) - abs(dc)) >> 1)], 1u);
                }
            }
            if (bin == ATR_SIGHT_CENTRE) atomicAdd(&cnt[ATR_SIGHT_SEEN + bin], 1u);
            else if (bin == ATR_SIGHT_BIN_OUT) atomicAdd(&cnt[ATR_SIGHT_OUT], 1u);
            else if (bin == ATR_SIGHT_BIN_TERMINAL) atomicAdd(&cnt[ATR_SIGHT_TERMINAL], 1u);
            else if (bin == ATR_SIGHT_BIN_INCONSISTENT) atomicAdd(&cnt[ATR_SIGHT_INCONSISTENT], 1u);
            // the class each sample leaves to the next one, and the one it finds
            const int left = (cls < 0 || d_mine) ? -1 : cls;
            const int up = __shfl_up(left, 1);
            const int prev = lane == 0 ? carry : up;
            if (bin >= 0) {
                atomicAdd(&cnt[ATR_SIGHT_SAMPLES], 1u);
                if (prev >= 0 && cls >= 0) atomicAdd(&cnt[ATR_SIGHT_TRANS + prev * 3 + cls], 1u);
            }
            carry = __shfl(left, min(kSightChunk, a.T - t0) - 1);
        }
        if (lane == 0) a.carry[e] = carry;
    }
    __syncthreads();
    for (int i = tid; i < ATR_SIGHT_TABLE; i += kSightBlock) {
        const unsigned c = cnt[i];
        if (c) atomicAdd(a.tab + i, (u64)c);
    }
}

__global__ __launch_bounds__(256) void k_sight_drain(u64 *__restrict__ tab, u64 *__restrict__ out_tab)
{
    for (int i = threadIdx.x; i < ATR_SIGHT_TABLE; i += 256) {
        out_tab[i] = tab[i];
        tab[i] = 0ull;
    }
}

// (as csrc/tracking_stats_hip.hip: the refusals put their text into the calling thread's t2d_last_error() buffer)
static int sight_refuse(int code, const char *fmt, ...)
{
    char *buf = const_cast<char *>(t2d_last_error());
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, 256, fmt, ap);
    va_end(ap);
    return code;
}

static int sight_launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : sight_refuse(T2D_ERR_HIP, "%s: launch failed: %s", what, hipGetErrorString(e));
}

}  // namespace atr

using namespace atr;

extern "C" int atr_sight_stats(const void *obs, int obs_is_u8, long long obs_st, long long obs_se, long long obs_sp, const float *rew,
                               long long rew_st, long long rew_se, long long rew_sp, const unsigned char *done, long long done_st,
                               long long done_se, int *carry, unsigned long long *tab, int T, int N, int flags, void *stream)
{
    if (!obs || !rew || !done || !carry || !tab)
        return sight_refuse(T2D_ERR_INVALID, "atr_sight_stats: null pointer (obs %p rew %p done %p carry %p tab %p)", obs,
                            (const void *)rew, (const void *)done, (void *)carry, (void *)tab);
    if (N <= 0 || T <= 0) return sight_refuse(T2D_ERR_INVALID, "atr_sight_stats: needs N > 0 and T > 0 (N %d, T %d)", N, T);
    if (T > ATR_SIGHT_MAX_T) return sight_refuse(T2D_ERR_INVALID, "atr_sight_stats: T %d above %d steps per call", T, ATR_SIGHT_MAX_T);
    if (flags & ~ATR_SIGHT_NO_AUTO_RESET) return sight_refuse(T2D_ERR_INVALID, "atr_sight_stats: unknown flags 0x%x", flags);
    if (obs_st < 0 || obs_se < 0 || obs_sp < 0 || rew_st < 0 || rew_se < 0 || rew_sp < 0 || done_st < 0 || done_se < 0)
        return sight_refuse(T2D_ERR_INVALID, "atr_sight_stats: negative element stride");
    if ((uintptr_t)tab & 7u) return sight_refuse(T2D_ERR_INVALID, "atr_sight_stats: tab %p not 8-byte aligned", (void *)tab);
    if ((((uintptr_t)carry | (uintptr_t)rew) & 3u) || (!obs_is_u8 && ((uintptr_t)obs & 3u)))
        return sight_refuse(T2D_ERR_INVALID, "atr_sight_stats: carry / rew / float32 obs not 4-byte aligned");
    (void)rew_sp;        // (only player 0's reward is read: element p = 0)
    SightArgs a;
    a.obs = obs;
    a.obs_st = obs_st, a.obs_se = obs_se, a.obs_sp = obs_sp;
    a.rew = rew;
    a.rew_st = rew_st, a.rew_se = rew_se;
    a.done = (const uint8_t *)done;
    a.done_st = done_st, a.done_se = done_se;
    a.carry = carry, a.tab = tab;
    a.T = T, a.N = N, a.flags = flags;
    const dim3 grid((unsigned)((N + kSightWaves - 1) / kSightWaves)), block(kSightBlock);
    if (obs_is_u8)
        hipLaunchKernelGGL(k_sight_stats<uint8_t>, grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_sight_stats<float>, grid, block, 0, (hipStream_t)stream, a);
    return sight_launched("atr_sight_stats");
}

extern "C" int atr_sight_stats_drain(unsigned long long *tab, unsigned long long *out_tab, void *stream)
{
    if (!tab || !out_tab)
        return sight_refuse(T2D_ERR_INVALID, "atr_sight_stats_drain: null pointer (tab %p out_tab %p)", (void *)tab, (void *)out_tab);
    if (((uintptr_t)tab | (uintptr_t)out_tab) & 7u)
        return sight_refuse(T2D_ERR_INVALID, "atr_sight_stats_drain: a table is not 8-byte aligned");
    hipLaunchKernelGGL(k_sight_drain, dim3(1), dim3(256), 0, (hipStream_t)stream, tab, out_tab);
    return sight_launched("atr_sight_stats_drain");
}
