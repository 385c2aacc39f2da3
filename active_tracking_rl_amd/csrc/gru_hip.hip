// gru_hip.hip — the GRU recurrent core of the 'maze-gru' / 'tat-maze-gru' networks (C ABI and the cell's equations in
// include/atr_gru.h): torch.nn.GRUCell(256 -> R), gate order (r, z, n), on the path that keeps no rollout cache.
//
//   atr_gru_cell_forward    one step for P players: the element-wise half of the cell between the caller's two GEMMs
//                           (ig = x W_ih^T + b_ih, hg = h_prev W_hh^T), the previous step's episode mask k applied to the hidden
//                           product AND to the z h term, b_hh added after the mask (b_hn sits inside r * (.), so it cannot be
//                           folded into ig as the LSTM's is). Optionally stores (r, z, n, q) for the backward pass.
//   atr_gru_cell_backward   one step of back-propagation through time (the per-step path): dG = (dr_pre, dz_pre, dn_pre,
//                           dn_pre r) and the direct part dh z of the gradient into k h_prev; the caller's GEMM adds dG W_hh.
//   atr_gru_bptt            the whole recurrence backward of a rollout as ONE launch for R = 128, shaped like k_lstm_bptt
//                           (bptt_hip.hip): the recurrence is independent per row (env), so a workgroup takes 16 rows of one
//                           player through all T steps. W_hh [3R, R] = [384, 128] stays in registers as f32 MFMA B operands
//                           (wave w of the 8 owns hidden units [16 w, 16 w + 16): 96 VGPRs); the accumulator layout of
//                           v_mfma_f32_16x16x4_f32 (lane = unit column, 4 rows) is the ownership of the element-wise cell
//                           backward, so the gradient arriving through the hidden GEMM and the direct part never leave the
//                           registers of the thread that needs them at step t - 1. Per step: cell backward of the thread's 4
//                           (row, unit) pairs, dG streamed out, the three hidden-side gradients parked in a double-buffered LDS
//                           tile [16 x 384], ONE barrier, 96 MFMAs per wave with the next step's activations fetched under them.
//   atr_gru_bptt_sums       the same launch, compiled with the by-action column sums of dG's input-side columns for the
//                           tracker-aware target's embedding fold (include/atr_gru_sums.h); atr_gru_bptt's code has none of it.
// The cell kernels are HBM-bound streaming kernels: one thread per 4 hidden units (16-byte accesses), grid-stride.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/atr_gru.h"
#include "atr_cell.h"

namespace atr {

struct GruFwd {
    const float *ig[2];        // per player [N, 3R]: x W_ih^T + b_ih
    const float *hg;           // [P, N, 3R]: h_prev W_hh^T (h_prev un-masked)
    const float *bhh[2];       // per player [3R]
    const float *h_prev;       // + p * h_prev_ps + n * R
    long long h_prev_ps;
    const float *keep;         // [N] float mask of the previous step (nullable)
    const unsigned char *done; // [N] done flags of the previous step (nullable; k = done == 0)
    float *h_out;              // + p * h_ps + n * R
    long long h_ps;
    float *acts;               // nullable: + p * acts_ps + n * 4R : (r, z, n, q)
    long long acts_ps;
    int P, N, R;
};

__global__ __launch_bounds__(256) void k_gru_cell_fwd(GruFwd a)
{
    const int rq = a.R >> 2;
    const long long total = (long long)a.P * a.N * rq;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(idx % rq) * 4;
        const long long row = idx / rq;
        const int n = (int)(row % a.N), p = (int)(row / a.N);
        const float k = a.keep ? a.keep[n] : (a.done ? (a.done[n] == 0 ? 1.0f : 0.0f) : 1.0f);
        const float *ig = a.ig[p] + (long long)n * 3 * a.R + j;
        const float *hg = a.hg + ((long long)p * a.N + n) * 3 * a.R + j;
        const float *bh = a.bhh[p] + j;
        // hidden pre-activations: mask first, then b_hh
        const float4 hr = fma4(k, ld4(hg), ld4(bh));
        const float4 hz = fma4(k, ld4(hg + a.R), ld4(bh + a.R));
        const float4 q = fma4(k, ld4(hg + 2 * a.R), ld4(bh + 2 * a.R));
        const float4 ir = ld4(ig), iz = ld4(ig + a.R), in = ld4(ig + 2 * a.R);
        const float4 hp = ld4(a.h_prev + p * a.h_prev_ps + (long long)n * a.R + j);
        const float irv[4] = {ir.x, ir.y, ir.z, ir.w}, izv[4] = {iz.x, iz.y, iz.z, iz.w}, inv[4] = {in.x, in.y, in.z, in.w};
        const float hrv[4] = {hr.x, hr.y, hr.z, hr.w}, hzv[4] = {hz.x, hz.y, hz.z, hz.w}, qv[4] = {q.x, q.y, q.z, q.w};
        const float hpv[4] = {hp.x, hp.y, hp.z, hp.w};
        float r[4], z[4], nn[4], h[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            r[u] = sigmoidf_(irv[u] + hrv[u]);
            z[u] = sigmoidf_(izv[u] + hzv[u]);
            nn[u] = tanhf_(inv[u] + r[u] * qv[u]);
            h[u] = (1.0f - z[u]) * nn[u] + z[u] * (k * hpv[u]);
        }
        st4(a.h_out + p * a.h_ps + (long long)n * a.R + j, make_float4(h[0], h[1], h[2], h[3]));
        if (a.acts) {
            float *ac = a.acts + p * a.acts_ps + (long long)n * 4 * a.R + j;
            st4(ac, make_float4(r[0], r[1], r[2], r[3]));
            st4(ac + a.R, make_float4(z[0], z[1], z[2], z[3]));
            st4(ac + 2 * a.R, make_float4(nn[0], nn[1], nn[2], nn[3]));
            st4(ac + 3 * a.R, q);
        }
    }
}

// The cell backward of ONE (row, unit) pair — the expressions both backward kernels evaluate, in one place.
// dh: the whole gradient of this step's h (heads + what step t + 1 sent, masked); khp = k_{t-1} h_{t-1}.
struct GruGrad { float dr, dz, dn, dq, direct; };
__device__ __forceinline__ GruGrad gru_grad(float dh, float r, float z, float n, float q, float khp)
{
    GruGrad g;
    g.dn = dh * (1.0f - z) * (1.0f - n * n);            // through n = tanh(.)
    g.dz = dh * (khp - n) * z * (1.0f - z);             // through z = sigmoid(.)
    g.dr = g.dn * q * r * (1.0f - r);                   // through r = sigmoid(.), n's argument holds r q
    g.dq = g.dn * r;                                    // into q = k hg_n + b_hn
    g.direct = dh * z;                                  // into k h_prev through the z h term
    return g;
}

struct GruBwd {
    const float *dh_out;       // + p * dh_ps + n * R
    long long dh_ps;
    float *dh_carry;           // [P, N, R]: in = what step t + 1 sent (un-masked, ignored if !has_next); out = dh z
    const float *keep_out;     // nullable [N]: k_t
    const float *keep_in;      // nullable [N]: k_{t-1}
    const float *acts;         // + p * acts_ps + n * 4R
    long long acts_ps;
    const float *h_prev;       // + p * h_prev_ps + n * R
    long long h_prev_ps;
    float *dg;                 // + p * dg_ps + n * 4R
    long long dg_ps;
    int has_next;
    int P, N, R;
};

__global__ __launch_bounds__(256) void k_gru_cell_bwd(GruBwd a)
{
    const int rq = a.R >> 2;
    const long long total = (long long)a.P * a.N * rq;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(idx % rq) * 4;
        const long long row = idx / rq;
        const int n = (int)(row % a.N), p = (int)(row / a.N);
        const long long o1 = ((long long)p * a.N + n) * a.R + j;
        const float ko = a.keep_out ? a.keep_out[n] : 1.0f, ki = a.keep_in ? a.keep_in[n] : 1.0f;
        float4 dh = ld4(a.dh_out + p * a.dh_ps + (long long)n * a.R + j);
        if (a.has_next) dh = fma4(ko, ld4(a.dh_carry + o1), dh);
        const float *ac = a.acts + p * a.acts_ps + (long long)n * 4 * a.R + j;
        const float4 r = ld4(ac), z = ld4(ac + a.R), nn = ld4(ac + 2 * a.R), q = ld4(ac + 3 * a.R);
        const float4 hp = ld4(a.h_prev + p * a.h_prev_ps + (long long)n * a.R + j);
        const GruGrad g0 = gru_grad(dh.x, r.x, z.x, nn.x, q.x, ki * hp.x), g1 = gru_grad(dh.y, r.y, z.y, nn.y, q.y, ki * hp.y);
        const GruGrad g2 = gru_grad(dh.z, r.z, z.z, nn.z, q.z, ki * hp.z), g3 = gru_grad(dh.w, r.w, z.w, nn.w, q.w, ki * hp.w);
        float *dg = a.dg + p * a.dg_ps + (long long)n * 4 * a.R + j;
        st4(dg, make_float4(g0.dr, g1.dr, g2.dr, g3.dr));
        st4(dg + a.R, make_float4(g0.dz, g1.dz, g2.dz, g3.dz));
        st4(dg + 2 * a.R, make_float4(g0.dn, g1.dn, g2.dn, g3.dn));
        st4(dg + 3 * a.R, make_float4(g0.dq, g1.dq, g2.dq, g3.dq));
        st4(a.dh_carry + o1, make_float4(g0.direct, g1.direct, g2.direct, g3.direct));
    }
}

static unsigned gru_grid_for(long long work)
{
    long long b = (work + 255) / 256;
    if (b > 8192) b = 8192;
    return (unsigned)(b < 1 ? 1 : b);
}

// ---- the one-launch BPTT ---------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kGR = 128;                    // hidden units
constexpr int kGK = 3 * kGR;                // contraction length: the three hidden-side gradients (dr_pre, dz_pre, dq)
constexpr int kGW = 4 * kGR;                // row width of the acts / dG stores
constexpr int kGRows = 16;                  // rows per workgroup (one MFMA M tile)
constexpr int kGLd = kGK + 4;               // LDS row stride (floats): 16-B reads of 8 lanes hit 32 distinct banks
constexpr int kGSteps = kGK / 16;           // 24 groups of 4 MFMAs per wave and step

struct GruBptt {
    const float *dh[2];        // per player: dL/dh_t from the heads [T, N, R] (nullable: zero)
    const float *keep;         // [T, N]
    const float *acts;         // + p * acts_ps + (t * N + n) * 4R : (r, z, n, q)
    long long acts_ps;
    const float *h_all;        // + p * h_ps + (t * N + n) * R : slot t = the un-masked state step t starts from
    long long h_ps;
    const float *whh[2];       // per player weight_hh [3R, R]
    float *dg;                 // + p * dg_ps + (t * N + n) * 4R (out)
    long long dg_ps;
    float *dh0;                // [P, N, R] (out)
    // SUMS only: per row tile of player emb_player, the column sums of dG's INPUT-side columns (dr_pre, dz_pre, dn_pre) over the
    // tile's rows and all T steps BY THE TRACKER'S ACTION of the row (int64, act + t * act_ts + n) — [tiles][4][3R]. S = their
    // sum over the tiles is all the tracker-action embedding needs of the backward pass (include/atr_gru_sums.h: atr_gru_bptt_sums)
    const long long *act;
    long long act_ts;
    int emb_player;
    float *act_sums;
    int P, T, N;
};

// SUMS: the by-action column sums. The LDS tile holds (dr, dz, dq) — the MFMA's K — and not dn_pre, and a fourth LDS block for it
// would pass the 64 KB default limit (2 x 16 x 516 floats), so the sums are taken in registers from the thread's own 4 (row, unit)
// pairs: 4 actions x 3 gates = 12 accumulators of unit u (the kernel without them is at 194 of the 256 VGPRs __launch_bounds__(512,
// 1) allows), then reduced ONCE over the 4 row groups q through the LDS tile after the last step.
template <bool SUMS = false>
__global__ __launch_bounds__(512, 1) void k_gru_bptt(GruBptt a)
{
    extern __shared__ __attribute__((aligned(16))) float tileG[];      // [2][kGRows][kGLd]
    const int tid = (int)threadIdx.x, l = tid & 63, w = tid >> 6;
    const int col = l & 15, q = l >> 4;
    const int tiles = (a.N + kGRows - 1) / kGRows;
    const int p = (int)blockIdx.x / tiles, rt = (int)blockIdx.x - p * tiles;
    const int row0 = rt * kGRows;
    const int u = 16 * w + col;                                         // this lane's hidden unit
    // ---- this wave's slice of W_hh as MFMA B operands: step s = 4 g + t, slot q  <->  k = 16 g + 4 q + t, where k runs over
    // weight_hh's rows (r block, z block, n block) and over the LDS tile's columns (dr_pre, dz_pre, dq) alike
    const float *W = a.whh[p];
    float B[4 * kGSteps];
#pragma unroll
    for (int g = 0; g < kGSteps; g++)
#pragma unroll
        for (int t = 0; t < 4; t++) B[4 * g + t] = W[(size_t)(16 * g + 4 * q + t) * kGR + u];
    // ---- the 4 (row, unit) pairs of this thread: rows row0 + 4 q + i — the rows of its MFMA accumulator. Rows past N are
    // clamped for the loads (their results are never stored) and skipped by the stores.
    int rows[4];
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { rows[i] = row0 + 4 * q + i; ok[i] = rows[i] < a.N; rows[i] = min(rows[i], a.N - 1); }
    const float *acts = a.acts + (size_t)p * a.acts_ps;
    const float *hall = a.h_all + (size_t)p * a.h_ps;
    const float *dhp = a.dh[p];
    float *dg = a.dg + (size_t)p * a.dg_ps;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};          // dG_{t+1}[hidden columns] W_hh for this thread's pairs
    float dir[4] = {0.f, 0.f, 0.f, 0.f};       // dh_{t+1} z_{t+1}: the direct part of what step t + 1 sends into k_t h_t
    // staged inputs of one step (fetched one step ahead, under the MFMAs)
    float gr[4], gz[4], gn[4], gq[4], hpv[4], dhh[4], ko[4], ki[4];
    // SUMS: the action of the thread's 4 rows (-1: a row past N, or not a move of the four-entry table — counted nowhere)
    const bool sums = SUMS && p == a.emb_player;
    int ai[4] = {-1, -1, -1, -1};
    float sr[4] = {0.f, 0.f, 0.f, 0.f}, sz[4] = {0.f, 0.f, 0.f, 0.f}, sn[4] = {0.f, 0.f, 0.f, 0.f};      // [action]
#define GRU_FETCH(t_)                                                                                                  \
    do {                                                                                                               \
        const int tt_ = (t_);                                                                                          \
        _Pragma("unroll") for (int i = 0; i < 4; i++) {                                                                \
            const size_t r_ = (size_t)tt_ * a.N + rows[i];                                                             \
            const float *ac_ = acts + r_ * kGW + u;                                                                    \
            gr[i] = ac_[0]; gz[i] = ac_[kGR]; gn[i] = ac_[2 * kGR]; gq[i] = ac_[3 * kGR];                              \
            hpv[i] = hall[r_ * kGR + u];                         /* h before step t: slot t */                         \
            dhh[i] = dhp ? dhp[r_ * kGR + u] : 0.0f;                                                                   \
            ko[i] = a.keep[r_];                                                                                        \
            ki[i] = tt_ > 0 ? a.keep[r_ - a.N] : 1.0f;                                                                 \
            if (SUMS && sums && ok[i]) ai[i] = (int)a.act[(size_t)tt_ * a.act_ts + rows[i]];                           \
        }                                                                                                              \
    } while (0)
    GRU_FETCH(a.T - 1);
#pragma unroll 1
    for (int t = a.T - 1; t >= 0; t--) {
        float *At = tileG + (size_t)(t & 1) * kGRows * kGLd;
        const bool has_next = t < a.T - 1;
        // ---- cell backward of this thread's 4 pairs (k_gru_cell_bwd's expressions)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            float dh = dhh[i];
            if (has_next) dh = fmaf(ko[i], acc[i] + dir[i], dh);
            const GruGrad g = gru_grad(dh, gr[i], gz[i], gn[i], gq[i], ki[i] * hpv[i]);
            dir[i] = g.direct;
            float *ar = At + (4 * q + i) * kGLd + u;
            ar[0] = g.dr; ar[kGR] = g.dz; ar[2 * kGR] = g.dq;
            if (ok[i]) {
                float *o = dg + ((size_t)t * a.N + rows[i]) * kGW + u;
                __builtin_nontemporal_store(g.dr, o); __builtin_nontemporal_store(g.dz, o + kGR);       // streamed out: the
                __builtin_nontemporal_store(g.dn, o + 2 * kGR); __builtin_nontemporal_store(g.dq, o + 3 * kGR);  // GEMMs read dG later
            }
            if (SUMS && sums) {                            // (fmaf(1, v, s) = s + v, fmaf(0, v, s) = s: exact either way)
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const float m = ai[i] == c ? 1.0f : 0.0f;
                    sr[c] = fmaf(m, g.dr, sr[c]); sz[c] = fmaf(m, g.dz, sz[c]); sn[c] = fmaf(m, g.dn, sn[c]);
                }
            }
        }
        __syncthreads();                                   // the tile of step t is complete (the other buffer: step t + 1's
                                                           // reads finished before this step's writes began two barriers ago)
        if (t > 0) GRU_FETCH(t - 1);                       // next step's inputs: in flight under the MFMAs
        // ---- acc = dG_t[rows, hidden columns] W_hh[:, units of this wave]
        acc = (f32x4){0.f, 0.f, 0.f, 0.f};
        f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
        const float *rd = At + col * kGLd + 4 * q;         // MFMA A layout: lane (row col, K slot q)
        // the A operands run kDepth reads ahead of the MFMAs that consume them (a ring of registers: an LDS read issued right
        // before its use costs its full latency on a wave that has the SIMD to itself)
        constexpr int kDepth = 6;
        float4 ring[kDepth];
#pragma unroll
        for (int g = 0; g < kDepth; g++) ring[g] = *reinterpret_cast<const float4 *>(rd + 16 * g);
#pragma unroll
        for (int g = 0; g < kGSteps; g++) {
            const float4 av = ring[g % kDepth];
            if (g + kDepth < kGSteps) ring[g % kDepth] = *reinterpret_cast<const float4 *>(rd + 16 * (g + kDepth));
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, B[4 * g + 0], acc, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, B[4 * g + 1], acc2, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, B[4 * g + 2], acc, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, B[4 * g + 3], acc2, 0, 0, 0);
        }
        // (scheduling directives for the block above: kDepth LDS reads, then 4 MFMAs : 1 LDS read, then the remaining MFMAs)
        __builtin_amdgcn_sched_group_barrier(0x100, kDepth, 0);
#pragma unroll
        for (int g = 0; g < kGSteps - kDepth; g++) {
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 4 * kDepth, 0);
        acc += acc2;
    }
#undef GRU_FETCH
    if (SUMS && sums) {
        // ---- the 4 row groups' partial sums of unit u meet in LDS: red [q][action][gate][R] = 6144 floats, summed in the fixed order
        // q = 0..3; thread tid writes columns tid, tid + 512, tid + 1024 of the tile's [4][3R] block (all of it, zeros included)
        __syncthreads();                                   // every wave's MFMA reads of the last step's tile are done
        float *red = tileG;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            float *o = red + (size_t)((q * 4 + c) * 3) * kGR + u;
            o[0] = sr[c]; o[kGR] = sz[c]; o[2 * kGR] = sn[c];
        }
        __syncthreads();
        float *out = a.act_sums + (size_t)rt * 4 * kGK;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int o = tid + 512 * k;                   // = action * 3R + gate * R + unit: red's own order within one q
            out[o] = ((red[o] + red[4 * kGK + o]) + red[2 * 4 * kGK + o]) + red[3 * 4 * kGK + o];
        }
    }
    // ---- gradient into the rollout's initial hidden state (slot 0 comes masked: no k here)
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (ok[i]) a.dh0[((size_t)p * a.N + rows[i]) * kGR + u] = acc[i] + dir[i];
}

} // namespace atr

using namespace atr;

extern "C" int atr_gru_cell_forward(const float *ig0, const float *ig1, const float *hg, const float *bhh0, const float *bhh1,
                                    const float *h_prev, long long h_prev_pstride, const float *keep, const unsigned char *done,
                                    float *h_out, long long h_pstride, float *acts, long long acts_pstride, int P, int N, int R,
                                    void *stream)
{
    if (!ig0 || !hg || !bhh0 || !h_prev || !h_out || P < 1 || P > 2 || (P == 2 && (!ig1 || !bhh1)) || N < 0 || R <= 0 || (R & 3))
        return -1;
    if (N == 0) return 0;
    GruFwd a;
    a.ig[0] = ig0; a.ig[1] = ig1; a.hg = hg; a.bhh[0] = bhh0; a.bhh[1] = bhh1; a.h_prev = h_prev; a.h_prev_ps = h_prev_pstride;
    a.keep = keep; a.done = done; a.h_out = h_out; a.h_ps = h_pstride; a.acts = acts; a.acts_ps = acts_pstride;
    a.P = P; a.N = N; a.R = R;
    hipLaunchKernelGGL(k_gru_cell_fwd, dim3(gru_grid_for((long long)P * N * (R / 4))), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int atr_gru_cell_backward(const float *dh_out, long long dh_pstride, float *dh_carry, const float *keep_out,
                                     const float *keep_in, const float *acts, long long acts_pstride, const float *h_prev,
                                     long long h_prev_pstride, float *dg, long long dg_pstride, int has_next, int P, int N,
                                     int R, void *stream)
{
    if (!dh_out || !dh_carry || !acts || !h_prev || !dg || P < 1 || P > 2 || N < 0 || R <= 0 || (R & 3)) return -1;
    if (N == 0) return 0;
    GruBwd a;
    a.dh_out = dh_out; a.dh_ps = dh_pstride; a.dh_carry = dh_carry; a.keep_out = keep_out; a.keep_in = keep_in; a.acts = acts;
    a.acts_ps = acts_pstride; a.h_prev = h_prev; a.h_prev_ps = h_prev_pstride; a.dg = dg; a.dg_ps = dg_pstride;
    a.has_next = has_next; a.P = P; a.N = N; a.R = R;
    hipLaunchKernelGGL(k_gru_cell_bwd, dim3(gru_grid_for((long long)P * N * (R / 4))), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

static int gru_bptt_launch(const float *dh0_heads, const float *dh1_heads, const float *keep, const float *acts,
                           long long acts_pstride, const float *h_all, long long h_pstride, const float *whh0,
                           const float *whh1, float *dg, long long dg_pstride, float *dh_init, int emb_player,
                           const long long *act_tracker, long long act_tstride, float *act_sums, int P, int T, int N, int R,
                           void *stream)
{
    if (!keep || !acts || !h_all || !whh0 || !dg || !dh_init || P < 1 || P > 2 || (P == 2 && !whh1) || T < 1 || N < 1 || R != kGR)
        return -1;
    GruBptt a;
    a.dh[0] = dh0_heads; a.dh[1] = dh1_heads; a.keep = keep; a.acts = acts; a.acts_ps = acts_pstride; a.h_all = h_all;
    a.h_ps = h_pstride; a.whh[0] = whh0; a.whh[1] = whh1; a.dg = dg; a.dg_ps = dg_pstride; a.dh0 = dh_init;
    a.act = act_tracker; a.act_ts = act_tstride; a.emb_player = emb_player; a.act_sums = act_sums;
    a.P = P; a.T = T; a.N = N;
    const size_t lds = (size_t)2 * kGRows * kGLd * sizeof(float);          // 49 664 bytes: under the 64 KB default limit
    const unsigned grid = (unsigned)(P * ((N + kGRows - 1) / kGRows));
    if (act_sums) hipLaunchKernelGGL(k_gru_bptt<true>, dim3(grid), dim3(512), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_gru_bptt<false>, dim3(grid), dim3(512), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int atr_gru_bptt(const float *dh0_heads, const float *dh1_heads, const float *keep, const float *acts,
                            long long acts_pstride, const float *h_all, long long h_pstride, const float *whh0,
                            const float *whh1, float *dg, long long dg_pstride, float *dh_init, int P, int T, int N, int R,
                            void *stream)
{
    return gru_bptt_launch(dh0_heads, dh1_heads, keep, acts, acts_pstride, h_all, h_pstride, whh0, whh1, dg, dg_pstride, dh_init,
                           -1, nullptr, 0, nullptr, P, T, N, R, stream);
}

extern "C" long long atr_gru_bptt_act_sums_floats(int N) { return (long long)((N + kGRows - 1) / kGRows) * 4 * kGK; }

extern "C" int atr_gru_bptt_sums(const float *dh0_heads, const float *dh1_heads, const float *keep, const float *acts,
                                 long long acts_pstride, const float *h_all, long long h_pstride, const float *whh0,
                                 const float *whh1, float *dg, long long dg_pstride, float *dh_init, int emb_player, int n_act,
                                 const long long *act_tracker, long long act_tstride, float *act_sums, int P, int T, int N, int R,
                                 void *stream)
{
    // (the by-action sums are built for the four-move action table)
    if (!act_sums || !act_tracker || n_act != 4 || emb_player < 0 || emb_player >= P) return -1;
    return gru_bptt_launch(dh0_heads, dh1_heads, keep, acts, acts_pstride, h_all, h_pstride, whh0, whh1, dg, dg_pstride, dh_init,
                           emb_player, act_tracker, act_tstride, act_sums, P, T, N, R, stream);
}
