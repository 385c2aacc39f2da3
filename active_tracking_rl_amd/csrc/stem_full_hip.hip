// stem_full_hip.hip — CNN_maze's conv stem on whole-map ('Full') frames, side S = 81 or 82 (include/atr_stem_full.h):
//
//     z1 = relu(conv(1 -> 16, k3, s2, p1)(x))  [16, 41, 41]       y = relu(conv(16 -> 32, k3, s2, p1)(z1))  [32, 21, 21]
//
// The unit of work is a BAND: 7 of a frame's 21 conv2 output rows (3 bands per frame). A band p0 .. p0+6 reads z1 rows
// 2 p0 - 1 .. 2 p0 + 13 (15 rows) and those read frame rows 4 p0 - 3 .. 4 p0 + 27 (31 rows). A workgroup walks bands with a
// grid stride; per band it
//   1. stages the 31 frame rows in LDS with a one-cell zero halo (rows / columns outside the frame are zero: for S = 81 the
//      last tap of z1 row / column 40 is padding, for S = 82 it is the real cell 81 — the only difference between the sides),
//   2. evaluates conv1 + ReLU on the VALU into LDS, halo included (z1 rows -1 and 41, columns -1 and 41 are zero); z1 never
//      goes to memory, and the backward recomputes it (and takes its ReLU mask from the recomputed value),
//   3. runs conv2 (forward) or its two backward products as implicit GEMMs on v_mfma_f32_16x16x4_f32 — exact f32 fma chains.
//
// LDS budget (floats): frame rows 31 x 84 = 2604, z1 16 x 15 x 43 = 10320, and in the backward g = dy * (y > 0) for the band's
// 7 rows plus the one below, 32 x 8 x 21 = 5376.
//   forward   12924 floats = 51.7 KB static            -> three workgroups per CU (160 KB)
//   backward  18300 floats = 73.2 KB dynamic (> 64 KB) -> two workgroups per CU; the attribute is set once, at the first call
// The z1 channel stride 645 is odd, so the two channels one half-wave of an MFMA operand read touch even and odd banks.
//
// MFMA operand maps (16x16x4, lane l, i = l & 15, g = l >> 4): a = A[i][k = g], b = B[k = g][i], d[r] = D[4 g + r][i]. The K
// order of a product is free as long as A and B agree, so every K here runs (tap-major, channel-minor): the channel quad and
// the tap of a k-step are compile-time constants and a lane's LDS address is one base plus a constant.
#include <hip/hip_runtime.h>
#include "../../include/atr_stem_full.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kH1 = 41, kH2 = 21;                  // z1 and y side
constexpr int kBand = 7, kBands = 3;               // conv2 rows per band, bands per frame
constexpr int kZR = 2 * kBand + 1, kZW = 43;       // z1 rows per band, row length with halo
constexpr int kZC = kZR * kZW;                     // z1 channel stride (645)
constexpr int kXR = 4 * kBand + 3, kXW = 84;       // frame rows per band, row length (column c holds frame column c - 1)
constexpr int kPos = kBand * kH2;                  // conv2 positions per band (147)
constexpr int kYF = 32 * kH2 * kH2;                // floats of y per frame (14112)
constexpr int kGR = kBand + 1, kGC = kGR * kH2;    // rows and channel stride of the backward's g tile (8, 168)
constexpr int kFwdThreads = 640, kBwdThreads = 384;
constexpr int kFwdPerCu = 3, kBwdPerCu = 2;
constexpr int kRecord = 4800;                      // dw2 4608 | db2 32 | dw1 144 | db1 16
constexpr int kOffDb2 = 4608, kOffDw1 = 4640, kOffDb1 = 4784;
constexpr int kFwdLds = kXR * kXW + 16 * kZC;      // 12924 floats
constexpr int kBwdLds = kFwdLds + 32 * kGC;        // 18300 floats

// frame rows 4 p0 - 3 .. 4 p0 + 27 into xs [31][84], zero outside the frame
template <int NT>
__device__ __forceinline__ void load_frame_rows(const float *__restrict__ xf, int S, int p0, float *xs, int tid)
{
    const int r0 = 4 * p0 - 3;
    for (int i = tid; i < kXR * kXW; i += NT) {
        const int rr = i / kXW, cc = i - rr * kXW;
        const int gy = r0 + rr, gx = cc - 1;
        float v = 0.f;
        if (gy >= 0 && gy < S && gx >= 0 && gx < S) v = xf[gy * S + gx];
        xs[i] = v;
    }
}

// z1 rows 2 p0 - 1 .. 2 p0 + 13 with halo into z1 [16][15][43]: four channels at a time, their 36 weights wave-uniform
template <int NT>
__device__ __forceinline__ void conv1_band(const float *xs, float *z1, const float *__restrict__ w1,
                                           const float *__restrict__ b1, int p0, int tid)
{
    const int q0 = 2 * p0 - 1;
#pragma unroll 1
    for (int cq = 0; cq < 4; cq++) {
        float w[4][9], b[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            b[j] = b1[cq * 4 + j];
#pragma unroll
            for (int t = 0; t < 9; t++) w[j][t] = w1[(cq * 4 + j) * 9 + t];
        }
        for (int cell = tid; cell < kZC; cell += NT) {
            const int r = cell / kZW, cx = cell - r * kZW;
            const int qy = q0 + r, qx = cx - 1;
            const bool ok = qy >= 0 && qy < kH1 && qx >= 0 && qx < kH1;
            float acc[4] = {b[0], b[1], b[2], b[3]};
            if (ok) {
                const float *xp = xs + (2 * r) * kXW + 2 * qx;      // frame row 2 qy - 1 + ky, LDS column 2 qx + kx
#pragma unroll
                for (int ky = 0; ky < 3; ky++)
#pragma unroll
                    for (int kx = 0; kx < 3; kx++) {
                        const float v = xp[ky * kXW + kx];
#pragma unroll
                        for (int j = 0; j < 4; j++) acc[j] = fmaf(w[j][ky * 3 + kx], v, acc[j]);
                    }
            }
#pragma unroll
            for (int j = 0; j < 4; j++) z1[(cq * 4 + j) * kZC + cell] = ok ? fmaxf(acc[j], 0.f) : 0.f;
        }
    }
}

// Forward. Ten waves: wave w owns the 16 output channels of half w & 1 (A = w2 rows, 36 k-steps of its fragment in registers for
// the whole launch) and the position tiles w >> 1 and (w >> 1) + 5 of the band's ten (B = z1 patches from LDS).
__global__ __launch_bounds__(kFwdThreads) void k_stem_full_fwd(const float *__restrict__ x, long long xs_stride, int S,
                                                               const float *__restrict__ w1, const float *__restrict__ b1,
                                                               const float *__restrict__ w2, const float *__restrict__ b2,
                                                               float *__restrict__ y, long long M)
{
    __shared__ float lds[kFwdLds];
    float *xs = lds, *z1 = lds + kXR * kXW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i16 = lane & 15;
    const int mt = wave & 1, nt0 = wave >> 1;
    float wa[36];                                    // A[co = 16 mt + i16][k-step tap * 4 + cq: channel 4 cq + g, tap]
#pragma unroll
    for (int tap = 0; tap < 9; tap++)
#pragma unroll
        for (int cq = 0; cq < 4; cq++) wa[tap * 4 + cq] = w2[(mt * 16 + i16) * 144 + (cq * 4 + g) * 9 + tap];
    float bias[4];
#pragma unroll
    for (int r = 0; r < 4; r++) bias[r] = b2[mt * 16 + g * 4 + r];
    const int pos_a = nt0 * 16 + i16, pos_b = pos_a + 80;         // pos_a <= 79 < 147 always
    const int pc_b = pos_b < kPos ? pos_b : kPos - 1;
    const int base_a = g * kZC + 2 * (pos_a / kH2) * kZW + 2 * (pos_a % kH2);
    const int base_b = g * kZC + 2 * (pc_b / kH2) * kZW + 2 * (pc_b % kH2);
    for (long long item = blockIdx.x; item < kBands * M; item += gridDim.x) {
        const long long m = item / kBands;
        const int p0 = (int)(item - m * kBands) * kBand;
        load_frame_rows<kFwdThreads>(x + m * xs_stride, S, p0, xs, tid);
        __syncthreads();
        conv1_band<kFwdThreads>(xs, z1, w1, b1, p0, tid);
        __syncthreads();
        f32x4 acc_a = {0.f, 0.f, 0.f, 0.f}, acc_b = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tap = 0; tap < 9; tap++)
#pragma unroll
            for (int cq = 0; cq < 4; cq++) {
                const int off = cq * 4 * kZC + (tap / 3) * kZW + tap % 3;      // z1 row 2 p + ky (band-relative), column 2 q + kx
                acc_a = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[tap * 4 + cq], z1[base_a + off], acc_a, 0, 0, 0);
                acc_b = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[tap * 4 + cq], z1[base_b + off], acc_b, 0, 0, 0);
            }
        float *yo = y + m * kYF + p0 * kH2;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int co = mt * 16 + g * 4 + r;
            yo[co * (kH2 * kH2) + pos_a] = fmaxf(acc_a[r] + bias[r], 0.f);
            if (pos_b < kPos) yo[co * (kH2 * kH2) + pos_b] = fmaxf(acc_b[r] + bias[r], 0.f);
        }
        __syncthreads();                             // the next band's staging overwrites xs / z1
    }
}

// One parity class (PY, PX) of dz1 and what hangs on it. z1 cell (2 a + PY, 2 b + PX) of the band's own rows (a = 0 .. 6 from
// conv2 row p0, b = 0 .. 20 - PX) receives from conv2 position (a + [ky == 0], b + [kx == 0]) through tap (ky, kx), with
// ky = 1 for PY = 0 and ky in {0, 2} for PY = 1 (kx alike): 1, 2 or 4 taps, each a product over the 32 output channels — a
// dense gather, no scatter. As a GEMM: D[position][c] = sum_k A[position][k] B[k][c], k = (tap, co); A = g from LDS, B = w2 from
// the registers wz (8 k-steps per tap). The lane then holds channel c = i16 of four cells: masked by the recomputed z1 > 0 they
// go straight into its dw1 / db1 accumulators (acc1[0..8] taps, acc1[9] bias).
template <int PY, int PX>
__device__ __forceinline__ void dz1_class(const float *xs, const float *z1, const float *gm, const float *wz, float *acc1,
                                          int p0, int wave, int g, int i16)
{
    constexpr int NB = kH2 - PX, NPOS = kBand * NB, TILES = (NPOS + 15) / 16, NTY = 1 + PY, NTX = 1 + PX;
    for (int tile = wave; tile < TILES; tile += kBwdThreads / 64) {
        const int pos = tile * 16 + i16, pc = pos < NPOS ? pos : NPOS - 1;
        const int a_base = g * kGC + (pc / NB) * kH2 + pc % NB;
        f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ty = 0; ty < NTY; ty++)
#pragma unroll
            for (int tx = 0; tx < NTX; tx++) {
                const int ky = PY ? 2 * ty : 1, kx = PX ? 2 * tx : 1;
                const int off = (ky == 0 ? kH2 : 0) + (kx == 0 ? 1 : 0);
#pragma unroll
                for (int coq = 0; coq < 8; coq++)
                    d = __builtin_amdgcn_mfma_f32_16x16x4f32(gm[a_base + coq * 4 * kGC + off], wz[(ty * NTX + tx) * 8 + coq], d,
                                                             0, 0, 0);
            }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int po = tile * 16 + g * 4 + r;
            if (po < NPOS) {
                const int a = po / NB, b = po - a * NB;
                const int qx = 2 * b + PX;
                const bool row_ok = 2 * (p0 + a) + PY < kH1;                     // z1 row 41 (last band, PY = 1) does not exist
                const float z = z1[i16 * kZC + (2 * a + PY + 1) * kZW + qx + 1];
                if (row_ok && z > 0.f) {
                    const float v = d[r];
                    const float *xp = xs + (4 * a + 2 * PY + 2) * kXW + 2 * qx;  // frame row 2 qy - 1 + ky, LDS column 2 qx + kx
                    acc1[9] += v;
#pragma unroll
                    for (int ky = 0; ky < 3; ky++)
#pragma unroll
                        for (int kx = 0; kx < 3; kx++) acc1[ky * 3 + kx] = fmaf(v, xp[ky * kXW + kx], acc1[ky * 3 + kx]);
                }
            }
        }
    }
}

// w2 fragments of one parity class into wz: B[k = (tap, co = 4 coq + g)][c = i16] = w2[co][c][ky][kx]
template <int PY, int PX>
__device__ __forceinline__ void dz1_weights(const float *__restrict__ w2, float *wz, int g, int i16)
{
    constexpr int NTY = 1 + PY, NTX = 1 + PX;
#pragma unroll
    for (int ty = 0; ty < NTY; ty++)
#pragma unroll
        for (int tx = 0; tx < NTX; tx++) {
            const int ky = PY ? 2 * ty : 1, kx = PX ? 2 * tx : 1;
#pragma unroll
            for (int coq = 0; coq < 8; coq++) wz[(ty * NTX + tx) * 8 + coq] = w2[(coq * 4 + g) * 144 + i16 * 9 + ky * 3 + kx];
        }
}

// Backward. Six waves. Per band: g = dy * (y > 0) of conv2 rows p0 .. p0 + 7 into LDS (rows past 20 zero); db2 on the VALU;
// dW2 [32, 144] += g [32, positions] z1patch [positions, 144] on the matrix cores (wave w: output-channel half w & 1, column
// tiles 3 (w >> 1) .. + 2, K = the band's 147 positions in 37 k-steps, accumulators live for the whole launch); dz1 by parity
// class (dz1_class) into dw1 / db1. At the end every workgroup writes one record; k_stem_full_reduce adds them in index order.
__global__ __launch_bounds__(kBwdThreads) void k_stem_full_bwd(const float *__restrict__ x, long long xs_stride, int S,
                                                               const float *__restrict__ y, const float *__restrict__ dy,
                                                               const float *__restrict__ w1, const float *__restrict__ b1,
                                                               const float *__restrict__ w2, float *__restrict__ ws, long long M)
{
    extern __shared__ float lds[];
    float *xs = lds, *z1 = lds + kXR * kXW, *gm = lds + kFwdLds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i16 = lane & 15;
    const int mt = wave & 1, ng = wave >> 1;
    float wz00[8], wz01[16], wz10[16], wz11[32];
    dz1_weights<0, 0>(w2, wz00, g, i16);
    dz1_weights<0, 1>(w2, wz01, g, i16);
    dz1_weights<1, 0>(w2, wz10, g, i16);
    dz1_weights<1, 1>(w2, wz11, g, i16);
    int col_off[3];                                  // dW2 column 16 nt + i16 = ci * 9 + tap -> its z1 offset
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int col = (ng * 3 + j) * 16 + i16, ci = col / 9, tap = col - ci * 9;
        col_off[j] = ci * kZC + (tap / 3) * kZW + tap % 3;
    }
    f32x4 acc2[3];
#pragma unroll
    for (int j = 0; j < 3; j++) acc2[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float acc1[10];
#pragma unroll
    for (int j = 0; j < 10; j++) acc1[j] = 0.f;
    float acc_b2 = 0.f;
    const int co_b2 = tid / 12, j_b2 = tid - co_b2 * 12;          // db2: 12 threads per output channel
    for (long long item = blockIdx.x; item < kBands * M; item += gridDim.x) {
        const long long m = item / kBands;
        const int p0 = (int)(item - m * kBands) * kBand;
        load_frame_rows<kBwdThreads>(x + m * xs_stride, S, p0, xs, tid);
        {
            const float *yf = y + m * kYF, *df = dy + m * kYF;
            for (int i = tid; i < 32 * kGC; i += kBwdThreads) {
                const int co = i / kGC, rem = i - co * kGC, at = p0 * kH2 + rem;
                float v = 0.f;
                if (at < kH2 * kH2) {
                    const int idx = co * (kH2 * kH2) + at;
                    v = yf[idx] > 0.f ? df[idx] : 0.f;
                }
                gm[i] = v;
            }
        }
        __syncthreads();
        conv1_band<kBwdThreads>(xs, z1, w1, b1, p0, tid);
        __syncthreads();
        for (int pos = j_b2; pos < kPos; pos += 12) acc_b2 += gm[co_b2 * kGC + pos];
#pragma unroll 1
        for (int ks = 0; ks < (kPos + 3) / 4; ks++) {
            const int pos = ks * 4 + g, pc = pos < kPos ? pos : kPos - 1;
            const int p = pc / kH2, q = pc - p * kH2;
            const int zb = 2 * p * kZW + 2 * q;
            const float a = pos < kPos ? gm[(mt * 16 + i16) * kGC + pos] : 0.f;
#pragma unroll
            for (int j = 0; j < 3; j++) acc2[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, z1[col_off[j] + zb], acc2[j], 0, 0, 0);
        }
        dz1_class<0, 0>(xs, z1, gm, wz00, acc1, p0, wave, g, i16);
        dz1_class<0, 1>(xs, z1, gm, wz01, acc1, p0, wave, g, i16);
        dz1_class<1, 0>(xs, z1, gm, wz10, acc1, p0, wave, g, i16);
        dz1_class<1, 1>(xs, z1, gm, wz11, acc1, p0, wave, g, i16);
        __syncthreads();                             // the next band's staging (and the reduction below) overwrites the LDS
    }
    float *rec = ws + (long long)blockIdx.x * kRecord;
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) rec[(mt * 16 + g * 4 + r) * 144 + (ng * 3 + j) * 16 + i16] = acc2[j][r];
    // the workgroup's db2 (12 addends per channel) and dw1 / db1 (24 per value: the lanes with the same i16), in index order
    float *red = lds;
    red[tid] = acc_b2;
#pragma unroll
    for (int j = 0; j < 10; j++) red[kBwdThreads + j * kBwdThreads + tid] = acc1[j];
    __syncthreads();
    if (tid < 32) {
        float s = 0.f;
        for (int j = 0; j < 12; j++) s += red[tid * 12 + j];
        rec[kOffDb2 + tid] = s;
    } else if (tid >= 64 && tid < 64 + 160) {
        const int o = tid - 64, c = o / 10, v = o - c * 10;
        float s = 0.f;
        for (int j = 0; j < kBwdThreads / 16; j++) s += red[kBwdThreads + v * kBwdThreads + j * 16 + c];
        rec[v < 9 ? kOffDw1 + c * 9 + v : kOffDb1 + c] = s;
    }
}

__global__ __launch_bounds__(256) void k_stem_full_reduce(const float *__restrict__ ws, int records, float *__restrict__ dw1,
                                                          float *__restrict__ db1, float *__restrict__ dw2,
                                                          float *__restrict__ db2)
{
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= kRecord) return;
    float s = 0.f;
    for (int r = 0; r < records; r++) s += ws[(long long)r * kRecord + o];
    if (o < kOffDb2) dw2[o] = s;
    else if (o < kOffDw1) db2[o - kOffDb2] = s;
    else if (o < kOffDb1) dw1[o - kOffDw1] = s;
    else db1[o - kOffDb1] = s;
}

int compute_units()
{
    static int cached = 0;      // queried once: far too slow for a per-launch call
    if (cached == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached = n;
    }
    return cached;
}

int full_grid(long long M, int per_cu)
{
    const long long cap = (long long)compute_units() * per_cu;
    const long long need = M > cap ? cap : kBands * M;
    return (int)(need < 1 ? 1 : (need < cap ? need : cap));
}

bool full_init()
{
    static bool done = false;
    if (!done) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_stem_full_bwd), hipFuncAttributeMaxDynamicSharedMemorySize,
                                kBwdLds * (int)sizeof(float)) != hipSuccess)
            return false;
        done = true;
    }
    return true;
}

} // namespace

extern "C" int atr_stem_full_forward(const float *x, long long x_stride, int S, const float *w1, const float *b1, const float *w2,
                                     const float *b2, float *y, long long M, void *stream)
{
    if (!x || !w1 || !b1 || !w2 || !b2 || !y || M < 0 || (S != 81 && S != 82) || x_stride < (long long)S * S) return -1;
    if (M == 0) return 0;
    if (!full_init()) return -2;
    hipLaunchKernelGGL(k_stem_full_fwd, dim3((unsigned)full_grid(M, kFwdPerCu)), dim3(kFwdThreads), 0, (hipStream_t)stream, x,
                       x_stride, S, w1, b1, w2, b2, y, M);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" long long atr_stem_full_workspace_floats(long long M)
{
    full_init();
    return (long long)full_grid(M, kBwdPerCu) * kRecord;
}

extern "C" int atr_stem_full_backward(const float *x, long long x_stride, int S, const float *y, const float *dy, const float *w1,
                                      const float *b1, const float *w2, float *dw1, float *db1, float *dw2, float *db2,
                                      float *workspace, long long M, void *stream)
{
    if (!x || !y || !dy || !w1 || !b1 || !w2 || !dw1 || !db1 || !dw2 || !db2 || !workspace || M < 0 || (S != 81 && S != 82) ||
        x_stride < (long long)S * S)
        return -1;
    if (M == 0) return 0;
    if (!full_init()) return -2;
    const int grid = full_grid(M, kBwdPerCu);
    hipLaunchKernelGGL(k_stem_full_bwd, dim3((unsigned)grid), dim3(kBwdThreads), kBwdLds * sizeof(float), (hipStream_t)stream, x,
                       x_stride, S, y, dy, w1, b1, w2, workspace, M);
    hipLaunchKernelGGL(k_stem_full_reduce, dim3((kRecord + 255) / 256), dim3(256), 0, (hipStream_t)stream, workspace, grid, dw1,
                       db1, dw2, db2);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
