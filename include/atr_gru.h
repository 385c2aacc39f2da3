/*
 * atr_gru.h — C ABI of the GRU recurrent core in libtrack2d_hip.so (csrc/gru_hip.hip): torch.nn.GRUCell(F, R) as the
 * reference's 'maze-gru' / 'tat-maze-gru' networks use it (model.py:120-124, 139-141 of the reference), for P in {1, 2}
 * players at once, on the path that keeps no rollout cache (model.A3C_Dueling.act, model.gru_sequence). Gate order (r, z, n):
 *
 *     r  = sigmoid(ig_r + k hg_r + b_hr)          ig = x W_ih^T + b_ih   [N, 3R]  (the caller's GEMM, b_ih included)
 *     z  = sigmoid(ig_z + k hg_z + b_hz)          hg = h_prev W_hh^T     [N, 3R]  (the caller's GEMM on the UN-masked h_prev)
 *     q  =           k hg_n + b_hn                k  = the previous step's episode mask (1: the episode goes on): row scaling
 *     n  = tanh(ig_n + r q)                            commutes with the GEMM, k (h W) == (k h) W; b_hh is added after the mask
 *     h' = (1 - z) n + z (k h_prev)
 *
 * The step's backward store is acts [N, 4R] = (r, z, n, q). Gradients come as dG [N, 4R] = (dr_pre, dz_pre, dn_pre, dn_pre r):
 * columns 0:3R are dL/d ig (their column sum is d b_ih); columns 0:2R and 3R:4R are dL/d(hidden pre-activations) (their column
 * sum is d b_hh, and they are the left operand of dW_hh and of the gradient into h_prev). The 4R-wide rows keep every stride
 * what the LSTM's stores have (include/atr_policy.h: atr_lstm_cell_backward, atr_lstm_bptt).
 * All pointers are device pointers to float32 (16-byte aligned, rows contiguous); `*_pstride` is the distance in floats between
 * the two players' blocks; `stream` is a hipStream_t. Every function returns 0, -1 (bad arguments) or -2 (launch failed).
 */
#ifndef ATR_GRU_H
#define ATR_GRU_H

#ifdef __cplusplus
extern "C" {
#endif

/* One step forward. ig0 / ig1 per player [N, 3R] (ig1 NULL when P == 1); hg [P, N, 3R]; bhh0 / bhh1 per player [3R];
 * h_prev + p * h_prev_pstride [N, R]; keep [N] float or done [N] uint8 of the PREVIOUS step (both nullable: k = 1; keep wins);
 * h_out + p * h_pstride [N, R]; acts (nullable) + p * acts_pstride [N, 4R]. R % 4 == 0. */
int atr_gru_cell_forward(const float *ig0, const float *ig1, const float *hg, const float *bhh0, const float *bhh1,
                         const float *h_prev, long long h_prev_pstride, const float *keep, const unsigned char *done,
                         float *h_out, long long h_pstride, float *acts, long long acts_pstride, int P, int N, int R,
                         void *stream);

/* One step of back-propagation through time (the per-step path). dh_out + p * dh_pstride [N, R]: dL/dh_t from the heads;
 * dh_carry [P, N, R], in (read when has_next): the gradient step t + 1 sends into k_t h_t (its dG W_hh + its direct part),
 * UN-masked — keep_out [N] (nullable: 1) = k_t is applied here; out: this step's direct part dh_t z_t, to which the caller adds
 * dG_t[:, hidden columns] W_hh. keep_in [N] (nullable: 1) = k_{t-1}, the mask on h_prev. acts + p * acts_pstride [N, 4R];
 * h_prev + p * h_prev_pstride [N, R] (un-masked); dg + p * dg_pstride [N, 4R] (out). R % 4 == 0. */
int atr_gru_cell_backward(const float *dh_out, long long dh_pstride, float *dh_carry, const float *keep_out,
                          const float *keep_in, const float *acts, long long acts_pstride, const float *h_prev,
                          long long h_prev_pstride, float *dg, long long dg_pstride, int has_next, int P, int N, int R,
                          void *stream);

/* The whole recurrence backward of a T-step rollout as ONE launch (R == 128). dh0_heads / dh1_heads per player [T, N, R]
 * (nullable: zero); keep [T, N] float; acts + p * acts_pstride [T, N, 4R]; h_all + p * h_pstride [T + 1, N, R] (slot t = the
 * un-masked state step t starts from, slot 0 already masked); whh0 / whh1 per player weight_hh [3R, R] (nn.GRUCell layout;
 * whh1 NULL when P == 1); dg + p * dg_pstride [T, N, 4R] (out); dh_init [P, N, R] (out): dL/dh of slot 0. */
int atr_gru_bptt(const float *dh0_heads, const float *dh1_heads, const float *keep, const float *acts, long long acts_pstride,
                 const float *h_all, long long h_pstride, const float *whh0, const float *whh1, float *dg,
                 long long dg_pstride, float *dh_init, int P, int T, int N, int R, void *stream);

/* atr_gru_bptt with the by-action column sums of dG the tracker-action embedding's fold needs (atr_gru_bptt_sums,
 * atr_gru_bptt_act_sums_floats): declared in atr_gru_sums.h, which this header brings along. */
#include "atr_gru_sums.h"

#ifdef __cplusplus
}
#endif

#endif
