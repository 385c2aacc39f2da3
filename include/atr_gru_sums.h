/*
 * atr_gru_sums.h — the GRU learner's entry points of csrc/gru_hip.hip, next to atr_gru_bptt (include/atr_gru.h, which includes
 * this header; conventions as there: device pointers to float32, `*_pstride` in floats, 0 / -1 / -2 returned).
 */
#ifndef ATR_GRU_SUMS_H
#define ATR_GRU_SUMS_H

#ifdef __cplusplus
extern "C" {
#endif

/* atr_gru_bptt with one more output, for the tracker-aware target ('tat-maze-gru': its features are f + E[a_tracker], E[a] =
 * fc_action_tracker(one_hot(a))): act_sums — atr_gru_bptt_act_sums_floats(N) floats, [row tiles of 16][4][3R]: per row tile of
 * player emb_player (0 <= emb_player < P), the column sums over the tile's real rows and all T steps of dG's INPUT-side columns
 * (dr_pre, dz_pre, dn_pre) = dG[..., 0:3R], grouped by the tracker's action of the row, act_tracker[t * act_tstride + n]
 * (int64: the rollout's action store, read in place; a value outside 0..3 is counted nowhere). n_act must be 4 (the four-move
 * action table). Every tile writes all of its 4 x 3R floats. dg and dh_init are bit-identical to atr_gru_bptt's.
 * With S [4][3R] = the sum of act_sums over the tiles, S[a] = sum over the rows with action a of dG[row, 0:3R], and E [4][F]:
 *     dW_ih [3R, F]                 = dG[:, 0:3R]^T (f + E[a]) = dG[:, 0:3R]^T f + S^T E     (f = the RAW fc features)
 *     d fc_action_tracker.weight    = (S W_ih)^T  [F, 4],   d fc_action_tracker.bias = its row sums
 * which is what atr_embed_fold (include/atr_policy.h) computes from act_sums with J = 3R — the learner then neither
 * materialises f + E[a] nor gathers dL/df by action. The q column (dG[..., 3R:4R]) takes no part: it is hidden-side only. */
long long atr_gru_bptt_act_sums_floats(int N);
int atr_gru_bptt_sums(const float *dh0_heads, const float *dh1_heads, const float *keep, const float *acts,
                      long long acts_pstride, const float *h_all, long long h_pstride, const float *whh0, const float *whh1,
                      float *dg, long long dg_pstride, float *dh_init, int emb_player, int n_act, const long long *act_tracker,
                      long long act_tstride, float *act_sums, int P, int T, int N, int R, void *stream);

#ifdef __cplusplus
}
#endif

#endif
