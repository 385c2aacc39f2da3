/*
 * atr_gru_step.h — C ABI of the GRU cores' fused rollout step in libtrack2d_hip.so (csrc/track2d_hip.hip: k_gru_step): the END
 * of a rollout step as ONE launch for the 'maze-gru' / 'tat-maze-gru' networks — atr_act_env_step (include/atr_policy.h) and
 * atr_eval_act_env_step (include/atr_eval.h) with torch.nn.GRUCell (include/atr_gru.h: gate order r, z, n) in place of
 * nn.LSTMCell. OPT-IN (main.py / gym_eval.py --fused-gru, ATR_FUSED_GRU=1); without the switch the GRU nets never reach it.
 * It is a header of its own because include/atr_gru.h is the ABI of the path without a rollout cache, held function for
 * function to csrc/gru_hip.hip.
 *
 * nn.GRUCell's two products become ONE 4R-wide product over the rows [features | k h_prev] (K = F + R) the LSTM's one-GEMM
 * step keeps, against a block weight per player:
 *
 *     W4 [4R, F + R] = [ W_ir | W_hr ]  -> r_pre          b4 [4R] = (b_ir + b_hr, b_iz + b_hz, b_in, b_hn)
 *                      [ W_iz | W_hz ]  -> z_pre          E4 [A, 4R] = ((fa.weight^T + fa.bias) W_ih^T | 0)   (tat only:
 *                      [ W_in |  0   ]  -> ig_n                        row a = fc_action_tracker(one_hot(a)) through W_ih)
 *                      [  0   | W_hn ]  -> k hg_n         (the episode mask k is already in the rows)
 *
 * The struct is atr_act_step, read as follows: ig[p] [N, 4R] = rows W4[p]^T (no bias), bias[p] = b4[p] (required), emb = E4
 * (nullable), hg must be NULL, c_prev / c_out / done_prev are not read (a GRU has no cell state and the mask is in the rows);
 * h_out[p] [N, R]; acts[p] (nullable) [N, 4R] receives (r, z, n, q) — the store atr_gru_bptt reads; actor_w / actor_b /
 * actions_out / counter / seed / ordinal / A / N / R / hm_out / hm_ld as for atr_act_env_step (same draw key: row, *counter,
 * ordinal + p). Per player, tracker first:
 *     r = sigmoid(g_r + b),  z = sigmoid(g_z + b),  q = g_q + b_hn,  n = tanh(g_n + b_in [+ E4[a_tracker]] + r q),
 *     h' = (1 - z) n + z (k h_prev)
 * h_prev0 / h_prev1: the masked previous hidden rows k h_prev [N, R] (16-byte aligned, row stride h_prev_ld floats >= R, a
 * multiple of 4): columns F : F + R of this step's rows. Then the actor heads, the draws (or the first maximal logit), the env
 * step and hm_out exactly as the LSTM forms do them. R must be 128, A 4 or 8.
 */
#ifndef ATR_GRU_STEP_H
#define ATR_GRU_STEP_H

#include "atr_eval.h"

#ifdef __cplusplus
extern "C" {
#endif

/* env == NULL: the policy half alone (the learner's bootstrap step; hm_out must be NULL). Returns 0 or a T2D_ERR_* code
 * (t2d_last_error). */
int atr_gru_act_env_step(struct t2d_handle *env, const atr_act_step *args, const float *h_prev0, const float *h_prev1,
                         long long h_prev_ld, void *obs, int obs_is_u8, float *rew, unsigned char *done, void *stream);

/* The evaluation form: the first maximal logit instead of the draw (args->counter is not read) and the accounts of
 * atr_eval_act_env_step, kept bit for bit as that entry keeps them. env must not be NULL. */
int atr_gru_eval_act_env_step(struct t2d_handle *env, const atr_act_step *args, const float *h_prev0, const float *h_prev1,
                              long long h_prev_ld, const atr_eval_out *out, void *obs, int obs_is_u8, float *rew,
                              unsigned char *done, void *stream);

#ifdef __cplusplus
}
#endif

#endif
