/*
 * atr_eval.h — C ABI of the evaluator's step in libtrack2d_hip.so: the rollout step's last launch (atr_act_env_step,
 * include/atr_policy.h) in its evaluation form. One launch per env step does what test.py:16-136 of the reference does per
 * step of an evaluation episode, for N envs at once:
 *   - both players' LSTM cells and actor heads exactly as atr_act_env_step evaluates them (same expressions, same lanes, same
 *     butterfly: h_out / c_out / hm_out are bit-identical), with the GREEDY action in place of the categorical draw: the lowest
 *     index among the maximal logits (prob.max(1)[1], model.py:45-46 of the reference, taken on the logits). No Philox, and
 *     args->counter is not read (it may be NULL). The tracker's greedy action feeds the tracker-aware target's embedding row
 *     as the drawn one does;
 *   - the env step + observation with those actions (in-launch auto-reset and generator schedule unchanged: an env that has
 *     finished its first episode keeps stepping);
 *   - the episode accounting, per env e, with the step's reward and done flag still in registers:
 *         rsum[e][p] += alive[e] ? rew[e][p] : 0      (float32, in step order)
 *         length[e]  += alive[e]
 *         alive[e]   &= !done[e]
 *     The caller zeroes rsum / length and sets alive to 1 before the first step of a round.
 * All pointers are device pointers; `stream` is a hipStream_t.
 */
#ifndef ATR_EVAL_H
#define ATR_EVAL_H

#include "atr_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rsum float32 [N,2] (8-byte aligned), length int32 [N], alive uint8 [N] */
typedef struct atr_eval_out {
    float *rsum;
    int *length;
    unsigned char *alive;
} atr_eval_out;

/* Arguments, argument checks and refusals of atr_act_env_step (RPF targets, 'Full' observations, numpy-stream Ram handles,
 * N != the handle's env count), except that env must not be NULL. Returns 0 or a T2D_ERR_* code (t2d_last_error). */
int atr_eval_act_env_step(struct t2d_handle *env, const atr_act_step *args, const atr_eval_out *out, void *obs, int obs_is_u8,
                          float *rew, unsigned char *done, void *stream);

#ifdef __cplusplus
}
#endif

#endif
