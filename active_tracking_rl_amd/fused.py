"""ctypes + autograd bindings of the policy-side HIP kernels (include/atr_policy.h). GPU tensors only — on CPU tensors the
model evaluates the same network with plain PyTorch ops (model.CNN_maze.forward_dense_stem / forward_conv2d, nn.LSTMCell).
The header's ABI is declared once: ATR_STRUCTS (its structs) and ATR_PROTOTYPES (its functions); lib() applies the table and
every launch goes through it, so a launch status other than 0 raises RuntimeError from one place (_errcheck).

  stem / stem_into / stem_into2 / stem_cached   CNN_maze's conv(1->16,k3,s2,p1)+ReLU+conv(16->32,k3,s2,p1)+ReLU on
                                                13x13 frames: one launch forward, two backward (csrc/stem_hip.hip)
  lstm_cell / lstm_cell_into / lstm_cell_act_into, lstm_sequence(_cached)
                                                masked LSTMCell step(s), the actor's cell + head + draw in one launch,
                                                the whole recurrence as one autograd node (csrc/lstm_hip.hip)
  gru_cell, gru_sequence                        the GRU cores' masked GRUCell step and their whole recurrence as one autograd
                                                node, on the path without a rollout cache (include/atr_gru.h, csrc/gru_hip.hip)
  stem_full                                     the same stem on the 'Full' ids' 81 / 82 wide frames (opt-in: --full-stem;
                                                include/atr_stem_full.h, csrc/stem_full_hip.hip)
  ActionSampler                                 actor head + categorical draw (csrc/policy_hip.hip)
  gae_returns, heads_values, heads_loss         returns / GAE, critic values, heads + A3C loss terms with analytic
                                                gradients (csrc/lstm_hip.hip, csrc/heads_hip.hip)
  gemm_tn                                       weight-gradient GEMMs x1^T x2 (+ bias gradient, row mask) on the f32
                                                matrix cores (csrc/gemm_tn_hip.hip)
  linear_relu_cached, lstm_sequence_cached      cached-forward autograd nodes of the rollout cache (model.RolloutCache)"""
import ctypes as C
import json
import os
import re
import sys

import torch

from . import vec_env

_lib = None


class ActStepArgs(C.Structure):
    """atr_act_step of include/atr_policy.h."""
    _fields_ = [("ig", C.c_void_p * 2), ("hg", C.c_void_p * 2), ("bias", C.c_void_p * 2), ("c_prev", C.c_void_p * 2),
                ("h_out", C.c_void_p * 2), ("c_out", C.c_void_p * 2), ("acts", C.c_void_p * 2),
                ("actor_w", C.c_void_p * 2), ("actor_b", C.c_void_p * 2), ("emb", C.c_void_p), ("done_prev", C.c_void_p),
                ("actions_out", C.c_void_p), ("counter", C.c_void_p), ("seed", C.c_ulonglong), ("ordinal", C.c_uint),
                ("A", C.c_int), ("N", C.c_int), ("R", C.c_int), ("hm_out", C.c_void_p * 2), ("hm_ld", C.c_longlong)]


class CoopStepArgs(C.Structure):
    """atr_coop_step of include/atr_policy.h."""
    _fields_ = [("y", C.c_void_p * 2), ("fc_w", C.c_void_p * 2), ("fc_b", C.c_void_p * 2), ("w_cat", C.c_void_p * 2),
                ("ldy", C.c_longlong * 2), ("kfc", C.c_int * 2), ("fh", C.c_void_p), ("gates", C.c_void_p),
                ("fh_pstride", C.c_longlong), ("fh_ld", C.c_longlong), ("F", C.c_int), ("workgroups", C.c_int),
                ("probe", C.c_void_p)]


class LinearArgs(C.Structure):
    """atr_linear_args of include/atr_policy.h."""
    _fields_ = [("a", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("c", C.c_void_p), ("lda", C.c_longlong),
                ("ldw", C.c_longlong), ("ldc", C.c_longlong), ("stride_a", C.c_longlong), ("stride_w", C.c_longlong),
                ("stride_c", C.c_longlong), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("batch", C.c_int),
                ("relu", C.c_int), ("workspace", C.c_void_p), ("workspace_bytes", C.c_longlong)]


class GateCellArgs(C.Structure):
    """atr_gate_cell_args of include/atr_policy.h."""
    _fields_ = [("a", C.c_void_p * 2), ("w", C.c_void_p * 2), ("bias", C.c_void_p * 2), ("pre", C.c_void_p * 2),
                ("c_prev", C.c_void_p * 2), ("h_out", C.c_void_p * 2), ("c_out", C.c_void_p * 2), ("done_prev", C.c_void_p),
                ("lda", C.c_longlong), ("cell", C.c_int * 2), ("N", C.c_int), ("K", C.c_int), ("R", C.c_int), ("probe", C.c_void_p)]


class PairLinearArgs(C.Structure):
    """atr_pair_linear_args of include/atr_policy.h."""
    _fields_ = [("a1", C.c_void_p * 2), ("w1", C.c_void_p * 2), ("a2", C.c_void_p * 2), ("w2", C.c_void_p * 2),
                ("bias", C.c_void_p * 2), ("c", C.c_void_p * 2), ("lda1", C.c_longlong * 2), ("lda2", C.c_longlong * 2),
                ("ldc", C.c_longlong * 2), ("k1", C.c_int * 2), ("k2", C.c_int * 2), ("done", C.c_void_p),
                ("M", C.c_int), ("N", C.c_int), ("relu", C.c_int)]


class HeadsLossArgs(C.Structure):
    """atr_heads_loss_args of include/atr_policy.h."""
    _fields_ = [("h", C.c_void_p), ("actions", C.c_void_p), ("act_n", C.c_longlong), ("act_tstride", C.c_longlong),
                ("ret", C.c_void_p), ("gae", C.c_void_p), ("val", C.c_void_p), ("stride", C.c_int), ("off", C.c_int),
                ("r_aux", C.c_void_p), ("aux_stride", C.c_int), ("aux_off", C.c_int), ("wa", C.c_void_p), ("ba", C.c_void_p),
                ("wc", C.c_void_p), ("waux", C.c_void_p), ("baux", C.c_void_p), ("scale", C.c_float),
                ("scale_aux", C.c_float), ("w_ent", C.c_float), ("dh", C.c_void_p), ("grads_and_sums", C.c_void_p),
                ("workspace", C.c_void_p), ("stats_out", C.c_void_p), ("rows", C.c_longlong), ("R", C.c_int), ("A", C.c_int)]


class GemmTnProblem(C.Structure):
    """atr_gemm_tn_problem of include/atr_policy.h."""
    _fields_ = [("x1", C.c_void_p), ("x2", C.c_void_p), ("c", C.c_void_p), ("row_scale", C.c_void_p),
                ("row_scale_shift", C.c_longlong), ("colsum0", C.c_void_p), ("colsum1", C.c_void_p), ("M", C.c_int),
                ("N", C.c_int), ("ld1", C.c_longlong), ("ld2", C.c_longlong)]


class RolloutConsts(C.Structure):
    """atr_rollout_consts of include/atr_policy.h."""
    _fields_ = [("w_ih", C.c_void_p * 2), ("w_hh", C.c_void_p * 2), ("b_ih", C.c_void_p * 2), ("b_hh", C.c_void_p * 2),
                ("bsum", C.c_void_p), ("w_cat", C.c_void_p), ("fa_w", C.c_void_p), ("fa_b", C.c_void_p), ("emb_ih", C.c_void_p),
                ("counter", C.c_void_p), ("fh0", C.c_void_p), ("fh_pstride", C.c_longlong), ("fh_ld", C.c_longlong),
                ("F", C.c_int), ("A_act", C.c_int)]


ATR_STRUCTS = {"atr_act_step": ActStepArgs, "atr_coop_step": CoopStepArgs, "atr_linear_args": LinearArgs,
               "atr_gate_cell_args": GateCellArgs, "atr_pair_linear_args": PairLinearArgs, "atr_heads_loss_args": HeadsLossArgs,
               "atr_gemm_tn_problem": GemmTnProblem, "atr_rollout_consts": RolloutConsts}
VALUE = "value"     # marks an int result that is not a launch status (or whose non-zero value the caller handles): no errcheck


def _prototypes():
    """{entry point: (restype, [argtypes]) or (restype, [argtypes], VALUE)} for every function include/atr_policy.h declares,
    called from Python or not (tests/test_abi_cpu.py holds the table and the structs above to the header)."""
    vp, cp, ll, i32, u32, u64, f32, f64 = (C.c_void_p, C.c_char_p, C.c_longlong, C.c_int, C.c_uint, C.c_ulonglong, C.c_float,
                                           C.c_double)
    ptr = C.POINTER
    stem_fwd = [vp, ll, vp, vp, vp, vp, vp, ll]                     # one stem problem: x, x_stride, w1, b1, w2, b2, y, M
    stem_bwd = [vp, ll] + [vp] * 10 + [ll, vp]
    draw = [vp, vp, u64, u32, i32, i32, vp]                         # actions_out, counter, seed, ordinal, N, R, stream
    bptt_pre = [vp, vp, vp, vp, ll, vp, vp, vp, i32, i32, vp, ll, vp, ll, vp, vp, vp, ll, vp, vp]
    begin = [vp, vp, vp, vp, ll, vp, vp, ll, i32, i32, i32]
    end = [vp, vp, ll, vp, vp, vp, vp, vp, i32, i32, i32, i32]
    linear = ptr(LinearArgs)
    return {
        "atr_stem_forward": (i32, stem_fwd + [vp]),
        "atr_stem_forward2": (i32, stem_fwd * 2 + [vp]),
        "atr_stem_workspace_floats": (ll, [ll]),
        "atr_stem_backward": (i32, stem_bwd),
        "atr_stem_forward_u8": (i32, stem_fwd + [vp]),
        "atr_stem_forward2_u8": (i32, stem_fwd * 2 + [vp]),
        "atr_stem_backward_u8": (i32, stem_bwd),
        "atr_sample_actions": (i32, [vp, vp, vp, vp, vp, u64, u32, i32, i32, i32, i32, vp]),
        "atr_lstm_cell_forward": (i32, [vp, vp, vp, vp, ll, vp, vp, vp, ll, vp, ll, vp, ll, i32, i32, i32, vp]),
        "atr_lstm_cell_forward_act": (i32, [vp] * 11 + [i32] + draw),
        "atr_lstm_cell_forward_act1": (i32, [vp] * 12 + [i32] + draw),
        "atr_lstm_cell_forward_act2": (i32, [vp] * 5 + [ll, vp, vp, ll, vp, ll, vp, ll] + [vp] * 4 + [i32] + draw),
        "atr_gate_cell": (i32, [ptr(GateCellArgs), vp]),
        "atr_gate_cell_workgroups": (i32, [i32], VALUE),
        "atr_act_env_step": (i32, [vp, ptr(ActStepArgs), vp, i32, vp, vp, vp]),
        "atr_coop_env_step": (i32, [vp, ptr(ActStepArgs), ptr(CoopStepArgs), vp, i32, vp, vp, vp]),
        "atr_lt_init": (i32, [cp], VALUE),                          # (the next candidate path is tried)
        "atr_linear": (i32, [linear, vp]),
        "atr_linear_plan_info": (i32, [linear, ptr(i32), ptr(i32), ptr(i32), ptr(f32), ptr(i32), ptr(i32)], VALUE),
        "atr_linear_set_choice": (i32, [linear, i32, i32], VALUE),  # (ignored in linear_lt, raised in linear_lt_set_choice)
        "atr_lt_library_info": (i32, [ptr(i32), ptr(i32), cp, i32], VALUE),
        "atr_linear_kernel_name": (i32, [linear, cp, i32], VALUE),
        "atr_lt_last_error": (cp, []),
        "atr_pair_linear": (i32, [ptr(PairLinearArgs), vp]),
        "atr_actor_step": (i32, [vp] * 12 + [i32, i32, i32, vp]),
        "atr_lstm_cell_backward": (i32, [vp, ll, vp, vp, vp, vp, vp, ll, vp, ll, vp, ll, vp, ll, i32, i32, i32, i32, vp]),
        "atr_lstm_bptt": (i32, [vp, vp, vp, vp, ll, vp, ll, vp, vp, vp, ll, vp, vp, i32, i32, i32, i32, vp]),
        "atr_lstm_bptt_pre": (i32, bptt_pre + [i32, i32, i32, i32, vp]),
        "atr_lstm_bptt_act_sums_floats": (ll, [i32]),
        "atr_lstm_bptt_pre2": (i32, bptt_pre + [vp, i32, i32, i32, i32, vp]),
        "atr_embed_fold": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]),
        "atr_embed_add": (i32, [vp, vp, vp, vp, ll, ll, ll, vp, ll, i32, i32, vp]),
        "atr_embed_add_ld": (i32, [vp, ll, vp, vp, vp, ll, ll, ll, vp, ll, i32, i32, vp]),
        "atr_relu_backward_ld": (i32, [vp, vp, ll, vp, ll, i32, vp]),
        "atr_embed_grad_workspace_floats": (ll, [ll, i32, i32]),
        "atr_embed_grad": (i32, [vp, vp, ll, ll, ll, vp, vp, vp, ll, i32, i32, vp]),
        "atr_gae_returns": (i32, [vp, vp, vp, f32, f32, vp, vp, i32, i32, i32, vp]),
        "atr_heads_values": (i32, [vp, vp, vp, vp, ll, i32, i32, i32, vp]),
        "atr_heads_values2": (i32, [vp, vp, vp, i32, vp, vp, vp, i32, vp, ll, i32, i32, vp]),
        "atr_heads_workspace_floats": (ll, [ll, i32, i32]),
        "atr_heads_loss": (i32, [vp, vp, vp, vp, vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp, f32, f32, f32, vp, vp, vp, ll,
                                 i32, i32, vp]),
        "atr_heads_loss_multi": (i32, [ptr(HeadsLossArgs), i32, f32, vp]),
        "atr_gemm_tn_workspace_floats": (ll, [ll, i32, i32]),
        "atr_gemm_tn": (i32, [vp, vp, vp, vp, ll, i32, i32, vp, vp, vp]),
        "atr_scatter_segments": (i32, [ptr(vp), ptr(ll), ptr(i32), i32, vp, vp]),
        "atr_gemm_tn_grouped_workspace_floats": (ll, [ptr(GemmTnProblem), i32, ll]),
        "atr_gemm_tn_set_corun": (i32, [i32], VALUE),               # (returns the previous mode)
        "atr_gemm_tn_grouped": (i32, [ptr(GemmTnProblem), i32, ll, vp, vp]),
        "atr_rollout_begin": (i32, begin + [vp]),
        "atr_rollout_begin2": (i32, begin + [ptr(RolloutConsts), vp]),
        "atr_rollout_end": (i32, end + [vp]),
        "atr_rollout_end2": (i32, end + [vp, vp, ll, vp, vp]),
        "atr_adam_step": (i32, [vp] * 7 + [f64] * 5 + [i32, ll, vp]),
        "atr_rmsprop_step": (i32, [vp] * 3 + [f64] * 4 + [ll, vp]),
    }


ATR_PROTOTYPES = _prototypes()
# the GRU core's header, include/atr_gru.h (held to it by tests/test_gru_cpu.py): bound and checked by lib() like the table above
GRU_PROTOTYPES = {
    "atr_gru_cell_forward": (C.c_int, [C.c_void_p] * 6 + [C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong,
                                       C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "atr_gru_cell_backward": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong,
                                        C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p]),
    "atr_gru_bptt": (C.c_int, [C.c_void_p] * 4 + [C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_longlong, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
}
# the GRU learner's BPTT with the by-action column sums, include/atr_gru_sums.h (held to the header by tests/test_gru_learner_cpu.py)
GRU_SUMS_PROTOTYPES = {
    "atr_gru_bptt_act_sums_floats": (C.c_longlong, [C.c_int]),
    # (atr_gru_bptt's arguments up to dh_init, then emb_player, n_act, act_tracker, act_tstride, act_sums, P, T, N, R, stream)
    "atr_gru_bptt_sums": (C.c_int, GRU_PROTOTYPES["atr_gru_bptt"][1][:12] + [C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p,
                                                                            C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
}
# the GRU cores' fused rollout step, include/atr_gru_step.h (opt-in: --fused-gru; held to the header by tests/test_gru_fused_cpu.py)
GRU_STEP_PROTOTYPES = {
    "atr_gru_act_env_step": (C.c_int, [C.c_void_p, C.POINTER(ActStepArgs), C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                       C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # (out: evaluator.EvalOut by reference — evaluator.py imports this module, so the class is not named here)
    "atr_gru_eval_act_env_step": (C.c_int, [C.c_void_p, C.POINTER(ActStepArgs), C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
}
# the whole-map ('Full' ids) conv stem, include/atr_stem_full.h (opt-in: --full-stem; held to the header by tests/test_stem_full_cpu.py)
STEM_FULL_PROTOTYPES = {
    "atr_stem_full_forward": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int] + [C.c_void_p] * 5 + [C.c_longlong, C.c_void_p]),
    "atr_stem_full_workspace_floats": (C.c_longlong, [C.c_longlong]),
    "atr_stem_full_backward": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int] + [C.c_void_p] * 10 + [C.c_longlong, C.c_void_p]),
}
# the library's own text for a failed launch, where it keeps one
_ERROR_DETAIL = {"atr_act_env_step": "t2d_last_error", "atr_coop_env_step": "t2d_last_error", "atr_linear": "atr_lt_last_error"}
_GRU_STEP_ERROR_DETAIL = {name: "t2d_last_error" for name in GRU_STEP_PROTOTYPES}


def _errcheck(name):
    """The ctypes errcheck of a status-returning entry point: a non-zero status raises, 0 is handed back to the caller."""
    def check(status, func=None, args=None):
        if status != 0:
            text = _ERROR_DETAIL.get(name) or _GRU_STEP_ERROR_DETAIL.get(name)
            detail = ": " + getattr(lib(), text)().decode() if text else ""
            raise RuntimeError("%s failed (%d)%s" % (name, status, detail))
        return status
    return check


def lib():
    global _lib
    if _lib is None:
        L = vec_env.load_library()
        for name, (restype, argtypes, *value) in (list(ATR_PROTOTYPES.items()) + list(GRU_PROTOTYPES.items())
                                                  + list(GRU_SUMS_PROTOTYPES.items()) + list(GRU_STEP_PROTOTYPES.items())
                                                  + list(STEM_FULL_PROTOTYPES.items())):
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
            if restype is C.c_int and not value:
                f.errcheck = _errcheck(name)
        _lib = L
    return _lib


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stem_fn(name, x):
    """The stem entry point for x's element type: float32 frames, or the env's u8 observations (decoded inside conv1)."""
    if x.dtype == torch.uint8:
        return getattr(lib(), name + "_u8")
    if x.dtype != torch.float32:
        raise TypeError("stem frames must be float32 or uint8, got %s" % x.dtype)
    return getattr(lib(), name)


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class _Stem(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        w1c, b1c, w2c, b2c = w1.contiguous(), b1.contiguous(), w2.contiguous(), b2.contiguous()
        M = x.shape[0]
        y = torch.empty((M, 512), dtype=torch.float32, device=x.device)
        _stem_fn("atr_stem_forward", x)(_p(x), x.stride(0), _p(w1c), _p(b1c), _p(w2c), _p(b2c), _p(y), M, _stream(x))
        ctx.save_for_backward(x, y, w1c, b1c, w2c)
        ctx.shapes = (w1.shape, w2.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, w1, b1, w2 = ctx.saved_tensors
        return (None,) + _stem_backward(x, y, dy, w1, b1, w2, ctx.shapes)


def _stem_backward(x, y, dy, w1, b1, w2, shapes):
    dy = dy.contiguous()
    M = x.shape[0]
    L = lib()
    ws = torch.empty(L.atr_stem_workspace_floats(M), dtype=torch.float32, device=x.device)
    dw1, db1 = torch.empty(144, device=x.device), torch.empty(16, device=x.device)
    dw2, db2 = torch.empty(4608, device=x.device), torch.empty(32, device=x.device)
    _stem_fn("atr_stem_backward", x)(_p(x), x.stride(0), _p(y), _p(dy), _p(w1), _p(b1), _p(w2), _p(dw1), _p(db1),
                                     _p(dw2), _p(db2), _p(ws), M, _stream(x))
    return dw1.view(shapes[0]), db1, dw2.view(shapes[1]), db2


class _StemCached(torch.autograd.Function):
    """The stem as an autograd node whose forward was already evaluated (by stem_into during the rollout, with the
    same weights): forward hands back the stored output, backward is the ordinary stem backward."""

    @staticmethod
    def forward(ctx, x, y, w1, b1, w2, b2):
        w1c, b1c, w2c = w1.contiguous(), b1.contiguous(), w2.contiguous()
        ctx.save_for_backward(x, y, w1c, b1c, w2c)
        ctx.shapes = (w1.shape, w2.shape)
        return y.view_as(y)

    @staticmethod
    def backward(ctx, dy):
        x, y, w1, b1, w2 = ctx.saved_tensors
        return (None, None) + _stem_backward(x, y, dy, w1, b1, w2, ctx.shapes)


@torch.no_grad()
def stem_into(x, conv1, conv2, out):
    """No-grad stem forward of frames x [..., 13, 13] written into out [M, 512] (a slot of the rollout cache)."""
    x = _frame_rows(x)
    M = x.shape[0]
    assert out.is_contiguous() and out.numel() == M * 512
    _stem_fn("atr_stem_forward", x)(_p(x), x.stride(0), _p(conv1.weight), _p(conv1.bias), _p(conv2.weight),
                                    _p(conv2.bias), _p(out), M, _stream(x))
    return out


@torch.no_grad()
def stem_into2(xa, enc_a, out_a, xb, enc_b, out_b):
    """stem_into for two encoders (different weights) in one launch: the rollout step's tracker and target stems."""
    xs = [_frame_rows(xa), _frame_rows(xb)]
    args = []
    for x, enc, out in ((xs[0], enc_a, out_a), (xs[1], enc_b, out_b)):
        assert out.is_contiguous() and out.numel() == x.shape[0] * 512
        args += [_p(x), x.stride(0), _p(enc.conv1.weight), _p(enc.conv1.bias), _p(enc.conv2.weight), _p(enc.conv2.bias),
                 _p(out), x.shape[0]]
    assert xs[0].dtype == xs[1].dtype
    _stem_fn("atr_stem_forward2", xs[0])(*(args + [_stream(xs[0])]))
    return out_a, out_b


def stem_cached(x, y, conv1, conv2):
    return _StemCached.apply(_frame_rows(x), y, conv1.weight, conv1.bias, conv2.weight, conv2.bias)


class _LinearReluCached(torch.autograd.Function):
    """relu(x W^T + b) whose value f is already known (computed in the rollout with the same weights): forward
    returns f, backward is the usual one (dx, dW, db through the ReLU mask f > 0)."""

    @staticmethod
    def forward(ctx, x, w, b, f):
        ctx.save_for_backward(x, w, f, b)
        return f.view_as(f)

    @staticmethod
    def backward(ctx, df):
        x, w, f, b = ctx.saved_tensors
        if f.is_cuda and not f.is_contiguous() and f.dim() == 2 and f.stride(1) == 1 and f.stride(0) % 4 == 0 and f.shape[1] % 4 == 0:
            dpre = relu_backward_ld(df.contiguous(), f)     # (f is a column block of the rollout's [features | k h] rows)
        else:
            dpre = torch.ops.aten.threshold_backward(df.contiguous(), f, 0.0)
        r = _deferred.add(dpre, x, w, biases=(b,)) if _deferred is not None else None
        if r is not None:                  # joins the backward pass's grouped weight-gradient launch
            dw, (db,) = r
        else:
            dw, db = gemm_tn(dpre, x, colsum=True)
        return dpre @ w, dw, db, None


def linear_relu_cached(x, linear, f):
    return _LinearReluCached.apply(x, linear.weight, linear.bias, f)


@torch.no_grad()
def relu_backward_ld(df, f):
    """df * (f > 0) for a dense df [rows, C] and an activation f [rows, C] whose rows are f.stride(0) floats apart."""
    rows, Cc = df.shape
    out = torch.empty_like(df)
    lib().atr_relu_backward_ld(_p(df), _p(f), f.stride(0), _p(out), rows, Cc, _stream(df))
    return out


_lt_ready = False


def _lt_init():
    """Hand csrc/lt_gemm.cpp the libhipblaslt.so PyTorch itself uses (it resolves the entry points from that copy)."""
    global _lt_ready
    if _lt_ready:
        return
    cands = [os.path.join(os.path.dirname(torch.__file__), "lib", "libhipblaslt.so")]
    try:
        for ln in open("/proc/self/maps"):
            if "libhipblaslt" in ln:
                cands.insert(0, ln.split()[-1])
                break
    except OSError:
        pass
    L = lib()
    for path in cands:
        if os.path.exists(path) and L.atr_lt_init(path.encode()) == 0:
            _lt_ready = True
            return
    raise RuntimeError("atr_lt_init failed: %s" % L.atr_lt_last_error().decode())


_lt_state = None


def lt_available():
    """Whether atr_linear can be used (PyTorch's libhipblaslt.so found and initialised). False only on an unexpected
    runtime: the model then keeps round 3's rollout step (library GEMMs through torch + two gate tensors) — slower, still the
    HIP path — and says so once on stderr."""
    global _lt_state
    if _lt_state is None:
        try:
            _lt_init()
            _lt_state = True
        except (RuntimeError, OSError) as ex:
            print("active_tracking_rl_amd: hipBLASLt direct path unavailable (%s); using the torch GEMM path" % (ex,), file=sys.stderr)
            _lt_state = False
    return _lt_state


def _linear_args(a, w, out, bias, relu, workspace):
    g = LinearArgs()
    if a.dim() == 2:
        a, w, out = a.unsqueeze(0), w.unsqueeze(0), out.unsqueeze(0)
    B, M, K = a.shape
    N = w.shape[1]
    assert w.shape == (B, N, K) and out.shape == (B, M, N)
    for t in (a, w, out):
        assert t.is_cuda and t.dtype == torch.float32 and t.stride(2) == 1 and t.data_ptr() % 16 == 0
    g.a, g.w, g.c = a.data_ptr(), w.data_ptr(), out.data_ptr()
    g.lda, g.ldw, g.ldc = a.stride(1), w.stride(1), out.stride(1)
    g.stride_a, g.stride_w, g.stride_c = a.stride(0), w.stride(0), out.stride(0)
    g.bias = bias.data_ptr() if bias is not None else None
    assert bias is None or (B == 1 and bias.is_contiguous() and bias.numel() == N)
    g.M, g.N, g.K, g.batch, g.relu = M, N, K, B, 1 if relu else 0
    if workspace is not None:
        g.workspace, g.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    return g


LT_TUNING_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lt_tuning_gfx950.json")
LT_SOURCES = {0: "none", 1: "timed", 2: "recorded", 3: "first-usable", 4: "refused", 5: "refused-timed"}
_lt_choices, _lt_seen, _lt_status = None, {}, "not loaded"


def _lt_key(g):
    # everything that selects a kernel, including the workspace limit handed to the heuristic (another limit = another list)
    return "M%d_N%d_K%d_b%d_lda%d_ldw%d_ldc%d_sa%d_sw%d_sc%d_relu%d_bias%d_ws%d" % (
        g.M, g.N, g.K, g.batch, g.lda, g.ldw, g.ldc, g.stride_a, g.stride_w, g.stride_c, g.relu, 1 if g.bias else 0,
        g.workspace_bytes if g.workspace else 0)


def _lt_family(key):
    """The problem key without the output's batch stride. A product must not change with the PLACE its batches are written to
    (the gate GEMM writes a [2, N, 512] scratch tensor or — since round 5 — slot t of the rollout's [2, T, N, 512] store: the
    same products), but hipBLASLt's heuristic takes the stride into account and a timing run can crown another tile shape,
    whose fp32 sums differ in the last bit: two runs of one seed then part ways at the first sampled action. So the kernel is
    chosen per FAMILY: every output stride runs the choice recorded (or first timed) for the family."""
    return re.sub(r"_sc\d+", "", key)


def _lt_family_choices():
    """{family: (candidate index, solution index)}: of a family's records the one with the largest output stride (the rollout
    store at the bench's rollout length — the default path)."""
    fam = {}
    for k, v in lt_choices().items():
        sc = int(re.search(r"_sc(\d+)", k).group(1)) if re.search(r"_sc(\d+)", k) else 0
        f = _lt_family(k)
        if f not in fam or sc > fam[f][0]:
            fam[f] = (sc, v)
    return {f: v for f, (sc, v) in fam.items()}


_lt_family_first = {}       # families without a record: the choice the first problem of the family ended up with


def lt_library():
    """{'version', 'git', 'header_version'} of the hipBLASLt build csrc/lt_gemm.cpp loaded (PyTorch's copy) and of the header it
    was compiled against."""
    _lt_init()
    v, hv, rev = C.c_int(0), C.c_int(0), C.create_string_buffer(256)
    if lib().atr_lt_library_info(C.byref(v), C.byref(hv), rev, 256) != 0:
        raise RuntimeError("atr_lt_library_info failed")
    return dict(version=v.value, git=rev.value.decode(errors="replace"), header_version=hv.value)


def lt_choices():
    """{problem key: (candidate index, solution index)} recorded by tools/tune_lt.py (lt_tuning_gfx950.json next to this file;
    ATR_LT_TUNING=0 ignores it): the kernel choices of csrc/lt_gemm.cpp are then the same in every run — what
    tunableop_gfx950.csv is for torch's GEMMs — and nothing is timed at first use. The record is only used when it was made
    with the hipBLASLt build that is loaded now (version + revision, as TunableOp's validators do): a position in the
    heuristic's list means nothing on another build. On a mismatch the file is ignored, every problem is timed at first use
    (outside capture) and lt_tuning_status() says so; within a matching build csrc/lt_gemm.cpp still checks each record's
    solution index against the list it gets."""
    global _lt_choices, _lt_status
    if _lt_choices is None:
        _lt_choices = {}
        if os.environ.get("ATR_LT_TUNING", "1") == "0":
            _lt_status = "timed at first use (ATR_LT_TUNING=0)"
        elif not os.path.exists(LT_TUNING_FILE):
            _lt_status = "timed at first use (no tuning file)"
        else:
            try:
                rec = json.load(open(LT_TUNING_FILE))
                have = lt_library()
                want = rec.get("hipblaslt") or {}
                if want.get("version") != have["version"] or want.get("git") != have["git"]:
                    _lt_status = ("timed at first use (tuning file made with hipBLASLt %s %s, loaded %s %s)"
                                  % (want.get("version"), want.get("git"), have["version"], have["git"]))
                else:
                    for k, v in rec.get("choices", {}).items():
                        idx, sol = int(v["index"]), int(v.get("solution", -1))
                        if idx >= 0:
                            _lt_choices[k] = (idx, sol)
                    _lt_status = "recorded (hipBLASLt %s %s, %d problems)" % (have["version"], have["git"], len(_lt_choices))
            except (ValueError, OSError, KeyError, TypeError, AttributeError) as ex:
                _lt_choices = {}
                _lt_status = "timed at first use (unreadable tuning file: %s)" % (ex,)
    return _lt_choices


def lt_tuning_status():
    """One line for the bench record: where the direct-hipBLASLt kernel choices of this process come from, and how many of the
    problems seen so far run a recorded / timed / refused choice."""
    if _lt_state is False:
        return "torch GEMM path (direct hipBLASLt unavailable)"
    if _lt_choices is None:
        return "not used"
    counts = {}
    for k, g in _lt_seen.items():
        info = _plan_info(g)
        if info is not None:
            counts[LT_SOURCES.get(info["source"], "?")] = counts.get(LT_SOURCES.get(info["source"], "?"), 0) + 1
    tail = ", ".join("%d %s" % (n, k) for k, n in sorted(counts.items()))
    return _lt_status + ("; in use: " + tail if tail else "")


def _plan_info(g):
    cand, ch, tu, us, sol, src = C.c_int(0), C.c_int(0), C.c_int(0), C.c_float(0), C.c_int(-1), C.c_int(0)
    if lib().atr_linear_plan_info(C.byref(g), C.byref(cand), C.byref(ch), C.byref(tu), C.byref(us), C.byref(sol), C.byref(src)) != 0:
        return None
    return dict(candidates=cand.value, chosen=ch.value, tuned=bool(tu.value), best_us=us.value, solution=sol.value,
                source=src.value)


def lt_chosen():
    """{problem key: plan info + kernel name} of every problem this process has run and timed (for tools/tune_lt.py)."""
    out = {}
    for k, g in _lt_seen.items():
        info = _plan_info(g)
        if info is not None and info["tuned"]:
            name = C.create_string_buffer(512)
            lib().atr_linear_kernel_name(C.byref(g), name, 512)
            info["kernel"] = name.value.decode(errors="replace")
            out[k] = info
    return out


@torch.no_grad()
def linear_lt(a, w, out, bias=None, relu=False, workspace=None):
    """out = act(a @ w.T + bias) through hipBLASLt called directly (atr_linear, csrc/lt_gemm.cpp): a [M, K], w [N, K] (nn.Linear
    layout), out [M, N] — or a batch of them as 3-D tensors (no bias then). Rows may be strided (a column block of wider rows:
    the fc output inside the rollout's [features | k h] rows). workspace: a uint8 device tensor private to the calling chain
    of launches (two streams must not share one); None = the library's own."""
    _lt_init()
    g = _linear_args(a, w, out, bias, relu, workspace)
    L = lib()
    key = _lt_key(g)
    fresh = key not in _lt_seen
    if fresh:
        _lt_seen[key] = g
        fam = _lt_family(key)
        rec = _lt_family_choices().get(fam) or _lt_family_first.get(fam)
        if rec is not None:
            L.atr_linear_set_choice(C.byref(g), rec[0], rec[1])
    L.atr_linear(C.byref(g), _stream(a))
    if fresh and rec is None:
        info = _plan_info(g)
        # (only a TIMED choice is handed to the family's other strides: a first-usable plan made inside a stream capture is
        # re-timed later and may change — its siblings would keep the untimed kernel and the family would split again)
        if info is not None and info["chosen"] >= 0 and info["solution"] >= 0 and info["tuned"]:
            _lt_family_first[fam] = (info["chosen"], info["solution"])
    return out


def linear_lt_info(a, w, out, bias=None, relu=False, workspace=None):
    """(candidates, chosen index, tuned?, best us) of the kernel choice for this problem (after its first linear_lt call)."""
    return _plan_info(_linear_args(a, w, out, bias, relu, workspace))


def linear_lt_set_choice(a, w, out, index, solution=-1, bias=None, relu=False, workspace=None):
    """Pre-select candidate `index` (and, with solution >= 0, insist that it is that solution) for this problem: what
    lt_choices() does from the tuning file, by hand (tests, A/B runs)."""
    _lt_init()
    g = _linear_args(a, w, out, bias, relu, workspace)
    _lt_seen.setdefault(_lt_key(g), g)
    if lib().atr_linear_set_choice(C.byref(g), int(index), int(solution)) != 0:
        raise RuntimeError("atr_linear_set_choice failed: %s" % lib().atr_lt_last_error().decode())


def _frame_stride(x, side):
    """The constant distance in elements between consecutive frames of x [..., side, side] when its rows are contiguous and
    its frames evenly strided and not overlapping (one agent's slice of the env's obs tensor, or of the stacked rollout buffer);
    None otherwise."""
    if x.stride(-1) != 1 or x.stride(-2) != side:
        return None
    lead = [(sz, st) for sz, st in zip(x.shape[:-2], x.stride()[:-2]) if sz != 1]
    stride = lead[-1][1] if lead else side * side
    for (sz, st), (sz2, st2) in zip(lead[:-1], lead[1:]):
        if st != sz2 * st2:
            return None
    return stride if stride >= side * side else None


def rows169(x):
    """View x [..., 13, 13]-shaped frames as [M, 169] rows WITHOUT copying when the frames are evenly strided (e.g.
    one agent's slice of the env's obs tensor, or of the stacked rollout buffer); falls back to reshape (copy)."""
    m = x.numel() // 169
    stride = _frame_stride(x, 13)
    if stride is not None:
        return x.as_strided((m, 169), (stride, 1), x.storage_offset())
    return x.reshape(m, 169)


def _frame_rows(x):
    """rows169(x) as the stem kernels read it: rows must be contiguous, the row stride is free (>= 169); else a copy."""
    x = rows169(x)
    if x.stride(1) != 1 or x.stride(0) < 169:
        x = x.contiguous()
    return x


def stem(x, conv1, conv2):
    """x: frames [..., 13, 13] float32 on the GPU (any evenly strided view) -> [M, 512]."""
    return _Stem.apply(_frame_rows(x), conv1.weight, conv1.bias, conv2.weight, conv2.bias)


STEM_FULL_SIDES = (81, 82)      # Maze maps, Block / Empty maps
STEM_FULL_OUT = 32 * 21 * 21    # floats of stem output per frame, (c, h, w) order
STEM_FULL_RECORD = 4800         # floats of one workgroup's partial record in the backward's workspace


def stem_full_workgroup_cap():
    """The most workgroups the whole-map stem's backward launches (three 7-row bands per frame up to this cap, then a grid stride)."""
    return lib().atr_stem_full_workspace_floats(1 << 40) // STEM_FULL_RECORD


def full_frames(x):
    """View x [..., S, S]-shaped frames as [M, S, S] WITHOUT copying when rows are contiguous and the frames evenly strided (one
    agent's planes of the env's obs tensor); a contiguous copy otherwise (stacked frames of several agents, transposed views)."""
    S = x.shape[-1]
    if x.dim() < 2 or x.shape[-2] != S:
        raise ValueError("square frames expected, got %s" % (tuple(x.shape),))
    m = x.numel() // (S * S)
    stride = _frame_stride(x, S)
    if stride is not None:
        return x.as_strided((m, S, S), (stride, S, 1), x.storage_offset())
    return x.reshape(m, S, S).contiguous()


class _StemFull(torch.autograd.Function):
    """CNN_maze's two convs + ReLUs on whole-map frames as one node: one launch forward, two backward (csrc/stem_full_hip.hip).
    Saves the frames (a view), the output and the weights — conv1's activation is recomputed inside the backward kernel."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        w1c, b1c, w2c, b2c = w1.contiguous(), b1.contiguous(), w2.contiguous(), b2.contiguous()
        M, S = x.shape[0], x.shape[-1]
        y = torch.empty((M, STEM_FULL_OUT), dtype=torch.float32, device=x.device)
        if M:                                        # (an empty tensor has no data pointer to hand over)
            lib().atr_stem_full_forward(_p(x), x.stride(0), S, _p(w1c), _p(b1c), _p(w2c), _p(b2c), _p(y), M, _stream(x))
        ctx.save_for_backward(x, y, w1c, b1c, w2c)
        ctx.shapes = (w1.shape, w2.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, w1, b1, w2 = ctx.saved_tensors
        dy = dy.contiguous()
        M, S = x.shape[0], x.shape[-1]
        L = lib()
        if M == 0:
            z = lambda n: torch.zeros(n, device=x.device)
            return None, z(144).view(ctx.shapes[0]), z(16), z(4608).view(ctx.shapes[1]), z(32)
        ws = torch.empty(L.atr_stem_full_workspace_floats(M), dtype=torch.float32, device=x.device)
        dw1, db1 = torch.empty(144, device=x.device), torch.empty(16, device=x.device)
        dw2, db2 = torch.empty(4608, device=x.device), torch.empty(32, device=x.device)
        L.atr_stem_full_backward(_p(x), x.stride(0), S, _p(y), _p(dy), _p(w1), _p(b1), _p(w2), _p(dw1), _p(db1), _p(dw2),
                                 _p(db2), _p(ws), M, _stream(x))
        return None, dw1.view(ctx.shapes[0]), db1, dw2.view(ctx.shapes[1]), db2


def stem_full(x, conv1, conv2):
    """x: single-channel frames [..., S, S], S in STEM_FULL_SIDES, float32 on the GPU (any evenly strided view is read in place)
    -> [M, 14112], the layout `relu(conv2(relu(conv1(x)))).reshape(M, -1)` has."""
    if not x.is_cuda or x.dtype != torch.float32:
        raise TypeError("stem_full frames must be float32 on the GPU, got %s on %s" % (x.dtype, x.device))
    if x.shape[-1] not in STEM_FULL_SIDES or x.shape[-2] != x.shape[-1]:
        raise ValueError("stem_full frames must be 81 x 81 or 82 x 82, got %s" % (tuple(x.shape[-2:]),))
    if conv1.in_channels != 1:
        raise ValueError("stem_full reads single-channel frames")
    return _StemFull.apply(full_frames(x), conv1.weight, conv1.bias, conv2.weight, conv2.bias)


class ActionSampler(object):
    """Fused actor head for the rollout: action ~ Categorical(softmax(W h + b)) in one launch (csrc/policy_hip.hip).
    Holds the device-side stream counter (hipGraph-safe) and the Philox seed. Stand-alone calls advance the counter
    themselves; inside begin_block() ... the counter is advanced once and the calls are told apart by their ordinal
    (saves one tiny launch per call in the rollout)."""

    def __init__(self, device, seed=None):
        self.counter = torch.zeros(1, dtype=torch.int64, device=device)
        self.seed = int(torch.initial_seed() if seed is None else seed) & 0xFFFFFFFFFFFFFFFF
        self._ordinal = None

    @torch.no_grad()
    def begin_block(self, launch=True):
        """Advance the counter once (in stream order); the following calls use ordinals 1, 2, ... until end_block.
        launch=False: the caller's next launch bumps the counter itself (fused.rollout_begin(counter=...))."""
        if not launch:
            self._ordinal = 0
            return
        dummy = self.counter
        lib().atr_sample_actions(_p(dummy), _p(dummy), _p(dummy), _p(dummy), _p(self.counter), self.seed, 0, 1,
                                 0, 4, 1, _stream(self.counter))
        self._ordinal = 0

    def end_block(self):
        if self._ordinal is not None:
            self._last = self._ordinal
        self._ordinal = None

    def reopen_block(self):
        """Continue the ordinals of the block that end_block() closed last (the learner's bootstrap step draws once more
        after the rollout, under the same counter value)."""
        self._ordinal = getattr(self, "_last", None)

    @torch.no_grad()
    def __call__(self, h, linear, out=None):
        h = h.contiguous()
        n, R = h.shape
        A = linear.weight.shape[0]
        actions = torch.empty(n, dtype=torch.int64, device=h.device) if out is None else out
        assert actions.is_contiguous() and actions.dtype == torch.int64 and actions.numel() == n
        if self._ordinal is None:
            ordinal, bump = 0, 1
        else:
            self._ordinal += 1
            ordinal, bump = self._ordinal, 0
        lib().atr_sample_actions(_p(h), _p(linear.weight), _p(linear.bias), _p(actions), _p(self.counter),
                                 self.seed, ordinal, bump, n, R, A, _stream(h))
        return actions


def _pn(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def lstm_cell(ig, hg, c_prev, keep=None, done=None):
    """One no-grad LSTMCell step for the rollout (csrc/lstm_hip.hip): ig [N,4R] = x W_ih^T + b_ih + b_hh, hg [N,4R] =
    h_prev W_hh^T with h_prev NOT masked; the previous step's episode-boundary mask (keep [N] float, or done [N] uint8)
    is applied inside. Returns (h, c) [N,R]."""
    N, R = c_prev.shape
    h, c = torch.empty_like(c_prev), torch.empty_like(c_prev)
    lib().atr_lstm_cell_forward(_p(ig), None, _p(hg), _p(c_prev), 0, _pn(keep), _pn(done), _p(h), 0, _p(c), 0,
                                None, 0, 1, N, R, _stream(ig))
    return h, c


class _LstmSeq(torch.autograd.Function):
    """Two (or one) independent LSTMCells over T time-major steps with the per-step episode mask, as ONE autograd
    node: per step one batched hidden GEMM + one fused cell launch forward, one fused cell-backward launch + one
    batched GEMM backward; the weight gradient of W_hh is a single GEMM over all T*N rows at the end.
    ig0/ig1 [T*N,4R] (input projections incl. both biases), whh [P,R,4R] (= W_hh^T per player), h0/c0 [P,N,R]
    (already masked), keep [T,N] float. Returns per player h_seq [T,N,R] (the un-masked step outputs, what the heads
    read) and, last, the un-masked final cell state [P,N,R] (not differentiable)."""

    @staticmethod
    def forward(ctx, ig0, ig1, whh, h0, c0, keep):
        L = lib()
        P, N, R = h0.shape
        T = keep.shape[0]
        dev = h0.device
        ig0, whh, keep = ig0.contiguous(), whh.contiguous(), keep.contiguous()
        ig1 = ig1.contiguous() if ig1 is not None else None
        h_all = torch.empty((P, T + 1, N, R), dtype=torch.float32, device=dev)   # slot 0 = h0, slot t+1 = h_t
        c_all = torch.empty((P, T + 1, N, R), dtype=torch.float32, device=dev)
        acts = torch.empty((P, T, N, 4 * R), dtype=torch.float32, device=dev)
        h_all[:, 0].copy_(h0)
        c_all[:, 0].copy_(c0)
        hg = torch.empty((P, N, 4 * R), dtype=torch.float32, device=dev)
        st = _stream(h0)
        ps, pa, step, astep = (T + 1) * N * R, T * N * 4 * R, N * R * 4, N * 4 * R * 4   # strides: floats / bytes
        for t in range(T):
            torch.bmm(h_all[:, t], whh, out=hg)
            off = t * N * 4 * R * 4
            L.atr_lstm_cell_forward(
                C.c_void_p(ig0.data_ptr() + off), C.c_void_p(ig1.data_ptr() + off) if ig1 is not None else None,
                _p(hg), C.c_void_p(c_all.data_ptr() + t * step), ps, _p(keep[t - 1]) if t else None, None,
                C.c_void_p(h_all.data_ptr() + (t + 1) * step), ps, C.c_void_p(c_all.data_ptr() + (t + 1) * step), ps,
                C.c_void_p(acts.data_ptr() + t * astep), pa, P, N, R, st)
        ctx.save_for_backward(whh, keep, h_all, c_all, acts)
        ctx.two = ig1 is not None
        c_last = c_all[:, T].clone()                                             # un-masked final cell state
        ctx.mark_non_differentiable(c_last)
        return tuple(h_all[p, 1:] for p in range(P)) + (c_last,)                 # per player [T,N,R], contiguous

    @staticmethod
    def backward(ctx, *dhs):
        whh, keep, h_all, c_all, acts = ctx.saved_tensors
        dG, dhn, dcc, dwhh = _lstm_bptt(whh, keep, h_all, c_all, acts, dhs[:-1])
        return dG[0], (dG[1] if ctx.two else None), dwhh, dhn, dcc, None


use_fused_bptt = True   # the whole recurrence backward as ONE launch (csrc/bptt_hip.hip) instead of 2 launches per step


def activate_preacts(pre, info):
    """The activated gates (i, f, g, o) [P, T, N, 4R] from stored pre-activations (`info`: see _lstm_bptt) with tensor ops — what
    the fused BPTT kernel recomputes in registers; only the per-step fallback recurrence needs them materialised."""
    P, T, N, R4 = pre.shape
    R = R4 // 4
    x = pre + torch.stack(list(info["bias"]), 0).view(P, 1, 1, R4)
    if info.get("emb") is not None and 0 <= info["emb_player"] < P:
        x[info["emb_player"]] = info["emb"][info["act"]] + x[info["emb_player"]]
    x = x.view(P, T, N, 4, R)
    return torch.stack([torch.sigmoid(x[..., 0, :]), torch.sigmoid(x[..., 1, :]), torch.tanh(x[..., 2, :]),
                        torch.sigmoid(x[..., 3, :])], -2).reshape(P, T, N, R4).contiguous()


def _fused_bptt_ok(h_all, *stores):
    """Whether the one-launch BPTT (csrc/bptt_hip.hip) can run: switched on, R = 128, on the GPU, `stores` contiguous."""
    return use_fused_bptt and h_all.shape[-1] == 128 and h_all.is_cuda and all(t.is_contiguous() for t in stores)


def _keep_prev(keep):
    """keep [T, N] shifted by one step: the mask on h_{t-1} (ones for step 0, whose previous state comes masked)."""
    return torch.cat([torch.ones_like(keep[:1]), keep[:-1]], 0)


def _lstm_bptt(whh, keep, h_all, c_all, acts, dhs, whh_nn=None, want_dwhh=True, pre=None):
    """Back-propagation through time over stored activations: dhs = per-player dL/dh_seq [T,N,R] (None = zero).
    Returns dG [P, T*N, 4R] (= dL/d ig), dL/dh0, dL/dc0 [P,N,R] and dL/dW_hh^T [P,R,4R]. whh_nn: per-player weight_hh [4R,R]
    (nn layout; made from whh [P,R,4R] when absent).
    pre: None, or dict(bias=[per-player b_ih + b_hh [4R]], emb=[n_act, 4R] or None, emb_player, act=[T, N] int64 view of the
    tracker's actions) — `acts` then holds the rollout's gate PRE-activations without bias (model._act_step's one-GEMM path keeps
    the GEMM's output instead of the activated gates) and the activations are recomputed inside the kernel."""
    L = lib()
    P, T1, N, R = h_all.shape
    T = T1 - 1
    dev = h_all.device
    fused_ok = _fused_bptt_ok(h_all, acts, c_all, keep)
    if pre is not None and not fused_ok:
        acts, pre = activate_preacts(acts, pre), None
    dG = torch.empty((P, T, N, 4 * R), dtype=torch.float32, device=dev)
    dhn = torch.empty((P, N, R), dtype=torch.float32, device=dev)
    dcc = torch.empty((P, N, R), dtype=torch.float32, device=dev)
    st = _stream(h_all)
    ps, pa, step, astep = (T + 1) * N * R, T * N * 4 * R, N * R * 4, N * 4 * R * 4
    if fused_ok:
        if whh_nn is None:
            wt = whh.transpose(1, 2).contiguous()
            whh_nn = [wt[p] for p in range(P)]
        whh_nn = [w if w.is_contiguous() else w.contiguous() for w in whh_nn]
        dh_c = [d.contiguous() if d is not None else None for d in dhs]
        if pre is not None:
            bias = [b.contiguous() for b in pre["bias"]]
            emb = pre.get("emb")
            ep = int(pre.get("emb_player", -1))
            if emb is None or not (0 <= ep < P):
                emb, ep, act, n_act, act_ts = None, -1, None, 0, 0
            else:
                emb, act = emb.contiguous(), pre["act"]
                assert act.dtype == torch.int64 and act.shape == (T, N) and act.stride(1) == 1
                n_act, act_ts = emb.shape[0], act.stride(0)
            sums = None
            if pre.get("want_sums") and emb is not None and n_act == 4:
                # per row tile of the embedding's player: column sums of dG by the row's tracker action (see embed_fold)
                sums = torch.empty(L.atr_lstm_bptt_act_sums_floats(N), dtype=torch.float32, device=dev)
            pre["act_sums"] = sums
            L.atr_lstm_bptt_pre2(_pn(dh_c[0]), _pn(dh_c[1]) if P > 1 else None, _p(keep), _p(acts), acts.stride(0),
                                 _p(bias[0]), _p(bias[1]) if P > 1 else None, _pn(emb), ep, n_act, _pn(act), act_ts,
                                 _p(c_all), ps, _p(whh_nn[0]), _p(whh_nn[1]) if P > 1 else None, _p(dG), pa, _p(dhn),
                                 _p(dcc), _pn(sums), P, T, N, R, st)
        else:
            L.atr_lstm_bptt(_pn(dh_c[0]), _pn(dh_c[1]) if P > 1 else None, _p(keep), _p(acts), pa, _p(c_all), ps,
                            _p(whh_nn[0]), _p(whh_nn[1]) if P > 1 else None, _p(dG), pa, _p(dhn), _p(dcc), P, T, N, R, st)
    else:
        dhs = [torch.zeros((T, N, R), dtype=torch.float32, device=dev) if d is None else d.contiguous() for d in dhs]
        pd = (dhs[1].data_ptr() - dhs[0].data_ptr()) // 4 if P > 1 else 0          # player stride between the two grads
        whh_t = whh.transpose(1, 2)                                               # [P,4R,R]
        for t in range(T - 1, -1, -1):
            L.atr_lstm_cell_backward(
                C.c_void_p(dhs[0].data_ptr() + t * step), pd, _p(dhn), _p(dcc), _p(keep[t]),
                _p(keep[t - 1]) if t else None, C.c_void_p(acts.data_ptr() + t * astep), pa,
                C.c_void_p(c_all.data_ptr() + (t + 1) * step), ps, C.c_void_p(c_all.data_ptr() + t * step), ps,
                C.c_void_p(dG.data_ptr() + t * astep), pa, 1 if t < T - 1 else 0, P, N, R, st)
            torch.bmm(dG[:, t], whh_t, out=dhn)                                   # gradient into h_{t-1}
    if not want_dwhh:          # (the caller registers dW_hh with the grouped weight-gradient launch)
        return dG.view(P, T * N, 4 * R), dhn, dcc, None
    # W_hh: sum_t (k_{t-1} h_{t-1})^T dG_t as one GEMM per player over all T*N rows
    kprev = _keep_prev(keep)
    dG = dG.view(P, T * N, 4 * R)
    if use_gemm_tn and R % 128 == 0 and T * N >= 4096:
        # the mask is applied to h's rows on their way into the GEMM kernel's LDS tiles
        dwhh = torch.stack([gemm_tn(h_all[p, :T].reshape(T * N, R), dG[p], row_scale=kprev.reshape(T * N))
                            for p in range(P)], 0)
    else:
        hm = (h_all[:, :T] * kprev.view(1, T, N, 1)).view(P, T * N, R)
        dwhh = bmm_tn(hm, dG)
    return dG, dhn, dcc, dwhh


BMM_TN_CHUNK = 512


def bmm_tn(a, b):
    """a^T b per batch for tall a [P, K, M], b [P, K, N] — dW_hh where gemm_tn does not take the shape (R no multiple of 128).
    From 4096 rows up (gemm_tn's own threshold) as partial products over chunks of BMM_TN_CHUNK rows, summed in a second step:
    the library product's one running fp32 sum over K = 4096 rows was measured at e = 1.2e-6 against float64 (R = 64, 1024 envs
    x 4 steps, tests/test_learner_f64_gpu.py), four times the error of PyTorch's own fp32 evaluation of the same gradient."""
    P, K, M = a.shape
    C = K // BMM_TN_CHUNK
    if K < 4096:
        return torch.bmm(a.transpose(1, 2), b)
    Kc = C * BMM_TN_CHUNK
    out = torch.bmm(a[:, :Kc].reshape(P * C, BMM_TN_CHUNK, M).transpose(1, 2),
                    b[:, :Kc].reshape(P * C, BMM_TN_CHUNK, b.shape[2])).view(P, C, M, b.shape[2]).sum(1)
    if Kc < K:
        out = out + torch.bmm(a[:, Kc:].transpose(1, 2), b[:, Kc:])
    return out


def gru_cell(ig, hg, b_hh, h_prev, keep=None, done=None):
    """One no-grad GRUCell step for the rollout (csrc/gru_hip.hip): ig [N,3R] = x W_ih^T + b_ih, hg [N,3R] = h_prev W_hh^T with
    h_prev [N,R] NOT masked; the previous step's episode-boundary mask (keep [N] float, or done [N] uint8) is applied inside, to
    the hidden product and to the z h term, and b_hh [3R] is added after it. Returns h [N,R]."""
    N, R = h_prev.shape
    h = torch.empty_like(h_prev)
    lib().atr_gru_cell_forward(_p(ig), None, _p(hg), _p(b_hh), None, _p(h_prev), 0, _pn(keep), _pn(done), _p(h), 0, None, 0,
                               1, N, R, _stream(ig))
    return h


class _GruSeq(torch.autograd.Function):
    """_LstmSeq for two (or one) independent GRUCells: T time-major steps with the per-step episode mask as ONE autograd node;
    per step one batched hidden GEMM + one cell launch forward, the backward is _gru_bptt.
    ig0/ig1 [T*N,3R] (input projections incl. b_ih), whh [P,R,3R] (= W_hh^T per player), bhh [P,3R], h0 [P,N,R] (already
    masked), keep [T,N] float. Returns per player h_seq [T,N,R] (the un-masked step outputs, what the heads read)."""

    @staticmethod
    def forward(ctx, ig0, ig1, whh, bhh, h0, keep):
        L = lib()
        P, N, R = h0.shape
        T = keep.shape[0]
        dev = h0.device
        ig0, whh, bhh, keep = ig0.contiguous(), whh.contiguous(), bhh.contiguous(), keep.contiguous()
        ig1 = ig1.contiguous() if ig1 is not None else None
        h_all = torch.empty((P, T + 1, N, R), dtype=torch.float32, device=dev)   # slot 0 = h0, slot t+1 = h_t
        acts = torch.empty((P, T, N, 4 * R), dtype=torch.float32, device=dev)    # (r, z, n, q)
        h_all[:, 0].copy_(h0)
        hg = torch.empty((P, N, 3 * R), dtype=torch.float32, device=dev)
        st = _stream(h0)
        ps, pa, step, astep, istep = (T + 1) * N * R, T * N * 4 * R, N * R * 4, N * 4 * R * 4, N * 3 * R * 4
        for t in range(T):
            torch.bmm(h_all[:, t], whh, out=hg)
            L.atr_gru_cell_forward(
                C.c_void_p(ig0.data_ptr() + t * istep), C.c_void_p(ig1.data_ptr() + t * istep) if ig1 is not None else None,
                _p(hg), _p(bhh[0]), _p(bhh[1]) if P > 1 else None, C.c_void_p(h_all.data_ptr() + t * step), ps,
                _p(keep[t - 1]) if t else None, None, C.c_void_p(h_all.data_ptr() + (t + 1) * step), ps,
                C.c_void_p(acts.data_ptr() + t * astep), pa, P, N, R, st)
        ctx.save_for_backward(whh, keep, h_all, acts)
        ctx.two = ig1 is not None
        return tuple(h_all[p, 1:] for p in range(P))                             # per player [T,N,R], contiguous

    @staticmethod
    def backward(ctx, *dhs):
        whh, keep, h_all, acts = ctx.saved_tensors
        R = h_all.shape[-1]
        dG, dh0, dwhh, dbhh = _gru_bptt(whh, keep, h_all, acts, dhs)
        return dG[0][:, :3 * R], (dG[1][:, :3 * R] if ctx.two else None), dwhh, dbhh, dh0, None


def gru_sequence(ig0, ig1, whh, bhh, h0, keep):
    return _GruSeq.apply(ig0, ig1, whh, bhh, h0, keep)


use_fused_gru_bptt = True   # the GRU recurrence backward as ONE launch (atr_gru_bptt) instead of 2 launches per step


def _hidden_cols(x, R):
    """The hidden-side columns (r, z, q) of a [..., 4R] tensor laid out as dG is: (dr_pre, dz_pre, dn_pre, dn_pre r)."""
    return torch.cat([x[..., :2 * R], x[..., 3 * R:]], -1)


def _fused_gru_bptt_ok(h_all, *stores):
    """Whether the one-launch GRU BPTT (atr_gru_bptt) can run: switched on, R = 128, on the GPU, the stores contiguous."""
    return bool(use_fused_gru_bptt and h_all.shape[-1] == 128 and h_all.is_cuda
                and all(t.is_contiguous() for t in (h_all,) + stores))


def _gru_bptt(whh, keep, h_all, acts, dhs, hm=None, want_dw=True, sums=None):
    """Back-propagation through time over a GRU recurrence's stored activations: whh [P,R,3R], keep [T,N], h_all [P,T+1,N,R],
    acts [P,T,N,4R] = (r, z, n, q), dhs = per-player dL/dh_seq [T,N,R] (None = zero). Returns dG [P, T*N, 4R] = (dr_pre, dz_pre,
    dn_pre, dn_pre r) — columns 0:3R are dL/d ig —, dL/dh0 [P,N,R], dL/dW_hh^T [P,R,3R] and dL/db_hh [P,3R] (both None when
    not want_dw: the caller registers those products with the grouped weight-gradient launch).
    hm: per player the masked rows k_{t-1} h_{t-1} [T*N,R] where the rollout stored them (row-strided views are fine): dW_hh
    contracts them as they are.
    sums: None, or dict(emb_player, act = [T, N] int64 view of the tracker's actions) — the one-launch kernel then also leaves,
    as sums['act_sums'], the column sums of dG[..., 0:3R] of player emb_player by the row's tracker action (atr_gru_bptt_sums:
    what embed_fold reads with J = 3R); None there when the per-step path ran."""
    L = lib()
    P, T1, N, R = h_all.shape
    T = T1 - 1
    dev = h_all.device
    dG = torch.empty((P, T, N, 4 * R), dtype=torch.float32, device=dev)
    dhn = torch.empty((P, N, R), dtype=torch.float32, device=dev)
    st = _stream(h_all)
    ps, pa, step, astep = (T + 1) * N * R, T * N * 4 * R, N * R * 4, N * 4 * R * 4
    whh_nn = whh.transpose(1, 2)                                                  # [P,3R,R]: nn.GRUCell's weight_hh
    if sums is not None:
        sums["act_sums"] = None
    if _fused_gru_bptt_ok(h_all, acts, keep):
        whh_nn = whh_nn.contiguous()
        dh_c = [d.contiguous() if d is not None else None for d in dhs]
        if sums is not None:
            act, ep = sums["act"], int(sums["emb_player"])
            assert act.dtype == torch.int64 and act.shape == (T, N) and act.stride(1) == 1 and 0 <= ep < P
            sums["act_sums"] = torch.empty(L.atr_gru_bptt_act_sums_floats(N), dtype=torch.float32, device=dev)
            L.atr_gru_bptt_sums(_pn(dh_c[0]), _pn(dh_c[1]) if P > 1 else None, _p(keep), _p(acts), pa, _p(h_all), ps,
                                _p(whh_nn[0]), _p(whh_nn[1]) if P > 1 else None, _p(dG), pa, _p(dhn), ep, 4, _p(act),
                                act.stride(0), _p(sums["act_sums"]), P, T, N, R, st)
        else:
            L.atr_gru_bptt(_pn(dh_c[0]), _pn(dh_c[1]) if P > 1 else None, _p(keep), _p(acts), pa, _p(h_all), ps, _p(whh_nn[0]),
                           _p(whh_nn[1]) if P > 1 else None, _p(dG), pa, _p(dhn), P, T, N, R, st)
    else:
        dhs = [torch.zeros((T, N, R), dtype=torch.float32, device=dev) if d is None else d.contiguous() for d in dhs]
        pd = (dhs[1].data_ptr() - dhs[0].data_ptr()) // 4 if P > 1 else 0          # player stride between the two grads
        # weight_hh with a zero block under dG's dn_pre columns: the step's hidden GEMM reads dG's rows as they are
        w4 = torch.cat([whh_nn[:, :2 * R], whh_nn.new_zeros((P, R, R)), whh_nn[:, 2 * R:]], 1)      # [P,4R,R]
        for t in range(T - 1, -1, -1):
            L.atr_gru_cell_backward(
                C.c_void_p(dhs[0].data_ptr() + t * step), pd, _p(dhn), _p(keep[t]), _p(keep[t - 1]) if t else None,
                C.c_void_p(acts.data_ptr() + t * astep), pa, C.c_void_p(h_all.data_ptr() + t * step), ps,
                C.c_void_p(dG.data_ptr() + t * astep), pa, 1 if t < T - 1 else 0, P, N, R, st)
            dhn.baddbmm_(dG[:, t], w4)                                            # + dG_t W_hh: the gradient into k h_{t-1}
    # W_hh: sum_t (k_{t-1} h_{t-1})^T dG_t[hidden columns] as one GEMM per player over all T*N rows; b_hh: their column sums
    dG = dG.view(P, T * N, 4 * R)
    if not want_dw:
        return dG, dhn, None, None
    if hm is not None:
        dwhh = _hidden_cols(torch.stack([gemm_tn(hm[p], dG[p]) for p in range(P)], 0), R)
    else:
        hm = (h_all[:, :T] * _keep_prev(keep).view(1, T, N, 1)).view(P, T * N, R)
        dwhh = _hidden_cols(torch.bmm(hm.transpose(1, 2), dG), R)
    dbhh = _hidden_cols(dG.sum(1), R)
    return dG, dhn, dwhh, dbhh


class _GruSeqCached(torch.autograd.Function):
    """_LstmSeqCached for the GRU cores (--fused-gru): the input projection + masked recurrence of both players as an autograd node
    whose forward the rollout already evaluated step by step (gru_act_env_step, same weights): h_all [P,T+1,N,R] and acts
    [P,T,N,4R] = (r, z, n, q) hold every step. Inputs: per-player features [T*N,F] and GRUCell parameters (+ fc_action_tracker's
    weight and bias when the tracker-action embedding is folded: the target's features are then its RAW fc features); output:
    per-player h_seq [T,N,R]. Backward: _gru_bptt on the stores, then per trained player dfeat = dG[:, :3R] W_ih and three
    weight-gradient products over dG's column blocks (include/atr_gru.h):
        dW_ih          = dG[:, 0:3R]^T f         column sums -> d b_ih
        dW_hh[0:2R]    = dG[:, 0:2R]^T (k h)     column sums -> d b_hh[0:2R]
        dW_hh[2R:3R]   = dG[:, 3R:4R]^T (k h)    column sums -> d b_hh[2R:3R]
    registered with the grouped launch of the backward pass (DeferredWeightGrads: a player joins with all three or with none)
    under _LstmSeqCached's conditions, computed on the spot otherwise. Folded, the embedding's share comes from the by-action
    column sums of dG the BPTT launch leaves (embed_fold with J = 3R): dW_ih += S^T E, d fc_action_tracker = (S W_ih)^T."""

    @staticmethod
    def forward(ctx, keep, h_all, acts, opts, *fw):
        P = h_all.shape[0]
        need, hm, fold = opts                     # fold: None or dict(emb_player, act) — see gru_sequence_cached
        ctx.fold = fold is not None
        assert len(fw) == 5 * P + (2 if ctx.fold else 0)
        ctx.save_for_backward(keep.contiguous(), h_all, acts, *fw, *(hm if hm is not None else ()),
                              *((fold["act"],) if ctx.fold else ()))
        ctx.P, ctx.has_hm, ctx.n_fw = P, hm is not None, len(fw)
        ctx.emb_player = int(fold["emb_player"]) if ctx.fold else -1
        ctx.need = tuple(bool(x) for x in need) if need is not None else (True,) * P
        return tuple(h_all[p, 1:] for p in range(P))

    @staticmethod
    def backward(ctx, *dhs):
        P = ctx.P
        keep, h_all, acts = ctx.saved_tensors[:3]
        feats, wih, whh_nn, bih, bhh = (ctx.saved_tensors[3 + i * P:3 + (i + 1) * P] for i in range(5))
        rest = ctx.saved_tensors[3 + ctx.n_fw:]
        hm = rest[:P] if ctx.has_hm else None
        fa_w, fa_b = ctx.saved_tensors[3 + 5 * P:5 + 5 * P] if ctx.fold else (None, None)
        act = rest[-1] if ctx.fold else None
        T, N, R = h_all.shape[1] - 1, h_all.shape[2], h_all.shape[3]
        dfeat, dwih, dwhh, dbih, dbhh = ([None] * P for _ in range(5))
        dfa = (None, None)
        q = _deferred
        # (a player the loss does not train — train-mode 0 / 1 — has none of its recurrence back-propagated)
        groups = [list(range(P))] if all(ctx.need) else [[p] for p in range(P) if ctx.need[p]]
        for grp in groups:
            a, b = grp[0], grp[-1] + 1
            defer = q is not None and _fused_gru_bptt_ok(h_all, acts, keep) and T * N >= 4096
            fold_p = ctx.emb_player if (ctx.fold and a <= ctx.emb_player < b) else -1
            sums = dict(emb_player=fold_p - a, act=act) if fold_p >= 0 else None      # (the player's index within the group)
            whh = torch.stack([w.t() for w in whh_nn[a:b]], 0)
            dG, _, dwhh_t, dbhh_g = _gru_bptt(whh, keep, h_all[a:b], acts[a:b], dhs[a:b], hm=hm[a:b] if hm is not None else None,
                                              want_dw=not defer, sums=sums)
            if fold_p >= 0 and sums["act_sums"] is None:
                raise RuntimeError("folded tracker-action embedding: the BPTT launch did not return the by-action sums of dG")
            for i, p in enumerate(grp):
                dGi = dG[i]
                dfeat[p] = dGi[:, :3 * R] @ wih[p]
                if p == fold_p:
                    # (feats[p] are the RAW fc features: dW_ih's product misses S^T E, added by embed_fold once the product is there)
                    fold_args = (sums["act_sums"], fa_w, fa_b, wih[p])
                    dfa = (torch.empty_like(fa_w), torch.empty_like(fa_b))
                if defer:
                    # k h rows stored by the rollout: nothing to mask, and the hidden columns' sums are d b_hh. Otherwise the
                    # mask on h_{t-1} is keep[t-1] = the keep array shifted by one step of N rows, applied to dG's rows on
                    # their way into the kernel — the column sums would carry it too, so d b_hh is summed here
                    if hm is not None:
                        x2h, rs, bh = hm[p], {}, (bhh[p],)
                    else:
                        x2h, rs, bh = h_all[p, :T].reshape(T * N, R), dict(row_scale=keep, shift=N), ()
                    r = q.add_all([dict(x1=dGi[:, :3 * R], x2=feats[p], weight=wih[p], biases=(bih[p],)),
                                   dict(x1=dGi[:, :2 * R], x2=x2h, weight=whh_nn[p], biases=bh, rows=(0, 2 * R), **rs),
                                   dict(x1=dGi[:, 3 * R:], x2=x2h, weight=whh_nn[p], biases=bh, rows=(2 * R, 3 * R), **rs)])
                    if r is not None:
                        dwih[p], dbih[p] = r[0][0], r[0][1][0]
                        dwhh[p] = r[1][0]
                        dbhh[p] = r[1][1][0] if bh else _hidden_cols(dGi.sum(0), R)
                        if p == fold_p:          # (the slice is filled by the grouped launch at flush(): the fold follows it)
                            q.after.append(lambda fa_=fold_args, dw_=dwih[p], out_=dfa: embed_fold(*fa_, dw_, *out_))
                        continue
                    # (no room in the group, or a product that does not fit it: this player's products on the spot)
                    if hm is not None:
                        dwhh[p] = _hidden_cols(gemm_tn(hm[p], dGi), R).t()
                    else:
                        kprev = _keep_prev(keep).reshape(T * N)
                        dwhh[p] = _hidden_cols(gemm_tn(h_all[p, :T].reshape(T * N, R), dGi, row_scale=kprev), R).t()
                    dbhh[p] = _hidden_cols(dGi.sum(0), R)
                else:
                    dwhh[p], dbhh[p] = dwhh_t[i].t(), dbhh_g[i]
                dw, cs = gemm_tn(dGi, feats[p], colsum=True)
                dwih[p], dbih[p] = dw[:3 * R], cs[:3 * R]
                if p == fold_p:
                    dwih[p] = dwih[p].contiguous()
                    embed_fold(*fold_args, dwih[p], *dfa)
        if ctx.fold and ctx.need[ctx.emb_player] and dfa[0] is None:
            raise RuntimeError("folded tracker-action embedding: no group of the backward pass produced its gradients")
        out = (None, None, None, None) + tuple(dfeat) + tuple(dwih) + tuple(dwhh) + tuple(dbih) + tuple(dbhh)
        return out + (tuple(dfa) if ctx.fold else ())


def gru_sequence_cached(cells, feats, keep, h_all, acts, need=None, hm=None, fold=None, act=None, emb_player=1):
    """lstm_sequence_cached for nn.GRUCells: feats per-player [T*N,F] (with grad), the rollout's stores h_all / acts = (r, z, n,
    q); need per player as there; hm per player the masked previous hidden rows [T*N,R] when the rollout stored every one.
    fold = the tracker-aware player's fc_action_tracker (see gru_embed_fold_ok): feats[emb_player] are then its RAW fc features
    (no f + E[a] materialised) and the embedding's gradients come from this node; act = the [T, N] int64 view of the tracker's
    actions (one player's column of the rollout's [T, players, N] store, read in place)."""
    args = list(feats) + [l.weight_ih for l in cells] + [l.weight_hh for l in cells] + [l.bias_ih for l in cells] + \
        [l.bias_hh for l in cells]
    fold_info = None
    if fold is not None:
        assert act is not None and act.dtype == torch.int64 and act.stride(1) == 1
        args += [fold.weight, fold.bias]
        fold_info = dict(emb_player=emb_player, act=act)
    return _GruSeqCached.apply(keep, h_all, acts, (need, hm, fold_info), *args)


def gru_embed_fold_ok(h_all, acts, keep, fa):
    """Whether gru_sequence_cached can fold the tracker-action embedding (the one-launch GRU BPTT, the four-move action table,
    parameters as the kernels read them)."""
    return bool(fold_embedding and _fused_gru_bptt_ok(h_all, acts, keep.contiguous()) and fa.weight.shape[1] == 4
                and fa.weight.is_contiguous() and fa.weight.data_ptr() % 16 == 0)


class _LstmSeqCached(torch.autograd.Function):
    """The input projection + masked recurrence of both players as an autograd node whose forward was already
    evaluated step by step during the rollout (lstm_cell_into, same weights): h_all/c_all/acts hold every step.
    Inputs: per-player features [T*N,F] and LSTMCell parameters; output: per-player h_seq [T,N,R]."""

    @staticmethod
    def forward(ctx, keep, h_all, c_all, acts, need, *fw):
        P = h_all.shape[0]
        feats, wih, whh_l = fw[:P], fw[P:2 * P], fw[2 * P:3 * P]
        # ([P, R, 4R] transposed copy: only the per-step fallback recurrence reads it — the fused BPTT kernel takes weight_hh as is)
        whh = h_all.new_empty(0) if _fused_bptt_ok(h_all) else torch.stack([w.t() for w in whh_l], 0).contiguous()
        ctx.save_for_backward(keep.contiguous(), h_all, c_all, acts, whh, *feats, *wih, *whh_l, *fw[3 * P:5 * P], *fw[5 * P:])
        ctx.P = P
        ctx.fold = len(fw) == 5 * P + 2           # fc_action_tracker's weight and bias ride along: the embedding is folded
        need, ctx.hm, ctx.pre = need              # (lstm_sequence_cached packs the non-tensor arguments together)
        ctx.need = tuple(bool(x) for x in need) if need is not None else (True,) * P
        return tuple(h_all[p, 1:] for p in range(P))

    @staticmethod
    def backward(ctx, *dhs):
        P = ctx.P
        keep, h_all, c_all, acts, whh = ctx.saved_tensors[:5]
        feats, wih = ctx.saved_tensors[5:5 + P], ctx.saved_tensors[5 + P:5 + 2 * P]
        whh_nn = ctx.saved_tensors[5 + 2 * P:5 + 3 * P]          # weight_hh [4R, R] as nn.LSTMCell holds it
        bih, bhh = ctx.saved_tensors[5 + 3 * P:5 + 4 * P], ctx.saved_tensors[5 + 4 * P:5 + 5 * P]
        fa_w, fa_b = (ctx.saved_tensors[5 + 5 * P], ctx.saved_tensors[5 + 5 * P + 1]) if ctx.fold else (None, None)
        dfa = (None, None)
        dfeat, dwih, db, dwhh_l = [None] * P, [None] * P, [None] * P, [None] * P
        db2 = None
        q = _deferred
        T, N, R = h_all.shape[1] - 1, h_all.shape[2], h_all.shape[3]
        if whh.numel() == 0 and not _fused_bptt_ok(h_all, acts, c_all, keep):     # (empty whh: forward saw h_all on the GPU)
            whh = torch.stack([w.t() for w in whh_nn], 0).contiguous()
        if all(ctx.need):
            groups = [list(range(P))]
        else:       # a player the loss does not train (train-mode 0 / 1): none of its recurrence is back-propagated
            groups = [[p] for p in range(P) if ctx.need[p]]
        for grp in groups:
            a, b = grp[0], grp[-1] + 1
            defer = q is not None and use_fused_bptt and R == 128 and T * N >= 4096
            pre = None
            if ctx.pre is not None:          # (this group's slice of the stored pre-activations' side information)
                pre = dict(ctx.pre, bias=list(ctx.pre["bias"][a:b]), emb_player=ctx.pre.get("emb_player", -1) - a)
                pre["want_sums"] = ctx.fold and a <= ctx.pre.get("emb_player", -1) < b
            dG, _, _, dwhh = _lstm_bptt(whh[a:b], keep, h_all[a:b], c_all[a:b], acts[a:b], dhs[a:b], whh_nn=list(whh_nn[a:b]),
                                        want_dwhh=not defer, pre=pre)
            fold_p = ctx.pre.get("emb_player", -1) if (ctx.fold and pre is not None and pre.get("want_sums")) else -1
            if fold_p >= 0 and pre.get("act_sums") is None:
                raise RuntimeError("folded tracker-action embedding: the BPTT launch did not return the by-action sums of dG")
            for i, p in enumerate(grp):
                dfeat[p] = dG[i] @ wih[p]
                if p == fold_p:
                    # (feats[p] are the RAW fc features: dW_ih's product misses S^T E, added by embed_fold once the product is there)
                    fold_args = (pre["act_sums"], fa_w, fa_b, wih[p])
                    dfa = (torch.empty_like(fa_w), torch.empty_like(fa_b))
                if defer:
                    # both products of this player contract dG: registered with the grouped launch. dW_hh^T = dG^T (k h):
                    # the mask on h_{t-1} is keep[t-1] = the keep array shifted by one step of N rows, applied to dG's rows
                    r1 = q.add(dG[i], feats[p], wih[p], biases=(bih[p], bhh[p]))
                    if r1 is None:
                        r2 = None
                    elif ctx.hm is not None:       # (k h rows stored by the rollout: nothing to mask)
                        r2 = q.add(dG[i], ctx.hm[p], whh_nn[p])
                    else:
                        r2 = q.add(dG[i], h_all[p, :T].reshape(T * N, R), whh_nn[p], row_scale=keep, shift=N)
                    if r1 is not None and r2 is not None:
                        dwih[p], (dbi, dbh) = r1
                        dwhh_l[p] = r2[0]
                        db[p] = dbi
                        db2 = db2 if db2 is not None else [None] * P
                        db2[p] = dbh
                        if p == fold_p:          # (the slice is filled by the grouped launch at flush(): the fold follows it)
                            q.after.append(lambda fa_=fold_args, dw_=dwih[p], out_=dfa: embed_fold(*fa_, dw_, *out_))
                        continue
                    if r1 is not None:         # (cannot happen for R = 128; keep the queue consistent if it ever does)
                        raise RuntimeError("grouped weight gradients: dW_hh could not join the group after dW_ih did")
                    kprev = _keep_prev(keep).reshape(T * N)
                    dwhh_l[p] = gemm_tn(h_all[p, :T].reshape(T * N, R), dG[i], row_scale=kprev).t()
                    dwih[p], db[p] = gemm_tn(dG[i], feats[p], colsum=True)
                    if p == fold_p:
                        dwih[p] = dwih[p].contiguous()
                        embed_fold(*fold_args, dwih[p], *dfa)
                    continue
                dwih[p], db[p] = gemm_tn(dG[i], feats[p], colsum=True)
                if p == fold_p:
                    dwih[p] = dwih[p].contiguous()
                    embed_fold(*fold_args, dwih[p], *dfa)
                dwhh_l[p] = dwhh[i].t()
        if ctx.fold and ctx.pre is not None and ctx.need[ctx.pre.get("emb_player", 0)] and dfa[0] is None:
            raise RuntimeError("folded tracker-action embedding: no group of the backward pass produced its gradients")
        db_hh = tuple(db2[p] if (db2 is not None and db2[p] is not None) else db[p] for p in range(P))
        out = (None, None, None, None, None) + tuple(dfeat) + tuple(dwih) + tuple(dwhh_l) + tuple(db) + db_hh
        return out + (tuple(dfa) if ctx.fold else ())


@torch.no_grad()
def embed_fold(act_sums, fa_w, fa_b, wih, dwih, dfa_w, dfa_b):
    """The tracker-action embedding's share of the target's backward pass from the by-action column sums of dG (atr_embed_fold):
    dwih [J, C] += S^T E in place, dfa_w [C, 4] / dfa_b [C] = the gradients of fc_action_tracker. act_sums: what
    atr_lstm_bptt_pre2 (J = 4R) or atr_gru_bptt_sums (J = 3R) left per row tile."""
    J, Cc = wih.shape
    assert fa_w.shape == (Cc, 4) and fa_w.is_contiguous() and fa_b.is_contiguous() and wih.is_contiguous() and dwih.is_contiguous()
    assert dwih.shape == (J, Cc) and act_sums.numel() % (4 * J) == 0
    S = torch.empty((4, J), dtype=torch.float32, device=wih.device)
    lib().atr_embed_fold(_p(act_sums), act_sums.numel() // (4 * J), _p(fa_w), _p(fa_b), _p(wih), _p(dwih), _p(dfa_w), _p(dfa_b),
                         _p(S), J, Cc, _stream(wih))


def lstm_sequence_cached(lstms, feats, keep, h_all, c_all, acts, need=None, hm=None, pre=None, fold=None):
    """feats: per-player [T*N, F] (with grad); lstms: the nn.LSTMCells; stored activations from the rollout.
    need: per player, whether anything upstream of its hidden sequence is trained (None = all).
    hm: per player the MASKED previous hidden rows k_{t-1} h_{t-1} as [T*N, R] (row-strided views are fine) when the rollout
    stored them (model._act_step's one-GEMM path) — dW_hh then needs no row factors.
    pre: `acts` holds gate pre-activations without bias instead of activated gates (see _lstm_bptt)."""
    P = len(lstms)
    args = list(feats) + [l.weight_ih for l in lstms] + [l.weight_hh for l in lstms] + \
        [l.bias_ih for l in lstms] + [l.bias_hh for l in lstms]
    if fold is not None:     # fold = the tracker-aware player's fc_action_tracker: feats[pre['emb_player']] are then its RAW fc
        args += [fold.weight, fold.bias]     # features (no f + E[a] materialised), the embedding's gradients come from this node
    return _LstmSeqCached.apply(keep, h_all, c_all, acts, (need, hm, pre), *args)


def embed_fold_ok(pre, h_all, c_all, keep, fa):
    """Whether lstm_sequence_cached can fold the tracker-action embedding (the fused BPTT launch over stored pre-activations,
    the four-move action table, parameters as the kernels read them)."""
    return bool(fold_embedding and pre is not None and pre.get("emb") is not None and _fused_bptt_ok(h_all, c_all, keep)
                and fa.weight.shape[1] == 4 and fa.weight.is_contiguous() and fa.weight.data_ptr() % 16 == 0)


fold_embedding = os.environ.get("ATR_FOLD_EMBEDDING", "1") != "0"


@torch.no_grad()
def lstm_cell_into(ig, hg, c_prev, done, h_out, c_out, acts):
    """The rollout's LSTM step for one player, writing h, c and the activated gates into rollout-cache slots."""
    N, R = c_prev.shape
    lib().atr_lstm_cell_forward(_p(ig), None, _p(hg), _p(c_prev), 0, None, _pn(done), _p(h_out), 0, _p(c_out), 0,
                                _p(acts), 0, 1, N, R, _stream(ig))


@torch.no_grad()
def lstm_cell_act2_into(ig, hg, biases, c_prev, done, h_out, c_out, acts, sampler, actors, actions_out):
    """Both players' actor step after the GEMMs in ONE launch (players independent of each other's action): ig / hg
    [2,N,4R] (ig without bias), biases = (b0, b1) [4R] each, c_prev / h_out / c_out [2,N,R] and acts [2,N,4R] views with
    a player stride, actions_out [2,N] int64 contiguous. Only valid inside sampler.begin_block(); consumes two ordinals."""
    P, N, R = c_prev.shape
    assert P == 2 and sampler._ordinal is not None and ig.is_contiguous() and hg.is_contiguous() and actions_out.is_contiguous()
    for t in (c_prev, h_out, c_out, acts):
        assert t.stride(-1) == 1 and t.stride(-2) == t.shape[-1]
    ordinal = sampler._ordinal + 1
    sampler._ordinal += 2
    lib().atr_lstm_cell_forward_act2(
        _p(ig), _p(hg), _p(biases[0]), _p(biases[1]), _p(c_prev), c_prev.stride(0), _pn(done), _p(h_out), h_out.stride(0),
        _p(c_out), c_out.stride(0), _pn(acts), acts.stride(0) if acts is not None else 0, _p(actors[0].weight),
        _p(actors[0].bias), _p(actors[1].weight), _p(actors[1].bias), actors[0].weight.shape[0], _p(actions_out),
        _p(sampler.counter), sampler.seed, ordinal, N, R, _stream(ig))
    return actions_out


@torch.no_grad()
def lstm_cell_act_into(ig, hg, c_prev, done, h_out, c_out, acts, sampler, actor, actions_out, emb=None, act_in=None,
                       bias=None):
    """The actor's whole per-player step after the two GEMMs in ONE launch: masked LSTM cell (+ optional
    emb[act_in] added to the gates) written into the rollout-cache slots, then actor head + categorical draw on the
    fresh hidden row into actions_out (int64 [N]). bias [4R]: added to the pre-activations here (ig from a bias-free
    GEMM). Only valid inside sampler.begin_block()."""
    N, R = c_prev.shape
    assert sampler._ordinal is not None
    sampler._ordinal += 1
    if bias is not None:
        lib().atr_lstm_cell_forward_act1(_p(ig), _p(hg), _p(bias), _p(c_prev), _pn(done), _p(h_out), _p(c_out),
                                         _pn(acts), _pn(emb), _pn(act_in), _p(actor.weight), _p(actor.bias),
                                         actor.weight.shape[0], _p(actions_out), _p(sampler.counter), sampler.seed,
                                         sampler._ordinal, N, R, _stream(ig))
    else:
        lib().atr_lstm_cell_forward_act(_p(ig), _p(hg), _p(c_prev), _pn(done), _p(h_out), _p(c_out), _pn(acts),
                                        _pn(emb), _pn(act_in), _p(actor.weight), _p(actor.bias), actor.weight.shape[0],
                                        _p(actions_out), _p(sampler.counter), sampler.seed, sampler._ordinal, N, R,
                                        _stream(ig))
    return actions_out


def _rows(t):
    """(pointer, row stride) of a 2-D float32 tensor whose rows are contiguous."""
    assert t.dim() == 2 and t.stride(1) == 1 and t.dtype == torch.float32 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0
    return t.data_ptr(), t.stride(0)


@torch.no_grad()
def pair_linear(a1, w1, out, bias=None, a2=None, w2=None, done=None, relu=False):
    """out[p] = act(a1[p] @ w1[p].T [+ (k a2[p]) @ w2[p].T] + bias[p]) for the two players in ONE launch
    (atr_pair_linear, csrc/pair_gemm_hip.hip) — made for small row counts. a1[p] [M, k1p], w1[p] [N, k1p] (nn.Linear
    layout, contiguous), a2 / w2 optional second term, done [M] uint8: k = (done == 0) scales a2's rows; out[p] [M, N]."""
    g = PairLinearArgs()
    M, N = a1[0].shape[0], w1[0].shape[0]
    for p in range(2):
        assert a1[p].shape[0] == M and w1[p].shape[0] == N and w1[p].is_contiguous() and w1[p].shape[1] == a1[p].shape[1]
        g.a1[p], g.lda1[p] = _rows(a1[p])
        g.w1[p], g.k1[p] = w1[p].data_ptr(), a1[p].shape[1]
        if a2 is not None:
            assert w2[p].is_contiguous() and w2[p].shape == (N, a2[p].shape[1]) and a2[p].shape[0] == M
            g.a2[p], g.lda2[p] = _rows(a2[p])
            g.w2[p], g.k2[p] = w2[p].data_ptr(), a2[p].shape[1]
        g.bias[p] = bias[p].data_ptr() if bias is not None and bias[p] is not None else None
        assert out[p].shape == (M, N)
        g.c[p], g.ldc[p] = _rows(out[p])
    g.done = done.data_ptr() if done is not None else None
    g.M, g.N, g.relu = M, N, 1 if relu else 0
    lib().atr_pair_linear(C.byref(g), _stream(a1[0]))
    return out


def _act_step_args(ig, hg, biases, c_prev, done, h_out, c_out, acts, sampler, actors, actions_out, emb, hm_out):
    """atr_act_step for act_env_step / coop_env_step (their arguments; ig / hg / biases / acts: None, or None per player).
    Takes the sampler's next two ordinals."""
    N, R = h_out[0].shape
    assert sampler._ordinal is not None and actions_out.is_contiguous() and actions_out.shape == (2, N)
    ig, hg, biases, acts = (ts if ts is not None else (None, None) for ts in (ig, hg, biases, acts))
    ptr = lambda t: t.data_ptr() if t is not None else None
    a = ActStepArgs()
    for p in range(2):
        for t in (ig[p], c_prev[p], h_out[p], c_out[p]):
            assert t is None or (t.is_contiguous() and t.dtype == torch.float32)
        assert (hg[p] is None or hg[p].is_contiguous()) and (acts[p] is None or acts[p].is_contiguous())
        # (ig[0] None: the tracker's cell already ran as the epilogue of the step's gate product, fused.gate_cell)
        a.ig[p], a.hg[p], a.bias[p], a.acts[p] = ptr(ig[p]), ptr(hg[p]), ptr(biases[p]), ptr(acts[p])
        a.c_prev[p], a.h_out[p], a.c_out[p] = ptr(c_prev[p]), h_out[p].data_ptr(), ptr(c_out[p])
        a.actor_w[p], a.actor_b[p] = actors[p].weight.data_ptr(), actors[p].bias.data_ptr()
    a.emb, a.done_prev = ptr(emb), ptr(done)
    a.actions_out, a.counter, a.seed = actions_out.data_ptr(), sampler.counter.data_ptr(), sampler.seed
    a.ordinal = sampler._ordinal + 1
    sampler._ordinal += 2
    a.A, a.N, a.R = actors[0].weight.shape[0], N, R
    if hm_out is not None:
        assert hm_out[0].shape == (N, R) and hm_out[1].shape == (N, R)
        assert hm_out[0].stride(1) == 1 and hm_out[1].stride(1) == 1 and hm_out[0].stride(0) == hm_out[1].stride(0)
        a.hm_out[0], a.hm_out[1], a.hm_ld = hm_out[0].data_ptr(), hm_out[1].data_ptr(), hm_out[0].stride(0)
    return a


def _env_out_args(env_out):
    """(obs, obs_is_u8, rew, done) of the env-stepping launches from env_out = (obs u8 | f32, rew, done)."""
    obs, rew, done_out = env_out
    assert obs.is_contiguous() and rew.is_contiguous() and done_out.is_contiguous() and obs.dtype in (torch.uint8, torch.float32)
    return _p(obs), 1 if obs.dtype == torch.uint8 else 0, _p(rew), _p(done_out)


@torch.no_grad()
def act_env_step(env_core, ig, hg, biases, c_prev, done, h_out, c_out, acts, sampler, actors, actions_out, emb=None,
                 env_out=None, hm_out=None, greedy=False, eval_out=None):
    """The END of a rollout step as ONE launch (atr_act_env_step, csrc/track2d_hip.hip k_act_step): both players' cells +
    actor heads + draws (tracker first; emb [A,4R] adds emb[a_tracker] to the target's pre-activations) and, with
    env_core (a vec_env.VecTrack2D) and env_out = (obs [N,2,13,13] u8 | f32, rew [N,2], done [N] u8), the env step with
    those actions. ig / hg: per-player [N,4R] contiguous (hg[p] None: ig[p] is the whole pre-activation); biases (b0, b1)
    [4R] or None; c_prev / h_out / c_out per-player [N,R]; acts per-player [N,4R] or None; actions_out int64 [2,N].
    hm_out (with the env step only): per-player [N,R] views with a common row stride — they receive the fresh hidden rows
    zeroed where this step's done flag is set (what the next step's LSTMCell GEMM reads).
    Same results as lstm_cell_act_into x 2 + env.step. Only valid inside sampler.begin_block(); consumes two ordinals.
    greedy (with the env step only) + eval_out = (rsum f32 [N,2], length i32 [N], alive u8 [N]): the evaluation form
    (atr_eval_act_env_step, include/atr_eval.h) — same cells, the first maximal logit instead of the draw, and the evaluator's
    episode accounting in the same launch."""
    assert hm_out is None or env_core is not None
    a = _act_step_args(ig, hg, biases, c_prev, done, h_out, c_out, acts, sampler, actors, actions_out, emb, hm_out)
    if greedy:
        from . import evaluator
        if env_core is None or eval_out is None:
            raise RuntimeError("the greedy step exists with the env step and the evaluator's accounts only (atr_eval_act_env_step)")
        evaluator.eval_act_env_step(env_core, a, eval_out, env_out, _stream(h_out[0]))
        return actions_out
    if env_core is None:
        lib().atr_act_env_step(None, C.byref(a), None, 0, None, None, _stream(h_out[0]))
    else:
        lib().atr_act_env_step(env_core.h, C.byref(a), *_env_out_args(env_out), _stream(h_out[0]))
    return actions_out


@torch.no_grad()
def gru_act_env_step(env_core, g, b4, hm_in, h_out, acts, sampler, actors, actions_out, emb=None, env_out=None, hm_out=None,
                     greedy=False, eval_out=None):
    """act_env_step for the GRU cores (atr_gru_act_env_step, csrc/track2d_hip.hip k_gru_step; opt-in, --fused-gru): g per-player
    [N,4R] contiguous = the step's ONE product [features | k h_prev] W4^T (model.gru_step_consts), b4 per-player [4R], hm_in
    per-player [N,R] views with a common row stride = the masked previous hidden rows (the h columns of this step's rows), h_out
    per-player [N,R], acts per-player [N,4R] or None: receives (r, z, n, q); emb = E4 [A,4R] or None. No cell state, no done
    flags (the mask is in the rows). Everything else — draws, ordinals, env_out, hm_out, greedy + eval_out — as act_env_step."""
    assert hm_out is None or env_core is not None
    N, R = h_out[0].shape
    a = _act_step_args(g, None, b4, (None, None), None, h_out, (None, None), acts, sampler, actors, actions_out, emb, hm_out)
    for p in range(2):
        assert hm_in[p].shape == (N, R) and hm_in[p].stride(1) == 1 and hm_in[p].dtype == torch.float32
    assert hm_in[0].stride(0) == hm_in[1].stride(0)
    rows = (_p(hm_in[0]), _p(hm_in[1]), hm_in[0].stride(0))
    if greedy:
        from . import evaluator
        if env_core is None or eval_out is None:
            raise RuntimeError("the greedy step exists with the env step and the evaluator's accounts only "
                               "(atr_gru_eval_act_env_step)")
        evaluator.gru_eval_act_env_step(env_core, a, rows, eval_out, env_out, _stream(h_out[0]))
    elif env_core is None:
        lib().atr_gru_act_env_step(None, C.byref(a), *rows, None, 0, None, None, _stream(h_out[0]))
    else:
        lib().atr_gru_act_env_step(env_core.h, C.byref(a), *rows, *_env_out_args(env_out), _stream(h_out[0]))
    return actions_out


@torch.no_grad()
def gate_cell(fh, w_cat, biases, pre, c_prev, done, h_out, c_out, cell=(True, False), probe=None):
    """The step's LSTMCell product with the cell as its epilogue (atr_gate_cell, csrc/gate_cell_hip.hip): fh [2, N, K] rows
    [features | k h_prev] (a common row stride), w_cat [2, 4R, K] contiguous, pre [2, N, 4R] with contiguous [N, 4R] slabs
    (receives the product without bias), and for players with cell[p]: c_prev / h_out / c_out per-player [N, R] contiguous, biases per-player [4R]."""
    P, N, K = fh.shape
    a = GateCellArgs()
    assert P == 2 and fh.stride(2) == 1 and w_cat.is_contiguous() and w_cat.shape[0] == 2 and w_cat.shape[2] == K
    assert pre is None or (pre.shape == (2, N, w_cat.shape[1]) and pre[0].is_contiguous() and pre[1].is_contiguous())
    for p in range(2):
        a.a[p], a.w[p] = fh[p].data_ptr(), w_cat[p].data_ptr()
        a.pre[p] = pre[p].data_ptr() if pre is not None else None
        a.cell[p] = 1 if cell[p] else 0
        if cell[p]:
            for t in (c_prev[p], h_out[p], c_out[p], biases[p]):
                assert t.is_contiguous() and t.dtype == torch.float32
            a.bias[p], a.c_prev[p] = biases[p].data_ptr(), c_prev[p].data_ptr()
            a.h_out[p], a.c_out[p] = h_out[p].data_ptr(), c_out[p].data_ptr()
    a.done_prev = done.data_ptr() if done is not None else None
    a.lda, a.N, a.K, a.R = fh.stride(1), N, K, w_cat.shape[1] // 4
    a.probe = probe.data_ptr() if probe is not None else None
    lib().atr_gate_cell(C.byref(a), _stream(fh))


_stream_cus = {}


def register_stream_cus(stream, n_cus):
    """A stream created with a CU mask (train.cu_masked_stream): kernels launched on it see only n_cus compute units. Launches
    whose workgroups wait for each other (coop_env_step) size their grid by it."""
    _stream_cus[int(stream.cuda_stream)] = int(n_cus)


def stream_cus(device, stream=None):
    """Compute units available to `stream` (default: the current one): its registered CU mask, else the whole device."""
    st = torch.cuda.current_stream(device) if stream is None else stream
    n = _stream_cus.get(int(st.cuda_stream))
    return n if n is not None else int(torch.cuda.get_device_properties(device).multi_processor_count)


COOP_MAX_UNITS, COOP_WAVES = 16, 8       # (csrc/coop_gemm.h: kCoopMaxUnits, kCoopWaves)
COOP_PROBE = None                        # an int64 device tensor [workgroups, 8]: the kernel's phase stamps (tools/coop_step_timeline.py)


def coop_step_supported(N, F, R, workgroups):
    """The shape limits of atr_coop_env_step: every XCD takes N / 8 envs in whole 16-row tiles, a workgroup at most
    COOP_MAX_UNITS tiles per layer and COOP_WAVES env pairs."""
    if R != 128 or F <= 0 or F % 32 or N % 128 or workgroups < 8 or workgroups % 8:
        return False
    P, Rx = workgroups // 8, N // 8
    units_a, units_b = 2 * (Rx // 16) * (F // 32), 2 * (Rx // 16) * (4 * R // 32)
    return (-(-units_a // P) <= COOP_MAX_UNITS and -(-units_b // P) <= COOP_MAX_UNITS and -(-(Rx // 2) // P) <= COOP_WAVES)


@torch.no_grad()
def coop_env_step(env_core, ys, fcs, fh_t, w_cat, gates, biases, c_prev, done, h_out, c_out, acts, sampler, actors, actions_out,
                  emb, env_out, hm_out, workgroups):
    """A rollout step after the stem as ONE launch (atr_coop_env_step, csrc/track2d_hip.hip k_coop_step): fc + ReLU of both
    encoders (ys[p] [N, K_p] stem outputs, fcs[p] nn.Linear) into the feature columns of fh_t [2, N, F + R], the LSTMCell GEMM
    of both players over those rows (w_cat [2, 4R, F + R]) into `gates` [2, N, 4R], then what act_env_step does (cells, heads,
    draws, env step; biases = b_ih + b_hh per player; hm_out: the next step's hidden columns). Every XCD owns an eighth of the
    envs end to end; `workgroups` = the CUs the launch's stream may use (all of them must be free to be resident at once)."""
    N, R = c_prev[0].shape
    Fd = fcs[0].weight.shape[0]
    assert fh_t.shape == (2, N, Fd + R) and fh_t.stride(2) == 1 and fh_t.stride(1) == Fd + R
    assert w_cat.is_contiguous() and w_cat.shape == (2, 4 * R, Fd + R) and gates.is_contiguous() and gates.shape == (2, N, 4 * R)
    k = CoopStepArgs()
    for p in range(2):
        for t in (c_prev[p], h_out[p], c_out[p], biases[p], ys[p]):
            assert t.is_contiguous() and t.dtype == torch.float32
        assert ys[p].shape == (N, fcs[p].weight.shape[1]) and fcs[p].weight.is_contiguous() and fcs[p].weight.shape[0] == Fd
        k.y[p], k.ldy[p], k.kfc[p] = ys[p].data_ptr(), ys[p].stride(0), ys[p].shape[1]
        k.fc_w[p], k.fc_b[p], k.w_cat[p] = fcs[p].weight.data_ptr(), fcs[p].bias.data_ptr(), w_cat[p].data_ptr()
    assert hm_out is not None
    a = _act_step_args(None, None, biases, c_prev, done, h_out, c_out, acts, sampler, actors, actions_out, emb, hm_out)
    k.fh, k.gates, k.fh_pstride, k.fh_ld, k.F, k.workgroups = fh_t.data_ptr(), gates.data_ptr(), fh_t.stride(0), Fd + R, Fd, int(workgroups)
    k.probe = COOP_PROBE.data_ptr() if COOP_PROBE is not None else None
    lib().atr_coop_env_step(env_core.h, C.byref(a), C.byref(k), *_env_out_args(env_out), _stream(gates))
    return actions_out


def actor_step_supported(F, R):
    return F == 256 and R == 128


@torch.no_grad()
def actor_step_into(f, h_prev, c_prev, done, lstm, bias, h_out, c_out, acts, emb=None, act_in=None):
    """The actor's LSTMCell step as ONE MFMA kernel (csrc/actor_step_hip.hip): gates = f W_ih^T + (k h_prev) W_hh^T + bias
    [+ emb[act_in]] run straight into the cell; h', c' and the activated gates are written into the given (rollout
    cache) slots. f [N,256], h_prev / c_prev [N,128] contiguous; k = (done == 0)."""
    N, F = f.shape
    R = h_prev.shape[1]
    assert f.is_contiguous() and h_prev.is_contiguous() and c_prev.is_contiguous() and h_out.is_contiguous() and c_out.is_contiguous()
    lib().atr_actor_step(_p(f), _p(h_prev), _p(c_prev), _pn(done), _p(lstm.weight_ih), _p(lstm.weight_hh), _p(bias),
                         _pn(emb), _pn(act_in), _p(h_out), _p(c_out), _pn(acts), N, F, R, _stream(f))
    return h_out, c_out


def lstm_sequence(ig0, ig1, whh, h0, c0, keep):
    return _LstmSeq.apply(ig0, ig1, whh, h0, c0, keep)


@torch.no_grad()
def gae_returns(rewards, values, notdone, gamma, tau):
    """rewards [T,N,A,1], values [T+1,N,A,1] (row T = bootstrap), notdone [T,N] float -> (returns, gae) [T,N,A,1]."""
    T, N, A = rewards.shape[0], rewards.shape[1], rewards.shape[2]
    rewards, values, notdone = rewards.contiguous(), values.contiguous(), notdone.contiguous()
    ret, gae = torch.empty_like(rewards), torch.empty_like(rewards)
    lib().atr_gae_returns(_p(rewards), _p(values), _p(notdone), float(gamma), float(tau), _p(ret), _p(gae),
                          T, N, A, _stream(rewards))
    return ret, gae


def _col_stride(t):
    """Floats between consecutive rows of a [..., A] or [..., A, 1] store whose column the heads kernels address: A."""
    return t.shape[-2] if t.shape[-1] == 1 else t.shape[-1]


@torch.no_grad()
def heads_values(h, critic, values, off):
    """values[..., off] = critic(h) for h [rows, R] (csrc/heads_hip.hip); values: contiguous [..., A] float32 whose
    leading dims flatten to >= rows."""
    h = h.contiguous()
    rows, R = h.shape
    A = _col_stride(values)
    lib().atr_heads_values(_p(h), _p(critic.weight), _p(critic.bias), _p(values), rows, R, A, off, _stream(h))


@torch.no_grad()
def heads_values2(hs, critics, values):
    """heads_values for both players in one launch: values[..., p] = critics[p](hs[p]) for p = 0, 1."""
    h0, h1 = hs[0].contiguous(), hs[1].contiguous()
    rows, R = h0.shape
    assert h1.shape == h0.shape
    A = _col_stride(values)
    lib().atr_heads_values2(_p(h0), _p(critics[0].weight), _p(critics[0].bias), 0, _p(h1), _p(critics[1].weight),
                            _p(critics[1].bias), 1, _p(values), rows, R, A, _stream(h0))


def _act_layout(actions, rows):
    """(tensor whose data_ptr is the first action, act_n, act_tstride) for actions given as a flat [rows] vector or as a
    [T, N] view whose rows are contiguous (one player's column of the rollout's [T, players, N] store): read in place."""
    if actions.dim() == 2 and actions.stride(1) == 1 and actions.shape[0] * actions.shape[1] == rows:
        return actions, actions.shape[1], actions.stride(0)
    a = actions.reshape(rows).contiguous()
    return a, rows, 0


def _head_grads(dh, gs, A, R, has_aux):
    """[dh, dWa, dba, dWc, dbc, dWaux, dbaux] of one player from the kernel's grads_and_sums record (include/atr_policy.h)."""
    o = (A + 2) * R
    dwa, dwc, dwx = gs[:A * R].view(A, R), gs[A * R:(A + 1) * R].view(1, R), gs[(A + 1) * R:o].view(1, R)
    dba, dbc, dbx = gs[o:o + A], gs[o + A:o + A + 1], gs[o + A + 1:o + A + 2]
    return [dh, dwa, dba, dwc, dbc, dwx if has_aux else None, dbx if has_aux else None]


class _HeadsLossPair(torch.autograd.Function):
    """Both players' heads + A3C loss terms over all stored steps as ONE autograd node and one launch + one reduction launch
    (atr_heads_loss_multi): forward already produces dL/dh and the head-parameter gradients for coefficient 1; backward hands
    them out (the two outputs must enter the objective with coefficient 1 each — Agent._loss_fused_heads differentiates
    their sum). Inputs per player: h, actor w/b, critic w/b, aux w/b (None). Outputs: (term0, term1, stats [2, 4])."""

    @staticmethod
    def forward(ctx, cfg, *t):
        L = lib()
        arr = (HeadsLossArgs * 2)()
        hs, keep = [], []
        for p in range(2):
            h, wa, ba, wc, bc, waux, baux = t[7 * p:7 * p + 7]
            c = cfg[p]
            h = h.contiguous()
            rows, R = h.shape
            A = wa.shape[0]
            rec = (A + 2) * R + (A + 2) + 4
            dh = torch.empty_like(h)
            gs = torch.empty(rec + 1, dtype=torch.float32, device=h.device)
            ws = torch.empty(L.atr_heads_workspace_floats(rows, R, A), dtype=torch.float32, device=h.device)
            acts, act_n, act_ts = _act_layout(c["actions"], rows)
            ret = c["ret"]
            a = arr[p]
            a.h, a.actions, a.act_n, a.act_tstride = h.data_ptr(), acts.data_ptr(), act_n, act_ts
            a.ret, a.gae, a.val = ret.data_ptr(), c["gae"].data_ptr(), c["val"].data_ptr()
            a.stride = _col_stride(ret)
            a.off = c["off"]
            r_aux = c.get("r_aux")
            a.r_aux = r_aux.data_ptr() if r_aux is not None else None
            a.aux_stride = _col_stride(r_aux) if r_aux is not None else 0
            a.aux_off = c.get("aux_off", 0)
            a.wa, a.ba, a.wc = wa.data_ptr(), ba.data_ptr(), wc.data_ptr()
            a.waux = waux.data_ptr() if waux is not None else None
            a.baux = baux.data_ptr() if baux is not None else None
            a.scale, a.scale_aux, a.w_ent = float(c["scale"]), float(c["scale_aux"]), float(c["w_ent"])
            a.dh, a.grads_and_sums, a.workspace = dh.data_ptr(), gs.data_ptr(), ws.data_ptr()
            a.rows, a.R, a.A = rows, R, A
            hs.append((dh, gs, A, R, waux is not None, rec))
            keep += [h, acts, ws]
        stats = torch.empty((2, 4), dtype=torch.float32, device=hs[0][0].device)
        arr[0].stats_out, arr[1].stats_out = stats.data_ptr(), stats.data_ptr() + 16
        L.atr_heads_loss_multi(arr, 2, float(cfg[0]["stats_scale"]), _stream(hs[0][0]))
        ctx.save_for_backward(hs[0][0], hs[0][1], hs[1][0], hs[1][1])
        ctx.dims = [(x[2], x[3], x[4]) for x in hs]
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(stats)
        return hs[0][1][hs[0][5]], hs[1][1][hs[1][5]], stats

    @staticmethod
    def backward(ctx, g0, g1, gstats):
        sv = ctx.saved_tensors
        out = [None]
        for p in range(2):
            if (g0, g1)[p] is None:                 # this player's term is not part of the differentiated objective
                out += [None] * 7
            else:
                out += _head_grads(sv[2 * p], sv[2 * p + 1], *ctx.dims[p])
        return tuple(out)


def heads_loss_pair(hs, actors, critics, auxes, cfg):
    """-> (term0, term1, stats [2, 4]); cfg: per player dict(actions, ret, gae, val, off, r_aux, aux_off, scale, scale_aux, w_ent,
    stats_scale). The terms must be summed into the objective with coefficient 1 (their gradients are handed out as they are)."""
    t = []
    for p in range(2):
        aux = auxes[p]
        t += [hs[p], actors[p].weight, actors[p].bias, critics[p].weight, critics[p].bias,
              aux.weight if aux is not None else None, aux.bias if aux is not None else None]
    return _HeadsLossPair.apply(cfg, *t)


class _HeadsLoss(torch.autograd.Function):
    """One player's heads + A3C loss terms over all stored steps as ONE autograd node (csrc/heads_hip.hip): forward
    launches the fused kernel, which already produces dL/dh and the head-parameter gradients; backward hands them
    out. The output must enter the objective with coefficient 1 (Agent.loss_recompute adds the players' terms)."""

    @staticmethod
    def forward(ctx, h, wa, ba, wc, bc, waux, baux, actions, ret, gae, val, off, r_aux, aux_off, scale, scale_aux, w_ent,
                unit_coeff=False):
        L = lib()
        h = h.contiguous()
        rows, R = h.shape
        A = wa.shape[0]
        stride = _col_stride(ret)
        rec = (A + 2) * R + (A + 2) + 4
        dh = torch.empty_like(h)
        gs = torch.empty(rec + 1, dtype=torch.float32, device=h.device)
        ws = torch.empty(L.atr_heads_workspace_floats(rows, R, A), dtype=torch.float32, device=h.device)
        actions = actions.contiguous()
        aux_stride = _col_stride(r_aux) if r_aux is not None else 0
        L.atr_heads_loss(_p(h), _p(actions), _p(ret), _p(gae), _p(val), stride, off, _pn(r_aux), aux_stride, aux_off,
                         _p(wa), _p(ba), _p(wc), _pn(waux), _pn(baux), float(scale), float(scale_aux), float(w_ent),
                         _p(dh), _p(gs), _p(ws), rows, R, A, _stream(h))
        ctx.save_for_backward(dh, gs)
        ctx.dims = (A, R, waux is not None)
        ctx.unit_coeff = bool(unit_coeff)
        stats = gs[rec - 4:rec]
        ctx.mark_non_differentiable(stats)
        return gs[rec], stats

    @staticmethod
    def backward(ctx, gloss, gstats):
        dh, gs = ctx.saved_tensors
        if not ctx.unit_coeff:          # the kernel's gradients are those of coefficient 1: apply the incoming one
            dh, gs = dh * gloss, gs * gloss
        return tuple(_head_grads(dh, gs, *ctx.dims)) + (None,) * 11


def heads_loss(h, actor, critic, aux, actions, ret, gae, val, off, r_aux, aux_off, scale, scale_aux, w_ent,
               unit_coeff=False):
    """-> (objective contribution (0-dim, differentiable w.r.t. h and the head parameters),
           stats [4] = unscaled sums: policy term, value term, entropy, |aux error|).
    unit_coeff=True promises that the contribution enters the differentiated objective with coefficient exactly 1
    (Agent._loss_fused_heads adds the players' terms and differentiates the sum): backward then hands out the
    kernel's gradients as they are instead of scaling them by the incoming gradient."""
    return _HeadsLoss.apply(h, actor.weight, actor.bias, critic.weight, critic.bias,
                            aux.weight if aux is not None else None, aux.bias if aux is not None else None,
                            actions, ret, gae, val, off, r_aux, aux_off, scale, scale_aux, w_ent, unit_coeff)


class _EmbedAdd(torch.autograd.Function):
    """f + fc_action_tracker(one_hot(actions)) as a row gather (csrc/driver_hip.hip): forward one launch, backward the
    per-action column sums of the incoming gradient (two launches); the gradient w.r.t. f is the incoming one."""

    @staticmethod
    def forward(ctx, f, w, b, actions):
        if not (f.stride(1) == 1 and f.stride(0) >= f.shape[1] and f.stride(0) % 4 == 0):
            f = f.contiguous()       # (rows may be strided: the features as a column block of the rollout's [features | k h] rows)
        rows, Cc = f.shape
        A = w.shape[1]
        wc, bc = w.contiguous(), b.contiguous()
        out = torch.empty((rows, Cc), dtype=f.dtype, device=f.device)
        acts, act_n, act_ts = _act_layout(actions, rows)
        lib().atr_embed_add_ld(_p(f), f.stride(0), _p(wc), _p(bc), _p(acts), 1, act_n, act_ts, _p(out), rows, Cc, A,
                               _stream(f))
        ctx.save_for_backward(acts)
        ctx.dims = (Cc, A, act_n, act_ts)
        return out

    @staticmethod
    def backward(ctx, dout):
        (acts,) = ctx.saved_tensors
        Cc, A, act_n, act_ts = ctx.dims
        dout = dout.contiguous()
        rows = dout.shape[0]
        L = lib()
        ws = torch.empty(L.atr_embed_grad_workspace_floats(rows, Cc, A), dtype=torch.float32, device=dout.device)
        dw = torch.empty((Cc, A), dtype=torch.float32, device=dout.device)
        db = torch.empty(Cc, dtype=torch.float32, device=dout.device)
        L.atr_embed_grad(_p(dout), _p(acts), 1, act_n, act_ts, _p(dw), _p(db), _p(ws), rows, Cc, A, _stream(dout))
        return dout, dw, db, None


def embed_add(f, linear, actions):
    """f [rows, C] + linear(one_hot(actions, A)) for linear = nn.Linear(A, C); actions int64: a flat [rows] vector, or a [T, N]
    view with contiguous rows (one player's column of the rollout's [T, players, N] store, read in place)."""
    assert actions.dtype == torch.int64 and f.dim() == 2 and actions.numel() == f.shape[0]
    return _EmbedAdd.apply(f, linear.weight, linear.bias, actions)


use_gemm_tn = True
use_grouped_dw = True       # the learner's weight-gradient GEMMs of one backward pass as ONE grouped launch (DeferredWeightGrads)
_deferred = None            # the open DeferredWeightGrads of the backward pass in flight, if any


class DeferredWeightGrads(object):
    """The weight-gradient GEMMs of one backward pass, collected and launched together (atr_gemm_tn_grouped).

    Each cached-forward autograd node used to launch its own split-K GEMM, reduction and bias column-sum as it ran: 16
    launches for six products that share K = T*N rows, the small ones split into 128 K-slices to fill the chip on their own.
    Opened around torch.autograd.grad by Agent.compute_grads, this object lets those nodes only REGISTER their product
    (operands, the parameter it belongs to) and hands them the parameter's slice of the flat gradient bucket as the gradient
    they return — filled when flush() launches all products as one grouped GEMM + one reduction that writes straight into
    those slices (so FlatParams.set_grads has nothing to copy for them). Operands are kept alive until the flush."""

    MAX = 8

    def __init__(self, bucket):
        self.views = {}
        for prm, v in zip(bucket.params, bucket.grad_views()):
            self.views[prm.data_ptr()] = v
        self.problems, self.K, self.registered = [], None, set()
        self.after = []           # launches that need the group's outputs in place (run at the end of flush(), in order)

    def view(self, prm):
        return self.views.get(prm.data_ptr()) if prm is not None else None

    def _problem(self, x1, x2, weight, biases=(), row_scale=None, shift=0, rows=None):
        """The record of dW = x1^T x2 as add() describes it, or None when the product cannot join a group with K rows."""
        K, M = x1.shape
        N = x2.shape[1]
        whole = self.view(weight)
        bw = [self.view(b) for b in biases]
        if whole is None or any(v is None for v in bw) or len(bw) > 2:
            return None
        dst, bv = whole, bw
        if rows is not None:
            if whole.dim() != 2 or not (0 <= rows[0] < rows[1] <= whole.shape[0]):
                return None
            dst, bv = whole[rows[0]:rows[1]], [v[rows[0]:rows[1]] for v in bw]
        if ((self.K is not None and K != self.K) or K < 4096 or M % 128 or N % 128
                or not (x1.is_cuda and x1.dtype == torch.float32 and x2.dtype == torch.float32
                        and x1.stride(1) == 1 and x1.stride(0) >= M and x1.stride(0) % 4 == 0 and x1.data_ptr() % 16 == 0
                        and x2.stride(1) == 1 and x2.stride(0) >= N and x2.stride(0) % 4 == 0
                        and x2.data_ptr() % 16 == 0)
                or tuple(dst.shape) != (M, N) or any(tuple(v.shape) != (M,) for v in bv)
                or any(v.data_ptr() % 16 for v in [dst] + bv)
                or (row_scale is not None and not row_scale.is_contiguous())):
            return None
        return (x1, x2, dst, row_scale, int(shift), bv, M, N), (whole, bw)

    def _commit(self, rec):
        prob, (whole, bw) = rec
        self.K = prob[0].shape[0]
        self.problems.append(prob)
        self.registered.update(v.data_ptr() for v in [whole] + bw)       # (check(): what autograd gets back is the WHOLE slice)
        return whole, bw

    def add(self, x1, x2, weight, biases=(), row_scale=None, shift=0, rows=None):
        """Register dW = x1^T x2 -> `weight`'s gradient slice, colsum(x1) -> the slices of `biases` (<= 2). x1 may be a column
        block of a wider row-major tensor (16-byte aligned, row stride a multiple of 4 floats). rows = (r0, r1): the product is
        rows r0:r1 of the weight's gradient and its column sums rows r0:r1 of the biases' (the caller registers the other rows
        too). Returns (the parameter's WHOLE dW view, [whole bias views]) or None when this product cannot join the group
        (shape class, parameter not in the bucket, a different K, group full): the caller then computes it on the spot."""
        if len(self.problems) >= self.MAX:
            return None
        rec = self._problem(x1, x2, weight, biases, row_scale, shift, rows)
        return self._commit(rec) if rec is not None else None

    def add_all(self, products):
        """add() for products that join the group together or not at all (a list of add()'s keyword arguments): the list of
        their results, or None — the room is checked first, nothing is registered for a group that is merely full."""
        if len(self.problems) + len(products) > self.MAX:
            return None
        recs = [self._problem(**kw) for kw in products]
        if any(rec is None for rec in recs) or len(set(rec[0][0].shape[0] for rec in recs)) > 1:
            return None
        return [self._commit(rec) for rec in recs]

    def check(self, grads):
        """The gradients autograd handed back for the registered parameters must BE the bucket slices the nodes returned (a
        parameter feeding two nodes would make autograd sum into a fresh tensor before the slice is filled)."""
        got = set(g.data_ptr() for g in grads if g is not None)
        if not self.registered <= got:
            raise RuntimeError("grouped weight gradients: autograd did not return the registered bucket slices as they are "
                               "(a parameter with more than one gradient contribution?); set fused.use_grouped_dw = False")

    @torch.no_grad()
    def flush(self):
        if not self.problems:
            return
        n = len(self.problems)
        arr = (GemmTnProblem * n)()
        for q, (x1, x2, dst, rs, shift, bv, M, N) in enumerate(self.problems):
            arr[q].x1, arr[q].x2, arr[q].c = x1.data_ptr(), x2.data_ptr(), dst.data_ptr()
            arr[q].row_scale = rs.data_ptr() if rs is not None else None
            arr[q].row_scale_shift = shift
            arr[q].colsum0 = bv[0].data_ptr() if len(bv) > 0 else None
            arr[q].colsum1 = bv[1].data_ptr() if len(bv) > 1 else None
            arr[q].M, arr[q].N = M, N
            arr[q].ld1, arr[q].ld2 = x1.stride(0), x2.stride(0)
        L = lib()
        x0 = self.problems[0][0]
        ws = torch.empty(L.atr_gemm_tn_grouped_workspace_floats(arr, n, self.K), dtype=torch.float32, device=x0.device)
        L.atr_gemm_tn_grouped(arr, n, self.K, _p(ws), _stream(x0))
        self.problems, self.K = [], None
        for fn in self.after:
            fn()
        self.after = []


class deferred_weight_grads(object):
    """with deferred_weight_grads(bucket) as q: grads = torch.autograd.grad(...); q.flush()"""

    def __init__(self, bucket):
        self.bucket = bucket

    def __enter__(self):
        global _deferred
        self.q = DeferredWeightGrads(self.bucket) if (use_grouped_dw and use_gemm_tn and self.bucket.grad.is_cuda) else None
        _deferred = self.q
        return self.q

    def __exit__(self, *exc):
        global _deferred
        _deferred = None
        return False



class gemm_tn_corun(object):
    """`with fused.gemm_tn_corun(True):` — the weight-gradient launches issued (or captured) inside are planned for ONE workgroup
    per CU (atr_gemm_tn_set_corun, csrc/gemm_tn_hip.hip): ~1.4x the kernel's own time, but a chain of short kernels on another
    stream keeps running beside it. The pipelined schedule captures its learner graphs like this (train.PipelinedIteration)."""

    def __init__(self, on=True):
        self.on, self.was = bool(on), None

    def __enter__(self):
        self.was = lib().atr_gemm_tn_set_corun(1 if self.on else 0)
        return self

    def __exit__(self, *exc):
        lib().atr_gemm_tn_set_corun(self.was)
        return False


@torch.no_grad()
def gemm_tn(x1, x2, row_scale=None, colsum=False):
    """x1.t() @ x2 for tall row-major x1 [K,M], x2 [K,N] — the weight-gradient GEMMs (csrc/gemm_tn_hip.hip) when the
    shape fits the kernel (CUDA fp32, contiguous, 16-byte aligned, M and N multiples of 128), otherwise the library GEMM.
    row_scale [K]: x1's rows are multiplied by it first; colsum=True: also return (scaled x1).sum(0) — the bias
    gradient that goes with the weight gradient — from the same pass."""
    K, M = x1.shape
    N = x2.shape[1]
    if (use_gemm_tn and x1.is_cuda and x1.dtype == torch.float32 and x2.dtype == torch.float32 and M % 128 == 0
            and N % 128 == 0 and K >= 4096 and x1.is_contiguous() and x2.is_contiguous()
            and x1.data_ptr() % 16 == 0 and x2.data_ptr() % 16 == 0):       # (the kernel reads both 16 bytes at a time)
        L = lib()
        ws = torch.empty(L.atr_gemm_tn_workspace_floats(K, M, N), dtype=torch.float32, device=x1.device)
        c = torch.empty((M, N), dtype=torch.float32, device=x1.device)
        cs = torch.empty(M, dtype=torch.float32, device=x1.device) if colsum else None
        rs = row_scale.contiguous() if row_scale is not None else None
        L.atr_gemm_tn(_p(x1), _p(x2), _p(c), _p(ws), K, M, N, _pn(rs), _pn(cs), _stream(x1))
        return (c, cs) if colsum else c
    if row_scale is not None:
        x1 = x1 * row_scale.unsqueeze(1)
    c = x1.t() @ x2
    return (c, x1.sum(0)) if colsum else c


def rollout_consts_ok(consts):
    """Whether atr_rollout_begin2 can make these constants (contiguous, 16-byte aligned parameters)."""
    ts = []
    for l in consts["lstm"]:
        ts += [l.weight_ih, l.weight_hh, l.bias_ih, l.bias_hh]
    if "fa" in consts:
        ts += [consts["fa"].weight, consts["fa"].bias]
    return all(t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.data_ptr() % 16 == 0 for t in ts)


@torch.no_grad()
def rollout_begin(hxs, cxs, h_all, c_all, obs_src=None, obs_dst=None, consts=None, counter=None):
    """hxs/cxs [N,A,R] -> h_all/c_all[:, 0] ([A,T+1,N,R] rollout stores); optionally obs_src -> obs_dst (same bytes).
    consts (model.new_cache(defer_consts=True).consts) + counter (the action sampler's): the per-rollout constants of the actor
    and the counter bump in the same launch (atr_rollout_begin2)."""
    N, A, R = hxs.shape
    assert hxs.is_contiguous() and cxs.is_contiguous() and h_all.is_contiguous() and c_all.is_contiguous()
    assert h_all.shape[0] == A and h_all.shape[2] == N and h_all.shape[3] == R and hxs.dtype == torch.float32
    nbytes = 0
    if obs_src is not None:
        assert obs_src.is_contiguous() and obs_dst.is_contiguous()
        nbytes = obs_src.numel() * obs_src.element_size()
        assert nbytes == obs_dst.numel() * obs_dst.element_size() and nbytes % 4 == 0
    if consts is None:
        lib().atr_rollout_begin(_p(hxs), _p(cxs), _p(h_all), _p(c_all), h_all.stride(0), _pn(obs_src), _pn(obs_dst), nbytes,
                                N, A, R, _stream(hxs))
        return
    k = RolloutConsts()
    for p, l in enumerate(consts["lstm"]):
        k.w_ih[p], k.w_hh[p] = l.weight_ih.data_ptr(), l.weight_hh.data_ptr()
        k.b_ih[p], k.b_hh[p] = l.bias_ih.data_ptr(), l.bias_hh.data_ptr()
    k.bsum = consts["bsum"].data_ptr()
    k.F = int(consts["F"])
    if "w_cat" in consts:
        k.w_cat = consts["w_cat"].data_ptr()
        fh = consts["fh_all"]
        k.fh0, k.fh_pstride, k.fh_ld = fh.data_ptr(), fh.stride(0), fh.stride(2)
    if "emb_ih" in consts:
        fa = consts["fa"]
        k.fa_w, k.fa_b, k.emb_ih, k.A_act = fa.weight.data_ptr(), fa.bias.data_ptr(), consts["emb_ih"].data_ptr(), fa.weight.shape[1]
    if counter is not None:
        k.counter = counter.data_ptr()
    lib().atr_rollout_begin2(_p(hxs), _p(cxs), _p(h_all), _p(c_all), h_all.stride(0), _pn(obs_src), _pn(obs_dst), nbytes,
                              N, A, R, C.byref(k), _stream(hxs))


@torch.no_grad()
def rollout_end(h_all, c_all, dones, hxs, cxs, eps_len, keep, obs_src=None, obs_dst=None, done_dst=None):
    """Slot T of h_all/c_all [A,T+1,N,R], masked by dones[T-1], -> hxs/cxs [N,A,R] (in place); eps_len [N] int32 advanced
    over the rollout's dones [T,N] uint8 (in place); keep [T,N] float32 = (dones == 0). Optionally, in the same launch:
    obs_src -> obs_dst (same bytes: the observation the next rollout starts from) and dones[T-1] -> done_dst [N] uint8."""
    A, T1, N, R = h_all.shape
    T = T1 - 1
    assert dones.shape == (T, N) and dones.dtype == torch.uint8 and dones.is_contiguous()
    assert hxs.shape == (N, A, R) and hxs.is_contiguous() and cxs.is_contiguous() and keep.is_contiguous()
    assert eps_len.dtype == torch.int32 and eps_len.is_contiguous() and keep.shape == (T, N)
    nbytes = 0
    if obs_src is not None:
        assert obs_src.is_contiguous() and obs_dst.is_contiguous() and obs_src.dtype == obs_dst.dtype
        nbytes = obs_src.numel() * obs_src.element_size()
        assert nbytes == obs_dst.numel() * obs_dst.element_size() and nbytes % 4 == 0
    if done_dst is not None:
        assert done_dst.dtype == torch.uint8 and done_dst.is_contiguous() and done_dst.numel() == N
    lib().atr_rollout_end2(_p(h_all[0, T]), _p(c_all[0, T]), h_all.stride(0), _p(dones), _p(hxs), _p(cxs), _p(eps_len),
                           _p(keep), T, N, A, R, _pn(obs_src), _pn(obs_dst), nbytes, _pn(done_dst), _stream(hxs))


@torch.no_grad()
def adam_step(p, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, scalars, step_size, lr, beta1, beta2, eps, weight_decay,
              torch_eps=False):
    """SharedAdam.step over the flat bucket (csrc/driver_hip.hip): scalars = [step, beta1^step, beta2^step] float64;
    step_size: two floats of scratch. torch_eps: torch.optim.Adam's placement of eps and the bias corrections."""
    lib().atr_adam_step(_p(p), _p(grad), _p(exp_avg), _p(exp_avg_sq), _pn(max_exp_avg_sq), _p(scalars), _p(step_size),
                        float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), 1 if torch_eps else 0,
                        p.numel(), _stream(p))


@torch.no_grad()
def rmsprop_step(p, grad, square_avg, lr, alpha, eps, weight_decay):
    """SharedRMSprop.step (momentum 0, not centered) over the flat bucket (csrc/driver_hip.hip)."""
    lib().atr_rmsprop_step(_p(p), _p(grad), _p(square_avg), float(lr), float(alpha), float(eps), float(weight_decay),
                           p.numel(), _stream(p))
