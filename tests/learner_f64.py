"""Float64 reference of one learner pass, built on the package's CPU path (no project kernel anywhere).

The learner turns a stored rollout into the flat gradient bucket. This module re-evaluates the same loss from the same
inputs with plain PyTorch ops in float64 on the CPU, so that the GPU learner (stem backward, one-launch BPTT, embedding
fold, grouped dW launch, heads + loss kernel, GAE) can be compared with something that shares none of its code:

    snap = snapshot(player)                   # rollout stores, starting LSTM state, bootstrap draw, weights -> CPU
    ref = reference(snap, mode)               # float64 on the CPU
    floor = reference(snap, mode, dtype=torch.float32, device="cuda:0")   # PyTorch's own fp32, project kernels off

The evaluation is the one of Agent.loss_recompute: the encoder over every stored frame (CNN_maze's Toeplitz GEMMs on
the CPU), both recurrent cells through model.lstm_sequence / gru_sequence (masked after each step), the heads, the
bootstrap forward with the tracker action the learner's bootstrap step drew, then the host returns / GAE loop and the
loss of the training mode. tests/test_learner_f64_cpu.py pins it to the reference-shaped per-step path (Agent.action_train + Agent.loss).
"""
import argparse
import contextlib

import torch
import torch.nn.functional as F

from active_tracking_rl_amd import fused
from active_tracking_rl_amd import model as model_mod
from active_tracking_rl_amd.environment import _spaces
from active_tracking_rl_amd.model import CNN_maze, _recurrence, build_model

TERMS = ("policy", "value", "entropy", "aux")
# the tolerance rule of tests/test_learner_f64_gpu.py (its module docstring) and tests/f64_rule.py
FACTOR, FLOOR, ATEN_MAX, RESOLUTION = 4.0, 1e-6, 1e-4, 10.0
# The stored hidden states come from the rollout's cell kernels, whose sigmoid / tanh are the hardware exp + reciprocal forms
# of csrc/atr_cell.h (tanh(x) = 1 - 2 / (1 + e^2x): ~1e-7 ABSOLUTE, so a larger relative error on small states than libm's).
# Measured on MI355X over every case below: e(hip) 1.07e-6 .. 2.10e-6 against e(aten32) 2.1e-7 .. 2.6e-7 (up to 8.2x). The
# learner's gradients are held to the rule above; the hidden states to max(4 e(aten32), HIDDEN_FLOOR). What that still
# resolves: e is taken per player over all T steps, so an error confined to one step must reach ~sqrt(T) x 4e-6 of that
# step's own norm (about 2e-5 at T = 20) to show — a done mask applied one step late moves the hidden rows of every env that
# ended there by O(1), orders of magnitude above it; the cell kernels' own rounding does not reach it.
# The GRU cores' cached step (k_gru_step, --fused-gru; tests/test_gru_learner_f64_gpu.py, 130 x 8 eager to 1024 x 4 captured)
# measured e(hip) 1.91e-7 .. 2.30e-7 against e(aten32) 1.18e-7 .. 1.97e-7 (at most 1.8x): inside 4 e(aten32) already, so the GRU
# cases use this floor as it is and no GRU_HIDDEN_FLOOR exists. Against it a done mask applied one step late still shows: with a
# 37-step TimeLimit about 1 env in 37 ends at a given step, its next hidden row moves by O(1) of its norm, which is e ~ sqrt(1 / (37 T))
# = 0.06 at T = 8 over the player's whole h_all — four orders of magnitude above the floor.
HIDDEN_FLOOR = 4e-6


def snapshot(player, boot_action=None, actions=None):
    """CPU copies of what the learner of `player`'s last rollout read: observations [T+1, N, 2, 13, 13] (slot T is the
    bootstrap state), rewards [T, N, 2], dones [T, N], actions [T, N, 2], the LSTM state the rollout started from
    (h0 / c0 [2, N, R], already masked by the previous rollout's last done), the tracker action of the bootstrap step
    (tat networks), the weights, and the loss coefficients. boot_action: the bootstrap draw when it is not in the
    rollout cache. actions [T, N, 2]: the rollout's actions where it ran without a cache (the GRU cores; taken before the
    learner clears the Agent's lists) — h0 / c0 are then the Agent's own."""
    cache, buf = player._cache, player._buf
    assert buf is not None, "a rollout stored in place"
    m = player.model
    if cache is not None:
        T = cache.T
        actions = player._actions_buf.transpose(1, 2)
        h0, c0 = cache.h_all[:, 0], cache.c_all[:, 0]
        if boot_action is None and m.tat:
            boot_action = cache.boot.actions[0]
    else:
        assert actions is not None, "a rollout without a cache: pass its actions"
        T = actions.shape[0]
        h0, c0 = player.h0.transpose(0, 1), player.c0.transpose(0, 1)
    a = player.args
    return dict(obs=buf[0][:T + 1].detach().cpu().clone(), rewards=buf[1][:T].detach().cpu().clone(),
                dones=buf[2][:T].detach().cpu().clone(), actions=actions.cpu().clone(),
                h0=h0.detach().cpu().clone(), c0=c0.detach().cpu().clone(),
                boot_action=boot_action.detach().cpu().clone() if boot_action is not None else None,
                weights={k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
                gamma=float(a.gamma), tau=float(a.tau), entropy=float(a.entropy),
                w_entropy_target=float(player.w_entropy_target), aux=str(a.aux), network=str(a.network),
                rnn_out=int(a.rnn_out))


@contextlib.contextmanager
def _no_project_kernels():
    """Every launch of the package's HIP kernels goes through fused.lib(): make it an error while the reference runs."""
    saved = fused.lib

    def refuse():
        raise AssertionError("the reference evaluation reached a project kernel")
    fused.lib = refuse
    saved_lstm, saved_gru = model_mod.fused_lstm, model_mod.fused_gru
    model_mod.fused_lstm = model_mod.fused_gru = False
    try:
        yield
    finally:
        fused.lib = saved
        model_mod.fused_lstm, model_mod.fused_gru = saved_lstm, saved_gru


@contextlib.contextmanager
def _bootstrap_draw(action):
    """sample_action's multinomial returns `action` for the first draw (the tracker's) and the argmax after it."""
    saved = torch.Tensor.multinomial
    calls = [0]

    def draw(self, n, *a, **k):
        calls[0] += 1
        if calls[0] == 1 and action is not None:
            return action.to(self.device).view(-1, 1)
        return self.argmax(1, keepdim=True)
    torch.Tensor.multinomial = draw
    try:
        yield
    finally:
        torch.Tensor.multinomial = saved


def build_reference_model(snap, dtype=torch.float64, device="cpu"):
    """The network of `snap` with its weights, in `dtype` on `device`, every CNN_maze on its PyTorch stem."""
    args = argparse.Namespace(network=snap["network"], stack_frames=1, rnn_out=snap["rnn_out"], single=False)
    obs_s, act_s = _spaces(tuple(snap["obs"].shape[-2:]))
    with torch.random.fork_rng(devices=[]):
        m = build_model(obs_s, act_s, args, torch.device("cpu"))
    m = m.to(device=device, dtype=dtype)
    m.load_state_dict(snap["weights"])
    for mod in m.modules():
        if isinstance(mod, CNN_maze):
            mod.use_fused = False
            mod._dense = None
    m.fused_sampling = False
    # (a GRU model reads ATR_FUSED_GRU from the environment when it is built: the reference never takes the cached, env-fused step)
    m.fused_gru_step = False
    return m


def _slice_envs(snap, envs):
    out = dict(snap)
    for k in ("obs", "rewards", "dones", "actions"):
        out[k] = snap[k][:, envs]
    for k in ("h0", "c0"):
        out[k] = snap[k][:, envs]
    if snap["boot_action"] is not None:
        out["boot_action"] = snap["boot_action"][envs]
    return out


def reference(snap, mode, dtype=torch.float64, device="cpu", envs=None, model=None):
    """Loss and gradients of the learner pass over `snap` for training mode `mode` (-1 both players, 0 tracker, 1 target).
    envs: a subset of env indices (the loss is then the mean over those envs). Returns a dict:
      grads    {parameter name: gradient} (zeros where the loss does not depend on the parameter)
      terms    {"policy", "value", "entropy": [2], "aux": [1]} averaged over envs
      boot_v   [N, 2] the bootstrap values V(s_T)
      h        [T, 2, N, R] the un-masked hidden state of every step (what the rollout stores in h_all[:, 1:])"""
    if envs is not None:
        snap = _slice_envs(snap, envs)
    dev = torch.device(device)
    if dev.type == "cpu":
        for k, v in snap.items():
            if torch.is_tensor(v):
                assert v.device.type == "cpu", k
        for k, v in snap["weights"].items():
            assert v.device.type == "cpu", k
    if model is None:
        model = build_reference_model(snap, dtype, dev)
    assert not getattr(model, "fused_gru_step", False), "the reference model must not take the GRU cores' fused rollout step"
    blas = None
    if dev.type == "cuda":
        # (the floor's GEMMs on the BLAS library's classic kernels: the Lt heuristic's pick for some ragged shapes — the
        # tracker's stem / fc weight gradients over 20020 rows — was measured 50x less accurate than fp32 summation elsewhere)
        blas = torch.backends.cuda.preferred_blas_library()
        torch.backends.cuda.preferred_blas_library("cublas")
    try:
        with _no_project_kernels():
            out = _evaluate(model, snap, mode, dtype, dev)
    finally:
        if blas is not None:
            torch.backends.cuda.preferred_blas_library(blas)
    if dev.type == "cpu":
        for k, v in out["grads"].items():
            assert v.device.type == "cpu" and v.dtype == dtype, k
    return out


def _evaluate(model, snap, mode, dtype, dev):
    obs = snap["obs"].to(dev).to(dtype)                      # (u8 frames converted here: CNN_maze casts them to float32)
    T, N = snap["dones"].shape
    hw = obs.shape[-2:]
    rewards = snap["rewards"].to(dev).to(dtype).unsqueeze(3)  # [T, N, 2, 1]
    nd = (snap["dones"].to(dev) == 0).to(dtype)              # [T, N]
    actions = snap["actions"].to(dev).long()                 # [T, N, 2]
    h0, c0 = snap["h0"].to(dev).to(dtype), snap["c0"].to(dev).to(dtype)
    p0, p1 = model.player0, model.player1
    st = obs[:T].reshape(T, N, 2, 1, 1, *hw)
    f0 = p0.sequence_features(st[:, :, 0])
    if model.tat:
        a2t = F.one_hot(actions[:, :, 0], model.action_dim_tracker).to(dtype)
        f1 = p1.sequence_features(st.reshape(T, N, 2, 1, *hw), a2t)
    else:
        f1 = p1.sequence_features(st[:, :, 1])
    # (a stacked [T, P, N, F] tensor: lstm_sequence's ATen form)
    h_seq, hT, cT = _recurrence(p0.lstm)([p0.lstm, p1.lstm], torch.stack([f0, f1], 1), h0, c0, nd)
    v0, e0, l0 = p0.sequence_heads(h_seq[:, 0], actions[:, :, 0])
    R_pred = None
    if model.tat:
        v1, e1, l1, R_pred = p1.sequence_heads(h_seq[:, 1], actions[:, :, 1])
    else:
        v1, e1, l1 = p1.sequence_heads(h_seq[:, 1], actions[:, :, 1])
    values, entropies, log_probs = torch.stack([v0, v1], 2), torch.stack([e0, e1], 2), torch.stack([l0, l1], 2)
    with torch.no_grad(), _bootstrap_draw(snap["boot_action"]):
        # V(s_T) (player_util.py:109-117): one more forward from the final state, masked by the last done
        boot = model((obs[T].reshape(N, 2, 1, 1, *hw), (hT.transpose(0, 1), cT.transpose(0, 1))))[0]
    gamma, tau = snap["gamma"], snap["tau"]
    with torch.no_grad():                                    # returns and GAE: the CPU branch of Agent.loss_recompute
        v = torch.cat([values.detach(), boot.unsqueeze(0)], 0)
        ndv = nd.view(T, N, 1, 1)
        R = torch.empty_like(rewards)
        gae = torch.empty_like(rewards)
        r_run, g_run = v[T], torch.zeros_like(v[T])
        for i in reversed(range(T)):
            r_run = gamma * r_run * ndv[i] + rewards[i]
            delta_t = rewards[i] + gamma * v[i + 1] * ndv[i] - v[i]
            g_run = g_run * gamma * tau * ndv[i] + delta_t
            R[i], gae[i] = r_run, g_run
    w_ent = torch.tensor([snap["entropy"], snap["w_entropy_target"]], dtype=dtype, device=dev).view(1, 1, 2, 1)
    value_loss = (0.5 * (R - values).pow(2)).sum(0)          # [N, 2, 1]
    policy_loss = (-(log_probs * gae) - w_ent * entropies).sum(0)
    use_aux = 'reward' in snap["aux"] and R_pred is not None
    pred_loss = (R_pred - rewards[:, :, 0]).abs().sum(0) if use_aux else torch.zeros(N, 1, dtype=dtype, device=dev)
    loss_tracker = (policy_loss[:, 0] + 0.5 * value_loss[:, 0]).mean()
    loss_target = (policy_loss[:, 1] + 0.5 * value_loss[:, 1]).mean()
    loss = loss_tracker if mode == 0 else loss_target if mode == 1 else loss_tracker + loss_target
    if use_aux and mode != 0:
        loss = loss + pred_loss.mean()
    names = [n for n, _ in model.named_parameters()]
    params = [p for _, p in model.named_parameters()]
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    grads = {n: (g if g is not None else torch.zeros_like(p)).detach() for n, p, g in zip(names, params, grads)}
    terms = dict(policy=policy_loss.detach().mean(0).view(2), value=value_loss.detach().mean(0).view(2),
                 entropy=entropies.detach().sum(0).mean(0).view(2), aux=pred_loss.detach().mean(0).view(1))
    return dict(grads=grads, terms=terms, boot_v=boot.detach().view(N, 2), h=h_seq.detach(), loss=loss.detach())


def rel_err(x, ref):
    """e(x) = ||x - ref|| / ||ref|| in float64 (inf when ref is zero and x is not, 0 when both are)."""
    x, ref = x.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    d, r = float((x - ref).norm()), float(ref.norm())
    if r == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / r
