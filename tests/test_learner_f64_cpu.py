"""The float64 learner reference (tests/learner_f64.py) against the reference-shaped per-step path in float64.

Agent.action_train + Agent.loss is the path tests/test_agent_loss.py and tests/test_model.py pin to the reference's
golden outputs. Run in float64 on a FakeVecEnv rollout — a non-zero starting LSTM state, episode ends inside the
window — it must give the helper's gradients and loss terms to 1e-10, for tat-maze-lstm (aux 'reward') and maze-lstm
(aux 'none') in every training mode. That makes the helper, which tests/test_learner_f64_gpu.py holds the HIP learner
to, a restatement of the tested CPU path rather than a formula of its own."""
import numpy as np
import pytest
import torch

import learner_f64
from test_distributed_cpu import FakeVecEnv
from active_tracking_rl_amd.model import build_model
from active_tracking_rl_amd.player_util import Agent
from active_tracking_rl_amd.train import default_args, rollout

N, T = 5, 7


class _RecordingEnv(FakeVecEnv):
    """FakeVecEnv with float64 observations that keeps every step's actions, observations, rewards and done flags."""

    def __init__(self, ids):
        super(_RecordingEnv, self).__init__(ids)
        self.log = None

    def reset(self):
        return super(_RecordingEnv, self).reset().double()

    def step(self, actions):
        o, r, d, info = super(_RecordingEnv, self).step(actions)
        if self.log is not None:
            self.log.append((torch.stack([a.reshape(-1) for a in actions], 1).clone(), o.clone(), r.clone(), d.clone()))
        return o.double(), r, d, info


def _per_step_run(network, aux, mode, draw="argmax"):
    """Two rollouts of the per-step path (the first one only moves the envs and the LSTM state on); the loss and
    gradients of the second, and the snapshot the helper takes in. draw: every categorical draw takes the most ("argmax")
    or the least ("argmin") likely action."""
    draws = []

    def argmax_draw(self, n, *a, **k):
        out = (self.argmax if draw == "argmax" else self.argmin)(1, keepdim=True)
        draws.append(out.view(-1).clone())
        return out
    saved_mult, saved_dtype = torch.Tensor.multinomial, torch.get_default_dtype()
    torch.Tensor.multinomial = argmax_draw
    torch.set_default_dtype(torch.float64)      # (Agent.loss's zero / coefficient tensors follow the default dtype)
    try:
        args = default_args(network=network, aux=aux, num_envs=N, num_steps=T, train_mode=mode)
        torch.manual_seed(4)
        env = _RecordingEnv(range(N))
        model = build_model(env.observation_space, env.action_space, args, torch.device("cpu")).double()
        if "gru" in network:
            # (biases start at zero, where b_hn inside r * (W_hn h + b_hn) cannot tell: the GRU case moves every 1-D parameter)
            g = torch.Generator().manual_seed(9)
            with torch.no_grad():
                for p in model.parameters():
                    if p.dim() == 1:
                        p.normal_(0, 0.1, generator=g)
        ag = Agent(model, env, args, None, torch.device("cpu"))
        ag.reset()
        rollout(ag, T, fast=False)
        ag.clear_actions()
        h0, c0 = ag.hxs.transpose(0, 1).detach().clone(), ag.cxs.transpose(0, 1).detach().clone()
        obs0 = ag.state.clone()
        env.log = []
        hs = []
        ag.update_rnn_hiden()
        for _ in range(T):                                   # (rollout(fast=False), keeping each step's masked state)
            ag.action_train()
            hs.append(ag.hxs.detach().transpose(0, 1).clone())
        del draws[:]
        loss, pl, vl, en, pr = ag.loss(mode)
        boot_action = draws[0].clone()                      # the bootstrap forward's tracker draw
        model.zero_grad()
        loss.backward()
        grads = {n: p.grad.clone() if p.grad is not None else None for n, p in model.named_parameters()}
    finally:
        torch.Tensor.multinomial = saved_mult
        torch.set_default_dtype(saved_dtype)
    acts, obs, rew, done = (torch.stack(x, 0) for x in zip(*env.log))
    snap = dict(obs=torch.cat([obs0.float().unsqueeze(0), obs], 0).reshape(T + 1, N, 2, 13, 13).float(), rewards=rew,
                dones=done, actions=acts, h0=h0, c0=c0, boot_action=boot_action,
                weights={k: v.detach().clone() for k, v in model.state_dict().items()},
                gamma=float(args.gamma), tau=float(args.tau), entropy=float(args.entropy),
                w_entropy_target=float(ag.w_entropy_target), aux=aux, network=network, rnn_out=int(args.rnn_out))
    terms = dict(policy=pl.detach().mean(0).view(2), value=vl.detach().mean(0).view(2), entropy=en.detach().mean(0).view(2),
                 aux=pr.detach().mean(0).view(1))
    snap["h_masked"] = torch.stack(hs, 0)                   # [T, 2, N, R]
    return snap, grads, terms, float(loss.detach())


@pytest.mark.parametrize("mode", [-1, 0, 1])
@pytest.mark.parametrize("network,aux", [("tat-maze-lstm", "reward"), ("maze-lstm", "none"), ("tat-maze-gru", "reward")])
def test_float64_reference_equals_the_per_step_path(network, aux, mode, draw="argmax"):
    snap, grads, terms, loss = _per_step_run(network, aux, mode, draw)
    dones = snap["dones"]
    assert snap["rnn_out"] == 128
    if "gru" in network:        # (a GRU's cell state is never written: what tests/test_gru_learner_f64_gpu.py's snapshots hold too)
        assert float(snap["c0"].abs().max()) == 0.0
    assert float(snap["h0"].abs().max()) > 0, "the window starts from a non-zero LSTM state"
    assert int(dones[:T - 1].sum()) >= 2 and len(set(np.nonzero(dones[:T - 1].numpy())[0].tolist())) >= 2, \
        "episode ends inside the window"
    ref = learner_f64.reference(snap, mode)
    assert abs(float(ref["loss"]) - loss) <= 1e-10 * abs(loss)
    n_cmp = 0
    for name, g in ref["grads"].items():
        want = grads[name]
        if want is None or float(want.abs().max()) == 0.0:
            assert float(g.abs().max()) == 0.0, name          # no gradient on the per-step path: none here either
            continue
        assert learner_f64.rel_err(g, want) <= 1e-10, (name, learner_f64.rel_err(g, want))
        n_cmp += 1
    assert n_cmp >= (10 if mode != -1 else 20)
    for k in learner_f64.TERMS:
        if k == "aux" and aux == "none":
            assert float(ref["terms"][k].abs().max()) == 0.0
            continue
        assert learner_f64.rel_err(ref["terms"][k], terms[k]) <= 1e-10, (k, ref["terms"][k], terms[k])
    # the hidden states: step t's output, masked by its done flag, is the state the per-step path carried on
    keep = (dones == 0).double().view(T, 1, N, 1)
    assert ref["h"].shape == (T, 2, N, snap["rnn_out"])
    assert learner_f64.rel_err(ref["h"] * keep, snap["h_masked"]) <= 1e-12


@pytest.mark.parametrize("mode", [-1, 1])
def test_bootstrap_draw_that_is_not_the_argmax_is_substituted(mode):
    """The helper's bootstrap forward takes the tracker action the learner drew, not the one its own fallback (the argmax)
    would take: with least-likely draws everywhere the recorded action differs from the argmax, and the helper still
    equals the per-step path (whose target value depends on that action)."""
    snap, _, _, _ = _per_step_run("tat-maze-lstm", "reward", mode, "argmin")
    ref_argmax = learner_f64.reference(dict(snap, boot_action=None), mode)
    assert learner_f64.rel_err(ref_argmax["boot_v"][:, 1], learner_f64.reference(snap, mode)["boot_v"][:, 1]) > 1e-6
    test_float64_reference_equals_the_per_step_path("tat-maze-lstm", "reward", mode, draw="argmin")


def test_reference_model_never_takes_the_fused_gru_step(monkeypatch):
    """model.py reads ATR_FUSED_GRU when a model is built: the reference's model has the switch off whatever the environment says,
    and reference() refuses a model handed in with it on."""
    snap, _, _, _ = _per_step_run("tat-maze-gru", "reward", -1)
    monkeypatch.setenv("ATR_FUSED_GRU", "1")
    args = default_args(network="tat-maze-gru")
    env = FakeVecEnv(range(N))
    assert build_model(env.observation_space, env.action_space, args, torch.device("cpu")).fused_gru_step is True
    m = learner_f64.build_reference_model(snap)
    assert m.fused_gru_step is False and m.gru_core and not m.cacheable_core
    m.fused_gru_step = True
    with pytest.raises(AssertionError, match="fused rollout step"):
        learner_f64.reference(snap, -1, model=m)


def test_env_subset_is_that_envs_share_of_the_gradient():
    """reference(envs=[j]) is env j's own loss terms (what the GPU test's resolution check divides by N): the per-env
    gradients, weighted 1/N, sum to the whole batch's gradient."""
    snap, _, _, _ = _per_step_run("tat-maze-lstm", "reward", -1)
    whole = learner_f64.reference(snap, -1)
    parts = [learner_f64.reference(snap, -1, envs=[j]) for j in range(N)]
    for name, g in whole["grads"].items():
        s = sum(p["grads"][name] for p in parts) / N
        if float(g.norm()) == 0.0:
            assert float(s.norm()) == 0.0
            continue
        assert learner_f64.rel_err(s, g) <= 1e-12, name
