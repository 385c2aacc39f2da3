"""What tests/test_greedy_eval_cpu.py and tests/test_greedy_eval_gpu.py share: the policy fixture of the whole-round tests, the
near-tie rule, and the reference path of a greedy evaluation round on the CPU (the eager model over the C oracle).

The fixture: the seeded initial weights of build_model with both actor_linear weights multiplied by 100. The actor rows are
initialised with norm 0.01 (model.norm_col_init), so the initial logit gaps would be of the order of the 1e-7 arithmetic
differences between two evaluations of the cells; x 100 puts them at the order of 0.1, and an argmax is then a statement about
the policy and not about rounding.

A near-tie is a row whose top-2 logit gap is at most NEAR_TIE (1e-4); at most CAP (1 %) of a round's rows may be near-ties."""
import numpy as np
import torch

from oracle import oracle as orc

NEAR_TIE = 1e-4
CAP = 0.01
ACTOR_SCALE = 100.0
EVAL_BASE = 1 << 20         # test.evaluate's env_id_base


def fixture_args(env_id, episodes, **over):
    from active_tracking_rl_amd.train import default_args
    return default_args(env=env_id, env_base=env_id, test_eps=episodes, num_envs=max(2, episodes), seed=1, **over)


def fixture_model(args, device="cpu"):
    """The fixture policy, built on the CPU from args.seed (the same weights on every device)."""
    from active_tracking_rl_amd.environment import _spaces
    from active_tracking_rl_amd.model import build_model
    torch.manual_seed(args.seed)
    obs_space, act_space = _spaces((13, 13))
    model = build_model(obs_space, act_space, args, torch.device("cpu"))
    with torch.no_grad():
        for p in (model.player0, model.player1):
            p.actor.actor_linear.weight.mul_(ACTOR_SCALE)
    return model.to(device)


def top2_gap(logits):
    s = np.sort(np.asarray(logits, np.float64), axis=-1)
    return s[..., -1] - s[..., -2]


def oracle_batch(env_id, n, seed=1, base=EVAL_BASE, max_steps=None):
    from active_tracking_rl_amd import registry
    sp = registry.spec(env_id)
    ms = sp["max_episode_steps"] if max_steps is None else max_steps
    return orc.OracleBatch([orc.OracleEnv(sp["map_type"], sp["target_mode"], sp["level"], ms, orc.RNG_PHILOX, seed, base + i)
                            for i in range(n)])


@torch.no_grad()
def eager_logits(model, obs, h_prev, c_prev):
    """The eager policy (A3C_Dueling.forward, test=True) on obs [N,2,13,13] and states [2,N,R] (already masked): both players'
    logits [2,N,A] (numpy float64 of the float32 values), actions [2,N], and the new states."""
    dev = next(model.parameters()).device
    st = torch.as_tensor(obs, dtype=torch.float32, device=dev).view(-1, 2, 1, 1, 13, 13)
    hx = torch.as_tensor(h_prev, dtype=torch.float32, device=dev).transpose(0, 1).contiguous()
    cx = torch.as_tensor(c_prev, dtype=torch.float32, device=dev).transpose(0, 1).contiguous()
    _, acts, _, _, (hx, cx), _ = model((st, (hx, cx)), True)
    players = (model.player0, model.player1)
    logits = np.stack([players[p].actor.actor_linear(hx[:, p]).double().cpu().numpy() for p in range(2)])
    return logits, np.stack([a.cpu().numpy() for a in acts]), hx.transpose(0, 1).cpu().numpy(), cx.transpose(0, 1).cpu().numpy()


def reference_round(model, env_id, episodes, seed=1, max_steps=None, limit=500):
    """The greedy round by the reference path alone: the eager model on the CPU over the oracle envs test.evaluate's shard
    names (env_id_base 1 << 20, the same seed), every env until its first episode ends. Returns dict(rsum, length, rows,
    near_ties): rows = (alive env, player) rows evaluated, near_ties = those with a top-2 gap <= NEAR_TIE."""
    n = max(2, episodes)
    ob = oracle_batch(env_id, n, seed, max_steps=max_steps)
    obs = ob.reset()
    R = model.player0.lstm.hidden_size
    h, c = np.zeros((2, n, R), np.float32), np.zeros((2, n, R), np.float32)
    rsum, length, alive = np.zeros((n, 2), np.float32), np.zeros(n, np.int32), np.ones(n, bool)
    rows = ties = 0
    for _ in range(limit):
        logits, acts, h, c = eager_logits(model, obs, h, c)
        gap = top2_gap(logits)                                        # [2, N]
        rows += 2 * int(alive.sum())
        ties += int((gap[:, alive] <= NEAR_TIE).sum())
        obs, rew, done = ob.step(np.ascontiguousarray(acts.T))
        rsum = (rsum + np.where(alive[:, None], rew.astype(np.float32), np.float32(0))).astype(np.float32)
        length += alive.astype(np.int32)
        alive &= done == 0
        keep = (done == 0).astype(np.float32)[None, :, None]
        h, c = h * keep, c * keep
        if not alive.any():
            break
    return dict(rsum=rsum[:episodes], length=length[:episodes], rows=rows, near_ties=ties)
