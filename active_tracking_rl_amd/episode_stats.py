"""episode_stats — returns and lengths of the episodes that END during training, kept on the device (include/atr_stats.h;
csrc/episode_stats_hip.hip).

The reference's worker adds `player.reward` to `reward_sum` on the host every env step and writes train/reward_0 / train/reward_1
when the episode ends (train.py:63-88). A replayed rollout graph cannot read the host per step, so here the accounts of all N
envs of a shard live in four device tensors and advance in ONE launch per rollout (train.rollout calls update() on the step
rewards and done flags the rollout has just stored — inside the captured rollout graph where there is one):

    run_ret f32 [N,2], run_len i32 [N]    the episode each env is in: return so far per player, steps so far
    fin     f64 [N,8]                     per env, over its finished episodes: count, sum R0, R1, R0^2, R1^2, L, L^2, successes
    totals  f64 [8]                       drain(): the sum of fin over the shard (fin zeroed by the same launch)

The accounts belong to the ENV SHARD (env.episode_stats), not to a player: the two replicas of train.PipelinedIteration
alternate rollouts over one shard and an episode routinely begins in one replica's rollout and ends in the other's. Sums of
sums pool exactly, which is why the kernel keeps squares and not variances: across ranks the float64 totals are all-reduced
(pooled) and summarize() turns them into what gym_eval.py:110-125 of the reference reports (population mean / std of return
and length, success rate = share of episodes that reached the time limit, mean reward per step).

The binding of the new header is declared here (STATS_PROTOTYPES, held to include/atr_stats.h by tests/test_episode_stats_cpu.py),
apart from fused.ATR_PROTOTYPES and evaluator.EVAL_PROTOTYPES."""
import ctypes as C
import math

import numpy as np
import torch

from . import vec_env

FIELDS = 8             # ATR_STATS_FIELDS: count, R0, R1, R0^2, R1^2, L, L^2, successes
DRAIN_LANES = 32       # ATR_STATS_DRAIN_LANES: row lanes of the drain's summation order
TAGS = ("train/reward_0", "train/reward_1", "train/eps_len", "train/success_rate", "train/episodes", "train/reward_step_0",
        "train/reward_step_1")

# {entry point: (restype, [argtypes])} for every function include/atr_stats.h declares
STATS_PROTOTYPES = {
    "atr_episode_stats": (C.c_int, [C.c_void_p, C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p, C.c_longlong, C.c_longlong,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "atr_episode_stats_drain": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
}
_lib = None


def _errcheck(name):
    """As fused._errcheck: a non-zero status raises RuntimeError naming the entry point, with the library's own text."""
    def check(status, func=None, args=None):
        if status != 0:
            raise RuntimeError("%s failed (%d): %s" % (name, status, vec_env.load_library().t2d_last_error().decode()))
        return status
    return check


def lib():
    global _lib
    if _lib is None:
        L = vec_env.load_library()
        for name, (restype, argtypes) in STATS_PROTOTYPES.items():
            f = getattr(L, name)         # (a library without the symbol is an error: there is no other accounting)
            f.restype, f.argtypes = restype, argtypes
            f.errcheck = _errcheck(name)
        _lib = L
    return _lib


def account(rew, done, run_ret=None, run_len=None, fin=None, success_len=500):
    """Host model of k_episode_stats: rew [T,N,2] f32 and done [T,N] of consecutive steps -> (run_ret f32 [N,2], run_len i32 [N],
    fin f64 [N,8]), continuing from the given accounts (default: a fresh shard's zeros). The kernel's expressions in the kernel's
    order — float32 sums in step order, every float64 product rounded before it is added — so equal bit for bit."""
    rew, done = np.asarray(rew, np.float32), np.asarray(done)
    T, n = rew.shape[0], rew.shape[1]
    rew = rew.reshape(T, n, 2)
    run_ret = np.zeros((n, 2), np.float32) if run_ret is None else np.array(run_ret, np.float32)
    run_len = np.zeros(n, np.int32) if run_len is None else np.array(run_len, np.int32)
    fin = np.zeros((n, FIELDS), np.float64) if fin is None else np.array(fin, np.float64)
    for t in range(T):
        run_ret = (run_ret + rew[t]).astype(np.float32)
        run_len = (run_len + 1).astype(np.int32)
        d = np.asarray(done[t]).reshape(n) != 0
        if d.any():
            R = run_ret[d].astype(np.float64)
            L = run_len[d].astype(np.float64)
            add = np.stack([np.ones_like(L), R[:, 0], R[:, 1], R[:, 0] * R[:, 0], R[:, 1] * R[:, 1], L, L * L,
                            (run_len[d] >= int(success_len)).astype(np.float64)], 1)
            fin[d] = fin[d] + add
            run_ret[d] = 0.0
            run_len[d] = 0
    return run_ret, run_len, fin


def drain_model(fin):
    """Host model of k_episode_stats_drain: totals f64 [8] in the order include/atr_stats.h states — 32 row lanes, lane r adds
    rows r, r + 32, r + 64, ... in that order, then the 32 partial rows are added in lane order."""
    fin = np.asarray(fin, np.float64).reshape(-1, FIELDS)
    part = np.zeros((DRAIN_LANES, FIELDS), np.float64)
    for i in range(0, fin.shape[0], DRAIN_LANES):
        rows = fin[i:i + DRAIN_LANES]
        part[:rows.shape[0]] = part[:rows.shape[0]] + rows
    totals = np.zeros(FIELDS, np.float64)
    for r in range(DRAIN_LANES):
        totals = totals + part[r]
    return totals


def summarize(totals):
    """totals f64 [8] (drain(), pooled over ranks or shards by plain addition) -> dict: episodes, R_mean [2], R_std [2], EL_mean,
    EL_std, S_rate, R_step [2]. Means and stds are population values as in gym_eval.py:117-125 (np.mean / np.std of the episode
    list); R_step = R_mean / EL_mean, the reference's `reward_mean / len_mean`. No finished episode: NaNs."""
    t = totals.detach().cpu().numpy() if torch.is_tensor(totals) else totals
    t = np.asarray(t, np.float64).reshape(FIELDS)
    n = float(t[0])
    if n <= 0:
        nan = float("nan")
        return dict(episodes=0, R_mean=[nan, nan], R_std=[nan, nan], EL_mean=nan, EL_std=nan, S_rate=nan, R_step=[nan, nan])
    r_mean = t[1:3] / n
    r_std = np.sqrt(np.maximum(t[3:5] / n - r_mean * r_mean, 0.0))
    l_mean = t[5] / n
    l_std = math.sqrt(max(t[6] / n - l_mean * l_mean, 0.0))
    return dict(episodes=int(round(n)), R_mean=[float(v) for v in r_mean], R_std=[float(v) for v in r_std], EL_mean=float(l_mean),
                EL_std=float(l_std), S_rate=float(t[7] / n), R_step=[float(v) for v in r_mean / l_mean])


def pooled(totals):
    """The totals of all ranks: dist.all_reduce(SUM) of the float64 vector where a process group spans more than one rank."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        totals = totals.clone()
        dist.all_reduce(totals, op=dist.ReduceOp.SUM)
    return totals


def write_scalars(writer, summary, n_steps):
    """train/reward_0 and train/reward_1 (the reference's tags, train.py:86-87: here the MEAN return of the episodes finished
    since the last record) and the rest of TAGS. A record without a finished episode writes only train/episodes = 0."""
    writer.add_scalar("train/episodes", summary["episodes"], n_steps)
    if summary["episodes"] == 0:
        return
    for p in range(2):
        writer.add_scalar("train/reward_%d" % p, summary["R_mean"][p], n_steps)
        writer.add_scalar("train/reward_step_%d" % p, summary["R_step"][p], n_steps)
    writer.add_scalar("train/eps_len", summary["EL_mean"], n_steps)
    writer.add_scalar("train/success_rate", summary["S_rate"], n_steps)


def describe(summary):
    """One line for stderr."""
    if summary["episodes"] == 0:
        return "episodes 0"
    return ("episodes %d  R_mean [%.3f, %.3f]  R_std [%.3f, %.3f]  EL_mean %.1f  EL_std %.1f  S_rate %.3f  R_step [%.4f, %.4f]"
            % (summary["episodes"], summary["R_mean"][0], summary["R_mean"][1], summary["R_std"][0], summary["R_std"][1],
               summary["EL_mean"], summary["EL_std"], summary["S_rate"], summary["R_step"][0], summary["R_step"][1]))


def episode_stats(rew, rew_strides, done, done_strides, run_ret, run_len, fin, T, N, success_len, stream):
    """atr_episode_stats on raw device addresses (ints; 0 = NULL) and element strides: the one place the entry point is called."""
    lib().atr_episode_stats(rew or None, rew_strides[0], rew_strides[1], rew_strides[2], done or None, done_strides[0],
                            done_strides[1], run_ret or None, run_len or None, fin or None, int(T), int(N), int(success_len), stream)


def episode_stats_drain(fin, totals, N, stream):
    lib().atr_episode_stats_drain(fin or None, totals or None, int(N), stream)


def _env_clocks(env):
    """Step counter of every env of the shard (host array), or None where the env has no device handle to ask."""
    core = getattr(env, "core", None)
    if core is None or not hasattr(core, "get_state"):
        return None
    return np.asarray(core.get_state()["t"])


class EpisodeStats(object):
    """The accounts of one env shard (module docstring). Attaches itself as env.episode_stats; train.rollout then calls
    update() after the steps of every rollout over that shard, whichever player ran it. The shard must be freshly reset —
    every env at step 0 — so that the first counted episode of every env is a whole one; Agent.reset() (which resets the shard)
    zeroes the running accounts of an attached object. success_len: the episode length that counts as a success
    (gym_eval.py:114-115: `eps_len >= 500`), by default the env's time limit core_max_steps()."""

    def __init__(self, env, device, success_len=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("EpisodeStats lives on the GPU (there is no host accounting path)")
        lib()
        if getattr(env, "episode_stats", None) is not None:
            raise RuntimeError("this env shard already has episode statistics attached")
        clocks = _env_clocks(env)
        if clocks is None:
            raise RuntimeError("EpisodeStats needs an env with a device handle (env.core.get_state) to see that the shard is fresh")
        if clocks.any():
            raise RuntimeError("EpisodeStats must be attached to a freshly reset shard (every env at step 0): %d of %d envs have "
                               "already stepped, their first counted episode would be a partial one"
                               % (int((clocks != 0).sum()), clocks.size))
        n = self.num_envs = int(env.num_envs)
        self.success_len = int(env.core_max_steps() if success_len is None else success_len)
        self.run_ret = torch.zeros((n, 2), dtype=torch.float32, device=self.device)
        self.run_len = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.fin = torch.zeros((n, FIELDS), dtype=torch.float64, device=self.device)
        self.totals = torch.zeros(FIELDS, dtype=torch.float64, device=self.device)
        self.env = env
        env.episode_stats = self

    def detach(self):
        if getattr(self.env, "episode_stats", None) is self:
            self.env.episode_stats = None

    def reset_running(self):
        """The shard has been reset: whatever episode an env was in is gone (finished episodes not yet drained stay)."""
        self.run_ret.zero_()
        self.run_len.zero_()

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def update(self, rew, done):
        """One launch on the current stream: rew [T, N, 2] f32 (trailing unit dimensions allowed) and done [T, N] u8 / bool of
        the T consecutive steps the shard has just taken, any strides (the rollout store, a slice of it, a stacked list).
        Capturable: the tensors are read in place, nothing is copied and the host is not asked."""
        T, n = int(done.shape[0]), self.num_envs
        while rew.dim() > 3 and rew.shape[-1] == 1:
            rew = rew.squeeze(-1)
        if rew.dtype != torch.float32 or tuple(rew.shape) != (T, n, 2) or rew.device != self.device:
            raise ValueError("rew must be float32 [T, %d, 2] on %s, got %s %s on %s" % (n, self.device, rew.dtype,
                                                                                       tuple(rew.shape), rew.device))
        if done.dtype not in (torch.uint8, torch.bool) or tuple(done.shape) != (T, n) or done.device != self.device:
            raise ValueError("done must be uint8 [T, %d] on %s, got %s %s on %s" % (n, self.device, done.dtype,
                                                                                    tuple(done.shape), done.device))
        episode_stats(rew.data_ptr(), rew.stride(), done.data_ptr(), done.stride(), self.run_ret.data_ptr(),
                      self.run_len.data_ptr(), self.fin.data_ptr(), T, n, self.success_len, self._stream())

    def drain(self):
        """totals = sum of fin over the shard, fin zeroed, one launch on the current stream; returns totals (still on the device,
        overwritten by the next drain). The running accounts carry on: an episode in flight is counted when it ends."""
        episode_stats_drain(self.fin.data_ptr(), self.totals.data_ptr(), self.num_envs, self._stream())
        return self.totals

    def record(self, writer, n_steps, rank=0, label="train"):
        """A log record: drain, pool over ranks, summarise, write TAGS; rank 0 prints one stderr line. Returns the summary."""
        import sys
        summary = summarize(pooled(self.drain()))
        write_scalars(writer, summary, n_steps)
        if rank == 0:
            print("%s episodes at %d env steps: %s" % (label, n_steps, describe(summary)), file=sys.stderr, flush=True)
        return summary
