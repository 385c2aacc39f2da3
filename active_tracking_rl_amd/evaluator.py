"""evaluator — a greedy evaluation round (test.evaluate: test.py:16-136 of the reference, `test_eps` episodes as one batch)
on the rollout's own kernels, replayed as a hipGraph.

test.evaluate drives Agent.action_test: per env step the eager forward (about twenty small launches), a separate env.step, the
accounting as tensor ops and one host synchronisation. Here a step is the training rollout's step — stem, fc pair, LSTMCell
product, and ONE last launch that runs both cells, both actor heads and the env step — in its evaluation form
(atr_eval_act_env_step, include/atr_eval.h; csrc/track2d_hip.hip k_eval_step): the action is the first maximal logit instead of
the categorical draw, and the round's accounts (reward sums, lengths, who is still in the first episode) are kept by that same
launch. A chunk of --num-steps such steps is captured once per round with the helpers the training drivers share
(train._GraphedSchedule: the carry, train.rollout) and replayed until nobody is alive; the host reads the device once per chunk.

The binding of the new header is declared here (EVAL_STRUCTS / EVAL_PROTOTYPES, held to include/atr_eval.h by
tests/test_greedy_eval_cpu.py), apart from fused.ATR_PROTOTYPES, which is include/atr_policy.h's table."""
import ctypes as C
import math
import time

import numpy as np
import torch

from . import fused, vec_env
from .environment import create_env, eval_args
from .player_util import Agent
from .train import _GraphedSchedule, rollout


class Unsupported(RuntimeError):
    """Graphed evaluation does not exist for this env / model / flags (supported() is false)."""


class EvalOut(C.Structure):
    """atr_eval_out of include/atr_eval.h."""
    _fields_ = [("rsum", C.c_void_p), ("length", C.c_void_p), ("alive", C.c_void_p)]


EVAL_STRUCTS = {"atr_eval_out": EvalOut}
# {entry point: (restype, [argtypes])} for every function include/atr_eval.h declares
EVAL_PROTOTYPES = {
    "atr_eval_act_env_step": (C.c_int, [C.c_void_p, C.POINTER(fused.ActStepArgs), C.POINTER(EvalOut), C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
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
        for name, (restype, argtypes) in EVAL_PROTOTYPES.items():
            f = getattr(L, name)         # (a library without the symbol is an error: there is no other evaluation step)
            f.restype, f.argtypes = restype, argtypes
            f.errcheck = _errcheck(name)
        _lib = L
    return _lib


def _eval_out(act_args, eval_out):
    """EvalOut of eval_out = (rsum f32 [N,2], length i32 [N], alive u8 [N]), contiguous, on the env's device."""
    rsum, length, alive = eval_out
    n = act_args.N
    assert rsum.dtype == torch.float32 and rsum.shape == (n, 2) and rsum.is_contiguous()
    assert length.dtype == torch.int32 and length.shape == (n,) and length.is_contiguous()
    assert alive.dtype == torch.uint8 and alive.shape == (n,) and alive.is_contiguous()
    return EvalOut(rsum.data_ptr(), length.data_ptr(), alive.data_ptr())


def eval_act_env_step(env_core, act_args, eval_out, env_out, stream):
    """atr_eval_act_env_step on fused.act_env_step's arguments (act_args: its fused.ActStepArgs); eval_out = (rsum f32 [N,2],
    length i32 [N], alive u8 [N]), contiguous, on the env's device."""
    out = _eval_out(act_args, eval_out)
    lib().atr_eval_act_env_step(env_core.h, C.byref(act_args), C.byref(out), *fused._env_out_args(env_out), stream)


def gru_eval_act_env_step(env_core, act_args, rows, eval_out, env_out, stream):
    """atr_gru_eval_act_env_step (include/atr_gru_step.h; bound by fused.lib(): fused.GRU_STEP_PROTOTYPES) on
    fused.gru_act_env_step's arguments; rows = (k h_prev of player 0, of player 1, their row stride)."""
    out = _eval_out(act_args, eval_out)
    fused.lib().atr_gru_eval_act_env_step(env_core.h, C.byref(act_args), *rows, C.byref(out), *fused._env_out_args(env_out), stream)


def account(rew, done, rsum=None, length=None, alive=None):
    """Host model of the kernel's episode accounting: rew [T,N,2] f32 and done [T,N] of consecutive steps ->
    (rsum f32 [N,2], length i32 [N], alive u8 [N]); float32 sums in step order, `x + 0` for an env that is no longer alive —
    the kernel's expressions, so equal bit for bit. rsum / length / alive: the accounts to continue from (default: a fresh
    round's)."""
    rew, done = np.asarray(rew, np.float32), np.asarray(done)
    n = rew.shape[1]
    rsum = np.zeros((n, 2), np.float32) if rsum is None else np.array(rsum, np.float32)
    length = np.zeros(n, np.int32) if length is None else np.array(length, np.int32)
    alive = np.ones(n, np.uint8) if alive is None else np.array(alive, np.uint8)
    for t in range(rew.shape[0]):
        al = alive != 0
        rsum = (rsum + np.where(al[:, None], rew[t], np.float32(0.0))).astype(np.float32)
        length = (length + al.astype(np.int32)).astype(np.int32)
        alive = (al & (done[t] == 0)).astype(np.uint8)
    return rsum, length, alive


def supported(env, model):
    """True exactly when the rollout's fused env step would be taken for this env and model: the env offers fused_step_out
    (not for RPF targets, 'Full' observations, --rescale, stacked frames, --occlusion, --fov, --footprints, --map-memory, --noise-*, --egocentric, NumpyVecEnv), both players are present, R = 128 and the
    model's switches lead every step of a cached rollout to fused.act_env_step."""
    if not hasattr(env, "fused_step_out") or not hasattr(env, "rollout_buffers") or not hasattr(model, "new_cache"):
        return False
    if getattr(model, "single", True) or not hasattr(model, "player1"):
        return False
    if not getattr(model, "cacheable_core", True):       # (GRU cores: no cached rollout, hence no fused step)
        return False
    buf = env.rollout_buffers(1)
    if buf is None or env.fused_step_out((buf[0][1], buf[1][0], buf[2][0])) is None:
        return False
    p0, p1 = model.player0, model.player1
    R = p0.lstm.hidden_size
    if R != 128 or p1.lstm.hidden_size != R or not model._env_fused_static(env.num_envs, R):
        return False
    st = torch.empty((env.num_envs, 2, 1, 1) + tuple(buf[0].shape[-2:]), dtype=buf[0].dtype, device=buf[0].device)
    cache = model.new_cache(1, st, env_fused=True)
    if cache is not None and getattr(cache, "gru", False):       # (--fused-gru: a GRU cache exists in the fused one-GEMM form only)
        return True
    return cache is not None and cache.f_all is not None and bool(getattr(cache, "has_wih_t", False)) and cache.actions is not None


class GreedyEvaluator(_GraphedSchedule):
    """One evaluation round of `episodes` envs of `env_id`, graph-replayed (module docstring). The env shard is test.evaluate's
    (same num_envs, env_id_base, seed: a round starts from the episodes the eager evaluator starts from), with byte
    observations. run() -> (rsum [episodes, 2], length [episodes]) numpy, what test.evaluate returns; stats afterwards:
    replays, host_reads, steps, and the seconds spent in warm-up (first use of a model at this batch size: one eager chunk on a
    throw-away shard, so that no library initialises inside the capture) and capture. record=True keeps the round's per-step
    observations (u8), actions, rewards, done flags and both players' hidden / cell rows in `self.record`."""

    def __init__(self, model, env_id, args, device, episodes, record=False, env=None):
        """env: a ready VecEnv to run the round on instead of the shard built here (tests: another TimeLimit)."""
        self.model, self.env_id, self.args, self.device = model, env_id, args, torch.device(device)
        self.episodes, self.keep = int(episodes), bool(record)
        self.num_steps = int(getattr(args, "num_steps", 20))
        self.env = env if env is not None else self._make_env()
        if not supported(self.env, model):
            self.env.close()
            raise Unsupported("graphed greedy evaluation exists where the rollout's fused env step does (evaluator.supported): "
                              "not for %s with this model and these flags" % env_id)
        n = self.env.num_envs
        self.rsum = torch.zeros((n, 2), dtype=torch.float32, device=self.device)
        self.length = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.alive = torch.ones(n, dtype=torch.uint8, device=self.device)
        self._alive_host = torch.empty(n, dtype=torch.uint8).pin_memory()
        self.sampler = fused.ActionSampler(self.device, seed=0)      # (the greedy step draws nothing: it only carries ordinals)
        self.stats, self.record = {}, None
        self.map_index = None            # with --eval-map-bank: int32 [episodes], each evaluation episode's bank index

    def _make_env(self):
        return create_env(self.env_id, eval_args(self.args), num_envs=max(2, self.episodes), device=str(self.device),
                          env_id_base=getattr(self.args, "eval_env_id_base", 1 << 20), obs_u8=True,
                          views=False)              # (--view draws the eager round: test.evaluate)

    def _player(self, env, accounts):
        p = Agent(self.model, env, self.args, None, self.device)
        p.greedy_eval = accounts
        p.reset()
        return p

    def _warm_up(self):
        """One eager chunk on a throw-away shard of the same size, once per model and batch size."""
        warm = self.model.__dict__.setdefault("_greedy_eval_warm", set())
        key = (self.env.num_envs, self.num_steps, str(self.device))
        if key in warm:
            return
        env = self._make_env()
        try:
            n = env.num_envs
            p = self._player(env, (torch.zeros((n, 2), device=self.device), torch.zeros(n, dtype=torch.int32, device=self.device),
                                   torch.ones(n, dtype=torch.uint8, device=self.device)))
            rollout(p, self.num_steps)
            torch.cuda.synchronize(self.device)
        finally:
            env.close()
        warm.add(key)

    def close(self):
        if self.env is not None:
            self.env.close()
            self.env = None

    @torch.no_grad()
    def run(self):
        """The round. The shard is used up by it (an evaluator runs one round; per-round capture is the design)."""
        if self.env is None:
            raise RuntimeError("this evaluator's round has been run")
        model, dev, T = self.model, self.device, self.num_steps
        was_training, own = model.training, model.__dict__.get("_sampler")
        model.eval()
        model._sampler = self.sampler
        try:
            t0 = time.perf_counter()
            self._warm_up()
            t1 = time.perf_counter()
            player = self.master = self._player(self.env, (self.rsum, self.length, self.alive))
            if getattr(self.env, "map_bank", None) is not None:
                self.map_index = self.env.map_index()[:self.episodes].cpu().numpy()
            self._new_carry()
            if self.keep:
                first_obs = player.state.reshape(player.num_envs, 2, 13, 13).clone()
            self.env.flush()                 # no generator launch in flight and stamp 0 when the capture starts
            torch.cuda.synchronize(dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"), self._carried(player):
                rollout(player, T)
                self.env.generator_join()
            self._bind_carry(player)
            if not (getattr(model, "env_stepped", False) and player._cache is not None and player._buf is not None):
                raise RuntimeError("the captured chunk did not end its steps in the fused env step")
            t2 = time.perf_counter()
            max_replays = int(math.ceil(self.env.core_max_steps() / float(T)))
            replays = reads = 0
            chunks = []
            stream = torch.cuda.current_stream(dev)
            while replays < max_replays:
                g.replay()
                replays += 1
                if self.keep:
                    c, b = player._cache, player._buf
                    chunks.append((b[0][1:].clone(), c.actions.clone(), b[1].clone(), b[2].clone(), c.h_all[:, 1:].clone(),
                                   c.c_all[:, 1:].clone()))
                self._alive_host.copy_(self.alive, non_blocking=True)      # the chunk's one host read
                stream.synchronize()
                reads += 1
                if not bool(self._alive_host.any()):
                    break
            if self.env.core.faults() != 0:
                raise RuntimeError("the env kernels flagged a fault during the evaluation round")
            rsum = self.rsum[:self.episodes].cpu().numpy()
            length = self.length[:self.episodes].cpu().numpy()
            self.stats = dict(replays=replays, host_reads=reads, steps=replays * T, warmup_s=t1 - t0, capture_s=t2 - t1,
                              replay_s=time.perf_counter() - t2)
            if self.keep:
                cat = lambda i, dim=0: torch.cat([ch[i] for ch in chunks], dim).cpu().numpy()
                obs = np.concatenate([first_obs.cpu().numpy()[None], cat(0)], 0)
                self.record = dict(obs=obs, actions=cat(1), rew=cat(2), done=cat(3), h=cat(4, 1), c=cat(5, 1),
                                   rsum=self.rsum.cpu().numpy(), length=self.length.cpu().numpy(), alive=self.alive.cpu().numpy())
            del g
            return rsum, length
        finally:
            if own is None:
                model.__dict__.pop("_sampler", None)
            else:
                model._sampler = own
            if hasattr(model, "cache_dense"):
                model.cache_dense(False)
            if was_training:
                model.train()
            self.close()
