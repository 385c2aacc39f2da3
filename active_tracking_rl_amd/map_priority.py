"""map_priority — prioritized map replay on a map bank (include/track2d_bank_prio.h; csrc/track2d_hip.hip).

Prioritized Level Replay (Jiang et al., 2021) on the maps of a --map-bank: the handle keeps a per-map account of the training
episodes that end on each map (t2d_bank_prio_score, one launch per rollout, inside the captured rollout graph), and every
--map-priority-every iterations refresh() drains the accounts, turns them into weights with priorities() — tensor code on the
device, nothing is read back — and hands the weights to the handle (t2d_bank_prio_set_weights), whose generator pass draws
every further episode's map from the table they make. role: whose difficulty counts — 'tracker' serves the maps on which the
tracker's return is low, 'target' the maps on which the target's is.

The rule (priorities()), per refresh number c = 1, 2, ...: a map with n_i > 0 finished episodes since the last refresh gets
    m_i = clip(0.5 * (1 - sum_rq_i / 65536 / (n_i * t_max)), 0, 1)      sum_rq: the role's column of the accounts, t_max the time limit
    h_i <- (1 - alpha) * h_i + alpha * m_i,   stamp_i <- c
(other maps keep h_i and stamp_i; they start from h_i = 1, stamp_i = 0), and then for every map
    rank_i = 1 + #{j : h_j > h_i}                  (ties share a rank: an untouched bank is uniform)
    P_S(i) = rank_i^(-1/beta) / sum_j rank_j^(-1/beta)
    P_C(i) = (c - stamp_i) / sum_j (c - stamp_j)   (uniform if that sum is 0)
    w_i    = (1 - rho) * P_S(i) + rho * P_C(i)
beta = 0.1 and rho = 0.1 are the paper's rank-prioritisation settings and alpha = 1.0 replaces a map's score by its latest;
nobody has measured which values suit this task.

The binding of the new header is declared here (PRIO_PROTOTYPES, held to include/track2d_bank_prio.h by
tests/test_map_priority_cpu.py), apart from map_bank.BANK_PROTOTYPES."""
import ctypes as C
import math
import os

import numpy as np
import torch

FIELDS = 5              # T2D_PRIO_FIELDS: episodes, steps, successes, sum llrint(R0 * 65536), sum llrint(R1 * 65536)
RING = 8                # T2D_PRIO_RING
KEEP = 5                # T2D_PRIO_KEEP
ROLES = {"tracker": 3, "target": 4}      # the role's column of the accounts
PER_MAP_LOG_MAX = 64    # banks of at most this many maps get train/map/<idx>/hardness
BETA, RHO, ALPHA, EVERY = 0.1, 0.1, 1.0, 10
TAGS = ("train/map_priority/weight_entropy", "train/map_priority/max_weight", "train/map_priority/seen_fraction",
        "train/map_priority/unattributed")

_P = C.c_void_p
_LL = C.c_longlong
# {entry point: (restype, [argtypes])} for every function include/track2d_bank_prio.h declares
PRIO_PROTOTYPES = {
    "t2d_bank_prio_enable": (C.c_int, [_P, _P]),
    "t2d_bank_prio_set_weights": (C.c_int, [_P, _P, _P]),
    "t2d_bank_prio_score": (C.c_int, [_P, _P, _LL, _LL, _LL, _P, _LL, _LL, C.c_int, C.c_int, _P]),
    "t2d_bank_prio_drain": (C.c_int, [_P, _P, _P]),
}
_lib = None


def lib():
    global _lib
    if _lib is None:
        from . import map_bank, vec_env
        L = vec_env.load_library()
        for name, (restype, argtypes) in PRIO_PROTOTYPES.items():
            f = getattr(L, name)         # (a library without the symbol is an error: there is no other path)
            f.restype, f.argtypes = restype, argtypes
            f.errcheck = map_bank._errcheck(name)
        _lib = L
    return _lib


def _column(sum_rq, role):
    if role not in ROLES:
        raise ValueError("map priority: role %r, expected 'tracker' or 'target'" % (role,))
    if sum_rq.dim() == 2:                # [K, 2] = (R0, R1) columns: the role picks
        return sum_rq[:, ROLES[role] - 3]
    return sum_rq


def weights(h, stamp, c, beta=BETA, rho=RHO):
    """w float32 [K] from the scores h f64 [K], the stamps i64 [K] and the refresh number c (module docstring). Tensor code on
    h's device: no synchronisation."""
    K = h.shape[0]
    hs, _ = torch.sort(h)
    greater = K - torch.searchsorted(hs, h.contiguous(), right=True)       # #{j : h_j > h_i}
    rank = (greater + 1).to(torch.float64)
    ps = torch.pow(rank, -1.0 / float(beta))
    ps = ps / ps.sum()
    stale = (int(c) - stamp).to(torch.float64)
    tot = stale.sum()
    pc = torch.where(tot > 0, stale / torch.where(tot > 0, tot, torch.ones_like(tot)), torch.full_like(stale, 1.0 / K))
    return ((1.0 - float(rho)) * ps + float(rho) * pc).to(torch.float32)


def priorities(h, stamp, n, sum_rq, c, role="tracker", t_max=500, beta=BETA, rho=RHO, alpha=ALPHA):
    """(h', stamp', w): one refresh of the rule. h f64 [K], stamp i64 [K], n i64 [K] episodes finished per map since the last
    refresh, sum_rq i64 [K] the role's sum of llrint(R * 65536) over them (or [K, 2] for both players: `role` picks the
    column), c the number of this refresh. A pure function on tensors of any device, float64 throughout, no synchronisation;
    w is float32, what t2d_bank_prio_set_weights takes."""
    rq = _column(sum_rq, role)
    seen = n > 0
    nn = torch.where(seen, n, torch.ones_like(n)).to(torch.float64)
    mean = rq.to(torch.float64) / 65536.0 / (nn * float(t_max))
    m = torch.clamp(0.5 * (1.0 - mean), 0.0, 1.0)
    h2 = torch.where(seen, (1.0 - float(alpha)) * h + float(alpha) * m, h)
    stamp2 = torch.where(seen, torch.full_like(stamp, int(c)), stamp)
    return h2, stamp2, weights(h2, stamp2, c, beta, rho)


def pooled(drained):
    """The accounts of all ranks: dist.all_reduce(SUM) of the int64 tensor where a process group spans more than one rank, so
    that every rank builds the same table."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        drained = drained.clone()
        dist.all_reduce(drained, op=dist.ReduceOp.SUM)
    return drained


class PriorityTable(object):
    """The host-free half of a MapPriority: scores, stamps, refresh counter, cumulative counts and the current weights of a
    bank of K maps, on any device. absorb(drained) is one refresh without the two launches around it."""

    def __init__(self, count, device="cpu", role="tracker", t_max=500, beta=BETA, rho=RHO, alpha=ALPHA):
        if role not in ROLES:
            raise ValueError("map priority: role %r, expected 'tracker' or 'target'" % (role,))
        if not (float(beta) > 0 and 0 <= float(rho) <= 1 and 0 <= float(alpha) <= 1):
            raise ValueError("map priority: needs beta > 0, 0 <= rho <= 1, 0 <= alpha <= 1 (beta %r, rho %r, alpha %r)"
                             % (beta, rho, alpha))
        self.count, self.device, self.role = int(count), torch.device(device), role
        self.t_max, self.beta, self.rho, self.alpha = int(t_max), float(beta), float(rho), float(alpha)
        self.h = torch.ones(self.count, dtype=torch.float64, device=self.device)
        self.stamp = torch.zeros(self.count, dtype=torch.int64, device=self.device)
        self.c = 0
        self.episodes = torch.zeros(self.count, dtype=torch.int64, device=self.device)     # per map, since the start
        self.unattributed = torch.zeros((), dtype=torch.int64, device=self.device)
        self.w = weights(self.h, self.stamp, self.c, self.beta, self.rho)

    def absorb(self, drained):
        """drained: int64 [K * 5 + 1] of t2d_bank_prio_drain (this rank's). Pools over ranks, applies the rule, returns w."""
        d = pooled(drained)
        stat = d[:self.count * FIELDS].view(self.count, FIELDS)
        self.c += 1
        self.h, self.stamp, self.w = priorities(self.h, self.stamp, stat[:, 0], stat[:, ROLES[self.role]], self.c, self.role,
                                                self.t_max, self.beta, self.rho, self.alpha)
        self.episodes = self.episodes + stat[:, 0]
        self.unattributed = self.unattributed + d[self.count * FIELDS]
        return self.w

    def state_dict(self):
        return dict(h=self.h.cpu().numpy(), stamp=self.stamp.cpu().numpy(), c=np.int64(self.c),
                    episodes=self.episodes.cpu().numpy(), unattributed=np.int64(int(self.unattributed)))

    def load_state_dict(self, sd):
        h, stamp = np.asarray(sd["h"], np.float64), np.asarray(sd["stamp"], np.int64)
        if h.shape != (self.count,) or stamp.shape != (self.count,):
            raise ValueError("map priority: the saved table has %s map(s), the bank has %d" % (h.shape, self.count))
        self.h = torch.as_tensor(h, device=self.device)
        self.stamp = torch.as_tensor(stamp, device=self.device)
        self.c = int(sd["c"])
        if "episodes" in sd:
            self.episodes = torch.as_tensor(np.asarray(sd["episodes"], np.int64), device=self.device)
        if "unattributed" in sd:
            self.unattributed = torch.as_tensor(np.int64(sd["unattributed"]), device=self.device)
        self.w = weights(self.h, self.stamp, self.c, self.beta, self.rho)
        return self.w


def summarize(w, episodes, unattributed):
    """The record's scalars from host arrays: entropy (nats) and maximum of the normalised weights, the share of maps that have
    finished an episode, the unattributed count."""
    p = np.asarray(w, np.float64)
    p = p / p.sum()
    nz = p[p > 0]
    return {TAGS[0]: float(-(nz * np.log(nz)).sum()), TAGS[1]: float(p.max()),
            TAGS[2]: float((np.asarray(episodes) > 0).mean()), TAGS[3]: float(int(unattributed))}


class MapPriority(object):
    """The priorities of one env shard (module docstring). env: a VecEnv (or anything with .core = a VecTrack2D) whose handle has
    a bank and priorities enabled (VecTrack2D.enable_map_priority); attaches itself as env.map_priority. train.rollout then
    calls update() after the steps of every rollout over that shard, and the schedules call tick() before every rollout they
    issue, which refreshes the table every `every`-th time."""

    def __init__(self, env, device, role="tracker", every=EVERY, beta=BETA, rho=RHO, alpha=ALPHA, t_max=None, success_len=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("MapPriority lives on the GPU (the table and the accounts belong to the env handle)")
        lib()
        if getattr(env, "map_priority", None) is not None:
            raise RuntimeError("this env shard already has map priorities attached")
        self.core = getattr(env, "core", env)
        if not getattr(self.core, "map_priority_enabled", False):
            raise RuntimeError("MapPriority needs a handle with priorities enabled (VecTrack2D.enable_map_priority)")
        self.num_envs = int(self.core.num_envs)
        limit = int(env.core_max_steps()) if hasattr(env, "core_max_steps") else int(self.core.max_episode_steps)
        self.success_len = limit if success_len is None else int(success_len)
        self.every = max(1, int(every))
        self.table = PriorityTable(self.core.map_bank_count, self.device, role, limit if t_max is None else t_max, beta, rho, alpha)
        self.drained = torch.zeros(self.table.count * FIELDS + 1, dtype=torch.int64, device=self.device)
        self.w_dev = self.table.w.clone()
        self.ticks = 0
        self.env = env
        env.map_priority = self

    role = property(lambda self: self.table.role)
    w = property(lambda self: self.table.w)

    def detach(self):
        if getattr(self.env, "map_priority", None) is self:
            self.env.map_priority = None

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def update(self, rew, done):
        """One launch on the current stream: rew [T, N, 2] f32 (trailing unit dimensions allowed) and done [T, N] u8 / bool of
        the T consecutive steps the shard has just taken, any strides. Capturable: read in place, the host is not asked."""
        T, n = int(done.shape[0]), self.num_envs
        while rew.dim() > 3 and rew.shape[-1] == 1:
            rew = rew.squeeze(-1)
        if rew.dtype != torch.float32 or tuple(rew.shape) != (T, n, 2) or rew.device != self.device:
            raise ValueError("rew must be float32 [T, %d, 2] on %s, got %s %s on %s" % (n, self.device, rew.dtype,
                                                                                       tuple(rew.shape), rew.device))
        if done.dtype not in (torch.uint8, torch.bool) or tuple(done.shape) != (T, n) or done.device != self.device:
            raise ValueError("done must be uint8 [T, %d] on %s, got %s %s on %s" % (n, self.device, done.dtype,
                                                                                    tuple(done.shape), done.device))
        rs, ds = rew.stride(), done.stride()
        lib().t2d_bank_prio_score(self.core.h, rew.data_ptr(), rs[0], rs[1], rs[2], done.data_ptr(), ds[0], ds[1], T,
                                  self.success_len, self._stream())

    def drain(self):
        """The accounts since the last drain, int64 [K * 5 + 1] on the device (overwritten by the next drain); one launch."""
        lib().t2d_bank_prio_drain(self.core.h, self.drained.data_ptr(), self._stream())
        return self.drained

    def set_weights(self, w):
        """w: [K] float32 on the device -> the handle's table; one launch on the current stream."""
        self.w_dev.copy_(w)
        lib().t2d_bank_prio_set_weights(self.core.h, self.w_dev.data_ptr(), self._stream())

    def refresh(self, stream=None):
        """Drain, pool over ranks, apply the rule, set the weights: issued eagerly between two rollouts, in stream order on
        `stream` (default: the current one) — the stream the shard's rollouts and generator passes run on. Slots that are
        already generated keep their choice. No synchronisation."""
        if stream is not None and stream != torch.cuda.current_stream(self.device):
            with torch.cuda.stream(stream):
                return self.refresh()
        self.set_weights(self.table.absorb(self.drain()))
        return self.table.w

    def tick(self, stream=None):
        """Before every rollout a schedule issues: the `every`-th one is preceded by a refresh."""
        self.ticks += 1
        if self.ticks % self.every == 0:
            self.refresh(stream)

    def state_dict(self):
        return self.table.state_dict()

    def load_state_dict(self, sd, stream=None):
        """Continue a saved table (record()'s .npz, --map-priority-load): h, stamp, c and the counts; the weights follow from
        them by the rule, with this object's beta and rho, and go to the handle."""
        if isinstance(sd, str):
            with np.load(sd) as z:
                sd = {k: z[k] for k in z.files}
        self.set_weights(self.table.load_state_dict(sd))
        return self.table.w

    def record(self, writer, n_steps, rank=0, log_dir=None):
        """A log record (the only place that synchronises): TAGS, train/map/<idx>/hardness for banks of at most 64 maps, and
        <log_dir>/map_priority.npz = state_dict() + w. Returns the scalars."""
        t = self.table
        sd = t.state_dict()                                 # (.cpu(): the synchronisation)
        w = t.w.cpu().numpy()
        out = summarize(w, sd["episodes"], sd["unattributed"])
        for tag in TAGS:
            writer.add_scalar(tag, out[tag], n_steps)
        if t.count <= PER_MAP_LOG_MAX:
            for i in range(t.count):
                writer.add_scalar("train/map/%d/hardness" % i, float(sd["h"][i]), n_steps)
        if log_dir is not None and rank == 0:
            os.makedirs(log_dir, exist_ok=True)
            with open(os.path.join(log_dir, "map_priority.npz"), "wb") as f:
                np.savez(f, w=w, role=np.array(t.role), **sd)
        if rank == 0:
            import sys
            print("map priority (%s) at %d env steps: refresh %d, %d episodes on %d of %d maps, weight entropy %.3f of %.3f, "
                  "max weight %.4f, unattributed %d" % (t.role, n_steps, t.c, int(sd["episodes"].sum()),
                                                        int((sd["episodes"] > 0).sum()), t.count, out[TAGS[0]],
                                                        math.log(t.count) if t.count > 1 else 0.0, out[TAGS[1]],
                                                        int(sd["unattributed"])), file=sys.stderr, flush=True)
        return out
