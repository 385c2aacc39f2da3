"""tracking_stats — how the two policies behave, counted on the device (include/atr_track_stats.h; csrc/tracking_stats_hip.hip).

Where does the target sit relative to the tracker, how often is it in view, in reward range or on the tracker's own cell, does
the tracker step toward it, does the target step away? The reference can only answer from info['traces'] on the host, one env
at a time; a replayed rollout graph cannot ask the host at all. The rollout store already holds what the answers need — both
players' 13 x 13 windows, the step rewards, the done flags, the actions — so the counts of all N envs of a shard advance in ONE
launch per rollout (train.rollout calls update() on the store, inside the captured rollout graph where there is one):

    carry    i32 [N]            the bin of the state each env is in (the next action belongs to it), -1: none
    hist     u64 [176]          bins 0..168 = target offset (dr + 6) * 13 + (dc + 6) in the tracker's window (84: co-located),
                                169 OUT of view, 170 TERMINAL, 171 INCONSISTENT, 172 SAMPLES
    act_hist u64 [2][170][8]    per player, per bin (0..168, OUT), per action: the actions taken FROM a state of that bin

(torch has no arithmetic on uint64: the tables are int64 tensors, the same bits below 2^63.) The tables belong to the ENV SHARD
(env.tracking_stats), as episode_stats.EpisodeStats does and for the same reason: the two replicas of train.PipelinedIteration
alternate rollouts over one shard. Counts pool across ranks by addition (pooled), summarize() turns them into rates in float64.
classify() is the host model of the kernel in numpy: integers, so the device tables must equal it exactly."""
import ctypes as C
import os

import numpy as np
import torch

from . import vec_env

WINDOW, SIDE, CENTRE = 169, 13, 84                       # ATR_TRACK_WINDOW, 13 x 13, ATR_TRACK_CENTRE
OUT, TERMINAL, INCONSISTENT, SAMPLES = 169, 170, 171, 172
HIST = 176                                               # ATR_TRACK_HIST
ACT_ROWS, MAX_ACTIONS = 170, 8                           # ATR_TRACK_ACT_ROWS, ATR_TRACK_MAX_ACTIONS
NO_AUTO_RESET = 1                                        # ATR_TRACK_NO_AUTO_RESET (flags bit 0)
# the move of every action (track_1v1.py:275-279): (d row, d column)
MOVES = {"VonNeumann": ((-1, 0), (1, 0), (0, -1), (0, 1)),
         "Moore": ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, 1), (1, 1), (-1, -1), (1, -1))}
TAGS = ("train/in_view_rate", "train/in_range_rate", "train/colocated_rate", "train/mean_distance", "train/centroid_dr",
        "train/centroid_dc", "train/tracker_toward_rate", "train/target_away_rate", "train/tracking_samples",
        "train/tracking_inconsistent")

_LL, _P = C.c_longlong, C.c_void_p
# {entry point: (restype, [argtypes])} for every function include/atr_track_stats.h declares
TRACK_PROTOTYPES = {
    "atr_track_stats": (C.c_int, [_P, C.c_int, _LL, _LL, _LL, _P, _LL, _LL, _LL, _P, _LL, _LL, _P, _LL, _LL, _LL, _P, _P, _P,
                                  C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "atr_track_stats_drain": (C.c_int, [_P, _P, _P, _P, _P]),
}
_lib = None


def _errcheck(name):
    """As episode_stats._errcheck: a non-zero status raises RuntimeError naming the entry point, with the library's own text."""
    def check(status, func=None, args=None):
        if status != 0:
            raise RuntimeError("%s failed (%d): %s" % (name, status, vec_env.load_library().t2d_last_error().decode()))
        return status
    return check


def lib():
    global _lib
    if _lib is None:
        L = vec_env.load_library()
        for name, (restype, argtypes) in TRACK_PROTOTYPES.items():
            f = getattr(L, name)         # (a library without the symbol is an error: there is no other counting path)
            f.restype, f.argtypes = restype, argtypes
            f.errcheck = _errcheck(name)
        _lib = L
    return _lib


def offsets():
    """(dr, dc) int64 [169] each: the target's offset from the tracker per window bin."""
    b = np.arange(WINDOW)
    return b // SIDE - 6, b % SIDE - 6


def sample_bins(obs, rew, done, flags=0):
    """The bin of every sample, int32 [T, N] (include/atr_track_stats.h): obs [T+1, N, 2, 13, 13] (or [..., 169]) uint8 / float32,
    rew [T, N, 2], done [T, N]. Slot 0 of obs is not classified."""
    obs, rew, done = np.asarray(obs), np.asarray(rew, np.float32), np.asarray(done)
    T, n = done.shape[0], done.shape[1]
    w = obs.reshape(T + 1, n, 2, WINDOW)[1:]
    rew = rew.reshape(T, n, 2)
    is4, is2 = w[:, :, 0] == 4, w[:, :, 1] == 2
    n4, n2 = is4.sum(-1), is2.sum(-1)
    i4, i2 = is4.argmax(-1), is2.argmax(-1)
    centres = (w[:, :, 0, CENTRE] == 2) & (w[:, :, 1, CENTRE] == 4)
    one = rew[:, :, 0] == np.float32(1.0)
    none = (n4 == 0) & (n2 == 0)
    bins = np.full((T, n), INCONSISTENT, np.int32)
    bins[centres & one & none] = CENTRE
    bins[centres & ~one & none] = OUT
    seen = centres & ~one & (n4 == 1) & (n2 == 1) & (i2 == WINDOW - 1 - i4)
    bins[seen] = i4[seen]
    if not (int(flags) & NO_AUTO_RESET):
        bins[done.reshape(T, n) != 0] = TERMINAL
    return bins


def classify(obs, rew, done, act=None, carry=None, flags=0, n_actions=4, hist=None, act_hist=None):
    """Host model of k_track_stats: -> (hist int64 [176], act_hist int64 [2, 170, 8], carry int32 [N]), continuing from the
    given accounts (default: a fresh shard's — zero tables, carry -1). act int [T, N, 2] or None."""
    done = np.asarray(done)
    T, n = done.shape[0], done.shape[1]
    bins = sample_bins(obs, rew, done, flags)
    d = done.reshape(T, n) != 0
    hist = np.zeros(HIST, np.int64) if hist is None else np.array(hist, np.int64).reshape(HIST)
    act_hist = (np.zeros((2, ACT_ROWS, MAX_ACTIONS), np.int64) if act_hist is None
                else np.array(act_hist, np.int64).reshape(2, ACT_ROWS, MAX_ACTIONS))
    carry = np.full(n, -1, np.int32) if carry is None else np.array(carry, np.int32).reshape(n)
    carry[(carry < -1) | (carry > OUT)] = -1
    if act is not None:
        act = np.asarray(act).reshape(T, n, 2).astype(np.int64)
    for t in range(T):
        if act is not None:
            paired = carry >= 0
            for p in range(2):
                a = act[t, :, p]
                ok = paired & (a >= 0) & (a < int(n_actions))
                np.add.at(act_hist[p], (carry[ok], a[ok]), 1)
                hist[INCONSISTENT] += int((paired & ~ok).sum())
        np.add.at(hist, bins[t], 1)
        hist[SAMPLES] += n
        carry = np.where((bins[t] > OUT) | d[t], -1, bins[t]).astype(np.int32)
    return hist, act_hist, carry


def _tables(hist, act_hist):
    h = hist.detach().cpu().numpy() if torch.is_tensor(hist) else hist
    a = act_hist.detach().cpu().numpy() if torch.is_tensor(act_hist) else act_hist
    return np.asarray(h, np.int64).reshape(HIST), np.asarray(a, np.int64).reshape(2, ACT_ROWS, MAX_ACTIONS)


def move_tables(action_type="VonNeumann"):
    """(toward bool [169, 8], away bool [169, 8]): from offset bin b, does action a of the TRACKER shorten the distance
    (|d - move|^2 < |d|^2), does action a of the TARGET lengthen it (|d + move|^2 > |d|^2)? Actions the type does not have: False."""
    dr, dc = offsets()
    toward, away = np.zeros((WINDOW, MAX_ACTIONS), bool), np.zeros((WINDOW, MAX_ACTIONS), bool)
    d2 = dr * dr + dc * dc
    for a, (mr, mc) in enumerate(MOVES[action_type]):
        toward[:, a] = (dr - mr) ** 2 + (dc - mc) ** 2 < d2
        away[:, a] = (dr + mr) ** 2 + (dc + mc) ** 2 > d2
    return toward, away


def summarize(hist, act_hist, action_type="VonNeumann"):
    """The tables (drain(), pooled over ranks or shards by plain addition) -> dict, in float64 from the integers: samples,
    terminal, inconsistent (counts); over the samples with a known relation (bins 0..168 and OUT): in_view_rate, in_range_rate
    (dr^2 + dc^2 <= 36: the reward's and the far counter's range, track_1v1.py:96-109), colocated_rate; over the in-view samples:
    mean_distance (Euclidean), centroid [mean dr, mean dc]; over the actions taken from in-view, non-co-located states:
    tracker_toward_rate, target_away_rate. An empty denominator gives NaN."""
    h, a = _tables(hist, act_hist)
    dr, dc = offsets()
    win = h[:WINDOW].astype(np.float64)
    view, known = float(h[:WINDOW].sum()), float(h[:WINDOW].sum() + h[OUT])
    nan = float("nan")
    ratio = lambda num, den: float(num) / den if den > 0 else nan
    s = dict(samples=int(h[SAMPLES]), terminal=int(h[TERMINAL]), inconsistent=int(h[INCONSISTENT]),
             in_view_rate=ratio(view, known), in_range_rate=ratio(h[:WINDOW][dr * dr + dc * dc <= 36].sum(), known),
             colocated_rate=ratio(h[CENTRE], known),
             mean_distance=ratio((win * np.sqrt((dr * dr + dc * dc).astype(np.float64))).sum(), view),
             centroid=[ratio((win * dr).sum(), view), ratio((win * dc).sum(), view)])
    toward, away = move_tables(action_type)
    apart = np.arange(WINDOW) != CENTRE
    rows0, rows1 = a[0, :WINDOW][apart], a[1, :WINDOW][apart]
    s["tracker_toward_rate"] = ratio(rows0[toward[apart]].sum(), float(rows0.sum()))
    s["target_away_rate"] = ratio(rows1[away[apart]].sum(), float(rows1.sum()))
    return s


def heat_image(hist, scale=16):
    """uint8 [13 * scale, 13 * scale, 3]: the 13 x 13 offset counts over their maximum, dark (never) to bright (most often), the
    tracker's own cell outlined by one red pixel row / column where scale allows it."""
    h = np.asarray(hist.detach().cpu().numpy() if torch.is_tensor(hist) else hist, np.int64).reshape(HIST)
    grid = h[:WINDOW].astype(np.float64).reshape(SIDE, SIDE)
    top = grid.max()
    v = np.sqrt(grid / top) if top > 0 else grid          # (square root: rare offsets stay visible beside the mode)
    scale = int(scale)
    if scale < 1:
        raise ValueError("scale must be >= 1")
    rgb = np.stack([255.0 * v, 255.0 * v ** 2, 64.0 + 96.0 * (1.0 - v)], -1).round().astype(np.uint8)
    img = np.repeat(np.repeat(rgb, scale, 0), scale, 1)
    if scale >= 4:
        a, b = 6 * scale, 7 * scale - 1
        img[a, a:b + 1] = img[b, a:b + 1] = img[a:b + 1, a] = img[a:b + 1, b] = (255, 0, 0)
    return img


def heat_png(hist, path, scale=16):
    """heat_image written as an 8-bit RGB PNG (utils.write_png); returns the image."""
    from .utils import write_png
    img = heat_image(hist, scale)
    write_png(path, img)
    return img


def pooled(hist, act_hist):
    """The tables of all ranks: dist.all_reduce(SUM) of the int64 tensors where a process group spans more than one rank."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        hist, act_hist = hist.clone(), act_hist.clone()
        dist.all_reduce(hist, op=dist.ReduceOp.SUM)
        dist.all_reduce(act_hist, op=dist.ReduceOp.SUM)
    return hist, act_hist


def write_scalars(writer, summary, n_steps):
    """TAGS; rates without a denominator (NaN) are left out of the record."""
    vals = dict(in_view_rate=summary["in_view_rate"], in_range_rate=summary["in_range_rate"],
                colocated_rate=summary["colocated_rate"], mean_distance=summary["mean_distance"],
                centroid_dr=summary["centroid"][0], centroid_dc=summary["centroid"][1],
                tracker_toward_rate=summary["tracker_toward_rate"], target_away_rate=summary["target_away_rate"],
                tracking_samples=summary["samples"], tracking_inconsistent=summary["inconsistent"])
    for key, v in vals.items():
        if v == v:
            writer.add_scalar("train/" + key, v, n_steps)


def describe(summary):
    """One line for stderr."""
    return ("samples %d  terminal %d  inconsistent %d  in_view %.3f  in_range %.3f  colocated %.3f  mean_distance %.2f  "
            "centroid [%.2f, %.2f]  tracker_toward %.3f  target_away %.3f"
            % (summary["samples"], summary["terminal"], summary["inconsistent"], summary["in_view_rate"], summary["in_range_rate"],
               summary["colocated_rate"], summary["mean_distance"], summary["centroid"][0], summary["centroid"][1],
               summary["tracker_toward_rate"], summary["target_away_rate"]))


def track_stats(obs, obs_is_u8, obs_strides, rew, rew_strides, done, done_strides, act, act_strides, carry, hist, act_hist, T, N,
                n_actions, flags, stream):
    """atr_track_stats on raw device addresses (ints; 0 = NULL) and element strides (t, e, p): the one place the entry point is
    called."""
    lib().atr_track_stats(obs or None, int(bool(obs_is_u8)), obs_strides[0], obs_strides[1], obs_strides[2], rew or None,
                          rew_strides[0], rew_strides[1], rew_strides[2], done or None, done_strides[0], done_strides[1],
                          act or None, act_strides[0], act_strides[1], act_strides[2], carry or None, hist or None, act_hist or None,
                          int(T), int(N), int(n_actions), int(flags), stream)


def track_stats_drain(hist, act_hist, out_hist, out_act_hist, stream):
    lib().atr_track_stats_drain(hist or None, act_hist or None, out_hist or None, out_act_hist or None, stream)


class TrackingStats(object):
    """The tables of one env shard (module docstring). Attaches itself as env.tracking_stats; train.rollout then calls update()
    after the steps of every rollout over that shard, whichever player ran it, and Agent.reset() (which resets the shard) calls
    reset_running(). Needs the rollout store (env.rollout_buffers: no stacked or rescaled frames) and 13 x 13 windows."""

    def __init__(self, env, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TrackingStats lives on the GPU (there is no host counting path)")
        lib()
        if getattr(env, "tracking_stats", None) is not None:
            raise RuntimeError("this env shard already has tracking statistics attached")
        if not hasattr(env, "rollout_buffers") or env.rollout_buffers(1) is None:
            raise RuntimeError("TrackingStats reads the rollout store (env.rollout_buffers): stacked or rescaled frames have none")
        core = getattr(env, "core", None)
        if tuple(getattr(core, "obs_hw", ())) != (SIDE, SIDE):
            raise RuntimeError("TrackingStats needs 13 x 13 'Partial' windows, this env has %r" % (getattr(core, "obs_hw", None),))
        n = self.num_envs = int(env.num_envs)
        self.n_actions = int(core.num_actions)
        self.action_type = core.action_type
        self.flags = 0 if core.auto_reset else NO_AUTO_RESET
        self.carry = torch.full((n,), -1, dtype=torch.int32, device=self.device)
        self.hist = torch.zeros(HIST, dtype=torch.int64, device=self.device)
        self.act_hist = torch.zeros((2, ACT_ROWS, MAX_ACTIONS), dtype=torch.int64, device=self.device)
        self.out_hist, self.out_act_hist = torch.zeros_like(self.hist), torch.zeros_like(self.act_hist)
        self.env = env
        env.tracking_stats = self

    def detach(self):
        if getattr(self.env, "tracking_stats", None) is self:
            self.env.tracking_stats = None

    def reset_running(self):
        """The shard has been reset: the state an env was in is gone, its next action pairs with nothing (the counts stay)."""
        self.carry.fill_(-1)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def update(self, obs, rew, done, act=None):
        """One launch on the current stream over the T consecutive steps the shard has just taken: obs [T+1, N, 2, 13, 13] uint8
        or float32 (slot 0: the state the steps started from), rew [T, N, 2] f32, done [T, N] u8 / bool, act [T, N, 2] int64 or
        None, any strides as long as a window's 169 cells are contiguous (trailing unit dimensions of rew / act allowed).
        Capturable: the tensors are read in place and the host is not asked."""
        T, n = int(done.shape[0]), self.num_envs
        while rew.dim() > 3 and rew.shape[-1] == 1:
            rew = rew.squeeze(-1)
        while obs.dim() > 5 and obs.shape[3] == 1:          # [T+1, N, 2, stack = 1, C = 1, 13, 13] as VecEnv hands states out
            obs = obs.squeeze(3)
        if (obs.dtype not in (torch.uint8, torch.float32) or tuple(obs.shape) != (T + 1, n, 2, SIDE, SIDE) or obs.device != self.device
                or obs.stride(4) != 1 or obs.stride(3) != SIDE):
            raise ValueError("obs must be uint8 / float32 [T + 1, %d, 2, 13, 13] on %s with contiguous windows, got %s %s strides %s "
                             "on %s" % (n, self.device, obs.dtype, tuple(obs.shape), tuple(obs.stride()), obs.device))
        if rew.dtype != torch.float32 or tuple(rew.shape) != (T, n, 2) or rew.device != self.device:
            raise ValueError("rew must be float32 [T, %d, 2] on %s, got %s %s on %s" % (n, self.device, rew.dtype,
                                                                                       tuple(rew.shape), rew.device))
        if done.dtype not in (torch.uint8, torch.bool) or tuple(done.shape) != (T, n) or done.device != self.device:
            raise ValueError("done must be uint8 [T, %d] on %s, got %s %s on %s" % (n, self.device, done.dtype,
                                                                                    tuple(done.shape), done.device))
        act_ptr, act_strides = 0, (0, 0, 0)
        if act is not None:
            while act.dim() > 3 and act.shape[-1] == 1:
                act = act.squeeze(-1)
            if tuple(act.shape) != (T, n, 2) or act.device != self.device or act.dtype not in (torch.int64, torch.int32):
                raise ValueError("act must be int64 [T, %d, 2] on %s, got %s %s on %s" % (n, self.device, act.dtype,
                                                                                         tuple(act.shape), act.device))
            if act.dtype != torch.int64:
                act = act.to(torch.int64)
            act_ptr, act_strides = act.data_ptr(), act.stride()
        track_stats(obs.data_ptr(), obs.dtype == torch.uint8, obs.stride()[:3], rew.data_ptr(), rew.stride(), done.data_ptr(),
                    done.stride(), act_ptr, act_strides, self.carry.data_ptr(), self.hist.data_ptr(), self.act_hist.data_ptr(), T, n,
                    self.n_actions, self.flags, self._stream())

    def drain(self):
        """(hist, act_hist) as counted since the last drain, both tables zeroed, one launch on the current stream; the returned
        tensors stay on the device and are overwritten by the next drain. carry is untouched: the pairing carries on."""
        track_stats_drain(self.hist.data_ptr(), self.act_hist.data_ptr(), self.out_hist.data_ptr(), self.out_act_hist.data_ptr(),
                          self._stream())
        return self.out_hist, self.out_act_hist

    def record(self, writer, n_steps, rank=0, log_dir=None, label="train"):
        """A log record: drain, pool over ranks, summarise, write TAGS; rank 0 prints one stderr line and, given log_dir, writes
        heatmaps/target_offset_<n_steps>.png and an .npz of both raw tables beside it. Returns the summary."""
        import sys
        hist, act_hist = _tables(*pooled(*self.drain()))
        summary = summarize(hist, act_hist, self.action_type)
        write_scalars(writer, summary, n_steps)
        if rank == 0:
            print("%s tracking at %d env steps: %s" % (label, n_steps, describe(summary)), file=sys.stderr, flush=True)
            if log_dir is not None:
                d = os.path.join(log_dir, "heatmaps")
                os.makedirs(d, exist_ok=True)
                heat_png(hist, os.path.join(d, "target_offset_%d.png" % n_steps))
                np.savez(os.path.join(d, "target_offset_%d.npz" % n_steps), hist=hist, act_hist=act_hist)
        return summary
