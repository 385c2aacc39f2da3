"""sight_stats — does the target use the obstacles? Counted on the device (include/atr_sight.h; csrc/sight_stats_hip.hip).

tracking_stats counts WHERE the target sits in the tracker's window; it does not look at the walls between the two. From the same
rollout store — both players' 13 x 13 windows, the step rewards, the done flags — this module counts, for all N envs of a shard in
ONE launch per rollout (train.rollout calls update() on the store, inside the captured rollout graph where there is one): whether
the tracker's line of sight to the target is clear or blocked by a wall, how long the shortest way round inside the window is
(an upper bound on the map's path distance: the true shortest path may leave the window), and how often sight is lost to a wall
rather than to range, and regained:

    carry   i32 [N]      the sight class of the state each env is in (0 CLEAR, 1 BLOCKED, 2 OUT), -1: none
    tab     u64 [776]    SEEN [169] samples per in-view bin, BLOCKED [169] of those with a wall on the line, NOPATH [169] of those
                         without a path inside the window, PATH [169] by path length P, DETOUR [85] by (P - |dr| - |dc|) / 2,
                         TRANS [9] by prev * 3 + cur, then OUT, TERMINAL, INCONSISTENT, SAMPLES

(torch has no arithmetic on uint64: the table is an int64 tensor, the same bits below 2^63.) The table belongs to the ENV SHARD
(env.sight_stats), as tracking_stats.TrackingStats does; the two hold separate carries and tables and run side by side. Counts
pool across ranks by addition (pooled), summarize() turns them into rates in float64. classify() is the host model of the kernel
in numpy: integers, so the device table must equal it exactly."""
import ctypes as C
import os

import numpy as np
import torch

from . import vec_env
from .tracking_stats import sample_bins

WINDOW, SIDE, CENTRE = 169, 13, 84                       # ATR_SIGHT_WINDOW, 13 x 13, ATR_SIGHT_CENTRE
BIN_OUT, BIN_TERMINAL, BIN_INCONSISTENT = 169, 170, 171  # ATR_SIGHT_BIN_*: the bins of tracking_stats.sample_bins
CLEAR, BLOCKED_CLASS, OUT_CLASS = 0, 1, 2                # ATR_SIGHT_CLEAR, ATR_SIGHT_BLOCKED_CLASS, ATR_SIGHT_OUT_CLASS
MAX_PATH = 168                                           # ATR_SIGHT_MAX_PATH
SEEN, BLOCKED, NOPATH, PATH, DETOUR, TRANS = 0, 169, 338, 507, 676, 761          # the segments of the table
N_DETOUR = 85
OUT, TERMINAL, INCONSISTENT, SAMPLES = 770, 771, 772, 773
TABLE = 776                                              # ATR_SIGHT_TABLE
NO_AUTO_RESET = 1                                        # ATR_SIGHT_NO_AUTO_RESET (flags bit 0)
TAGS = ("train/sight_clear_rate", "train/sight_occluded_rate", "train/sight_no_path_rate", "train/sight_unseen_rate",
        "train/sight_mean_path", "train/sight_mean_detour", "train/sight_lost_to_occlusion_rate", "train/sight_lost_to_range_rate",
        "train/sight_reacquire_rate", "train/sight_samples", "train/sight_inconsistent")

_LL, _P = C.c_longlong, C.c_void_p
# {entry point: (restype, [argtypes])} for every function include/atr_sight.h declares
SIGHT_PROTOTYPES = {
    "atr_sight_stats": (C.c_int, [_P, C.c_int, _LL, _LL, _LL, _P, _LL, _LL, _LL, _P, _LL, _LL, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "atr_sight_stats_drain": (C.c_int, [_P, _P, _P]),
}
_lib = None


def _errcheck(name):
    """As tracking_stats._errcheck: a non-zero status raises RuntimeError naming the entry point, with the library's own text."""
    def check(status, func=None, args=None):
        if status != 0:
            raise RuntimeError("%s failed (%d): %s" % (name, status, vec_env.load_library().t2d_last_error().decode()))
        return status
    return check


def lib():
    global _lib
    if _lib is None:
        L = vec_env.load_library()
        for name, (restype, argtypes) in SIGHT_PROTOTYPES.items():
            f = getattr(L, name)         # (a library without the symbol is an error: there is no other counting path)
            f.restype, f.argtypes = restype, argtypes
            f.errcheck = _errcheck(name)
        _lib = L
    return _lib


def line_cells(dr, dc):
    """The window cells (row, column) of the tracker's line to a target at offset (dr, dc), end cells excluded
    (include/atr_sight.h "The LINE")."""
    dr, dc = int(dr), int(dc)
    ar, ac = abs(dr), abs(dc)
    m = max(ar, ac)
    sr, sc = (dr > 0) - (dr < 0), (dc > 0) - (dc < 0)
    return [(6 + sr * ((2 * k * ar + m) // (2 * m)), 6 + sc * ((2 * k * ac + m) // (2 * m))) for k in range(1, m)]


def line_masks():
    """uint16 [169, 13]: per bin, per window row, the line cells as bits (bit c = column c) — the kernel's constant table."""
    masks = np.zeros((WINDOW, SIDE), np.uint16)
    for b in range(WINDOW):
        for r, c in line_cells(b // SIDE - 6, b % SIDE - 6):
            masks[b, r] |= np.uint16(1 << c)
    return masks


_LINE_BOOL = None


def _line_bool():
    """bool [169, 169]: per bin, the line cells as a flat window mask."""
    global _LINE_BOOL
    if _LINE_BOOL is None:
        m = line_masks()
        _LINE_BOOL = ((m[:, :, None] >> np.arange(SIDE, dtype=np.uint16)) & 1).astype(bool).reshape(WINDOW, WINDOW)
    return _LINE_BOOL


def window_paths(walls, bins):
    """The flood of the kernel for S samples at once: walls bool [S, 13, 13], bins int [S] in 0 .. 168 and not 84 -> int32 [S],
    the length of the shortest 4-connected path over free cells from (6, 6) to the bin's cell, 0 where there is none."""
    walls, bins = np.asarray(walls, bool), np.asarray(bins, np.int64)
    S = len(bins)
    free = np.zeros((S, SIDE + 2, SIDE + 2), bool)
    free[:, 1:-1, 1:-1] = ~walls
    reach = np.zeros_like(free)
    reach[:, 7, 7] = True
    path, active, idx = np.zeros(S, np.int32), np.ones(S, bool), np.arange(S)
    tr, tc = bins // SIDE + 1, bins % SIDE + 1
    for level in range(1, MAX_PATH + 1):
        if not active.any():
            break
        nxt = reach.copy()
        nxt[:, 1:] |= reach[:, :-1]
        nxt[:, :-1] |= reach[:, 1:]
        nxt[:, :, 1:] |= reach[:, :, :-1]
        nxt[:, :, :-1] |= reach[:, :, 1:]
        nxt &= free
        hit = nxt[idx, tr, tc] & active
        grown = (nxt != reach).any((1, 2))
        path[hit] = level
        active &= ~hit & grown
        reach = nxt
    return path


def classify(obs, rew, done, carry=None, flags=0, tab=None):
    """Host model of k_sight_stats: -> (tab int64 [776], carry int32 [N]), continuing from the given accounts (default: a fresh
    shard's — a zero table, carry -1). obs [T+1, N, 2, 13, 13] (or [..., 169]) uint8 / float32, rew [T, N, 2], done [T, N]."""
    obs, done = np.asarray(obs), np.asarray(done)
    T, n = done.shape[0], done.shape[1]
    bins = sample_bins(obs, rew, done, flags)
    d = done.reshape(T, n) != 0
    walls = obs.reshape(T + 1, n, 2, WINDOW)[1:, :, 0] == 1
    tab = np.zeros(TABLE, np.int64) if tab is None else np.array(tab, np.int64).reshape(TABLE)
    carry = np.full(n, -1, np.int32) if carry is None else np.array(carry, np.int32).reshape(n)
    carry[(carry < -1) | (carry > OUT_CLASS)] = -1
    seen = bins < WINDOW
    apart = seen & (bins != CENTRE)
    blocked = np.zeros((T, n), bool)
    blocked[apart] = (walls[apart] & _line_bool()[bins[apart]]).any(-1)
    cls = np.full((T, n), -1, np.int32)
    cls[seen] = blocked[seen]
    cls[bins == BIN_OUT] = OUT_CLASS
    b = bins[apart].astype(np.int64)
    path = window_paths(walls[apart].reshape(-1, SIDE, SIDE), b)
    manhattan = np.abs(b // SIDE - 6) + np.abs(b % SIDE - 6)
    np.add.at(tab, SEEN + bins[seen], 1)
    np.add.at(tab, BLOCKED + bins[blocked], 1)
    np.add.at(tab, NOPATH + b[path == 0], 1)
    np.add.at(tab, PATH + path[path > 0], 1)
    np.add.at(tab, DETOUR + (path[path > 0] - manhattan[path > 0]) // 2, 1)
    tab[OUT] += int((bins == BIN_OUT).sum())
    tab[TERMINAL] += int((bins == BIN_TERMINAL).sum())
    tab[INCONSISTENT] += int((bins == BIN_INCONSISTENT).sum())
    tab[SAMPLES] += T * n
    for t in range(T):
        pair = (carry >= 0) & (cls[t] >= 0)
        np.add.at(tab, TRANS + carry[pair] * 3 + cls[t][pair], 1)
        carry = np.where((cls[t] < 0) | d[t], -1, cls[t]).astype(np.int32)
    return tab, carry


def _table(tab):
    t = tab.detach().cpu().numpy() if torch.is_tensor(tab) else tab
    return np.asarray(t, np.int64).reshape(TABLE)


def summarize(tab):
    """The table (drain(), pooled over ranks or shards by plain addition) -> dict, in float64 from the integers: samples,
    terminal, inconsistent, in_view, apart (in view and not co-located), blocked, no_path, out, transitions (counts); over the
    in-view, non-co-located samples: sight_clear_rate, occluded_rate, no_path_rate; over the samples with a known relation
    (in view or OUT): unseen_rate = (blocked + OUT) / known; over the samples with a path: mean_path, mean_detour; over the
    transitions from CLEAR: lost_to_occlusion_rate (to BLOCKED), lost_to_range_rate (to OUT); over the transitions from BLOCKED
    or OUT: reacquire_rate (into CLEAR). An empty denominator gives NaN."""
    t = _table(tab)
    nan = float("nan")
    ratio = lambda num, den: float(num) / float(den) if den > 0 else nan
    in_view = int(t[SEEN:SEEN + WINDOW].sum())
    apart = in_view - int(t[SEEN + CENTRE])
    blocked, no_path = int(t[BLOCKED:BLOCKED + WINDOW].sum()), int(t[NOPATH:NOPATH + WINDOW].sum())
    paths, detours = t[PATH:PATH + WINDOW].astype(np.float64), t[DETOUR:DETOUR + N_DETOUR].astype(np.float64)
    with_path = int(t[PATH:PATH + WINDOW].sum())
    trans = t[TRANS:TRANS + 9].reshape(3, 3)
    known = in_view + int(t[OUT])
    hidden = int(trans[BLOCKED_CLASS].sum() + trans[OUT_CLASS].sum())
    return dict(samples=int(t[SAMPLES]), terminal=int(t[TERMINAL]), inconsistent=int(t[INCONSISTENT]), in_view=in_view, apart=apart,
                blocked=blocked, no_path=no_path, out=int(t[OUT]), transitions=int(trans.sum()),
                sight_clear_rate=ratio(apart - blocked, apart), occluded_rate=ratio(blocked, apart), no_path_rate=ratio(no_path, apart),
                unseen_rate=ratio(blocked + int(t[OUT]), known),
                mean_path=ratio((paths * np.arange(WINDOW)).sum(), with_path),
                mean_detour=ratio((detours * 2.0 * np.arange(N_DETOUR)).sum(), with_path),
                lost_to_occlusion_rate=ratio(trans[CLEAR, BLOCKED_CLASS], trans[CLEAR].sum()),
                lost_to_range_rate=ratio(trans[CLEAR, OUT_CLASS], trans[CLEAR].sum()),
                reacquire_rate=ratio(trans[BLOCKED_CLASS, CLEAR] + trans[OUT_CLASS, CLEAR], hidden))


def occlusion_image(tab, scale=16):
    """uint8 [13 * scale, 13 * scale, 3]: per offset the ratio BLOCKED / SEEN, dark (never blocked, or never seen) to bright (always
    blocked), the tracker's own cell outlined by one red pixel row / column where scale allows it."""
    t = _table(tab)
    seen = t[SEEN:SEEN + WINDOW].astype(np.float64).reshape(SIDE, SIDE)
    blocked = t[BLOCKED:BLOCKED + WINDOW].astype(np.float64).reshape(SIDE, SIDE)
    v = np.divide(blocked, seen, out=np.zeros_like(seen), where=seen > 0)
    scale = int(scale)
    if scale < 1:
        raise ValueError("scale must be >= 1")
    rgb = np.stack([255.0 * v, 255.0 * v ** 2, 64.0 + 96.0 * (1.0 - v)], -1).round().astype(np.uint8)
    img = np.repeat(np.repeat(rgb, scale, 0), scale, 1)
    if scale >= 4:
        a, b = 6 * scale, 7 * scale - 1
        img[a, a:b + 1] = img[b, a:b + 1] = img[a:b + 1, a] = img[a:b + 1, b] = (255, 0, 0)
    return img


def occlusion_png(tab, path, scale=16):
    """occlusion_image written as an 8-bit RGB PNG (utils.write_png); returns the image."""
    from .utils import write_png
    img = occlusion_image(tab, scale)
    write_png(path, img)
    return img


def pooled(tab):
    """The table of all ranks: dist.all_reduce(SUM) of the int64 tensor where a process group spans more than one rank."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        tab = tab.clone()
        dist.all_reduce(tab, op=dist.ReduceOp.SUM)
    return tab


def write_scalars(writer, summary, n_steps):
    """TAGS; rates without a denominator (NaN) are left out of the record."""
    vals = dict(clear_rate=summary["sight_clear_rate"], occluded_rate=summary["occluded_rate"], no_path_rate=summary["no_path_rate"],
                unseen_rate=summary["unseen_rate"], mean_path=summary["mean_path"], mean_detour=summary["mean_detour"],
                lost_to_occlusion_rate=summary["lost_to_occlusion_rate"], lost_to_range_rate=summary["lost_to_range_rate"],
                reacquire_rate=summary["reacquire_rate"], samples=summary["samples"], inconsistent=summary["inconsistent"])
    for key, v in vals.items():
        if v == v:
            writer.add_scalar("train/sight_" + key, v, n_steps)


def describe(summary):
    """One line for stderr."""
    return ("samples %d  terminal %d  inconsistent %d  clear %.3f  occluded %.3f  no_path %.3f  unseen %.3f  mean_path %.2f  "
            "mean_detour %.2f  lost_to_occlusion %.3f  lost_to_range %.3f  reacquire %.3f"
            % (summary["samples"], summary["terminal"], summary["inconsistent"], summary["sight_clear_rate"], summary["occluded_rate"],
               summary["no_path_rate"], summary["unseen_rate"], summary["mean_path"], summary["mean_detour"],
               summary["lost_to_occlusion_rate"], summary["lost_to_range_rate"], summary["reacquire_rate"]))


def sight_stats(obs, obs_is_u8, obs_strides, rew, rew_strides, done, done_strides, carry, tab, T, N, flags, stream):
    """atr_sight_stats on raw device addresses (ints; 0 = NULL) and element strides (t, e, p): the one place the entry point is
    called."""
    lib().atr_sight_stats(obs or None, int(bool(obs_is_u8)), obs_strides[0], obs_strides[1], obs_strides[2], rew or None,
                          rew_strides[0], rew_strides[1], rew_strides[2], done or None, done_strides[0], done_strides[1],
                          carry or None, tab or None, int(T), int(N), int(flags), stream)


def sight_stats_drain(tab, out_tab, stream):
    lib().atr_sight_stats_drain(tab or None, out_tab or None, stream)


class SightStats(object):
    """The table of one env shard (module docstring). Attaches itself as env.sight_stats; train.rollout then calls update() after
    the steps of every rollout over that shard, whichever player ran it, and Agent.reset() (which resets the shard) calls
    reset_running(). Needs the rollout store (env.rollout_buffers: no stacked or rescaled frames) and 13 x 13 windows."""

    def __init__(self, env, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("SightStats lives on the GPU (there is no host counting path)")
        lib()
        if getattr(env, "sight_stats", None) is not None:
            raise RuntimeError("this env shard already has sight statistics attached")
        if not hasattr(env, "rollout_buffers") or env.rollout_buffers(1) is None:
            raise RuntimeError("SightStats reads the rollout store (env.rollout_buffers): stacked or rescaled frames have none")
        core = getattr(env, "core", None)
        if tuple(getattr(core, "obs_hw", ())) != (SIDE, SIDE):
            raise RuntimeError("SightStats needs 13 x 13 'Partial' windows, this env has %r" % (getattr(core, "obs_hw", None),))
        n = self.num_envs = int(env.num_envs)
        self.flags = 0 if core.auto_reset else NO_AUTO_RESET
        self.carry = torch.full((n,), -1, dtype=torch.int32, device=self.device)
        self.tab = torch.zeros(TABLE, dtype=torch.int64, device=self.device)
        self.out_tab = torch.zeros_like(self.tab)
        self.env = env
        env.sight_stats = self

    def detach(self):
        if getattr(self.env, "sight_stats", None) is self:
            self.env.sight_stats = None

    def reset_running(self):
        """The shard has been reset: the state an env was in is gone, its next sample follows nothing (the counts stay)."""
        self.carry.fill_(-1)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def update(self, obs, rew, done):
        """One launch on the current stream over the T consecutive steps the shard has just taken: obs [T+1, N, 2, 13, 13] uint8
        or float32 (slot 0: the state the steps started from), rew [T, N, 2] f32, done [T, N] u8 / bool, any strides as long as a
        window's 169 cells are contiguous (trailing unit dimensions of rew allowed). Capturable: the tensors are read in place and
        the host is not asked."""
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
        sight_stats(obs.data_ptr(), obs.dtype == torch.uint8, obs.stride()[:3], rew.data_ptr(), rew.stride(), done.data_ptr(),
                    done.stride(), self.carry.data_ptr(), self.tab.data_ptr(), T, n, self.flags, self._stream())

    def drain(self):
        """The table as counted since the last drain, and the table zeroed, one launch on the current stream; the returned tensor
        stays on the device and is overwritten by the next drain. carry is untouched: the transitions carry on."""
        sight_stats_drain(self.tab.data_ptr(), self.out_tab.data_ptr(), self._stream())
        return self.out_tab

    def record(self, writer, n_steps, rank=0, log_dir=None, label="train"):
        """A log record: drain, pool over ranks, summarise, write TAGS; rank 0 prints one stderr line and, given log_dir, writes
        heatmaps/occlusion_<n_steps>.png and an .npz of the raw table beside it. Returns the summary."""
        import sys
        tab = _table(pooled(self.drain()))
        summary = summarize(tab)
        write_scalars(writer, summary, n_steps)
        if rank == 0:
            print("%s sight at %d env steps: %s" % (label, n_steps, describe(summary)), file=sys.stderr, flush=True)
            if log_dir is not None:
                d = os.path.join(log_dir, "heatmaps")
                os.makedirs(d, exist_ok=True)
                occlusion_png(tab, os.path.join(d, "occlusion_%d.png" % n_steps))
                np.savez(os.path.join(d, "occlusion_%d.npz" % n_steps), tab=tab)
        return summary
