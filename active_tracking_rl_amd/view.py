"""view — player views: draw what each player was shown (include/atr_view.h; csrc/view_hip.hip, csrc/atr_view_rule.h).

The renderer of track2d_trace.h rebuilds the tracker's window from the map, so it cannot show what the passes over stored windows
(occlusion, field of view, footprints, map memory, sensor noise, the egocentric turn) made of it. These two launches read the
windows themselves: view_cells() gives the map panel's codes (band * 16 + value: band 0 what the viewer was shown, band 1 the
truth under a hidden cell, band 2 the truth outside the window, 255 outside the map) and both windows' codes as given; view_rgb()
gives the same, coloured, on a canvas of 82 x 242 cells (map panel, the tracker's window, the target's window).
VecEnv(..., views=True) keeps a reference to the raw windows its last reset() / step() / observe() produced and offers both.

There is no host path: the library's launches are the only implementation (tests/view_spec.py holds the rule in numpy for the
tests)."""
import ctypes as C

import torch

from . import vec_env
from .occlusion import window_grid

WINDOW, SIDE, MAP_SIDE = 169, 13, 82    # ATR_VIEW_WINDOW, the window's side, T2D_MAX_SIDE
CELLS_H, CELLS_W = 82, 242              # ATR_VIEW_CELLS_H / _W
MAX_SCALE = 8                           # ATR_VIEW_MAX_SCALE
UNKNOWN, OUTSIDE, HIDDEN = 15, 255, 5   # ATR_VIEW_UNKNOWN / OUTSIDE / HIDDEN
BAND_HIDDEN, BAND_BEYOND = 16, 32       # ATR_VIEW_BAND_HIDDEN / BEYOND
VIEWERS = {"tracker": 0, "target": 1}

_LL, _P = C.c_longlong, C.c_void_p
# {entry point: (restype, [argtypes])} for every function include/atr_view.h declares
VIEW_PROTOTYPES = {
    "atr_view_cells": (C.c_int, [_P, _P, C.c_int, _LL, _LL, _P, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P]),
    "atr_view_rgb": (C.c_int, [_P, _P, C.c_int, _LL, _LL, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
}
_lib = None


def _errcheck(name):
    """As noise._errcheck: a non-zero status raises RuntimeError naming the entry point, with the library's own text."""
    def check(status, func=None, args=None):
        if status != 0:
            raise RuntimeError("%s failed (%d): %s" % (name, status, vec_env.load_library().t2d_last_error().decode()))
        return status
    return check


def lib():
    global _lib
    if _lib is None:
        L = vec_env.load_library()
        for name, (restype, argtypes) in VIEW_PROTOTYPES.items():
            f = getattr(L, name)         # (a library without the symbol is an error: there is no other path)
            f.restype, f.argtypes = restype, argtypes
            f.errcheck = _errcheck(name)
        _lib = L
    return _lib


def viewer_of(viewer):
    """0 / 1 of a `viewer` argument (0, 1, "tracker" or "target"). ValueError for anything else."""
    if viewer in VIEWERS:
        return VIEWERS[viewer]
    if isinstance(viewer, bool) or viewer not in (0, 1):
        raise ValueError("viewer must be 0 / 'tracker' or 1 / 'target', got %r" % (viewer,))
    return int(viewer)


def min_pitch(scale):
    """The smallest row pitch of a frame at `scale`: 726 * scale bytes rounded up to a multiple of 16."""
    return (3 * CELLS_W * int(scale) + 15) // 16 * 16


def view_cells_raw(h, obs, is_u8, se, sp, facing, turned, env_ids, count, viewer, cells, windows, stream):
    """atr_view_cells on a handle, raw device addresses (ints; 0 / None = NULL) and element strides: the one place the entry
    point is called."""
    lib().atr_view_cells(h or None, obs or None, int(bool(is_u8)), int(se), int(sp), facing or None, int(turned), env_ids or None,
                         int(count), int(viewer), cells or None, windows or None, stream)


def view_rgb_raw(h, obs, is_u8, se, sp, facing, turned, env_ids, count, viewer, scale, rgb, pitch, stream):
    """atr_view_rgb likewise."""
    lib().atr_view_rgb(h or None, obs or None, int(bool(is_u8)), int(se), int(sp), facing or None, int(turned), env_ids or None,
                       int(count), int(viewer), int(scale), rgb or None, int(pitch), stream)


def _check_windows(who, obs, facing, turned, core):
    if not torch.is_tensor(obs) or obs.device.type != "cuda":
        raise RuntimeError("%s runs on the GPU (there is no host path)" % who)
    if (obs.dtype not in (torch.uint8, torch.float32) or obs.dim() != 4 or tuple(obs.shape[-2:]) != (SIDE, SIDE)
            or obs.shape[1] != 2 or obs.stride(-1) != 1 or obs.stride(-2) != SIDE):
        raise ValueError("%s: obs must be uint8 / float32 [N, 2, 13, 13] with contiguous windows, got %s %s strides %s"
                         % (who, obs.dtype, tuple(obs.shape), tuple(obs.stride())))
    n = int(obs.shape[0])
    window_grid(obs.shape[:2], obs.stride()[:2])          # (ValueError where windows would overlap)
    if n != int(core.num_envs):
        raise ValueError("%s: obs holds %d envs, the handle %d" % (who, n, core.num_envs))
    if turned not in (0, 1, 2, 3):
        raise ValueError("%s: turned must be 0 .. 3, got %r" % (who, turned))
    if facing is None:
        if turned:
            raise ValueError("%s: turned=%d needs the facing bytes" % (who, turned))
    elif (not torch.is_tensor(facing) or facing.dtype != torch.uint8 or facing.device != obs.device or tuple(facing.shape) != (n, 2)
            or not facing.is_contiguous()):
        raise ValueError("%s: facing must be a contiguous uint8 [%d, 2] tensor on %s" % (who, n, obs.device))


def view_cells(obs, core, env_ids, viewer=0, facing=None, turned=0, out=None):
    """One launch: (cells u8 [count, 82, 82], windows u8 [count, 2, 13, 13]) of the listed envs. obs [N, 2, 13, 13] uint8 or
    float32 on the device, the windows' 169 cells contiguous, any strides over N and the players that keep the windows apart; core
    a VecTrack2D of N envs; env_ids as VecTrack2D._env_ids takes them (host ids are checked here, device ids are clamped by the
    kernel, which sets FAULT_RENDER_ID); facing uint8 [N, 2] or None; turned: bit p set when window p is egocentric. out: an
    optional (cells, windows) pair to write, either of which may be None. Launches on the current stream of obs' device.
    Capturable."""
    viewer = viewer_of(viewer)
    _check_windows("view_cells", obs, facing, turned, core)
    ids = core._env_ids(env_ids, "view_cells")
    count = int(ids.numel())
    if out is None:
        out = (torch.empty((count, MAP_SIDE, MAP_SIDE), dtype=torch.uint8, device=obs.device),
               torch.empty((count, 2, SIDE, SIDE), dtype=torch.uint8, device=obs.device))
    cells, windows = out
    for t, numel in ((cells, count * MAP_SIDE * MAP_SIDE), (windows, count * 2 * WINDOW)):
        if t is not None and (t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() != numel or t.device != obs.device):
            raise ValueError("view_cells: an output must be a contiguous uint8 device tensor of %d elements" % numel)
    if count == 0:
        return cells, windows
    view_cells_raw(core.h, obs.data_ptr(), obs.dtype == torch.uint8, obs.stride(0), obs.stride(1),
                   None if facing is None else facing.data_ptr(), turned, ids.data_ptr(), count, viewer,
                   None if cells is None else cells.data_ptr(), None if windows is None else windows.data_ptr(),
                   C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream))
    return cells, windows


def view_rgb(obs, core, env_ids, scale=4, viewer=0, facing=None, turned=0, pitch=None, out=None):
    """One launch: u8 [count, 82 * scale, 242 * scale, 3], one frame per listed env — a view of the pitched canvas `out`
    (u8 [count, 82 * scale, pitch], pitch a multiple of 16 and at least 726 * scale; pad bytes are written 0) without its row
    padding. The other arguments as view_cells. Capturable."""
    viewer = viewer_of(viewer)
    _check_windows("view_rgb", obs, facing, turned, core)
    ids = core._env_ids(env_ids, "view_rgb")
    count, scale = int(ids.numel()), int(scale)
    if not 1 <= scale <= MAX_SCALE:
        raise ValueError("view_rgb: scale must be 1 .. %d, got %r" % (MAX_SCALE, scale))
    row = 3 * CELLS_W * scale
    pitch = min_pitch(scale) if pitch is None else int(pitch)
    if out is None:
        out = torch.empty((count, CELLS_H * scale, max(pitch, 0)), dtype=torch.uint8, device=obs.device)
    if out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != count * CELLS_H * scale * pitch or out.device != obs.device:
        raise ValueError("view_rgb: out must be a contiguous uint8 device tensor [%d, %d, %d]" % (count, CELLS_H * scale, pitch))
    if count:
        view_rgb_raw(core.h, obs.data_ptr(), obs.dtype == torch.uint8, obs.stride(0), obs.stride(1),
                     None if facing is None else facing.data_ptr(), turned, ids.data_ptr(), count, viewer, scale, out.data_ptr(),
                     pitch, C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream))
    return out.view(count, CELLS_H * scale, pitch)[:, :, :row].unflatten(2, (CELLS_W * scale, 3))
