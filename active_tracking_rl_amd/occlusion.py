"""occlusion — occluded observations: walls hide what is behind them (include/atr_occlusion.h; csrc/occlusion_hip.hip).

A 13 x 13 window as the env writes it shows everything inside it, through any number of walls. occlude_() rewrites stored windows
in place, one launch for any number of them: every cell whose two lines of sight to the window's centre (the line of
include/atr_sight.h drawn from the centre, and the same rule drawn from the cell) both hold a wall becomes the value `hidden`
(default 5); every other cell stays what it was. The rule is symmetric — the tracker sees the target exactly when the target sees
the tracker — and a pure function of the window's 169 cells, so it has no state: VecEnv(..., occlusion=True) runs it behind every
reset(), step() and observe() on the raw window, before rescaling and frame stacking.

There is no host path: the library's launch is the only implementation (tests/occlusion_spec.py holds the rule in numpy loops for
the tests)."""
import ctypes as C

import torch

from . import vec_env

WINDOW, SIDE = 169, 13          # ATR_OCCLUDE_WINDOW, ATR_OCCLUDE_SIDE
WALL, HIDDEN = 1, 5             # ATR_OCCLUDE_WALL, ATR_OCCLUDE_HIDDEN
MAX_WINDOWS = (1 << 31) - 1     # ATR_OCCLUDE_MAX_WINDOWS

_LL, _P = C.c_longlong, C.c_void_p
# {entry point: (restype, [argtypes])} for every function include/atr_occlusion.h declares
OCCLUSION_PROTOTYPES = {
    "atr_occlude_windows": (C.c_int, [_P, _P, C.c_int, _LL, _LL, _LL, _LL, C.c_int, _P]),
}
_lib = None


def _errcheck(name):
    """As sight_stats._errcheck: a non-zero status raises RuntimeError naming the entry point, with the library's own text."""
    def check(status, func=None, args=None):
        if status != 0:
            raise RuntimeError("%s failed (%d): %s" % (name, status, vec_env.load_library().t2d_last_error().decode()))
        return status
    return check


def lib():
    global _lib
    if _lib is None:
        L = vec_env.load_library()
        for name, (restype, argtypes) in OCCLUSION_PROTOTYPES.items():
            f = getattr(L, name)         # (a library without the symbol is an error: there is no other path)
            f.restype, f.argtypes = restype, argtypes
            f.errcheck = _errcheck(name)
        _lib = L
    return _lib


def occlude_windows(src, dst, is_u8, n_env, n_win, se, sp, hidden, stream):
    """atr_occlude_windows on raw device addresses (ints; 0 = NULL) and element strides: the one place the entry point is called."""
    lib().atr_occlude_windows(src or None, dst or None, int(bool(is_u8)), int(n_env), int(n_win), int(se), int(sp), int(hidden),
                              stream)


def window_grid(shape, strides):
    """The leading dimensions of an [..., 13, 13] tensor as the (n_env, n_win, se, sp) of the ABI: unit dimensions dropped,
    neighbours that one stride walks merged, what is left at most two. ValueError when more are left, or when windows would
    overlap (a stride below a window, an expanded dimension)."""
    dims = [(int(n), int(s)) for n, s in zip(shape, strides) if n != 1]
    merged = []
    for n, s in dims:
        if merged and merged[-1][1] == n * s:
            merged[-1] = (merged[-1][0] * n, s)
        else:
            merged.append((n, s))
    if len(merged) > 2:
        raise ValueError("occlude_: leading shape %s with strides %s needs more than the two strides of the ABI"
                         % (tuple(shape), tuple(strides)))
    reach = WINDOW                       # elements a walk over the inner dimensions covers
    for n, s in sorted(merged, key=lambda d: d[1]):
        if s < reach:
            raise ValueError("occlude_: windows overlap (leading shape %s, strides %s)" % (tuple(shape), tuple(strides)))
        reach = (n - 1) * s + reach
    merged = [(1, 0)] * (2 - len(merged)) + merged
    return merged[0][0], merged[1][0], merged[0][1], merged[1][1]


def occlude_(obs, hidden=HIDDEN):
    """In place, one launch: obs [..., 13, 13] uint8 or float32 on the device, the windows' 169 cells contiguous, any leading
    strides the ABI can express (window_grid: the rollout store, a slot of it, a slice of a larger store). Launches on the current
    stream of obs' device — the one an env step before it was enqueued on. Capturable. Returns obs."""
    if not torch.is_tensor(obs) or obs.device.type != "cuda":
        raise RuntimeError("occlude_ runs on the GPU (there is no host path)")
    if (obs.dtype not in (torch.uint8, torch.float32) or obs.dim() < 2 or tuple(obs.shape[-2:]) != (SIDE, SIDE)
            or obs.stride(-1) != 1 or obs.stride(-2) != SIDE):
        raise ValueError("occlude_: obs must be uint8 / float32 [..., 13, 13] with contiguous windows, got %s %s strides %s"
                         % (obs.dtype, tuple(obs.shape), tuple(obs.stride())))
    if obs.numel() == 0:
        return obs
    n_env, n_win, se, sp = window_grid(obs.shape[:-2], obs.stride()[:-2])
    occlude_windows(obs.data_ptr(), obs.data_ptr(), obs.dtype == torch.uint8, n_env, n_win, se, sp, hidden,
                    C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream))
    return obs
