"""fov — facing and field of view: a player sees only a cone ahead (include/atr_fov.h; csrc/fov_hip.hip, csrc/atr_fov_rule.h).

A 13 x 13 window as the env writes it shows everything round the player. restrict_() keeps one facing byte per player (0 .. 3: the
VonNeumann move it last chose; NONE = 255: looks all round), turns it with a step's actions (done -> NONE, else an action in 0 .. 3 ->
that action, else unchanged) and then rewrites, in place and in the same launch, every cell of every window that is neither in the
cone of its player's aperture (90 / 180 / 270 degrees about the facing; 360 = this player is not restricted) nor within `near`
cells of the centre as the value `hidden` (default 5, the "unseen" of occlusion.py). The rule has state, the facing tensor, which
the caller owns: VecEnv(..., fov=...) keeps it and runs the pass behind every step() and observe(), after the occlusion pass.

There is no host path: the library's launch is the only implementation (tests/fov_spec.py holds the rule in numpy loops for the
tests)."""
import ctypes as C

import torch

from . import vec_env
from .occlusion import window_grid

WINDOW, SIDE = 169, 13          # ATR_FOV_WINDOW, ATR_FOV_SIDE
NONE, HIDDEN = 255, 5           # ATR_FOV_NONE, ATR_FOV_HIDDEN
NEAR, MAX_NEAR = 1, 6           # ATR_FOV_NEAR, ATR_FOV_MAX_NEAR
MAX_WINDOWS = (1 << 31) - 1     # ATR_FOV_MAX_WINDOWS
APERTURES = (90, 180, 270, 360)

_LL, _P = C.c_longlong, C.c_void_p
# {entry point: (restype, [argtypes])} for every function include/atr_fov.h declares
FOV_PROTOTYPES = {
    "atr_fov_windows": (C.c_int, [_P, _P, C.c_int, _LL, C.c_int, _LL, _LL, _P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                  C.c_int, _P]),
}
_lib = None


def _errcheck(name):
    """As occlusion._errcheck: a non-zero status raises RuntimeError naming the entry point, with the library's own text."""
    def check(status, func=None, args=None):
        if status != 0:
            raise RuntimeError("%s failed (%d): %s" % (name, status, vec_env.load_library().t2d_last_error().decode()))
        return status
    return check


def lib():
    global _lib
    if _lib is None:
        L = vec_env.load_library()
        for name, (restype, argtypes) in FOV_PROTOTYPES.items():
            f = getattr(L, name)         # (a library without the symbol is an error: there is no other path)
            f.restype, f.argtypes = restype, argtypes
            f.errcheck = _errcheck(name)
        _lib = L
    return _lib


def apertures_of(fov):
    """(tracker, target) apertures of a `fov` argument: one aperture for both players, or a pair. ValueError for anything else."""
    pair = tuple(fov) if isinstance(fov, (tuple, list)) else (fov, fov)
    if len(pair) != 2 or any(isinstance(a, bool) or a not in APERTURES for a in pair):
        raise ValueError("fov must be an aperture out of %s or a (tracker, target) pair of them, got %r" % (APERTURES, fov))
    return int(pair[0]), int(pair[1])


def fov_windows(src, dst, is_u8, n_env, n_win, se, sp, facing, a0, a1, act_dtype, done, aperture0, aperture1, near, hidden, stream):
    """atr_fov_windows on raw device addresses (ints; 0 / None = NULL) and element strides: the one place the entry point is
    called."""
    lib().atr_fov_windows(src or None, dst or None, int(bool(is_u8)), int(n_env), int(n_win), int(se), int(sp), facing or None,
                          a0 or None, a1 or None, int(act_dtype), done or None, int(aperture0), int(aperture1), int(near),
                          int(hidden), stream)


def restrict_(obs, facing, actions=None, done=None, apertures=(90, 90), near=NEAR, hidden=HIDDEN):
    """In place, one launch: obs [N, P, 13, 13] (P = 1 or 2 players) uint8 or float32 on the device, the windows' 169 cells
    contiguous, any strides over N and P that keep the windows apart (a slot of the rollout store, a slice of a larger store);
    facing uint8 [N, P] contiguous, read and written. actions: None, or (a_tracker, a_target), each None or [N] uint8 / int32 /
    int64 contiguous, both of one dtype; done: None or uint8 [N]. Launches on the current stream of obs' device. Capturable.
    Returns obs."""
    if not torch.is_tensor(obs) or obs.device.type != "cuda":
        raise RuntimeError("restrict_ runs on the GPU (there is no host path)")
    if (obs.dtype not in (torch.uint8, torch.float32) or obs.dim() != 4 or tuple(obs.shape[-2:]) != (SIDE, SIDE)
            or obs.shape[1] not in (1, 2) or obs.stride(-1) != 1 or obs.stride(-2) != SIDE):
        raise ValueError("restrict_: obs must be uint8 / float32 [N, 1 or 2, 13, 13] with contiguous windows, got %s %s strides %s"
                         % (obs.dtype, tuple(obs.shape), tuple(obs.stride())))
    n, p = int(obs.shape[0]), int(obs.shape[1])
    window_grid(obs.shape[:2], obs.stride()[:2])          # (ValueError where windows would overlap)
    if (not torch.is_tensor(facing) or facing.dtype != torch.uint8 or facing.device != obs.device or tuple(facing.shape) != (n, p)
            or not facing.is_contiguous()):
        raise ValueError("restrict_: facing must be a contiguous uint8 [%d, %d] tensor on %s" % (n, p, obs.device))
    ap = apertures_of(apertures)
    acts = tuple(actions) if actions is not None else ()
    acts = (acts + (None, None))[:2]
    given = [a for a in acts if a is not None]
    for a in given:
        if (not torch.is_tensor(a) or a.dtype not in vec_env._ACT_DTYPE or a.dtype != given[0].dtype or a.device != obs.device
                or a.numel() != n or not a.is_contiguous()):
            raise ValueError("restrict_: actions must be contiguous [%d] uint8 / int32 / int64 tensors of one dtype on %s" % (n, obs.device))
    if done is not None and (not torch.is_tensor(done) or done.dtype != torch.uint8 or done.device != obs.device
                             or done.numel() != n or not done.is_contiguous()):
        raise ValueError("restrict_: done must be a contiguous uint8 [%d] tensor on %s" % (n, obs.device))
    if n == 0:
        return obs
    ptr = lambda t: None if t is None else t.data_ptr()
    fov_windows(obs.data_ptr(), obs.data_ptr(), obs.dtype == torch.uint8, n, p, obs.stride(0), obs.stride(1), facing.data_ptr(),
                ptr(acts[0]), ptr(acts[1]), vec_env._ACT_DTYPE[given[0].dtype] if given else 0, ptr(done), ap[0], ap[1], near,
                hidden, C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream))
    return obs
