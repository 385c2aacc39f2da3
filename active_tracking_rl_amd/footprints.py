"""footprints — players leave a trail the other can see (include/atr_footprints.h; csrc/footprints_hip.hip,
csrc/atr_footprint_rule.h).

Each player leaves footprints on the last K cells it stepped off; the other player's 13 x 13 window shows them as `value` (default
6, the reference's trace colour) wherever it reads 0 there. mark_() keeps the trail — uint16 [N, 2, K + 1]: entry 0 the cell the
player stands on, entries 1 .. K its prints, newest first, EMPTY = 0xFFFF — which the caller owns: BEGIN starts every env's trail
afresh, STEP records a move (or restarts the envs whose `done` flag is set), PEEK records nothing; every mode then paints, in
place and in the same launch. The positions come from the env handle, not from the windows: the windows must be the ones the
handle's last launch wrote. VecEnv(..., footprints=K) keeps the trail and runs the pass behind every reset(), step() and
observe(), after the occlusion and field-of-view passes.

There is no host path: the library's launch is the only implementation (tests/footprints_spec.py holds the rule in numpy loops for
the tests)."""
import ctypes as C

import torch

from . import vec_env
from .occlusion import window_grid

WINDOW, SIDE = 169, 13          # ATR_FOOTPRINT_WINDOW, ATR_FOOTPRINT_SIDE
EMPTY, VALUE, MAX_K = 0xFFFF, 6, 63       # ATR_FOOTPRINT_EMPTY, ATR_FOOTPRINT_VALUE, ATR_FOOTPRINT_MAX_K
PEEK, STEP, BEGIN = 0, 1, 2     # ATR_FOOTPRINT_PEEK / STEP / BEGIN
ROLES = {"tracker": 1, "target": 2, "both": 3}        # whose window is painted (bit 0: the tracker's, bit 1: the target's)

_LL, _P = C.c_longlong, C.c_void_p
# {entry point: (restype, [argtypes])} for every function include/atr_footprints.h declares
FOOTPRINT_PROTOTYPES = {
    "atr_footprint_windows": (C.c_int, [_P, _P, C.c_int, _LL, _LL, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
}
_lib = None


def _errcheck(name):
    """As fov._errcheck: a non-zero status raises RuntimeError naming the entry point, with the library's own text."""
    def check(status, func=None, args=None):
        if status != 0:
            raise RuntimeError("%s failed (%d): %s" % (name, status, vec_env.load_library().t2d_last_error().decode()))
        return status
    return check


def lib():
    global _lib
    if _lib is None:
        L = vec_env.load_library()
        for name, (restype, argtypes) in FOOTPRINT_PROTOTYPES.items():
            f = getattr(L, name)         # (a library without the symbol is an error: there is no other path)
            f.restype, f.argtypes = restype, argtypes
            f.errcheck = _errcheck(name)
        _lib = L
    return _lib


def count_of(footprints):
    """K of a `footprints` argument: an int in 1 .. 63. ValueError for anything else."""
    if isinstance(footprints, bool) or not isinstance(footprints, int) or not 1 <= footprints <= MAX_K:
        raise ValueError("footprints must be a trail length K in 1 .. %d, got %r" % (MAX_K, footprints))
    return int(footprints)


def roles_of(footprints_for):
    """The `roles` bits of a `footprints_for` argument ("tracker", "target" or "both"). ValueError for anything else."""
    if footprints_for not in ROLES:
        raise ValueError("footprints_for must be one of %s, got %r" % (sorted(ROLES), footprints_for))
    return ROLES[footprints_for]


def new_trail(num_envs, k, device):
    """An all-EMPTY trail uint16 [num_envs, 2, k + 1] on `device` (filled as int16 -1: the same bits, and a dtype every device
    op knows)."""
    return torch.full((int(num_envs), 2, count_of(k) + 1), -1, dtype=torch.int16, device=device).view(torch.uint16)


def footprint_windows(h, obs, is_u8, se, sp, trail, k, roles, mode, done, value, stream):
    """atr_footprint_windows on a handle, raw device addresses (ints; 0 / None = NULL) and element strides: the one place the
    entry point is called."""
    lib().atr_footprint_windows(h or None, obs or None, int(bool(is_u8)), int(se), int(sp), trail or None, int(k), int(roles),
                                int(mode), done or None, int(value), stream)


def mark_(obs, trail, core, mode, done=None, roles=1, value=VALUE):
    """In place, one launch: obs [N, 2, 13, 13] uint8 or float32 on the device, the windows' 169 cells contiguous, any strides over
    N and the players that keep the windows apart (a slot of the rollout store, a slice of a larger store) — the windows that the
    last launch of `core` (a VecTrack2D of N envs) wrote; trail uint16 [N, 2, K + 1] contiguous, read and written; mode PEEK /
    STEP / BEGIN; done: None or uint8 [N]; roles 1 (paint the tracker's window), 2 (the target's) or 3. Launches on the current
    stream of obs' device. Capturable. Returns obs."""
    if not torch.is_tensor(obs) or obs.device.type != "cuda":
        raise RuntimeError("mark_ runs on the GPU (there is no host path)")
    if (obs.dtype not in (torch.uint8, torch.float32) or obs.dim() != 4 or tuple(obs.shape[-2:]) != (SIDE, SIDE)
            or obs.shape[1] != 2 or obs.stride(-1) != 1 or obs.stride(-2) != SIDE):
        raise ValueError("mark_: obs must be uint8 / float32 [N, 2, 13, 13] with contiguous windows, got %s %s strides %s"
                         % (obs.dtype, tuple(obs.shape), tuple(obs.stride())))
    n = int(obs.shape[0])
    window_grid(obs.shape[:2], obs.stride()[:2])          # (ValueError where windows would overlap)
    if n != int(core.num_envs):
        raise ValueError("mark_: obs holds %d envs, the handle %d" % (n, core.num_envs))
    if (not torch.is_tensor(trail) or trail.dtype != torch.uint16 or trail.device != obs.device or trail.dim() != 3
            or tuple(trail.shape[:2]) != (n, 2) or not 1 <= trail.shape[2] - 1 <= MAX_K or not trail.is_contiguous()):
        raise ValueError("mark_: trail must be a contiguous uint16 [%d, 2, K + 1] tensor (K in 1 .. %d) on %s" % (n, MAX_K, obs.device))
    if mode not in (PEEK, STEP, BEGIN):
        raise ValueError("mark_: mode must be PEEK (0), STEP (1) or BEGIN (2), got %r" % (mode,))
    if done is not None and (not torch.is_tensor(done) or done.dtype != torch.uint8 or done.device != obs.device
                             or done.numel() != n or not done.is_contiguous()):
        raise ValueError("mark_: done must be a contiguous uint8 [%d] tensor on %s" % (n, obs.device))
    if n == 0:
        return obs
    footprint_windows(core.h, obs.data_ptr(), obs.dtype == torch.uint8, obs.stride(0), obs.stride(1), trail.data_ptr(),
                      trail.shape[2] - 1, roles, mode, None if done is None else done.data_ptr(), value,
                      C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream))
    return obs
