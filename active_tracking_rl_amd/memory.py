"""memory — map memory: hidden cells show walls a player has seen (include/atr_memory.h; csrc/memory_hip.hip,
csrc/atr_memory_rule.h).

Under occlusion or a field of view most of a 13 x 13 window reads 5 ("unseen"). With map memory a player keeps, per episode, the
set of map cells it has had in view — `seen`, uint32 [N, 2, 256]: one bit-packed tile per (env, player) in the layout of the
handle's map tiles, which the caller owns — and a hidden cell it has seen before reads `wall_value` (7) where the map has a wall
and `free_value` (8) where it has none. remember_() clears (BEGIN: every env; STEP: the envs whose `done` flag is set; KEEP: none),
records the cells visible now and paints, in place and in one launch. The positions, the map side and the map come from the env
handle: the windows must be the ones the handle's last launch wrote, after the occlusion, field-of-view and footprint passes.
VecEnv(..., map_memory=...) keeps the tiles and runs the pass behind every reset(), step() and observe(), ahead of the egocentric
turn.

There is no host path: the library's launch is the only implementation (tests/memory_spec.py holds the rule in numpy loops for the
tests)."""
import ctypes as C

import torch

from . import vec_env
from .occlusion import window_grid

WINDOW, SIDE = 169, 13          # ATR_MEMORY_WINDOW, ATR_MEMORY_SIDE
TILE_WORDS, ROW_WORDS, MAX_SIDE = 256, 3, 82      # ATR_MEMORY_TILE_WORDS, ATR_MEMORY_ROW_WORDS, ATR_MEMORY_MAX_SIDE
HIDDEN, WALL, FREE = 5, 7, 8    # ATR_MEMORY_HIDDEN, ATR_MEMORY_WALL, ATR_MEMORY_FREE
KEEP, STEP, BEGIN = 0, 1, 2     # ATR_MEMORY_KEEP / STEP / BEGIN
ROLES = {"tracker": 1, "target": 2, "both": 3}        # whose memory is kept (bit 0: the tracker's, bit 1: the target's)

_LL, _P = C.c_longlong, C.c_void_p
# {entry point: (restype, [argtypes])} for every function include/atr_memory.h declares
MEMORY_PROTOTYPES = {
    "atr_memory_windows": (C.c_int, [_P, _P, C.c_int, _LL, _LL, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
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
        for name, (restype, argtypes) in MEMORY_PROTOTYPES.items():
            f = getattr(L, name)         # (a library without the symbol is an error: there is no other path)
            f.restype, f.argtypes = restype, argtypes
            f.errcheck = _errcheck(name)
        _lib = L
    return _lib


def roles_of(map_memory):
    """The `roles` bits of a `map_memory` argument ("tracker", "target" or "both"). ValueError for anything else."""
    if not isinstance(map_memory, str) or map_memory not in ROLES:
        raise ValueError("map_memory must be one of %s, got %r" % (sorted(ROLES), map_memory))
    return ROLES[map_memory]


def new_seen(num_envs, device):
    """All-zero seen tiles uint32 [num_envs, 2, 256] on `device` (made as int32: the same bits, and a dtype every device op
    knows)."""
    return torch.zeros((int(num_envs), 2, TILE_WORDS), dtype=torch.int32, device=device).view(torch.uint32)


def unpack(seen, side):
    """bool [N, 2, side, side] of seen tiles uint32 [N, 2, 256]: element (e, p, r, c) is bit c & 31 of word 3 r + (c >> 5).
    Tensor ops, on seen's device."""
    side = int(side)
    if not 1 <= side <= MAX_SIDE:
        raise ValueError("unpack: side must be 1 .. %d, got %r" % (MAX_SIDE, side))
    if not torch.is_tensor(seen) or seen.dtype != torch.uint32 or seen.dim() != 3 or tuple(seen.shape[1:]) != (2, TILE_WORDS):
        raise ValueError("unpack: seen must be a uint32 [N, 2, %d] tensor" % TILE_WORDS)
    words = seen.view(torch.int32)[:, :, :side * ROW_WORDS].reshape(seen.shape[0], 2, side, ROW_WORDS)
    shifts = torch.arange(32, dtype=torch.int32, device=seen.device)
    bits = (words.unsqueeze(-1) >> shifts) & 1                     # [N, 2, side, 3, 32] (an arithmetic shift: the & 1 takes bit i)
    return bits.reshape(seen.shape[0], 2, side, ROW_WORDS * 32)[..., :side] != 0


def memory_windows(h, obs, is_u8, se, sp, seen, roles, mode, done, hidden, wall_value, free_value, stream):
    """atr_memory_windows on a handle, raw device addresses (ints; 0 / None = NULL) and element strides: the one place the entry
    point is called."""
    lib().atr_memory_windows(h or None, obs or None, int(bool(is_u8)), int(se), int(sp), seen or None, int(roles), int(mode),
                             done or None, int(hidden), int(wall_value), int(free_value), stream)


def remember_(obs, seen, core, mode, done=None, roles=1, hidden=HIDDEN, wall_value=WALL, free_value=FREE):
    """In place, one launch: obs [N, 2, 13, 13] uint8 or float32 on the device, the windows' 169 cells contiguous, any strides over
    N and the players that keep the windows apart (a slot of the rollout store, a slice of a larger store) — the windows that the
    last launch of `core` (a VecTrack2D of N envs) wrote; seen uint32 [N, 2, 256] contiguous, read and written; mode KEEP / STEP /
    BEGIN; done: None or uint8 [N]; roles 1 (the tracker's memory), 2 (the target's) or 3. Launches on the current stream of obs'
    device. Capturable. Returns obs."""
    if not torch.is_tensor(obs) or obs.device.type != "cuda":
        raise RuntimeError("remember_ runs on the GPU (there is no host path)")
    if (obs.dtype not in (torch.uint8, torch.float32) or obs.dim() != 4 or tuple(obs.shape[-2:]) != (SIDE, SIDE)
            or obs.shape[1] != 2 or obs.stride(-1) != 1 or obs.stride(-2) != SIDE):
        raise ValueError("remember_: obs must be uint8 / float32 [N, 2, 13, 13] with contiguous windows, got %s %s strides %s"
                         % (obs.dtype, tuple(obs.shape), tuple(obs.stride())))
    n = int(obs.shape[0])
    window_grid(obs.shape[:2], obs.stride()[:2])          # (ValueError where windows would overlap)
    if n != int(core.num_envs):
        raise ValueError("remember_: obs holds %d envs, the handle %d" % (n, core.num_envs))
    if (not torch.is_tensor(seen) or seen.dtype != torch.uint32 or seen.device != obs.device or seen.dim() != 3
            or tuple(seen.shape) != (n, 2, TILE_WORDS) or not seen.is_contiguous()):
        raise ValueError("remember_: seen must be a contiguous uint32 [%d, 2, %d] tensor on %s" % (n, TILE_WORDS, obs.device))
    if mode not in (KEEP, STEP, BEGIN):
        raise ValueError("remember_: mode must be KEEP (0), STEP (1) or BEGIN (2), got %r" % (mode,))
    if done is not None and (not torch.is_tensor(done) or done.dtype != torch.uint8 or done.device != obs.device
                             or done.numel() != n or not done.is_contiguous()):
        raise ValueError("remember_: done must be a contiguous uint8 [%d] tensor on %s" % (n, obs.device))
    if n == 0:
        return obs
    memory_windows(core.h, obs.data_ptr(), obs.dtype == torch.uint8, obs.stride(0), obs.stride(1), seen.data_ptr(), roles, mode,
                   None if done is None else done.data_ptr(), hidden, wall_value, free_value,
                   C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream))
    return obs
