"""ego — the egocentric view: windows turn with the player, moves are relative (include/atr_ego.h; csrc/ego_hip.hip,
csrc/atr_ego_rule.h).

A 13 x 13 window as the env writes it is drawn north-up, and the four actions are compass moves. With this rule a player's facing
byte (fov.py: 0 .. 3 the VonNeumann move it last chose, NONE = 255) is its HEADING (NONE and what is no facing: 0, up):
to_absolute() turns the policy's relative actions (0 forward, 1 back, 2 left, 3 right) into the env's absolute ones, ABS[heading][k],
before the step, and turn_() turns the stored windows, in place, so that the player looks up — after it has turned the facing bytes
with the step's absolute actions and done flags, where nothing else (the field of view's pass) has done so already.
VecEnv(..., egocentric=...) keeps the bytes and the absolute-action buffers and runs both passes round every step().

There is no host path: the library's launches are the only implementation (tests/ego_spec.py holds the rule in numpy loops for the
tests)."""
import ctypes as C

import torch

from . import vec_env
from .occlusion import window_grid

WINDOW, SIDE, CENTRE = 169, 13, 6               # ATR_EGO_WINDOW, ATR_EGO_SIDE, ATR_EGO_CENTRE
NONE = 255                                      # ATR_FOV_NONE: counts as heading 0
FORWARD, BACK, LEFT, RIGHT = 0, 1, 2, 3         # ATR_EGO_FORWARD / BACK / LEFT / RIGHT
MAX_WINDOWS = (1 << 31) - 1                     # ATR_EGO_MAX_WINDOWS
ROLES = {"tracker": 1, "target": 2, "both": 3}  # ATR_EGO_TRACKER, ATR_EGO_TARGET: whose window turns, whose actions are relative
ABS = ((0, 1, 2, 3), (1, 0, 3, 2), (2, 3, 1, 0), (3, 2, 0, 1))       # ABS[heading][relative action]
REL = ((0, 1, 2, 3), (1, 0, 3, 2), (3, 2, 0, 1), (2, 3, 1, 0))       # REL[heading][absolute action]: the rows' inverses

_LL, _P = C.c_longlong, C.c_void_p
# {entry point: (restype, [argtypes])} for every function include/atr_ego.h declares
EGO_PROTOTYPES = {
    "atr_ego_actions": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _LL, C.c_int, _P]),
    "atr_ego_windows": (C.c_int, [_P, _P, C.c_int, _LL, C.c_int, _LL, _LL, _P, _P, _P, C.c_int, _P, C.c_int, _P]),
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
        for name, (restype, argtypes) in EGO_PROTOTYPES.items():
            f = getattr(L, name)         # (a library without the symbol is an error: there is no other path)
            f.restype, f.argtypes = restype, argtypes
            f.errcheck = _errcheck(name)
        _lib = L
    return _lib


def roles_of(egocentric):
    """The `roles` bits of an `egocentric` argument ("tracker", "target" or "both"). ValueError for anything else (True, "every
    model-driven player", is resolved by the env, which knows whether the id's target is scripted)."""
    if isinstance(egocentric, bool) or egocentric not in ROLES:
        raise ValueError("egocentric must be one of %s, got %r" % (sorted(ROLES), egocentric))
    return ROLES[egocentric]


def relative(actions, facing, table):
    """REL[heading][abs] as tensor ops on any device: actions [N] integers (absolute moves; a value outside 0 .. 3 passes through),
    facing uint8 [N] (NONE and what is no facing: heading 0), table the int64 [4, 4] tensor of REL on that device. Returns [N] of
    actions' dtype."""
    a = actions.reshape(-1).to(torch.int64)
    f = facing.reshape(-1).to(torch.int64)
    heading = torch.where(f <= 3, f, torch.zeros_like(f))
    inside = (a >= 0) & (a <= 3)
    return torch.where(inside, table[heading, a.clamp(0, 3)], a).to(actions.dtype).reshape(actions.shape)


def ego_actions(facing, rel0, rel1, abs0, abs1, act_dtype, n_env, roles, stream):
    """atr_ego_actions on raw device addresses (ints; 0 / None = NULL): the one place the entry point is called."""
    lib().atr_ego_actions(facing or None, rel0 or None, rel1 or None, abs0 or None, abs1 or None, int(act_dtype), int(n_env),
                          int(roles), stream)


def ego_windows(src, dst, is_u8, n_env, n_win, se, sp, facing, a0, a1, act_dtype, done, roles, stream):
    """atr_ego_windows on raw device addresses (ints; 0 / None = NULL) and element strides: the one place the entry point is
    called."""
    lib().atr_ego_windows(src or None, dst or None, int(bool(is_u8)), int(n_env), int(n_win), int(se), int(sp), facing or None,
                          a0 or None, a1 or None, int(act_dtype), done or None, int(roles), stream)


def _roles_bits(roles):
    if isinstance(roles, bool) or roles not in (1, 2, 3):
        raise ValueError("roles must be 1 (the tracker), 2 (the target) or 3 (both), got %r" % (roles,))
    return int(roles)


def to_absolute(rel, facing, roles, out):
    """One launch: rel = (r_tracker, r_target), each [N] uint8 / int32 / int64 contiguous on the device and of one dtype, the
    target's may be None (a scripted target); facing uint8 [N, 2] contiguous, only read; out = (o_tracker, o_target) of rel's
    dtype and sizes (out[p] may be rel[p] itself; o_target None exactly where r_target is). out[p][e] becomes
    ABS[heading][rel[p][e]] for a player in `roles`, rel[p][e] for the other. Launches on the current stream of facing's device.
    Capturable. Returns out."""
    roles = _roles_bits(roles)
    if not torch.is_tensor(facing) or facing.device.type != "cuda":
        raise RuntimeError("to_absolute runs on the GPU (there is no host path)")
    if facing.dtype != torch.uint8 or facing.dim() != 2 or facing.shape[1] != 2 or not facing.is_contiguous():
        raise ValueError("to_absolute: facing must be a contiguous uint8 [N, 2] tensor, got %s %s" % (facing.dtype, tuple(facing.shape)))
    n = int(facing.shape[0])
    rel = (tuple(rel) + (None,))[:2]
    out = (tuple(out) + (None,))[:2]
    if rel[0] is None or out[0] is None or (rel[1] is None) != (out[1] is None):
        raise ValueError("to_absolute: the tracker's actions and output are required, the target's go together")
    for a in rel + out:
        if a is not None and (not torch.is_tensor(a) or a.dtype not in vec_env._ACT_DTYPE or a.dtype != rel[0].dtype
                              or a.device != facing.device or a.numel() != n or not a.is_contiguous()):
            raise ValueError("to_absolute: actions must be contiguous [%d] uint8 / int32 / int64 tensors of one dtype on %s"
                             % (n, facing.device))
    if n == 0:
        return out
    ptr = lambda t: None if t is None else t.data_ptr()
    ego_actions(facing.data_ptr(), ptr(rel[0]), ptr(rel[1]), ptr(out[0]), ptr(out[1]), vec_env._ACT_DTYPE[rel[0].dtype], n, roles,
                C.c_void_p(torch.cuda.current_stream(facing.device).cuda_stream))
    return out


def turn_(obs, facing, actions=None, done=None, roles=3):
    """In place, one launch: obs [N, P, 13, 13] (P = 1 or 2 players) uint8 or float32 on the device, the windows' 169 cells
    contiguous, any strides over N and P that keep the windows apart (a slot of the rollout store, a slice of a larger store);
    facing uint8 [N, P] contiguous, read and written. actions: None, or (a_tracker, a_target) ABSOLUTE actions, each None or [N]
    uint8 / int32 / int64 contiguous, both of one dtype; done: None or uint8 [N]: the facings of the players in `roles` turn with
    them first (None: they stand — something else has turned them), then those players' windows are turned so that they look up.
    Launches on the current stream of obs' device. Capturable. Returns obs."""
    roles = _roles_bits(roles)
    if not torch.is_tensor(obs) or obs.device.type != "cuda":
        raise RuntimeError("turn_ runs on the GPU (there is no host path)")
    if (obs.dtype not in (torch.uint8, torch.float32) or obs.dim() != 4 or tuple(obs.shape[-2:]) != (SIDE, SIDE)
            or obs.shape[1] not in (1, 2) or obs.stride(-1) != 1 or obs.stride(-2) != SIDE):
        raise ValueError("turn_: obs must be uint8 / float32 [N, 1 or 2, 13, 13] with contiguous windows, got %s %s strides %s"
                         % (obs.dtype, tuple(obs.shape), tuple(obs.stride())))
    n, p = int(obs.shape[0]), int(obs.shape[1])
    window_grid(obs.shape[:2], obs.stride()[:2])          # (ValueError where windows would overlap)
    if (not torch.is_tensor(facing) or facing.dtype != torch.uint8 or facing.device != obs.device or tuple(facing.shape) != (n, p)
            or not facing.is_contiguous()):
        raise ValueError("turn_: facing must be a contiguous uint8 [%d, %d] tensor on %s" % (n, p, obs.device))
    acts = tuple(actions) if actions is not None else ()
    acts = (acts + (None, None))[:2]
    given = [a for a in acts if a is not None]
    for a in given:
        if (not torch.is_tensor(a) or a.dtype not in vec_env._ACT_DTYPE or a.dtype != given[0].dtype or a.device != obs.device
                or a.numel() != n or not a.is_contiguous()):
            raise ValueError("turn_: actions must be contiguous [%d] uint8 / int32 / int64 tensors of one dtype on %s" % (n, obs.device))
    if done is not None and (not torch.is_tensor(done) or done.dtype != torch.uint8 or done.device != obs.device
                             or done.numel() != n or not done.is_contiguous()):
        raise ValueError("turn_: done must be a contiguous uint8 [%d] tensor on %s" % (n, obs.device))
    if n == 0:
        return obs
    ptr = lambda t: None if t is None else t.data_ptr()
    ego_windows(obs.data_ptr(), obs.data_ptr(), obs.dtype == torch.uint8, n, p, obs.stride(0), obs.stride(1), facing.data_ptr(),
                ptr(acts[0]), ptr(acts[1]), vec_env._ACT_DTYPE[given[0].dtype] if given else 0, ptr(done), roles,
                C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream))
    return obs
