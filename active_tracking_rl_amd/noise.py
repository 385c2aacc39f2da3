"""noise — sensor noise: flicker, missed and false detections (include/atr_noise.h; csrc/noise_hip.hip, csrc/atr_noise_rule.h).

A player's 13 x 13 window is disturbed by three kinds of draw: a free cell or a wall off the centre flickers to the other of the
two (threshold `flicker`, per cell), the other player vanishes from the window (`miss`, per window), and a free cell shows the
other player where it is not (`ghost`, per window). Every draw is a Philox4x32-10 word keyed by (key; global env id, the window's
clock, player, block), so the result is a pure function of those and does not depend on how envs are sharded. noise_() keeps the
clock — uint32 [N, 2], which the caller owns: ADVANCE moves a noisy window's clock on by one and draws with the new value, PEEK
draws with the clock as it stands and stores nothing to it — and disturbs the windows in place, in the same launch.
VecEnv(..., sensor_noise={...}) keeps the clock and runs the pass behind every reset(), step() and observe(), after the occlusion,
field-of-view, footprint and map-memory passes and ahead of the egocentric turn.

There is no host path: the library's launch is the only implementation (tests/noise_spec.py holds the rule in numpy for the
tests)."""
import ctypes as C

import torch

from . import vec_env
from .occlusion import window_grid

WINDOW, SIDE, CENTRE = 169, 13, 84      # ATR_NOISE_WINDOW, the window's side, ATR_NOISE_CENTRE
ONE = 1 << 24                           # ATR_NOISE_ONE: the threshold of probability 1
TAG = 0x4E5E0000                        # ATR_NOISE_TAG
PEEK, ADVANCE = 0, 1                    # ATR_NOISE_PEEK / ADVANCE
ROLES = {"tracker": 1, "target": 2, "both": 3}        # whose window is noisy (bit 0: the tracker's, bit 1: the target's)
KINDS = ("flicker", "miss", "ghost")
KEY_SALT = 0x6E6F6973655F7632           # "noise_v2": the noise shares a key with no stream keyed by the raw seed

_LL, _P = C.c_longlong, C.c_void_p
# {entry point: (restype, [argtypes])} for every function include/atr_noise.h declares
NOISE_PROTOTYPES = {
    "atr_noise_windows": (C.c_int, [_P, _P, C.c_int, _LL, _LL, _P, C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
}
_lib = None


def _errcheck(name):
    """As footprints._errcheck: a non-zero status raises RuntimeError naming the entry point, with the library's own text."""
    def check(status, func=None, args=None):
        if status != 0:
            raise RuntimeError("%s failed (%d): %s" % (name, status, vec_env.load_library().t2d_last_error().decode()))
        return status
    return check


def lib():
    global _lib
    if _lib is None:
        L = vec_env.load_library()
        for name, (restype, argtypes) in NOISE_PROTOTYPES.items():
            f = getattr(L, name)         # (a library without the symbol is an error: there is no other path)
            f.restype, f.argtypes = restype, argtypes
            f.errcheck = _errcheck(name)
        _lib = L
    return _lib


def threshold_of(p):
    """The integer threshold round(p * 2**24) of a probability p in [0, 1]. ValueError for anything else."""
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:        # (a nan fails the comparison)
        raise ValueError("a sensor-noise rate must be a number in [0, 1], got %r" % (p,))
    return int(round(float(p) * ONE))


def thresholds_of(sensor_noise):
    """(flicker, miss, ghost) thresholds of a `sensor_noise` argument: a dict with keys out of 'flicker' / 'miss' / 'ghost' and
    rates in [0, 1], at least one of which gives a threshold above 0. ValueError for anything else."""
    if not isinstance(sensor_noise, dict):
        raise ValueError("sensor_noise must be a dict with keys out of %s, got %r" % (list(KINDS), sensor_noise))
    unknown = sorted(str(k) for k in sensor_noise if k not in KINDS)
    if unknown:
        raise ValueError("sensor_noise: unknown key(s) %s (the rates are %s)" % (unknown, list(KINDS)))
    t = tuple(threshold_of(sensor_noise.get(k, 0.0)) for k in KINDS)
    if not any(t):
        raise ValueError("sensor_noise=%r: every rate is 0, so the pass would change nothing (leave sensor_noise out)"
                         % (sensor_noise,))
    return t


def roles_of(noise_for):
    """The `roles` bits of a `noise_for` argument ("tracker", "target" or "both"). ValueError for anything else."""
    if noise_for not in ROLES:
        raise ValueError("noise_for must be one of %s, got %r" % (sorted(ROLES), noise_for))
    return ROLES[noise_for]


def key_of(seed):
    """The 64-bit Philox key of a run's seed."""
    return (int(seed) & (2 ** 64 - 1)) ^ KEY_SALT


def new_clock(num_envs, device):
    """An all-zero clock uint32 [num_envs, 2] on `device` (made as int32: the same bits, and a dtype every device op knows)."""
    return torch.zeros((int(num_envs), 2), dtype=torch.int32, device=device).view(torch.uint32)


def noise_windows(h, obs, is_u8, se, sp, clock, key, flicker, miss, ghost, roles, mode, stream):
    """atr_noise_windows on a handle, raw device addresses (ints; 0 / None = NULL) and element strides: the one place the entry
    point is called."""
    lib().atr_noise_windows(h or None, obs or None, int(bool(is_u8)), int(se), int(sp), clock or None, int(key) & (2 ** 64 - 1),
                            int(flicker), int(miss), int(ghost), int(roles), int(mode), stream)


def noise_(obs, clock, core, mode, key, thresholds, roles=1):
    """In place, one launch: obs [N, 2, 13, 13] uint8 or float32 on the device, the windows' 169 cells contiguous, any strides over
    N and the players that keep the windows apart (a slot of the rollout store, a slice of a larger store); clock uint32 [N, 2]
    contiguous, read and (under ADVANCE) written; core a VecTrack2D of N envs, which gives the global env ids; mode PEEK / ADVANCE;
    key a 64-bit int (key_of); thresholds (flicker, miss, ghost) in 0 .. ONE; roles 1 (the tracker's window is noisy), 2 (the
    target's) or 3. Launches on the current stream of obs' device. Capturable. Returns obs."""
    if not torch.is_tensor(obs) or obs.device.type != "cuda":
        raise RuntimeError("noise_ runs on the GPU (there is no host path)")
    if (obs.dtype not in (torch.uint8, torch.float32) or obs.dim() != 4 or tuple(obs.shape[-2:]) != (SIDE, SIDE)
            or obs.shape[1] != 2 or obs.stride(-1) != 1 or obs.stride(-2) != SIDE):
        raise ValueError("noise_: obs must be uint8 / float32 [N, 2, 13, 13] with contiguous windows, got %s %s strides %s"
                         % (obs.dtype, tuple(obs.shape), tuple(obs.stride())))
    n = int(obs.shape[0])
    window_grid(obs.shape[:2], obs.stride()[:2])          # (ValueError where windows would overlap)
    if n != int(core.num_envs):
        raise ValueError("noise_: obs holds %d envs, the handle %d" % (n, core.num_envs))
    if (not torch.is_tensor(clock) or clock.dtype != torch.uint32 or clock.device != obs.device or tuple(clock.shape) != (n, 2)
            or not clock.is_contiguous()):
        raise ValueError("noise_: clock must be a contiguous uint32 [%d, 2] tensor on %s" % (n, obs.device))
    if mode not in (PEEK, ADVANCE):
        raise ValueError("noise_: mode must be PEEK (0) or ADVANCE (1), got %r" % (mode,))
    flicker, miss, ghost = thresholds
    if n == 0:
        return obs
    noise_windows(core.h, obs.data_ptr(), obs.dtype == torch.uint8, obs.stride(0), obs.stride(1), clock.data_ptr(), key, flicker,
                  miss, ghost, roles, mode, C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream))
    return obs
