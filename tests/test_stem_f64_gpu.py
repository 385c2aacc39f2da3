"""-m gpu: the hot-path conv stem (csrc/stem_hip.hip: k_stem_fwd, k_stem_fwd16, k_stem_bwd, k_stem_bwd16, k_stem_reduce, each on
float and on byte frames) against the float64 statement of the operation in tests/stem_spec.py, through fused.stem,
fused.stem_into, fused.stem_into2, fused._stem_backward and the C entry point (the checks themselves: tests/stem_f64_worker.py).

EXACT cases are integer-valued (stem_spec.lattice_case: every abs-sum below 2^24, so fp32 cannot round, in any summation order):
y and all four gradients must be torch.equal to float32(float64 result) — one wrong tap at one border position of one frame is a
wrong integer, and exact ties z1 == 0, z2 == 0 pin the ReLU masks to `> 0`. ROUNDING cases are real-valued with every
pre-activation at least 4 derived error bounds from 0 (stem_spec.margin_case), so no correct fp32 evaluation flips a mask: y is
held element by element to the derived worst case e2, the gradients to the per-tensor rule of tests/f64_rule.py.

Which kernel form and loop trip a case reaches (256 CUs; the tests derive it from the device's CU count):
  k_stem_fwd    first trip: M <= 3071 cases; later trips: M = 16 (2 CUs + CUs / 4) - 5 = 9211, 3 trips, one-problem and paired
                (asserted by the restated dispatch rule); at 16391 frames in the forced child process
  k_stem_fwd16  M = 4133 (259 passes on 512 slots), 16391, 40007, the paired (4096, 8192) [G == 2 C, CU-aware numbering] and
                (5000, 11003); at 1 .. 49 and 169 frames in the forced child process
  k_stem_bwd    every M < 16384; later trips at 4133 (3 trips, the last 37 frames) and 9211; 16391 in the forced child
  k_stem_bwd16  16391 and 40007 (157 workgroups x 16 passes, ragged); 1 .. 49 and 169 frames in the forced child

Measured on MI355X (this module and both child processes):
  forward    max |y - y64| / e2 = 0.013 .. 0.030 over the 16 (rounding case, frame form) runs: 37 / 1000 / 9211 / 33 frames
  dw1        e(hip) 1.2e-07 .. 2.6e-07      e(aten32) 1.4e-07 .. 2.3e-06      e(hip) / allowed <= 0.26
  db1        e(hip) 8.9e-08 .. 3.2e-07      e(aten32) 9.3e-08 .. 2.0e-07      e(hip) / allowed <= 0.32
  dw2        e(hip) 1.0e-07 .. 2.1e-07      e(aten32) 1.2e-07 .. 1.7e-06      e(hip) / allowed <= 0.13
  db2        e(hip) 6.4e-08 .. 2.4e-07      e(aten32) 7.0e-08 .. 1.9e-07      e(hip) / allowed <= 0.24
The module takes 23 s, no case more than 4 s (the two child processes: 3.5 s each; the float64 reference of 40007 frames: 3 s).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import stem_f64_worker as K
import stem_spec as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def lattice(seed, M, kind):
    return S.lattice_case(seed, M, kind)


@functools.lru_cache(maxsize=None)
def margin(seed, M, kind):
    return S.margin_case(seed, M, kind)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def later_trip_frames():
    """The frame count that puts the wave-per-frame forward on its second and third trip on this device, checked by the restated
    dispatch rule: not the 16-frame kernel's, below 16384, more than one trip."""
    C = cus()
    M = S.later_trip_frames(C)
    passes = 2 * C + C // 4
    assert -(-M // 16) == passes and M < S.FWD16_ALWAYS_FROM
    assert not S.uses_fwd16(M, passes, C), "M = %d is the 16-frame kernel's on %d CUs" % (M, C)
    assert S.fwd_trips(M, S.wave_per_frame_grid(M, C)) == 3
    return M


@pytest.mark.parametrize("kind,M", [("obs", M) for M in (1, 2, 3, 4, 5, 63, 64, 65, 257)] + [("bytes", M) for M in (1, 17, 48)])
def test_small_launches_are_bit_equal_to_float64(kind, M):
    """k_stem_fwd / k_stem_bwd on their first trip: partly filled workgroups, one wave, more than one workgroup."""
    K.check_exact(lattice(1000 + M, M, kind))


def test_wave_per_frame_backward_on_later_trips_is_bit_equal_to_float64():
    """2 x 2048 + 37 frames: k_stem_bwd's 512 workgroups make three trips, the last one ragged (the forward of this size is
    k_stem_fwd16's: 259 passes on 512 slots)."""
    K.check_exact(lattice(2, 2 * 2048 + 37, "obs"))


def test_wave_per_frame_forward_on_later_trips_is_bit_equal_to_float64():
    """k_stem_fwd's frame loop prefetches the next trip's frame across its back-edge; three trips at 75 % fill of the third CU round."""
    M = later_trip_frames()
    K.check_exact(lattice(3, M, "obs"))


def test_paired_wave_per_frame_forward_on_later_trips_is_bit_equal_to_float64():
    """The same frame count as a two-problem launch (M / 3, M - M / 3) with two weight sets: the workgroups split 1 : 2, three trips
    on either side."""
    M = later_trip_frames()
    C, M0, M1 = cus(), M // 3, M - M // 3
    assert not S.uses_fwd16(M, -(-M0 // 16) + -(-M1 // 16), C)
    total = S.wave_per_frame_grid(M, C)
    g0 = (total * M0 + M // 2) // M
    assert S.fwd_trips(M0, g0) > 1 and S.fwd_trips(M1, total - g0) > 1
    for form in K.FORMS:
        K.check_exact_pair(lattice(4, M0, "obs"), lattice(5, M1, "obs"), form)


@pytest.mark.parametrize("M", [16391, 40007])
def test_sixteen_frame_kernels_under_production_dispatch_are_bit_equal_to_float64(M):
    """k_stem_fwd16 and k_stem_bwd16 where production runs them: ragged last passes, more than one pass per workgroup."""
    assert S.uses_fwd16(M, -(-M // 16), cus())
    K.check_exact(lattice(1, M, "obs"))


@pytest.mark.parametrize("M0,M1", [(4096, 8192), (5000, 11003)])
def test_paired_sixteen_frame_forward_is_bit_equal_to_float64(M0, M1):
    """The two-problem launch of k_stem_fwd16: the headline's rollout shape (768 passes on 2 CUs workgroups: the CU-aware pass
    numbering) and an uneven, ragged pair from 16384 frames up."""
    assert S.uses_fwd16(M0 + M1, -(-M0 // 16) + -(-M1 // 16), cus())
    for form in K.FORMS:
        K.check_exact_pair(lattice(6, M0, "obs"), lattice(7, M1, "obs"), form)


def test_structured_frames_are_bit_equal_to_float64():
    """All-zero frames (y is relu(b) carried through; only bias gradients), frames that are 1 on the outer ring and 0 inside and
    the inverse (every border tap of both layers beside padding), and a single 1 at each of the 169 pixels in turn under a
    one-hot dy."""
    for name, case in K.structured_cases():
        if name == "zero frames":
            assert (case.grads64[0] == 0).all() and (case.grads64[1] != 0).any()
        K.check_exact(case, label=name)


def test_dead_relu_gives_zero_gradients_not_nan():
    """b2 = -1e6: y == 0 everywhere, and all four gradients exactly 0."""
    case = S.lattice_case(8, 64, "obs", b2=np.full(32, -1.0e6))
    assert (case.y64 == 0).all() and all((g == 0).all() for g in case.grads64)
    K.check_exact(case, label="dead ReLU")


@pytest.mark.parametrize("seed,M,kind", [c for c in K.MARGIN_CASES if c[1] != 33])
def test_rounding_cases_stay_within_the_derived_bound_and_the_f64_rule(seed, M, kind):
    """Forward: |y - y64| <= e2 for every element (e2 = 146 U S2 + (1 + 146 U) conv(|w2|, 11 U S1): the worst case of ANY fp32
    evaluation; measured max |y - y64| / e2: 0.018 / 0.013 at 37 frames ("obs" / "float"), 0.019 / 0.021 at 1000, 0.030 / 0.028 at
    9211 — a guarantee, the resolution is the exact cases') and y == 0 exactly where the float64 y is 0.
    Gradients: e(hip) <= max(4 e(aten32), 1e-6), e(aten32) <= 1e-4."""
    K.check_rounding(margin(seed, later_trip_frames() if M is None else M, kind))


@pytest.mark.parametrize("M,form", [(1000, "float"), (2 * 2048 + 37, "strided"), (16391, "float"), (16391, "bytes")])
def test_backward_is_bit_reproducible(M, form):
    """'Fixed-order reduction (reproducible)': the same backward twice on real-valued data gives the same bits — k_stem_bwd on
    float and byte frames (one and three trips), k_stem_bwd16 on both."""
    K.check_reproducible(M, form, seed=M)


@pytest.mark.parametrize("M", [5, 2 * 2048 + 37])
def test_a_nan_filled_workspace_leaves_no_trace(M):
    """The C entry point with its workspace (atr_stem_workspace_floats(M) floats) full of NaN: the gradients are finite and the
    exact result, so every partial record the reduce kernel reads was written whole (2 and 512 records)."""
    K.check_exact(lattice(9 if M == 5 else 2, M, "obs"), forms=("float", "strided"), nan_workspace=True)


def _child(value):
    env = dict(os.environ, ATR_STEM_FWD16_MIN=value, ATR_STEM_BWD16_MIN=value)
    r = subprocess.run([sys.executable, os.path.join(HERE, "stem_f64_worker.py")], env=env, timeout=120, capture_output=True,
                       text=True)
    print(r.stdout)
    assert r.returncode == 0 and "STEM_F64_OK" in r.stdout, (r.stdout[-3000:], r.stderr[-4000:])


def test_sixteen_frame_kernels_at_their_smallest_shapes_in_a_fresh_process():
    """tests/stem_f64_worker.py with ATR_STEM_FWD16_MIN = ATR_STEM_BWD16_MIN = 1: k_stem_fwd16 / k_stem_bwd16 at 1 .. 49 frames
    (float, byte, strided byte), paired launches (16, 1), (1, 16), (17, 33), the single-pixel sweep and ring frames — a pass holds 16
    different frames, so a frame-to-MFMA-row mix-up is a wrong element — a NaN-filled workspace at 17 frames, and a margin case."""
    _child("1")


def test_wave_per_frame_kernels_at_16391_frames_in_a_fresh_process():
    """The same worker with both switches at 1000000: k_stem_fwd / k_stem_bwd at 16391 frames (6 and 9 trips), exact."""
    _child("1000000")
