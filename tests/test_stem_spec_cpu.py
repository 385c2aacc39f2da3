"""tests/stem_spec.py is right before any kernel is held to it (no GPU): the float64 index sums against F.conv2d + autograd in
float64, the tie rule at a pre-activation of exactly 0, the lattice cases' exactness claim on a second fp32 implementation (the
CPU's own F.conv2d / autograd), the margin cases' rejected share and mask stability, and the restated forward dispatch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stem_spec as S

# the seeds and shapes tests/test_stem_f64_gpu.py and tests/stem_f64_worker.py build their margin cases with
from stem_f64_worker import MARGIN_CASES


def _autograd(case, dtype):
    """y and the four gradients of sum(y dy) through F.conv2d + ReLU + autograd on the CPU in `dtype`."""
    w1, b1, w2, b2 = [torch.tensor(a, dtype=dtype, requires_grad=True) for a in case.weights()]
    x = torch.tensor(case.x, dtype=dtype).view(-1, 1, 13, 13)
    a1 = F.relu(F.conv2d(x, w1, b1, stride=2, padding=1))
    y = F.relu(F.conv2d(a1, w2, b2, stride=2, padding=1)).reshape(case.M, 512)
    grads = torch.autograd.grad((y * torch.tensor(case.dy, dtype=dtype)).sum(), [w1, b1, w2, b2])
    return y.detach().numpy(), [g.numpy() for g in grads], a1.detach().numpy().reshape(case.M, 16, 49)


@pytest.mark.parametrize("kind,M", [("obs", 1), ("float", 7), ("float", 300)])
def test_the_spec_is_conv2d_and_its_autograd_in_float64(kind, M):
    """Real-valued weights and frames (no margin filter: plain random cases). Both sides are float64 evaluations of the same sums
    in different orders; with u = 2^-53 each is within n u A of the exact value (n terms, A the sum of their absolute values, the
    error of the terms themselves carried along), so the two agree to twice that:
      y          forward_error()'s e2 with u in place of 2^-24
      dw2        n = 16 M + 11, A = the weight gradient of |dz2| against conv1's abs-sums (a1 itself is only known to 11 u S1)
      dw1, db1   n = 49 M + 289, A = the sums of (da1's abs-sums under the a1 mask) x |x| (dz1 is only known to 289 u of them)
      db2        n = 16 M, A = sum |dz2|
    which is agreement to about 1e-12 of the values (asserted as 1e-11 of the largest element as well)."""
    rs = np.random.RandomState(M)
    w = S.margin_weights(rs)
    x = rs.choice([0.0, 1.0, 2.0, 4.0], size=(M, 169)) if kind == "obs" else 1.5 * rs.randn(M, 169)
    case = S.evaluate(S.Case(kind, x, *w, dy=rs.randn(M, 512)))
    y, grads, _ = _autograd(case, torch.float64)
    u = 2.0 ** -53
    w1, b1, w2, b2 = [np.abs(a.astype(np.float64)) for a in case.weights()]
    xa = np.abs(case.x.astype(np.float64))
    sums = S.abs_sums(case.x, case.y64, case.dy, *case.weights())
    _, e2 = S.forward_error(case.x, *case.weights())
    assert (np.abs(y - case.y64) <= 2.0 * (u / S.U) * e2.reshape(M, 512)).all()
    dz2 = np.where(case.y64 > 0, np.abs(case.dy), 0.0).reshape(M, 32, 16)
    da1 = np.where(S.forward(case.x, *case.weights())[1] > 0, sums["da1"], 0.0)
    A = {"dw1": S.grad_w1(da1, xa), "db1": da1.sum(axis=(0, 2)), "dw2": S.grad_w2(dz2, S.col2(sums["z1"])), "db2": sums["db2"]}
    n = {"dw1": 49 * M + 289, "db1": 49 * M + 289, "dw2": 16 * M + 11, "db2": 16 * M}
    for name, got, want in zip(("dw1", "db1", "dw2", "db2"), grads, case.grads64):
        err = np.abs(got - want)
        assert (err <= 2.0 * n[name] * u * A[name].reshape(want.shape)).all(), (name, float(err.max()))
        assert float(err.max()) <= 1e-11 * float(np.abs(want).max()), (name, float(err.max()))


def test_a_pre_activation_of_exactly_zero_passes_no_gradient():
    """y > 0 and a1 > 0, not >=: an all-zero frame under zero biases has z1 == 0 and z2 == 0 everywhere; with dy = 1 nothing
    may flow. Then one bias of each layer lifted to 1: exactly that channel's paths open."""
    x = np.zeros((1, 169))
    w1, w2 = np.ones((16, 1, 3, 3)), np.ones((32, 16, 3, 3))
    b1, b2 = np.zeros(16), np.zeros(32)
    dy = np.ones((1, 512))
    z1, a1, z2, y = S.forward(x, w1, b1, w2, b2)
    assert (z1 == 0).all() and (z2 == 0).all() and (y == 0).all()
    for g in S.backward(x, y, dy, w1, b1, w2):
        assert (g == 0).all()
    # the conv2 mask is taken from the y handed in, not recomputed
    _, db1, _, db2 = S.backward(x, np.ones((1, 512)), dy, w1, b1, w2)
    assert (db2 == 16).all() and (db1 == 0).all()              # conv2's ReLU open by decree; conv1's (a1 == 0) still shut
    b2[5] = 1.0
    z1, a1, z2, y = S.forward(x, w1, b1, w2, b2)
    dw1, db1, dw2, db2 = S.backward(x, y, dy, w1, b1, w2)
    assert db2[5] == 16 and db2.sum() == 16 and (db1 == 0).all() and (dw2 == 0).all() and (dw1 == 0).all()
    b1[3] = 1.0                                                # a1[3] = 1 everywhere, z2 = (real taps) > 0 for every channel
    z1, a1, z2, y = S.forward(x, w1, b1, w2, b2)
    dw1, db1, dw2, db2 = S.backward(x, y, dy, w1, b1, w2)
    assert (db2 == 16).all() and db1[3] > 0 and np.delete(db1, 3).sum() == 0 and (dw1 == 0).all()
    assert (dw2[:, 3] > 0).all() and np.delete(dw2, 3, axis=1).sum() == 0
    # every a1 location is read by conv2 windows: 100 real (position, tap) pairs in all, times 32 output channels
    assert db1[3] == 100 * 32 and dw2[:, 3].sum() == 100 * 32


@pytest.mark.parametrize("kind,M,seed", [("obs", 257, 1), ("obs", 4133, 2), ("bytes", 48, 3), ("bytes", 17, 4)])
def test_lattice_cases_are_exact_in_fp32_on_a_second_implementation(kind, M, seed):
    """Every abs-sum below 2^24 (asserted where the case is built; shown here) — and the CPU's fp32 F.conv2d + autograd, whose
    summation order is its own, gives float32(float64 result) bit for bit. Ties z1 == 0 and z2 == 0 are present."""
    case = S.lattice_case(seed, M, kind)
    assert set(case.largest) == set(S.STAGES) and max(case.largest.values()) < 2.0 ** 24, case.largest
    y, grads, a1 = _autograd(case, torch.float32)
    assert np.array_equal(y, case.y64.astype(np.float32))
    for got, want in zip(grads, case.grads64):
        assert np.array_equal(got, want.astype(np.float32).reshape(got.shape))
    z1, _, z2, _ = S.forward(case.x, *case.weights())
    assert (z1 == 0).sum() > 0 and ((z2 == 0).sum() > 0 or kind == "bytes")
    assert (case.grads64[0] != 0).sum() >= 100 and (case.grads64[2] != 0).sum() >= 3500      # (dead conv1 channels leave zeros)


def test_the_largest_lattice_case_matches_the_figures_it_was_designed_to():
    """40007 frames of kind "obs": the abs-sums the case was sized by (z2 a few hundred, dw2 below 1e6, dw1 5.8e6, db1 3.0e6: all
    below 2^24 = 1.68e7), every dw1 element and more than 4400 of the 4608 dw2 elements non-zero."""
    case = S.lattice_case(1, 40007, "obs")
    L = case.largest
    assert L["z2"] < 1e3 and L["dw2"] < 1e6 and 5e6 < L["dw1"] < 7e6 and 2e6 < L["db1"] < 4e6, L
    assert (case.grads64[0] != 0).all() and (case.grads64[2] != 0).sum() > 4400


@pytest.mark.parametrize("seed,M,kind", MARGIN_CASES + [(11, 4000, "obs"), (12, 4000, "float")])
def test_margin_cases_reject_few_frames_and_keep_the_float64_masks_in_fp32(seed, M, kind):
    if M is None:
        M = S.later_trip_frames(256)
    case = S.margin_case(seed, M, kind)
    assert case.M == M and case.rejected <= S.MAX_REJECTED * case.drawn
    print("%s M=%d: %d of %d drawn frames rejected (%.1f %%)" % (kind, M, case.rejected, case.drawn, 100.0 * case.rejected / case.drawn))
    z1, a64, z2, y64 = S.forward(case.x, *case.weights())
    e1, e2 = S.forward_error(case.x, *case.weights())
    assert (np.abs(z1) >= 4 * e1).all() and (np.abs(z2) >= 4 * e2).all()
    assert np.array_equal(e2.reshape(M, 512), case.e2)
    y32, _, a32 = _autograd(case, torch.float32)
    assert np.array_equal(a32 > 0, a64 > 0) and np.array_equal(y32 > 0, y64 > 0)
    assert (np.abs(y32 - y64) <= case.e2).all()                # the CPU's fp32 forward is inside the derived bound too


def test_the_forward_bound_holds_for_fp32_sums_in_adversarial_orders():
    """forward_error()'s derivation, checked where it could be wrong: conv1 and conv2 evaluated in fp32 term by term in ascending,
    descending, by-magnitude and random orders (bias first or last) stay within e1 / e2 of the float64 values."""
    rs = np.random.RandomState(5)
    w1, b1, w2, b2 = S.margin_weights(rs)
    x = (1.5 * rs.randn(24, 169)).astype(np.float32)
    z1, a1, z2, _ = S.forward(x, w1, b1, w2, b2)
    e1, e2 = S.forward_error(x, w1, b1, w2, b2)

    def summed(terms, order):                                   # terms [..., n] float32, added left to right in `order`
        acc = np.zeros(terms.shape[:-1], dtype=np.float32)
        for j in order:
            acc = (acc + terms[..., j]).astype(np.float32)
        return acc
    worst = 0.0
    for trial in range(6):
        t1 = np.concatenate([(S.col1(x.astype(np.float64)).astype(np.float32)[:, None, :, :] *
                              w1.reshape(1, 16, 1, 9)).astype(np.float32),
                             np.broadcast_to(b1.reshape(1, 16, 1, 1), (24, 16, 49, 1))], axis=3)        # [M, 16, 49, 10]
        order1 = {0: range(10), 1: range(9, -1, -1)}.get(trial, rs.permutation(10))
        z1_32 = summed(t1, order1)
        assert (np.abs(z1_32 - z1) <= e1).all()
        a32 = np.maximum(z1_32, 0).astype(np.float64)
        c2 = S.col2(a32).astype(np.float32)                                                           # [M, 16, 144]
        t2 = np.concatenate([(c2[:, None, :, :] * w2.reshape(1, 32, 1, 144)).astype(np.float32),
                             np.broadcast_to(b2.reshape(1, 32, 1, 1), (24, 32, 16, 1))], axis=3)        # [M, 32, 16, 145]
        if trial == 2:
            order2 = np.argsort(np.abs(t2).sum(axis=(0, 1, 2)))[::-1]                                  # large terms first
        else:
            order2 = {0: range(145), 1: range(144, -1, -1)}.get(trial, rs.permutation(145))
        z2_32 = summed(t2, order2)
        assert (np.abs(z2_32 - z2) <= e2).all()
        worst = max(worst, float((np.abs(z2_32 - z2) / e2).max()))
    print("largest |z2(fp32, some order) - z2| / e2 = %.3f" % worst)
    assert 0.0 < worst <= 1.0


def test_the_restated_forward_dispatch_on_256_cus():
    """Hand-computed for 256 CUs (512 workgroup slots of the 16-frame kernel, 768 workgroups = 3072 frames per trip of the
    wave-per-frame kernel):
       9211 frames = 576 passes: more than 512 slots, 3 CU rounds 75 % full        -> wave per frame, 3 trips
       4099 frames = 257 passes: at most one per slot                              -> 16 frames per pass
      12288 frames = 768 passes: 3 rounds, 100 % full                              -> 16 frames per pass
      16384 frames                                                                 -> 16 frames per pass (always from there)
    and the windows in between: (8192, 10432] and (12288, 13920] are the wave-per-frame kernel's, on later trips."""
    cus = 256
    passes = lambda M: -(-M // 16)
    assert S.later_trip_frames(cus) == 9211 and passes(9211) == 576
    assert not S.uses_fwd16(9211, 576, cus)
    assert S.wave_per_frame_grid(9211, cus) == 768 and S.fwd_trips(9211, 768) == 3
    for M in (4099, 12288, 16384, 3072, 8192, 10433, 13921, 40007):
        assert S.uses_fwd16(M, passes(M), cus), M
    for M in (1, 64, 3071, 8193, 10432, 12289, 13920):
        assert not S.uses_fwd16(M, passes(M), cus), M
    # the paired launch of (M / 3, M - M / 3): 192 + 384 passes, 256 + 512 workgroups, three trips each
    M0, M1 = 9211 // 3, 9211 - 9211 // 3
    assert (M0, M1) == (3070, 6141) and passes(M0) + passes(M1) == 576
    assert S.fwd_trips(M0, 256) == 3 and S.fwd_trips(M1, 512) == 3
    # below one wave per frame the grid shrinks and the loop runs once
    assert S.wave_per_frame_grid(257, cus) == 65 and S.fwd_trips(257, 65) == 1
