"""The maze policies' conv stem in float64, written from the operation itself (numpy only, no import of the package):

    x [M, 169] (13 x 13 frames)  --conv(1 -> 16, k3, s2, p1)-->  z1 [M, 16, 7, 7]  --ReLU-->  a1
                                 --conv(16 -> 32, k3, s2, p1)-->  z2 [M, 32, 4, 4]  --ReLU-->  y [M, 512]  ((c, h, w) order)

Both layers are explicit index sums: output (oh, ow) of a layer reads the zero-bordered input at (2 oh + kh, 2 ow + kw),
kh, kw = 0..2 (IDX1 / IDX2 below: im2col by index arrays, then one einsum per layer). No F.conv2d.

The backward is the kernels' contract (csrc/stem_hip.hip): given (x, y, dy) it returns the four parameter gradients of
sum(y dy); the conv2 mask is y > 0 of the y HANDED IN, the conv1 mask is a1 > 0 with a1 recomputed from x; a pre-activation
of exactly 0 passes no gradient; there is no gradient to x.

Two things make a float32 kernel comparable with this without a tolerance that absorbs ReLU-mask flips:

  abs_sums()      for every output element of every stage (z1, z2, da1, dw2, db2, dw1, db1) the sum of the ABSOLUTE values of the
                  terms that are added into it. On integer-valued data every partial sum of a stage, taken in any order and
                  with or without fused multiply-adds, is an integer no larger than the element's abs-sum: below 2^24 it is a
                  float32 number and no operation rounds. lattice_case() builds such data and asserts the condition, so a
                  correct fp32 kernel reproduces the float64 result BIT FOR BIT, exact ties z1 == 0 and z2 == 0 included.
  forward_error() the worst-case error of an fp32 forward on real-valued data. U = 2^-24; a sum of n products and a bias in fp32, in
                  any order, fused or not, is within (n + 1) U (sum of |terms|) of its exact value to first order. conv1 adds 9
                  products and the bias (10 terms), conv2 144 products and the bias (145 terms), and the 146th U of conv2 is the
                  rounding of nothing: it is slack, kept because the bound is stated that way:
                      e1 = 11 U S1                                        S1 = abs-sum of z1
                      e2 = 146 U S2 + (1 + 146 U) conv(|w2|, e1)          S2 = abs-sum of z2 (with the float64 a1)
                  (ReLU is 1-Lipschitz: a1's error is at most z1's; conv(|w2|, e1) carries it through conv2.)
                  margin_case() keeps only frames whose every pre-activation is at least k = 4 of these bounds away from 0: every
                  correct fp32 evaluation of a kept frame has the float64 ReLU masks (that holds from k = 1; 4 is margin).

uses_fwd16() / fwd_trips() restate the library's forward dispatch from the CU count, for the tests that must land on a
particular kernel form and loop trip."""
import numpy as np

U = 2.0 ** -24
EXACT_BELOW = 2.0 ** 24
STAGES = ("z1", "z2", "da1", "dw2", "db2", "dw1", "db1")


def _window_index(out_side, padded_side):
    """[out_side^2, 9] indices into a flattened zero-bordered padded_side^2 map: output (oh, ow), tap (kh, kw) reads
    (2 oh + kh, 2 ow + kw)."""
    idx = np.empty((out_side * out_side, 9), dtype=np.int64)
    for oh in range(out_side):
        for ow in range(out_side):
            for kh in range(3):
                for kw in range(3):
                    idx[oh * out_side + ow, kh * 3 + kw] = (2 * oh + kh) * padded_side + (2 * ow + kw)
    return idx


IDX1 = _window_index(7, 15)         # conv1: 13 x 13 zero-bordered to 15 x 15 -> 7 x 7
IDX2 = _window_index(4, 9)          # conv2: 7 x 7 zero-bordered to 9 x 9 -> 4 x 4


def _f64(*arrays):
    return [np.asarray(a, dtype=np.float64) for a in arrays]


def _pad(a, side):
    """[..., side * side] -> [..., (side + 2)^2] with a border of zeros."""
    a = a.reshape(a.shape[:-1] + (side, side))
    out = np.zeros(a.shape[:-2] + (side + 2, side + 2), dtype=np.float64)
    out[..., 1:-1, 1:-1] = a
    return out.reshape(a.shape[:-2] + ((side + 2) * (side + 2),))


def _unpad(a, side):
    a = a.reshape(a.shape[:-1] + (side + 2, side + 2))
    return a[..., 1:-1, 1:-1].reshape(a.shape[:-2] + (side * side,))


IDX2F = (np.arange(16)[None, :, None] * 81 + IDX2[:, None, :]).reshape(16, 144)     # ... of all 16 channels: [position, (ci, tap)]


class _Frames(object):
    """What every function below needs of a batch of frames under conv1's parameters: the windows of x, z1, a1 and (built on first
    use, the one large array: 2304 numbers per frame) the windows of a1. Layouts are chosen so that each einsum is one matrix
    product over contiguous operands."""

    def __init__(self, x, w1, b1):
        self.x = np.asarray(x, dtype=np.float64).reshape(-1, 169)
        self.z1 = affine1(self.x, w1, b1)
        self.a1 = np.maximum(self.z1, 0.0)
        self._col2, self.masked = None, None

    @property
    def col2(self):
        if self._col2 is None:
            self._col2 = col2(self.a1)
        return self._col2


def col1(x):
    """x [M, 169] -> [M, 49, 9] (frame, output position, tap): conv1's windows."""
    return np.take(_pad(x, 13), IDX1, axis=1)


def col2(a):
    """a [M, 16, 49] -> [M, 16, 144] (frame, output position, (input channel, tap)): conv2's windows."""
    return np.take(_pad(a, 7).reshape(a.shape[0], 16 * 81), IDX2F, axis=1)


def affine1(x, w1, b1):
    """z1[m, c, p] = b1[c] + sum_k window(x)[m, p, k] w1[c, k]  -> [M, 16, 49]"""
    return np.einsum("mpk,ck->mpc", col1(x), w1.reshape(16, 9), optimize=True).transpose(0, 2, 1) + b1[None, :, None]


def affine2(c2, w2, b2):
    """z2[m, o, p] = b2[o] + sum_k window(a1)[m, p, k] w2[o, k], k = (ci, tap)  -> [M, 32, 16]; c2 = col2(a1)"""
    return np.einsum("mpk,ok->mpo", c2, w2.reshape(32, 144), optimize=True).transpose(0, 2, 1) + b2[None, :, None]


def grad_a1(dz2, w2):
    """The transpose of conv2's index sum: da1[m, ci, loc] = sum over (o, p, tap) with window(p, tap) = loc of
    dz2[m, o, p] w2[o, ci, tap]; dz2 [M, 32, 16] -> [M, 16, 49]. (Tap (kh, kw)'s 16 windows are the locations
    (2 oh + kh, 2 ow + kw) of the bordered map: IDX2[:, tap] as a strided slice, which numpy adds into far faster.)"""
    cols = np.einsum("ok,opm->kpm", w2.reshape(32, 144), np.ascontiguousarray(dz2.transpose(1, 2, 0)), optimize=True)
    cols = cols.reshape(16, 9, 4, 4, -1)                 # (ci, tap, oh, ow, frame): frames innermost, long inner loops
    out = np.zeros((16, 9, 9, dz2.shape[0]), dtype=np.float64)
    for kh in range(3):
        for kw in range(3):
            out[:, kh:kh + 7:2, kw:kw + 7:2] += cols[:, kh * 3 + kw]
    return np.ascontiguousarray(out[:, 1:8, 1:8].reshape(16, 49, -1).transpose(2, 0, 1))


def grad_w2(dz2, c2):
    """dw2[o, k] = sum_{m, p} dz2[m, o, p] window(a1)[m, p, k]"""
    return np.einsum("mpo,mpk->ok", np.ascontiguousarray(dz2.transpose(0, 2, 1)), c2, optimize=True).reshape(32, 16, 3, 3)


def grad_w1(dz1, x):
    """dw1[c, k] = sum_{m, p} dz1[m, c, p] window(x)[m, p, k]"""
    return np.einsum("mpc,mpk->ck", np.ascontiguousarray(dz1.transpose(0, 2, 1)), col1(x), optimize=True).reshape(16, 1, 3, 3)


def forward(x, w1, b1, w2, b2, frames=None):
    """-> z1 [M, 16, 49], a1 [M, 16, 49], z2 [M, 32, 16], y [M, 512], float64."""
    w1, b1, w2, b2 = _f64(w1, b1, w2, b2)
    f = frames or _Frames(x, w1, b1)
    z2 = affine2(f.col2, w2, b2)
    return f.z1, f.a1, z2, np.maximum(z2, 0.0).reshape(-1, 512)


def _masked(f, y, dy, w2):
    """dz2 = dy where y > 0, dz1 = da1 where a1 > 0 (kept on f: backward() and abs_sums() of the same (y, dy) share them)"""
    if f.masked is None or f.masked[0] is not y or f.masked[1] is not dy:
        dz2 = np.where(np.asarray(y, dtype=np.float64) > 0.0, np.asarray(dy, dtype=np.float64), 0.0).reshape(-1, 32, 16)
        f.masked = (y, dy, dz2, np.where(f.a1 > 0.0, grad_a1(dz2, w2), 0.0))
    return f.masked[2:]


def backward(x, y, dy, w1, b1, w2, frames=None):
    """-> dw1 [16, 1, 3, 3], db1 [16], dw2 [32, 16, 3, 3], db2 [32], float64; y is the forward's output as the caller has it."""
    w1, b1, w2 = _f64(w1, b1, w2)
    f = frames or _Frames(x, w1, b1)
    dz2, dz1 = _masked(f, y, dy, w2)
    return grad_w1(dz1, f.x), dz1.sum(axis=(0, 2)), grad_w2(dz2, f.col2), dz2.sum(axis=(0, 2))


def abs_sums(x, y, dy, w1, b1, w2, b2, frames=None):
    """{stage: abs-sum of every element of that stage} (module docstring), the real masks applied: the same index sums on
    absolute values. a1 >= 0 makes dw2's a plain weight gradient with |dz2|; dz1 (a finished value of the da1 stage) is dw1's
    and db1's term."""
    w1, b1, w2, b2 = _f64(w1, b1, w2, b2)
    f = frames or _Frames(x, w1, b1)
    dz2, dz1 = _masked(f, y, dy, w2)
    return {"z1": affine1(np.abs(f.x), np.abs(w1), np.abs(b1)), "z2": affine2(f.col2, np.abs(w2), np.abs(b2)),
            "da1": grad_a1(np.abs(dz2), np.abs(w2)), "dw2": grad_w2(np.abs(dz2), f.col2), "db2": np.abs(dz2).sum(axis=(0, 2)),
            "dw1": grad_w1(np.abs(dz1), np.abs(f.x)), "db1": np.abs(dz1).sum(axis=(0, 2))}


def forward_error(x, w1, b1, w2, b2, frames=None):
    """-> e1 [M, 16, 49], e2 [M, 32, 16]: what z1 and z2 of an fp32 forward may differ from forward()'s (module docstring)."""
    w1, b1, w2, b2 = _f64(w1, b1, w2, b2)
    f = frames or _Frames(x, w1, b1)
    e1 = 11.0 * U * affine1(np.abs(f.x), np.abs(w1), np.abs(b1))
    e2 = 146.0 * U * affine2(f.col2, np.abs(w2), np.abs(b2)) + (1.0 + 146.0 * U) * affine2(col2(e1), np.abs(w2), np.zeros(32))
    return e1, e2


class Case(object):
    """Inputs of one test case as float32 arrays: x [M, 169], w1 [16, 1, 3, 3], b1 [16], w2 [32, 16, 3, 3], b2 [32], dy [M, 512].
    Lattice cases carry `largest` ({stage: largest abs-sum}), margin cases e2 [M, 512] and the (drawn, rejected) frame counts; both
    the float64 results y64 and grads64 (evaluate())."""

    def __init__(self, kind, x, w1, b1, w2, b2, dy, **extra):
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        self.kind, self.M = kind, int(x.shape[0])
        self.x, self.w1, self.b1, self.w2, self.b2, self.dy = f32(x), f32(w1), f32(b1), f32(w2), f32(b2), f32(dy)
        self.__dict__.update(extra)

    def weights(self):
        return self.w1, self.b1, self.w2, self.b2


def evaluate(case, with_abs_sums=False, chunk=2048):
    """Fills in case.y64 [M, 512] and case.grads64 = (dw1, db1, dw2, db2), float64, the backward on the float64 y; with_abs_sums
    also case.largest = {stage: the largest abs-sum over the stage's elements}. `chunk` frames at a time, each chunk's windows
    built once (the gradients and their abs-sums are sums over frames)."""
    w = _f64(*case.weights())
    ys, grads, per_frame, total = [], None, dict.fromkeys(("z1", "z2", "da1"), 0.0), {}
    for i in range(0, case.M, chunk):
        x, dy = case.x[i:i + chunk], case.dy[i:i + chunk]
        f = _Frames(x, w[0], w[1])
        y = forward(x, *w, frames=f)[3]
        g = backward(x, y, dy, w[0], w[1], w[2], frames=f)
        grads = g if grads is None else tuple(p + q for p, q in zip(grads, g))
        ys.append(y)
        if with_abs_sums:
            s = abs_sums(x, y, dy, *w, frames=f)
            for k in per_frame:
                per_frame[k] = max(per_frame[k], float(s[k].max()))
            for k in ("dw2", "db2", "dw1", "db1"):
                total[k] = s[k] if k not in total else total[k] + s[k]
    case.y64, case.grads64 = np.concatenate(ys), grads
    if with_abs_sums:
        per_frame.update((k, float(v.max())) for k, v in total.items())
        case.largest = per_frame
    return case


def lattice_case(seed, M, kind, x=None, dy=None, b2=None):
    """Integer-valued inputs (float32-exact) on which the whole computation is exact in fp32 (module docstring). kind "obs": frames
    from {0, 1, 2, 4}, w1 and w2 from {-1, 0, 1}, b1 from [-2, 2], b2 from [-6, 6], dy from {-1, 0, 1} with a quarter of the
    entries non-zero. kind "bytes": frames from 0..255, w1 from [-2, 2], w2 from {-1, 0, 1}, b1 from [-300, 300], b2 from
    [-3000, 3000], dy from {-1, 0, 1} dense; at most 48 frames. x / dy / b2 replace the drawn frames / output gradient / conv2
    bias (structured cases). Asserts integer data and every stage's abs-sums below 2^24: a case that misses is a bug in the case."""
    rs = np.random.RandomState(seed)
    if kind == "obs":
        xd = rs.choice([0, 1, 2, 4], size=(M, 169))
        w1, w2 = rs.randint(-1, 2, size=(16, 1, 3, 3)), rs.randint(-1, 2, size=(32, 16, 3, 3))
        b1, b2d = rs.randint(-2, 3, size=16), rs.randint(-6, 7, size=32)
        dyd = rs.choice([-1, 1], size=(M, 512)) * (rs.rand(M, 512) < 0.25)
    elif kind == "bytes":
        assert M <= 48, "byte-valued lattice cases stay exact up to 48 frames"
        xd = rs.randint(0, 256, size=(M, 169))
        w1, w2 = rs.randint(-2, 3, size=(16, 1, 3, 3)), rs.randint(-1, 2, size=(32, 16, 3, 3))
        b1, b2d = rs.randint(-300, 301, size=16), rs.randint(-3000, 3001, size=32)
        dyd = rs.randint(-1, 2, size=(M, 512))
    else:
        raise ValueError(kind)
    case = Case(kind, xd if x is None else x, w1, b1, w2, b2d if b2 is None else b2, dyd if dy is None else dy)
    assert case.x.shape == (M, 169) and case.dy.shape == (M, 512)
    for a in (case.x, case.dy) + case.weights():
        assert np.array_equal(a, np.round(a)), "lattice cases are integer-valued"
    evaluate(case, with_abs_sums=True)
    for stage in STAGES:
        assert case.largest[stage] < EXACT_BELOW, (kind, M, stage, case.largest[stage])
    return case


MAX_REJECTED = 0.15


def margin_weights(rs):
    """nn.Conv2d's default init (uniform in +- 1 / sqrt(fan_in): fan_in 9 and 144) scaled as the stem's tests always scaled it:
    conv1.weight x 2, conv2.weight x 3, biases N(0, 0.2); rounded to float32."""
    w1 = rs.uniform(-1.0, 1.0, size=(16, 1, 3, 3)) / 3.0 * 2.0
    w2 = rs.uniform(-1.0, 1.0, size=(32, 16, 3, 3)) / 12.0 * 3.0
    return [a.astype(np.float32) for a in (w1, rs.normal(0.0, 0.2, size=16), w2, rs.normal(0.0, 0.2, size=32))]


def margin_case(seed, M, kind, k=4):
    """Real-valued inputs whose ReLU masks no correct fp32 evaluation can flip (module docstring): margin_weights(), frames from
    {0, 1, 2, 4} (kind "obs") or 1.5 randn (kind "float": fractional, negative), drawn 2048 at a time until M are kept (the first M
    kept ones are the case); a frame is kept when
    every pre-activation has |z1| >= k e1 and |z2| >= k e2. dy is randn. Asserts that at most 15 % of the drawn frames were
    rejected (k = 4 rejects about 9 %; a larger k would make the kept frames a different population)."""
    rs = np.random.RandomState(seed)
    w1, b1, w2, b2 = margin_weights(rs)
    kept_x, kept_e2, drawn, rejected, have = [], [], 0, 0, 0
    while have < M:
        n = 2048                 # whole batches are drawn and counted, so the rejected share is a statistic of >= 2048 frames
        if kind == "obs":
            x = rs.choice([0.0, 1.0, 2.0, 4.0], size=(n, 169)).astype(np.float32)
        elif kind == "float":
            x = (1.5 * rs.randn(n, 169)).astype(np.float32)
        else:
            raise ValueError(kind)
        f = _Frames(x, *_f64(w1, b1))
        z1, _, z2, _ = forward(x, w1, b1, w2, b2, frames=f)
        e1, e2 = forward_error(x, w1, b1, w2, b2, frames=f)
        keep = (np.abs(z1) >= k * e1).all(axis=(1, 2)) & (np.abs(z2) >= k * e2).all(axis=(1, 2))
        take = np.flatnonzero(keep)[:M - have]
        drawn, rejected = drawn + n, rejected + n - int(keep.sum())
        kept_x.append(x[take]); kept_e2.append(e2[take].reshape(-1, 512))
        have += take.size
    assert rejected <= MAX_REJECTED * drawn, (kind, M, seed, rejected, drawn)
    dy = rs.randn(M, 512)
    return evaluate(Case(kind, np.concatenate(kept_x), w1, b1, w2, b2, dy, e2=np.concatenate(kept_e2), drawn=drawn,
                         rejected=rejected))


# ---- the library's forward dispatch, restated (csrc/stem_hip.hip: use_fwd16, stem_grid; no environment switch set)
FWD16_ALWAYS_FROM = 16384


def uses_fwd16(M, passes, cus):
    """Whether a forward launch of M frames in `passes` 16-frame passes (over all its problems) runs 16 frames per workgroup pass:
    from 16384 frames up always; from 3072 up where the passes load the CUs evenly (at most one per workgroup slot, two slots
    per CU, or CU rounds that are at least 85 % full); else one wave per frame."""
    if M >= FWD16_ALWAYS_FROM:
        return True
    if M < 3072:
        return False
    rounds = (passes + cus - 1) // cus
    return passes <= 2 * cus or passes * 100 >= rounds * cus * 85


def fwd_trips(M, workgroups):
    """Trips of the wave-per-frame forward's frame loop: `workgroups` of 4 waves over M frames."""
    return -(-M // (4 * workgroups))


def wave_per_frame_grid(M, cus):
    """Workgroups of the wave-per-frame forward for M frames: one wave per frame up to three workgroups per CU."""
    return max(1, min(-(-M // 4), 3 * cus))


def later_trip_frames(cus):
    """A frame count that the wave-per-frame forward takes in THREE trips on `cus` CUs: passes = 2 cus + cus / 4 (three CU rounds
    at 75 % fill: not the 16-frame kernel's), M = 16 passes - 5 (a ragged last pass). 9211 at 256 CUs."""
    return 16 * (2 * cus + cus // 4) - 5
