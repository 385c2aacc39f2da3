"""The stem kernels (csrc/stem_hip.hip) held to tests/stem_spec.py: the checks that tests/test_stem_f64_gpu.py runs in-process
under the library's own dispatch, and — as a script, started by that module in ONE fresh child process — the same checks with
the library's crossover switches set in the environment (they are read once per process):

    ATR_STEM_FWD16_MIN = ATR_STEM_BWD16_MIN = 1         every launch takes k_stem_fwd16 / k_stem_bwd16: 16 frames per workgroup
                                                        pass at 1 .. 49 frames, where a pass holds 16 DIFFERENT frames whose
                                                        every element can be told apart (in-process these kernels start at 4099
                                                        / 16384 frames); ragged passes are the kernels' own contract (clamped
                                                        loads, guarded stores, dz2 zeroed past the last frame)
    ATR_STEM_FWD16_MIN = ATR_STEM_BWD16_MIN = 1000000   every launch takes the wave-per-frame kernels: 16391 frames, a size they
                                                        never see in-process

It prints one line per case and exits non-zero on the first failure.

Exact checks (lattice cases: integer data, every abs-sum below 2^24) demand torch.equal with float32(float64 spec) for y and all
four gradients; rounding checks (margin cases) hold y element by element to the spec's derived fp32 bound e2 and the gradients to
the per-tensor rule of tests/f64_rule.py against F.conv2d + autograd in fp32 on the GPU. Outputs are written in front of sentinel
values, which must survive."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import stem_spec as S  # noqa: E402

DEV = "cuda"
FORMS = ("float", "bytes", "strided")          # float32 frames; uint8 frames; agent 1 of a [M, 2, 13, 13] uint8 observation tensor
Y_SENTINEL_ROWS, G_SENTINEL = 3, 8
GRADS = ("dw1", "db1", "dw2", "db2")
# (seed, frames or None = stem_spec.later_trip_frames(CUs), kind) of every margin case the GPU checks build
MARGIN_CASES = [(21, 37, "obs"), (22, 37, "float"), (23, 1000, "obs"), (24, 1000, "float"), (25, None, "obs"), (26, None, "float"),
                (27, 33, "obs"), (28, 33, "float")]


class Enc(object):
    """conv1 / conv2 holding a case's weights on the GPU (what fused.stem* take)."""

    def __init__(self, case):
        self.conv1 = torch.nn.Conv2d(1, 16, 3, 2, 1).to(DEV)
        self.conv2 = torch.nn.Conv2d(16, 32, 3, 2, 1).to(DEV)
        with torch.no_grad():
            for p, a in zip((self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias), case.weights()):
                p.copy_(torch.from_numpy(a))

    def params(self):
        return [self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias]


def frames(case, form):
    """The case's frames on the GPU as [M, 13, 13]: float32; uint8; or the strided uint8 view obs[:, 1] of an [M, 2, 13, 13]
    tensor (frame stride 338 from an odd base: frames start at all four byte alignments), agent 0's frames other values."""
    x = torch.from_numpy(case.x).view(-1, 13, 13)
    if form == "float":
        return x.to(DEV)
    assert float(x.min()) >= 0 and float(x.max()) <= 255 and bool((x == x.round()).all()), "byte forms need byte-valued frames"
    if form == "bytes":
        return x.to(torch.uint8).to(DEV)
    obs = torch.empty((case.M, 2, 13, 13), dtype=torch.uint8)
    obs[:, 1] = x.to(torch.uint8)
    obs[:, 0] = 255 - obs[:, 1]
    view = obs.to(DEV)[:, 1]
    assert view.stride(0) == 338 and view.storage_offset() == 169
    return view


def forms_of(case):
    return FORMS if case.kind in ("obs", "bytes") else FORMS[:1]


def forward_all(x, enc, M):
    """y [M, 512] through fused.stem_into, written in front of 3 sentinel rows; fused.stem must give the same bits."""
    from active_tracking_rl_amd import fused
    buf = torch.full((M + Y_SENTINEL_ROWS, 512), -7.0, device=DEV)
    fused.stem_into(x, enc.conv1, enc.conv2, buf[:M])
    assert bool((buf[M:] == -7.0).all()), "stem_into wrote past its last row"
    with torch.no_grad():
        y = fused.stem(x, enc.conv1, enc.conv2)
    assert y.shape == (M, 512) and torch.equal(y, buf[:M]), "fused.stem and fused.stem_into disagree"
    return buf[:M]


def backward_raw(x, y, dy, enc, nan_workspace=False):
    """The C entry point itself: the four gradients written in front of 8 sentinel floats each, the workspace
    (atr_stem_workspace_floats(M) floats, 8 sentinels behind it too) pre-filled with NaN on request."""
    from active_tracking_rl_amd import fused
    L = fused.lib()
    x = fused._frame_rows(x)
    M = x.shape[0]
    n_ws = int(L.atr_stem_workspace_floats(M))
    ws = torch.full((n_ws + G_SENTINEL,), float("nan") if nan_workspace else 0.5, device=DEV)
    ws[n_ws:] = -7.0
    outs = [torch.full((n + G_SENTINEL,), -7.0, device=DEV) for n in (144, 16, 4608, 32)]
    w1, b1, w2 = [p.detach().contiguous() for p in enc.params()[:3]]
    dy = dy.contiguous()
    p = fused._p
    fused._stem_fn("atr_stem_backward", x)(p(x), x.stride(0), p(y), p(dy), p(w1), p(b1), p(w2), p(outs[0]), p(outs[1]), p(outs[2]),
                                           p(outs[3]), p(ws), M, fused._stream(x))
    for name, o, n in zip(GRADS, outs, (144, 16, 4608, 32)):
        assert bool((o[n:] == -7.0).all()), "the backward wrote past the end of " + name
    assert bool((ws[n_ws:] == -7.0).all()), "the backward wrote past the end of its workspace"
    return [o[:n] for o, n in zip(outs, (144, 16, 4608, 32))]


def backward_all(x, y, dy, enc, nan_workspace=False):
    """The gradients through fused._stem_backward and through the C entry point (sentinels, optional NaN workspace): same bits."""
    from active_tracking_rl_amd import fused
    w1, b1, w2 = [p.detach().contiguous() for p in enc.params()[:3]]
    got = fused._stem_backward(fused._frame_rows(x), y, dy, w1, b1, w2, (w1.shape, w2.shape))
    raw = backward_raw(x, y, dy, enc, nan_workspace)
    for name, a, b in zip(GRADS, got, raw):
        assert torch.equal(a.reshape(-1), b), "%s: fused._stem_backward and the C entry point disagree" % name
    return raw


def _equal(name, got, want64, label):
    want = torch.from_numpy(np.ascontiguousarray(want64, dtype=np.float32)).reshape(got.shape)
    got = got.detach().cpu()
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError("%s: %s differs from the float64 spec in %d of %d elements; first at flat index %d: %r != %r"
                             % (label, name, int(bad.sum()), bad.numel(), i, float(got.reshape(-1)[i]), float(want.reshape(-1)[i])))


def check_exact(case, forms=None, nan_workspace=False, label=""):
    """A lattice case through every frame form: y and all four gradients bit-equal to float32(float64 spec)."""
    enc = Enc(case)
    dy = torch.from_numpy(case.dy).to(DEV)
    for form in forms or forms_of(case):
        x = frames(case, form)
        tag = "%s %s M=%d %s" % (label, case.kind, case.M, form)
        y = forward_all(x, enc, case.M)
        _equal("y", y, case.y64, tag)
        for name, g, want in zip(GRADS, backward_all(x, y, dy, enc, nan_workspace), case.grads64):
            _equal(name, g, want, tag)


def check_exact_pair(case0, case1, form, label=""):
    """Two lattice cases (their own weights) through the two-problem launch fused.stem_into2, sentinel rows behind both outputs."""
    from active_tracking_rl_amd import fused
    encs = [Enc(case0), Enc(case1)]
    xs = [frames(case0, form), frames(case1, form)]
    bufs = [torch.full((c.M + Y_SENTINEL_ROWS, 512), -7.0, device=DEV) for c in (case0, case1)]
    fused.stem_into2(xs[0], encs[0], bufs[0][:case0.M], xs[1], encs[1], bufs[1][:case1.M])
    for k, (c, b) in enumerate(zip((case0, case1), bufs)):
        assert bool((b[c.M:] == -7.0).all()), "stem_into2 wrote past problem %d's last row" % k
        _equal("y of problem %d" % k, b[:c.M], c.y64, "%s pair (%d, %d) %s" % (label, case0.M, case1.M, form))


def aten32(case):
    """F.conv2d + ReLU + autograd in float32 on the GPU: the rule's yardstick. (PyTorch's own convolution — unfold + GEMM — not the
    vendor library's: that one builds kernels for every new batch size when it first meets it, 18 s at 9211 frames.)"""
    w = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in case.weights()]
    x = torch.from_numpy(case.x).to(DEV).view(-1, 1, 13, 13)
    was = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        a1 = F.relu(F.conv2d(x, w[0], w[1], stride=2, padding=1))
        y = F.relu(F.conv2d(a1, w[2], w[3], stride=2, padding=1)).reshape(case.M, 512)
        return [g.detach() for g in torch.autograd.grad((y * torch.from_numpy(case.dy).to(DEV)).sum(), w)]
    finally:
        torch.backends.cudnn.enabled = was


def check_rounding(case, label=""):
    """A margin case through every frame form it has. Forward: |y - y64| <= e2 element by element (multiplier 1: the derived worst
    case) and exactly 0 where y64 == 0. Gradients: tests/f64_rule.py's rule per tensor. Returns (largest |y - y64| / e2, rows)."""
    from f64_rule import Table
    enc = Enc(case)
    dy = torch.from_numpy(case.dy).to(DEV)
    y64, e2 = torch.from_numpy(case.y64), torch.from_numpy(case.e2)
    x32 = aten32(case)
    worst, rows = 0.0, []
    for form in forms_of(case):
        x = frames(case, form)
        tag = "%s margin %s M=%d %s" % (label, case.kind, case.M, form)
        y = forward_all(x, enc, case.M)
        err = (y.detach().cpu().double() - y64).abs()
        ratio = float((err / e2).max())
        print("%-44s max |y - y64| / e2 = %.4f" % (tag, ratio))
        assert bool((err <= e2).all()), "%s: y misses the derived fp32 bound: |y - y64| / e2 up to %.3f" % (tag, ratio)
        assert bool((y.detach().cpu()[y64 == 0] == 0).all()), tag + ": y != 0 where the float64 y is exactly 0"
        tab = Table(tag)
        for name, g, want, g32 in zip(GRADS, backward_all(x, y, dy, enc), case.grads64, x32):
            tab.rule(name, g, torch.from_numpy(np.ascontiguousarray(want)), g32)
        rows += tab.finish()
        worst = max(worst, ratio)
    return worst, rows


def check_reproducible(M, form, seed=0):
    """The same backward twice on plain random real data (no reference needed): the same bits."""
    rs = np.random.RandomState(seed)
    w = S.margin_weights(rs)
    case = S.Case("obs", rs.choice([0.0, 1.0, 2.0, 4.0], size=(M, 169)), *w, dy=rs.randn(M, 512))
    enc = Enc(case)
    x, dy = frames(case, form), torch.from_numpy(case.dy).to(DEV)
    y = forward_all(x, enc, M)
    a, b = backward_all(x, y, dy, enc), backward_all(x, y, dy, enc)
    for name, p, q in zip(GRADS, a, b):
        assert bool(torch.isfinite(p).all()) and torch.equal(p, q), "%s differs between two runs (M=%d %s)" % (name, M, form)


# ---- structured lattice cases
def ring_frames(M, inverse=False):
    """Frames that are 1 on the outer ring and 0 inside (or the inverse): every border tap of both layers sees padding beside data."""
    f = np.zeros((13, 13))
    f[0, :] = f[-1, :] = f[:, 0] = f[:, -1] = 1
    return np.tile((1 - f if inverse else f).reshape(1, 169), (M, 1))


def single_pixel_sweep():
    """169 frames, frame i a single 1 at pixel i, dy one-hot at an output the pixel can reach: channel i mod 32 at the output
    position whose window is centred nearest the pixel. Every (pixel, tap, channel) path is alone in some gradient element."""
    x, dy = np.eye(169), np.zeros((169, 512))
    for i in range(169):
        r, c = divmod(i, 13)
        dy[i, (i % 32) * 16 + min(3, (r + 2) // 4) * 4 + min(3, (c + 2) // 4)] = 1
    return x, dy


def structured_cases(seed=40):
    x, dy = single_pixel_sweep()
    return [("zero frames", S.lattice_case(seed, 64, "obs", x=np.zeros((64, 169)))),
            ("ring", S.lattice_case(seed + 1, 64, "obs", x=ring_frames(64))),
            ("inverse ring", S.lattice_case(seed + 2, 64, "obs", x=ring_frames(64, inverse=True))),
            ("single-pixel sweep", S.lattice_case(seed + 3, 169, "obs", x=x, dy=dy))]


# ---- the forced-dispatch child process
def _forced_sixteen():
    for M in (1, 2, 15, 16, 17, 31, 32, 33, 49):
        check_exact(S.lattice_case(100 + M, M, "obs"), label="fwd16/bwd16")
        print("OK exact obs M=%d float bytes strided" % M, flush=True)
    for M in (1, 17, 48):
        check_exact(S.lattice_case(200 + M, M, "bytes"), label="fwd16/bwd16")
        print("OK exact bytes M=%d float bytes strided" % M, flush=True)
    for M0, M1 in ((16, 1), (1, 16), (17, 33)):
        for form in FORMS:
            check_exact_pair(S.lattice_case(300 + M0, M0, "obs"), S.lattice_case(310 + M1, M1, "obs"), form, label="fwd16")
        print("OK exact pair (%d, %d)" % (M0, M1), flush=True)
    for name, case in structured_cases():
        check_exact(case, label="fwd16/bwd16 " + name)
        print("OK exact %s M=%d" % (name, case.M), flush=True)
    check_exact(S.lattice_case(217, 17, "obs"), nan_workspace=True, label="fwd16/bwd16 NaN workspace")
    print("OK exact obs M=17 with a NaN-filled workspace", flush=True)
    for seed, M, kind in MARGIN_CASES:
        if M == 33:
            worst, _ = check_rounding(S.margin_case(seed, M, kind), label="fwd16/bwd16")
            print("OK rounding %s M=33, |y - y64| / e2 <= %.4f" % (kind, worst), flush=True)
    check_reproducible(33, "float")
    check_reproducible(49, "strided")
    print("OK reproducible M=33 float, M=49 strided", flush=True)


def _forced_wave_per_frame():
    check_exact(S.lattice_case(1, 16391, "obs"), label="fwd/bwd (wave per frame)")
    print("OK exact obs M=16391 float bytes strided", flush=True)


def main():
    f16, b16 = os.environ.get("ATR_STEM_FWD16_MIN"), os.environ.get("ATR_STEM_BWD16_MIN")
    if f16 == b16 == "1":
        _forced_sixteen()
    elif f16 == b16 == "1000000":
        _forced_wave_per_frame()
    else:
        raise SystemExit("stem_f64_worker.py runs with ATR_STEM_FWD16_MIN = ATR_STEM_BWD16_MIN = 1 or 1000000 (got %r, %r)" % (f16, b16))
    torch.cuda.synchronize()
    print("STEM_F64_OK", flush=True)


if __name__ == "__main__":
    main()
