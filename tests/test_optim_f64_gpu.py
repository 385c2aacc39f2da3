"""The fused optimizer step (atr_adam_step / atr_rmsprop_step, csrc/driver_hip.hip) held to float64 at the sizes it runs at.

Both kernels launch at most 2048 workgroups of 256 threads = 524 288 elements per pass and walk the rest of the bucket in a
grid-stride loop; the tat-maze-lstm bucket is 801 300 floats, so every real update writes 277 012 elements in a second trip.
The reference is tests/optim_spec.py (the rules in float64, written from the rules) and the tolerance its derived one-step
rounding bound with multiplier 1, in "restart form": every step, float64 starts from the kernel's own fp32 state. The
bound is validated without a GPU by tests/test_optim_spec_cpu.py; the kernels round less than the tensor path it is
validated on (fmaf where that rounds twice; sqrtf and / correctly rounded, no contraction, no fast-math).

What is checked, and what each part would catch:
  * sizes n in SIZES through fused.adam_step / fused.rmsprop_step on views that start 12 bytes past a 16-byte boundary,
    sentinels on both sides: a skipped / repeated / shifted second trip, a dropped tail block, a write outside [0, n).
    The error is reported per region [0, 524288), [524288, n), last 256, so that a failure names the trip.
  * every configuration (both eps placements x amsgrad x weight decay; RMSprop eps 0.1 / 1e-8 x weight decay) at
    n = 801 300 over 12 steps of a gradient schedule spanning 1e-6 .. 1e3 with exact zeros: restart form each step,
    free-running against a free-running float64 under tests/f64_rule.Table.rule (x32 = the same optimizer with the fused
    path off, on the GPU), and the step counter / beta powers equal to the Python float64 products.
  * exact statements: zero gradient + zero moments keeps the weight's bits; AMSGrad's maximum never decreases and is
    above the second moment after the spike; padding stays zero.
  * the models' own buckets (tat-maze-lstm, maze-gru) under all four make_optimizer flag combinations.
  * the captured update (clip + step, as train._capture_update) replayed five times = five eager steps, bit for bit.

Measured on MI355X. Multiplier 1 holds; nothing on the device needs more. Worst error / bound over all steps:

    test                                      region               p      m      v      vmax
    sizes, Adam (amsgrad, wd 1e-2)  n=801300  [0, 524288)          0.990  0.787  0.552  0.539
                                              [524288, 801300)     0.997  0.794  0.548  0.534
                                              last 256             0.994  0.663  0.531  0.403
                                    n=1310723 [0, 524288)          0.970  0.799  0.546  0.539
                                              [524288, 1310723)    0.997  0.793  0.550  0.533
    sizes, RMSprop (wd 1e-2)        n=801300  [0, 524288)          1.000         0.534
                                              [524288, 801300)     1.000         0.538
    every configuration, n=801300   both trips (worst)             1.000  0.800  0.689  0.689
    tat-maze-lstm / maze-gru buckets (worst)                       1.000  0.730  0.690  0.690

(p reaches 1.000 where the update is below half an ulp of the weight: the weight keeps its bits and the error is the update.)
After 12 free-running steps, e = ||x - x64|| / ||x64||:

    configuration                       p: e(hip)  e(tensor32)      m: e(hip)  e(tensor32)     v: e(hip)  e(tensor32)
    Adam shared form amsgrad wd 0       8.498e-08  8.497e-08        1.149e-07  1.149e-07       1.191e-07  1.191e-07
    Adam torch form  amsgrad wd 1e-2    8.842e-08  8.842e-08        1.196e-07  1.196e-07       1.263e-07  1.262e-07
    Adam shared form no ams  wd 1e-2    8.783e-08  8.783e-08        1.197e-07  1.197e-07       1.265e-07  1.264e-07
    RMSprop eps 0.1   wd 0              6.840e-08  6.842e-08                                   7.232e-08  7.226e-08
    RMSprop eps 1e-8  wd 1e-2           9.089e-08  9.091e-08                                   8.963e-08  8.949e-08

(all twelve: p 6.8e-8 .. 9.2e-8, against FLOOR 1e-6 and ATEN_MAX 1e-4.)
"""
import itertools

import pytest
import torch

import f64_rule
import optim_spec as S
import test_optim_spec_cpu as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PASS = 2048 * 256                     # elements one pass of the capped grid covers
SIZES = [1, 255, 256, 257, PASS - 1, PASS, PASS + 1, 801300, 1310723]
BUCKET = 801300                       # tat-maze-lstm: 801 291 parameters in 32 slots + 9 padding floats
BETAS = H.BETAS
SENTINEL = -7.25


def regions(n):
    out = [("[0, %d)" % min(n, PASS), 0, min(n, PASS))]
    if n > PASS:
        out.append(("[%d, %d)" % (PASS, n), PASS, n))
    out.append(("last 256", max(0, n - 256), n))
    return out


def region_ratios(got, want, bound, n):
    """{region: worst |got - want| / bound}; the regions are the kernel's first pass, the later trips, and the ragged end."""
    err = (got.detach().double().cpu() - want).abs()
    r = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    return {name: float(r[a:b].max()) for name, a, b in regions(n)}


def check_regions(label, names, got, want, bound, n, worst):
    for k, a, b, d in zip(names, got, want, bound):
        for reg, r in region_ratios(a, b, d, n).items():
            worst[(k, reg)] = max(worst.get((k, reg), 0.0), r)
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, "%s: error / bound > 1 in %s" % (label, bad)


def guarded(n, fill=None):
    """A view [3 : 3 + n] of a buffer 256 floats longer filled with SENTINEL: (buffer, view)."""
    buf = torch.full((n + 256,), SENTINEL, device=DEV)
    view = buf[3:3 + n]
    assert view.data_ptr() % 16 == 12
    if fill is not None:
        view.copy_(fill)
    return buf, view


def assert_guards(bufs, n):
    for b in bufs:
        assert bool((b[:3] == SENTINEL).all()) and bool((b[3 + n:] == SENTINEL).all()), "a write outside [0, n)"


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
@pytest.mark.parametrize("n", SIZES)
def test_fused_step_at_grid_boundaries(n, kind):
    """Four steps in restart form at every size where the launch changes shape (one thread, one block +-1, a full grid +-1,
    the real bucket, three trips and a ragged tail), AMSGrad and weight decay on, misaligned views between sentinels."""
    from active_tracking_rl_amd import fused
    gen = torch.Generator().manual_seed(n)
    w0 = torch.randn(n, generator=gen) * torch.logspace(-3, 0, n)
    pb, p = guarded(n, w0)
    gb, g = guarded(n)
    names = ("p", "m", "v", "vmax") if kind == "adam" else ("p", "v")
    state = [guarded(n, torch.zeros(n)) for _ in names[1:]]
    scal = torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64, device=DEV)
    ss = torch.zeros(2, device=DEV)
    worst, t = {}, (0.0, 1.0, 1.0)
    for step in range(4):
        g.copy_(torch.randn(n, generator=gen) * (100.0 if step == 1 else 1.0))
        before = [x.double().cpu() for x in [p, g] + [s[1] for s in state]]
        if kind == "adam":
            t = S.advance(t, BETAS)
            want, bound = S.adam(*before, t, 1e-3, BETAS, 1e-3, 1e-2, True, False)
            fused.adam_step(p, g, state[0][1], state[1][1], state[2][1], scal, ss, 1e-3, BETAS[0], BETAS[1], 1e-3, 1e-2)
        else:
            want, bound = S.rmsprop(*before, 7e-4, 0.99, 0.1, 1e-2)
            fused.rmsprop_step(p, g, state[0][1], 7e-4, 0.99, 0.1, 1e-2)
        torch.cuda.synchronize()
        assert_guards([pb, gb] + [s[0] for s in state], n)
        assert torch.equal(g.cpu().double(), before[1])                                  # the gradient is read only
        check_regions("%s n=%d step %d" % (kind, n, step), names, [p] + [s[1] for s in state], want, bound, n, worst)
    if kind == "adam":
        assert scal.tolist() == list(t)
    print("%s n=%d" % (kind, n), {"%s %s" % k: "%.3f" % v for k, v in sorted(worst.items())})


def _optimizer(kind, cfg, w0, fused_path):
    from active_tracking_rl_amd.shared_optim import SharedAdam, SharedRMSprop
    p = torch.nn.Parameter(w0.to(DEV).clone())
    o = SharedAdam([p], lr=1e-3, betas=BETAS, **cfg) if kind == "adam" else SharedRMSprop([p], lr=1e-3, **cfg)
    o.fused = fused_path
    return o


@pytest.fixture(scope="module")
def schedule():
    """The 12-step run's start and gradients, made once on the CPU (read-only): weights randn * logspace(-4, 0), gradient
    scale 10^((7 t) % 10 - 6), every 17th gradient and all of step 5 exactly zero."""
    gen = torch.Generator().manual_seed(1)
    w0 = torch.randn(BUCKET, generator=gen) * torch.logspace(-4, 0, BUCKET)
    return w0, [H.scheduled_grad(s, BUCKET, gen) for s in range(12)]


CONFIGS = [("adam", c) for c in H.ADAM_CONFIGS] + [("rmsprop", c) for c in H.RMS_CONFIGS]


@pytest.mark.parametrize("kind,cfg", CONFIGS, ids=[k + "-" + H.config_id(c) for k, c in CONFIGS])
def test_every_configuration_at_the_real_bucket_size(kind, cfg, schedule):
    """n = 801 300, 12 steps: restart form each step (bound, multiplier 1); free-running weights and moments against
    free-running float64 under Table.rule with x32 = the tensor path on the GPU; _scalars = the Python products; the exact
    statements of the module docstring."""
    w0, grads = schedule
    hip, t32 = _optimizer(kind, cfg, w0, True), _optimizer(kind, cfg, w0, False)
    adam = kind == "adam"
    names = ("p", "m", "v", "vmax") if adam else ("p", "v")
    tensors = lambda o: [o.bucket.flat] + ([o.exp_avg, o.exp_avg_sq, o.max_exp_avg_sq] if adam else [o.square_avg])
    free = [w0.double()] + [torch.zeros(BUCKET, dtype=torch.float64) for _ in names[1:]]
    worst, t = {}, (0.0, 1.0, 1.0)
    for step, g in enumerate(grads):
        hip.bucket.grad.copy_(g)
        t32.bucket.grad.copy_(g)
        before = [x.double().cpu() for x in tensors(hip)]
        g64 = g.double()
        if adam:
            t = S.advance(t, BETAS)
            args = (t, 1e-3, BETAS, cfg["eps"], cfg["weight_decay"], cfg["amsgrad"], cfg["torch_eps"])
            want, bound = S.adam(before[0], g64, *before[1:], *args)
            free = list(S.adam(free[0], g64, *free[1:], *args)[0])
        else:
            args = (1e-3, 0.99, cfg["eps"], cfg["weight_decay"])
            want, bound = S.rmsprop(before[0], g64, before[1], *args)
            free = list(S.rmsprop(free[0], g64, free[1], *args)[0])
        hip.step()
        t32.step()
        torch.cuda.synchronize()
        check_regions("%s %s step %d" % (kind, H.config_id(cfg), step), names, tensors(hip), want, bound, BUCKET, worst)
        if adam:
            assert hip._scalars.tolist() == list(t) and t32._scalars.tolist() == list(t)
            if cfg["amsgrad"]:
                vmax, v = hip.max_exp_avg_sq.cpu(), hip.exp_avg_sq.cpu()
                assert bool((vmax.double() >= before[3]).all()) and bool((vmax >= v).all())
                if step == 5 and cfg["weight_decay"] == 0:   # an all-zero gradient after the 1e2 spike of step 4: v = beta2 v
                    assert bool((vmax > v)[v > 1e-30].all()) and int((v > 1e-30).sum()) > BUCKET // 2
            else:
                assert float(hip.max_exp_avg_sq.abs().max()) == 0.0
    print("%s %s" % (kind, H.config_id(cfg)), {"%s %s" % k: "%.3f" % v for k, v in sorted(worst.items())})
    if cfg["weight_decay"] == 0:                   # every 17th gradient was zero at every step: those weights keep their bits
        assert torch.equal(hip.bucket.flat.cpu()[::17], w0[::17])
        assert float((hip.bucket.flat.cpu() != w0).float().mean()) > 0.9
    table = f64_rule.Table("%s %s" % (kind, H.config_id(cfg)))
    for k, a, x64, x32 in zip(names, tensors(hip), free, tensors(t32)):
        if k == "vmax" and not cfg["amsgrad"]:
            continue
        table.rule(k + " after 12 steps", a, x64, x32)
    table.finish()


def _model_bucket(network, optimizer, shared):
    from active_tracking_rl_amd.environment import _spaces
    from active_tracking_rl_amd.model import build_model
    from active_tracking_rl_amd.shared_optim import make_optimizer
    from active_tracking_rl_amd.train import default_args
    args = default_args(network=network)
    args.optimizer, args.shared_optimizer = optimizer, shared
    torch.manual_seed(0)
    obs_s, act_s = _spaces()
    model = build_model(obs_s, act_s, args, torch.device(DEV)).to(DEV)
    return model, make_optimizer(list(model.parameters()), args), args


@pytest.mark.parametrize("optimizer,shared", list(itertools.product(("Adam", "RMSprop"), (True, False))))
@pytest.mark.parametrize("network", ["tat-maze-lstm", "maze-gru"])
def test_the_models_own_buckets(network, optimizer, shared):
    """build_model + make_optimizer, three steps of random gradients written into bucket.grad: restart form against the
    spec with the hyper-parameters make_optimizer documents; afterwards every parameter is still a view of `flat` at
    optim_spec.layout's offset and the padding is zero everywhere."""
    model, o, args = _model_bucket(network, optimizer, shared)
    b = o.bucket
    offsets, total = S.layout([tuple(p.shape) for p in b.params])
    assert b.offsets == offsets and b.numel == total
    if network == "tat-maze-lstm":
        assert total == BUCKET and b.param_numel == 801291 and len(b.params) == 32
    pad = H.padding_mask(b).to(DEV)
    adam = optimizer == "Adam"
    if adam:
        cfg = dict(eps=1e-3, amsgrad=bool(args.amsgrad), torch_eps=False) if shared else dict(eps=1e-8, amsgrad=False, torch_eps=True)
    else:
        cfg = dict(eps=0.1 if shared else 1e-8)
    names = ("p", "m", "v", "vmax") if adam else ("p", "v")
    tensors = lambda: [b.flat] + ([o.exp_avg, o.exp_avg_sq, o.max_exp_avg_sq] if adam else [o.square_avg])
    gen = torch.Generator().manual_seed(5)
    worst, t = {}, (0.0, 1.0, 1.0)
    for step in range(3):
        b.grad.copy_(torch.randn(total, generator=gen) * 10.0 ** (step - 2))
        b.grad[pad] = 0.0
        before = [x.double().cpu() for x in tensors()]
        g64 = b.grad.double().cpu()
        if adam:
            t = S.advance(t, BETAS)
            want, bound = S.adam(before[0], g64, *before[1:], t, args.lr, BETAS, cfg["eps"], 0, cfg["amsgrad"], cfg["torch_eps"])
        else:
            want, bound = S.rmsprop(before[0], g64, before[1], args.lr, 0.99, cfg["eps"], 0)
        o.step()
        torch.cuda.synchronize()
        check_regions("%s %s shared=%s step %d" % (network, optimizer, shared, step), names, tensors(), want, bound, total, worst)
    print(network, optimizer, shared, {"%s %s" % k: "%.3f" % v for k, v in sorted(worst.items())})
    for x in tensors() + [b.grad]:
        assert float(x[pad].abs().max()) == 0.0
    for p, off in zip(model.parameters(), offsets):
        assert p.data_ptr() == b.flat.data_ptr() + 4 * off and p.grad.data_ptr() == b.grad.data_ptr() + 4 * off
        assert torch.equal(p.detach().reshape(-1), b.flat[off:off + p.numel()])


def test_captured_update_replays_equal_eager_steps():
    """Clip + step captured as train._capture_update captures them, replayed five times with fresh gradients copied into
    bucket.grad: bit-equal to five eager steps (weights, moments, counters), the step counter reads 5, and the fifth step is
    within the spec's bound of float64 started from the state before it, given the clipped gradient the replay left behind."""
    from active_tracking_rl_amd import fused
    from active_tracking_rl_amd.shared_optim import SharedAdam
    from active_tracking_rl_amd.train import clip_flat_grad_
    fused.lib()
    shapes = [(BUCKET - 4097 - 1 - 14,), (4097,), (1,), (13,)]
    gen = torch.Generator().manual_seed(9)
    ws = [torch.randn(*s, generator=gen) * 0.1 for s in shapes]
    make = lambda: SharedAdam([torch.nn.Parameter(w.to(DEV).clone()) for w in ws], lr=1e-3, amsgrad=True)
    eager, graphed = make(), make()
    total = eager.bucket.numel
    assert total > PASS
    pad = H.padding_mask(eager.bucket)
    grads = [torch.randn(total, generator=gen) * (3.0 if s == 1 else 0.3) for s in range(5)]
    for g in grads:
        g[pad] = 0.0
    max_norm = 50.0                                                     # (the gradients' norms are ~270 and ~2700: the clip acts)
    for g in grads:
        eager.bucket.grad.copy_(g)
        clip_flat_grad_(eager, max_norm)
        eager.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        clip_flat_grad_(graphed, max_norm)
        graphed.step()
    assert float(graphed.step_t) == 0.0                                 # capturing ran nothing
    tensors = lambda o: [o.bucket.flat, o.exp_avg, o.exp_avg_sq, o.max_exp_avg_sq]
    t = (0.0, 1.0, 1.0)
    for s, g in enumerate(grads):
        graphed.bucket.grad.copy_(g)
        before = [x.double().cpu() for x in tensors(graphed)]
        graph.replay()
        torch.cuda.synchronize()
        t = S.advance(t, BETAS)
    assert float(graphed.step_t) == 5.0 and graphed._scalars.tolist() == list(t)
    for a, b in zip(tensors(eager) + [eager._scalars, eager.bucket.grad], tensors(graphed) + [graphed._scalars, graphed.bucket.grad]):
        assert torch.equal(a, b)
    clipped = graphed.bucket.grad.double().cpu()
    assert float(clipped.norm()) < 51.0 < float(grads[-1].double().norm())
    want, bound = S.adam(before[0], clipped, *before[1:], t, 1e-3, BETAS, 1e-3, 0, True, False)
    check_regions("captured update, step 5", ("p", "m", "v", "vmax"), tensors(graphed), want, bound, total, {})
