"""tests/optim_spec.py (the update rules in float64 + a derived fp32 rounding bound) held to three independent witnesses,
and the package's CPU tensor path (SharedAdam / SharedRMSprop with fused = False) held to the spec. This file is what
validates the bound without a GPU; tests/test_optim_f64_gpu.py then holds the HIP kernels to the same bound.

  * tests/golden/optim.npz: the reference's own SharedAdam / SharedRMSprop, run by tests/golden/make_golden_optim.py.
  * torch.optim.Adam (amsgrad off) and torch.optim.RMSprop run in float64: the spec's torch form, bound taken at U64.
  * the tensor path in "restart form": every step, float64 starts from the tensor path's own fp32 state, so the error of
    ONE step is compared with the ONE-step bound (multiplier 1).

Worst error / bound of the tensor path over 24 steps of 200 003 elements (weights randn * logspace(-4, 0), gradient scale
10^((7 t) % 10 - 6), every 17th gradient and all of step 5 exactly zero), measured on the CPU:

    configuration                                 p      m      v      vmax
    Adam  shared form  amsgrad      wd 0          1.000  0.798  0.686  0.686
    Adam  torch form   amsgrad      wd 0          1.000  0.798  0.686  0.686
    Adam  shared form  amsgrad      wd 1e-2       1.000  0.798  0.545  0.529
    Adam  torch form   amsgrad      wd 1e-2       1.000  0.799  0.544  0.519
    Adam  shared form  no amsgrad   wd 0          1.000  0.798  0.686
    Adam  torch form   no amsgrad   wd 0          1.000  0.798  0.686
    Adam  shared form  no amsgrad   wd 1e-2       1.000  0.799  0.545
    Adam  torch form   no amsgrad   wd 1e-2       0.999  0.799  0.544
    RMSprop eps 0.1    wd 0                       1.000         0.546
    RMSprop eps 0.1    wd 1e-2                    1.000         0.532
    RMSprop eps 1e-8   wd 0                       1.000         0.546
    RMSprop eps 1e-8   wd 1e-2                    1.000         0.533

(p reaches 1.000 where the update is below half an ulp of the weight: the weight keeps its bits, the error IS the update,
and the bound is half an ulp plus a d(upd) that is ~1e-7 of it.)

RMSprop with eps 1e-8 and weight decay missed a bound without underflow terms by 1e5: weight decay alone (gradient exactly
zero at every 17th element) walks one weight of this run to ~1e-41, where wd p is a subnormal with two significant bits,
its square is zero, and the update is that grid error over eps. The tensor path is right (float64 fed the same subnormal
weight agrees with it to the grid spacing over eps); the bound was wrong to assume relative rounding there. optim_spec's
"Underflow" paragraph has the corrected derivation, test_subnormal_weights_under_weight_decay the case on its own.
"""
import itertools
import os

import numpy as np
import pytest
import torch

import optim_spec as S
from conftest import GOLDEN
from active_tracking_rl_amd.shared_optim import FlatParams, SharedAdam, SharedRMSprop

BETAS = (0.9, 0.999)
ADAM_CONFIGS = [dict(amsgrad=a, weight_decay=w, torch_eps=te, eps=1e-8 if te else 1e-3)
                for a, w, te in itertools.product((True, False), (0, 1e-2), (False, True))]
RMS_CONFIGS = [dict(eps=e, weight_decay=w) for e, w in itertools.product((0.1, 1e-8), (0, 1e-2))]


def config_id(c):
    return "-".join("%s=%s" % kv for kv in sorted(c.items()))


def scheduled_grad(t, n, gen, device="cpu"):
    """The gradient schedule of the issue's draft run: scale 10^((7 t) % 10 - 6), every 17th entry and all of step 5 zero."""
    g = torch.randn(n, generator=gen, device=device) * 10.0 ** ((7 * t) % 10 - 6)
    g[::17] = 0
    if t == 5:
        g.zero_()
    return g


def worst_ratio(got, want, bound):
    """max over elements of |got - want| / bound (0 where the error is 0), with the index it is reached at."""
    err = (got.detach().double().cpu() - want).abs().reshape(-1)
    r = torch.where(err > 0, err / bound.reshape(-1).clamp_min(1e-300), torch.zeros_like(err))
    i = int(r.argmax())
    return float(r[i]), i


def adam_state(o):
    return [x.detach().double().cpu().clone() for x in (o.bucket.flat, o.bucket.grad, o.exp_avg, o.exp_avg_sq, o.max_exp_avg_sq)]


def restart_adam(o, t, lr, cfg):
    """One o.step() against optim_spec.adam started from o's own fp32 state: {name: (worst ratio, index)}."""
    st = adam_state(o)
    new, bound = S.adam(*st, t, lr, BETAS, cfg["eps"], cfg["weight_decay"], cfg["amsgrad"], cfg["torch_eps"])
    o.step()
    got = (o.bucket.flat, o.exp_avg, o.exp_avg_sq, o.max_exp_avg_sq)
    return {k: worst_ratio(a, b, d) for k, a, b, d in zip(("p", "m", "v", "vmax"), got, new, bound)}


def restart_rmsprop(o, lr, cfg, alpha=0.99):
    st = [x.detach().double().cpu().clone() for x in (o.bucket.flat, o.bucket.grad, o.square_avg)]
    new, bound = S.rmsprop(*st, lr, alpha, cfg["eps"], cfg["weight_decay"])
    o.step()
    return {k: worst_ratio(a, b, d) for k, a, b, d in zip(("p", "v"), (o.bucket.flat, o.square_avg), new, bound)}


def merge_worst(worst, step, ratios):
    for k, (r, i) in ratios.items():
        if r > worst.get(k, (-1.0,))[0]:
            worst[k] = (r, step, i)


def assert_within(worst, label, limit=1.0):
    print(label, {k: "%.3f (step %d, element %d)" % v for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v[0] <= limit}
    assert not bad, "%s: error / bound > %g: %s" % (label, limit, bad)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "optim.npz"))


def golden_configs(golden):
    return [str(c) for c in golden["configs"]]


def test_spec_reproduces_the_reference_optimizers_within_its_bound(golden):
    """Each step of the reference's run, from its own fp32 state of the step before, within the spec's one-step bound; the
    gradient spike must have left AMSGrad's maximum above the running second moment in most elements for the rest of the run
    (otherwise max() is not exercised; an element whose own spike gradient happened to be small may fall back)."""
    nsh, steps = len(golden["shapes"]), int(golden["steps"])
    for name in golden_configs(golden):
        G = lambda k: torch.from_numpy(golden[name + "/" + k]).double()
        kind, worst, t, above = str(golden[name + "/kind"]), {}, (0.0, 1.0, 1.0), []
        lr, eps, wd = (float(golden[name + "/" + k]) for k in ("lr", "eps", "weight_decay"))
        for s in range(steps):
            if kind == "adam":
                t = S.advance(t, tuple(golden[name + "/betas"]))
            for k in range(nsh):
                prev = lambda key, zero=True: (G("%s_%d" % (key, k))[s - 1] if s else
                                               (torch.zeros_like(G("w0_%d" % k)) if zero else G("w0_%d" % k)))
                g = G("g_%d" % k)[s]
                if kind == "adam":
                    ams = bool(golden[name + "/amsgrad"])
                    new, bound = S.adam(prev("p", False), g, prev("exp_avg"), prev("exp_avg_sq"), prev("max_exp_avg_sq"), t, lr,
                                        tuple(float(b) for b in golden[name + "/betas"]), eps, wd, ams, False)
                    keys = ("p", "exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if ams else ())
                    if ams and s > int(golden["spike"]):
                        above.append((G("max_exp_avg_sq_%d" % k)[s] > G("exp_avg_sq_%d" % k)[s]).reshape(-1))
                else:
                    new, bound = S.rmsprop(prev("p", False), g, prev("square_avg"), lr, float(golden[name + "/alpha"]), eps, wd)
                    keys = ("p", "square_avg")
                merge_worst(worst, s, {key: worst_ratio(G("%s_%d" % (key, k))[s], a, d) for key, a, d in zip(keys, new, bound)})
        assert_within(worst, name)
        assert not above or float(torch.cat(above).double().mean()) > 0.75


@pytest.mark.parametrize("wd", [0, 1e-2])
def test_spec_torch_form_against_torch_optim_in_float64(wd):
    """torch.optim.Adam (amsgrad off) and torch.optim.RMSprop in float64, each step from their own state, within the
    spec's bound evaluated at float64's unit roundoff, TWICE: here the spec is no more exact than what it is compared with
    (both evaluate the rule in float64, in different associations, e.g. s / sqrt(1 - beta2^t) against s * (1 / sqrt(..))),
    so each is within one bound of the exact value. torch.optim forms beta^t with pow(), so that is the t passed here (the
    running product differs from it by up to ~1000 t ulp64 in 1 - beta2^t, which is not what this test is about)."""
    gen = torch.Generator().manual_seed(3)
    w0 = torch.randn(4099, generator=gen, dtype=torch.float64) * torch.logspace(-3, 0, 4099, dtype=torch.float64)
    pa, pr = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(w0.clone())
    oa = torch.optim.Adam([pa], lr=1e-3, betas=BETAS, eps=1e-8, weight_decay=wd, foreach=False)
    orr = torch.optim.RMSprop([pr], lr=1e-3, alpha=0.99, eps=1e-8, weight_decay=wd, foreach=False)
    worst_a, worst_r = {}, {}
    z = torch.zeros_like(w0)
    for s in range(6):
        g = scheduled_grad(s, 4099, gen).double()
        pa.grad, pr.grad = g.clone(), g.clone()
        sa, sr = oa.state[pa], orr.state[pr]
        m, v = (sa["exp_avg"].clone(), sa["exp_avg_sq"].clone()) if s else (z, z)
        t = (s + 1.0, BETAS[0] ** (s + 1), BETAS[1] ** (s + 1))
        new, bound = S.adam(pa.detach().clone(), g, m, v, z, t, 1e-3, BETAS, 1e-8, wd, False, True, u=S.U64)
        oa.step()
        merge_worst(worst_a, s, {k: worst_ratio(a, b, d) for k, a, b, d in
                                 zip("pmv", (pa, sa["exp_avg"], sa["exp_avg_sq"]), new, bound)})
        new, bound = S.rmsprop(pr.detach().clone(), g, sr["square_avg"].clone() if s else z, 1e-3, 0.99, 1e-8, wd, u=S.U64)
        orr.step()
        merge_worst(worst_r, s, {k: worst_ratio(a, b, d) for k, a, b, d in zip("pv", (pr, sr["square_avg"]), new, bound)})
    assert_within(worst_a, "torch.optim.Adam float64 wd=%g" % wd, limit=2.0)
    assert_within(worst_r, "torch.optim.RMSprop float64 wd=%g" % wd, limit=2.0)


N_RUN, STEPS_RUN = 200003, 24


def _start(seed=1):
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(N_RUN, generator=gen) * torch.logspace(-4, 0, N_RUN)
    return gen, torch.nn.Parameter(w)


@pytest.mark.parametrize("cfg", ADAM_CONFIGS, ids=config_id)
def test_adam_tensor_path_each_step_within_the_bound(cfg):
    """SharedAdam with fused = False on the CPU, 24 steps in restart form (table: module docstring); the step counter and
    the beta powers equal the spec's running products exactly."""
    gen, p = _start()
    o = SharedAdam([p], lr=1e-3, betas=BETAS, **cfg)
    o.fused = False
    worst, t = {}, (0.0, 1.0, 1.0)
    for s in range(STEPS_RUN):
        o.bucket.grad.copy_(scheduled_grad(s, o.bucket.numel, gen))
        t = S.advance(t, BETAS)
        merge_worst(worst, s, restart_adam(o, t, 1e-3, cfg))
        assert o._scalars.tolist() == list(t)
    if not cfg["amsgrad"]:
        assert float(o.max_exp_avg_sq.abs().max()) == 0.0
    assert_within(worst, "SharedAdam tensor path " + config_id(cfg))


@pytest.mark.parametrize("cfg", RMS_CONFIGS, ids=config_id)
def test_rmsprop_tensor_path_each_step_within_the_bound(cfg):
    """SharedRMSprop with fused = False on the CPU, 24 steps in restart form (table: module docstring)."""
    gen, p = _start()
    o = SharedRMSprop([p], lr=1e-3, **cfg)
    o.fused = False
    worst = {}
    for s in range(STEPS_RUN):
        o.bucket.grad.copy_(scheduled_grad(s, o.bucket.numel, gen))
        merge_worst(worst, s, restart_rmsprop(o, 1e-3, cfg))
    assert_within(worst, "SharedRMSprop tensor path " + config_id(cfg))


def test_subnormal_weights_under_weight_decay():
    """The case the draft bound missed, on its own: weights on fp32's subnormal grid, gradient zero, weight decay 1e-2 and
    eps 1e-8. wd p has one to three significant bits and its square is zero in fp32; the update is (grid error) / eps away
    from float64's. Without optim_spec's underflow terms the error is ~1e5 bounds (checked below: the relative-only part of
    the bound is exceeded), with them it is within the bound."""
    p0 = torch.arange(1, 4097, dtype=torch.float64) * 2.0 ** -149 * 37.0
    for cls, kw in ((SharedRMSprop, dict(eps=1e-8, weight_decay=1e-2)),
                    (SharedAdam, dict(eps=1e-8, weight_decay=1e-2, amsgrad=False, torch_eps=True))):
        p = torch.nn.Parameter(p0.float())
        assert torch.equal(p.detach().double(), p0)
        o = cls([p], lr=1e-3, **kw)
        o.fused = False
        before = o.bucket.flat.double().clone()
        if cls is SharedRMSprop:
            r = restart_rmsprop(o, 1e-3, kw)
        else:
            r = restart_adam(o, S.advance((0.0, 1.0, 1.0), BETAS), 1e-3, kw)
        assert_within({k: (v[0], 0, v[1]) for k, v in r.items()}, cls.__name__ + " subnormal weights")
        if cls is SharedRMSprop:
            (want, _), _ = S.rmsprop(before, torch.zeros_like(before), torch.zeros_like(before), 1e-3, 0.99, 1e-8, 1e-2)
            err = (o.bucket.flat.double() - want).abs()
            assert float((err / (S.U32 * 16 * want.abs())).max()) > 1.0      # (no relative-rounding bound could hold here)


def _golden_run(golden, name, device="cpu", fused=False):
    """The package's optimizer of golden configuration `name` fed the golden gradients: weights after every step."""
    nsh, steps = len(golden["shapes"]), int(golden["steps"])
    params = [torch.nn.Parameter(torch.from_numpy(golden[name + "/w0_%d" % k]).to(device)) for k in range(nsh)]
    lr, eps, wd = (float(golden[name + "/" + k]) for k in ("lr", "eps", "weight_decay"))
    if str(golden[name + "/kind"]) == "adam":
        o = SharedAdam(params, lr=lr, betas=tuple(float(b) for b in golden[name + "/betas"]), eps=eps, weight_decay=wd,
                       amsgrad=bool(golden[name + "/amsgrad"]))
    else:
        o = SharedRMSprop(params, lr=lr, alpha=float(golden[name + "/alpha"]), eps=eps, weight_decay=wd)
    o.fused = fused
    out = []
    for s in range(steps):
        for k, p in enumerate(params):
            p.grad.copy_(torch.from_numpy(golden[name + "/g_%d" % k][s]))
        o.step()
        out.append([p.detach().cpu().clone() for p in params])
    return o, out


def test_tensor_path_follows_the_reference_weights_within_2_ulp(golden):
    """Free-running for the 8 golden steps, every weight within 2 ulp32 of the reference's (measured: at most 3.0e-8
    absolute); the padding of the (1,) and (13,) slots stays zero in the weights and every state tensor, weight decay included."""
    for name in golden_configs(golden):
        o, out = _golden_run(golden, name)
        worst = 0.0
        for s, ps in enumerate(out):
            for k, p in enumerate(ps):
                want = torch.from_numpy(golden[name + "/p_%d" % k][s]).double()
                ulps = ((p.double() - want).abs() / S.ulp32(want)).max()
                worst = max(worst, float(ulps))
        print(name, "worst distance to the reference's weights: %.2f ulp32" % worst)
        assert worst <= 2.0, (name, worst)
        assert_padding_zero(o)


def state_tensors(o):
    return [o.exp_avg, o.exp_avg_sq, o.max_exp_avg_sq] if isinstance(o, SharedAdam) else [o.square_avg]


def padding_mask(bucket):
    mask = torch.ones(bucket.numel, dtype=torch.bool)
    for p, off in zip(bucket.params, bucket.offsets):
        mask[off:off + p.numel()] = False
    return mask


def assert_padding_zero(o):
    mask = padding_mask(o.bucket)
    assert int(mask.sum()) == o.bucket.numel - o.bucket.param_numel
    for x in [o.bucket.flat, o.bucket.grad] + state_tensors(o):
        assert float(x.detach().cpu()[mask].abs().max() if mask.any() else 0.0) == 0.0


SHAPES = [(7, 5), (1,), (13,), (4, 4), (1,), (3, 2, 5), (2,)]


def test_flat_params_layout_alignment_and_views():
    """FlatParams against optim_spec.layout: offsets, total, 16-byte slot starts, parameters and gradients as views of the
    two buffers (a write through either is seen by the other), values carried over, padding zero."""
    torch.manual_seed(0)
    ws = [torch.randn(*s) for s in SHAPES]
    params = [torch.nn.Parameter(w.clone()) for w in ws]
    b = FlatParams(params)
    offsets, total = S.layout(SHAPES)
    assert b.offsets == offsets and b.numel == total == b.flat.numel() == b.grad.numel()
    assert b.param_numel == sum(w.numel() for w in ws) and total > b.param_numel
    for p, w, off in zip(params, ws, offsets):
        assert off % 4 == 0 and p.data_ptr() % 16 == 0 and p.grad.data_ptr() % 16 == 0
        assert p.data_ptr() == b.flat.data_ptr() + 4 * off and p.grad.data_ptr() == b.grad.data_ptr() + 4 * off
        assert torch.equal(p.detach(), w) and p.shape == w.shape
        b.flat[off] = 5.0
        assert float(p.detach().reshape(-1)[0]) == 5.0
        p.grad.reshape(-1)[-1] = 7.0
        assert float(b.grad[off + w.numel() - 1]) == 7.0
    mask = padding_mask(b)
    assert float(b.flat[mask].abs().max()) == 0.0 and float(b.grad[mask].abs().max()) == 0.0


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_padding_stays_zero_and_parameters_stay_views(kind):
    """Six steps with weight decay over slots of 1, 2 and 13 elements: the padding is exactly zero in the weights, the
    gradients and every state tensor afterwards, and every parameter is still a view of `flat`."""
    torch.manual_seed(1)
    params = [torch.nn.Parameter(torch.randn(*s)) for s in SHAPES]
    o = (SharedAdam(params, lr=1e-2, weight_decay=1e-2) if kind == "adam" else SharedRMSprop(params, lr=1e-2, weight_decay=1e-2))
    o.fused = False
    for s in range(6):
        o.bucket.set_grads([torch.randn(*sh) for sh in SHAPES])
        o.step()
    assert_padding_zero(o)
    for p, off in zip(params, o.bucket.offsets):
        assert p.data_ptr() == o.bucket.flat.data_ptr() + 4 * off
        assert float(p.detach().abs().max()) > 0


def test_set_grads_cpu_branch_with_none_entries_and_one_element_slots():
    """set_grads on a CPU bucket: None entries become zero over whatever the bucket held, the 1-element slots and their
    padding come out right, a non-contiguous gradient is flattened in logical order, p.grad is the bucket's view."""
    torch.manual_seed(2)
    params = [torch.nn.Parameter(torch.randn(*s)) for s in SHAPES]
    b = FlatParams(params)
    b.grad.fill_(9.0)                                                  # stale contents, padding included
    grads = [torch.randn(*s) for s in SHAPES]
    grads[0] = torch.randn(5, 7).t()                                   # non-contiguous (7, 5)
    grads[2], grads[4] = None, None                                    # a (13,) slot and a 1-element slot
    b.set_grads(grads)
    want = torch.zeros(b.numel)
    for g, off in zip(grads, b.offsets):
        if g is not None:
            want[off:off + g.numel()] = g.reshape(-1)
    assert torch.equal(b.grad, want)
    for p, g, off in zip(params, grads, b.offsets):
        assert p.grad.data_ptr() == b.grad.data_ptr() + 4 * off and p.grad.shape == p.shape
        assert torch.equal(p.grad, g if g is not None else torch.zeros_like(p))
