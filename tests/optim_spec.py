"""The optimizers' update rules in float64, written from the rules themselves (no import of the package), each with a
per-element first-order bound on what ONE step in fp32 may differ from it.

Rules (one step; p weights, g gradient, m / v first / second moment, vmax AMSGrad's running maximum; all elementwise):

    gw   = g + weight_decay p                                   (weight_decay != 0 only)
    Adam:     m' = beta1 m + (1 - beta1) gw       v' = beta2 v + (1 - beta2) gw^2       vmax' = max(vmax, v')
              s  = sqrt(vmax' if amsgrad else v')
              SharedAdam form (torch_eps False):  den = s + eps,                         step = lr sqrt(1 - beta2^t) / (1 - beta1^t)
              torch.optim form (torch_eps True):  den = s / sqrt(1 - beta2^t) + eps,     step = lr / (1 - beta1^t)
              p' = p - m' / den * step
    RMSprop:  v' = alpha v + (1 - alpha) gw^2     p' = p - lr gw / (sqrt(v') + eps)      (momentum 0, not centered)

t, beta1^t and beta2^t are Python floats kept as running products (advance()), the way SharedAdam keeps them; the
coefficients are the Python floats the caller passes (1 - beta is formed in float64, as the optimizers form it).

The bound. U = 2^-24 is fp32's unit roundoff: every fp32 operation returns its exact result times (1 + d), |d| <= U, and so
does the conversion of a float64 coefficient to fp32. An fp32 implementation that starts from the same fp32 p, g, m, v, vmax
and evaluates the expressions above in any association (fused multiply-adds included: they round less) differs from the
float64 value, to first order in U, by at most the sums below. Terms of order U^2 are dropped; no factor is added.

    d(gw)   = 3 U (|g| + |wd p|)                     coefficient wd, product wd p, the sum                    [3 roundings]
    d(m')   = 3 U (|beta1 m| + |(1-beta1) gw|) + (1-beta1) d(gw)
                                                     per term: coefficient + product; then the sum            [3 on each term]
    d(v')   = 4 U (beta2 v + (1-beta2) gw^2) + 2 (1-beta2) |gw| d(gw)
                                                     coefficient + up to two products per term; the sum       [4 on each term]
    d(vmax')= d(v')                                  max() is exact and 1-Lipschitz
    d(s)    = U s + d(second) / (2 s)                the root's rounding + its derivative (capped: see Underflow)
    d(den)  = k d(s) + U eps + U den  (+ 2 U k s when k = 1 / sqrt(1 - beta2^t) != 1: coefficient + product)
                                                     eps's conversion, the sum                                [2 (+2) roundings]
    Adam:     d(upd) = step (d(m') / den + |m'| d(den) / den^2) + 3 U |upd|
                                                     the divide, step's conversion, the product               [3 roundings]
    RMSprop:  d(upd) = lr (d(gw) / den + |gw| d(den) / den^2) + 3 U |upd|
                                                     lr's conversion, the product, the divide                 [3 roundings]
    d(p')   = ulp32(|p'| + d(upd)) / 2 + d(upd)      the last subtraction rounds to nearest; its exact argument lies within
                                                     d(upd) of p', so the spacing is taken at the far end     [1 rounding]

Where the derivative of the update w.r.t. gw is taken through BOTH its numerator and its denominator, the two paths are
bounded separately and added (an upper bound; they partly cancel when v' is dominated by this step's gw^2).

Underflow. The (1 + d) model holds for normal results only. A product or quotient that lands below 2^-126 is rounded to
the subnormal grid instead: an ABSOLUTE error of up to ETA = 2^-150, however small the result (sums and differences of fp32
numbers are exact there, and a root never lands there). With eps = 1e-8 that matters: a weight that weight decay has driven
to ~1e-41 has gw = wd p on that grid with two or three significant bits, its gw^2 is zero in fp32, and the update divides
the grid error by eps. So every product / quotient above also contributes ETA, propagated like the other terms:

    d(gw) += ETA       d(m') += 2 ETA       d(v') += 3 ETA max(1, |gw|)       d(upd) += ETA (1 + 1 / den)

(the last for step <= 1 and lr <= 1, either association of coefficient x numerator / den), and the root's first-order
slope d / (2 s), which has no meaning once d(second) is no longer small against second, is capped by the exact
|sqrt(a + d) - sqrt(a)| <= sqrt(d).

u: pass U64 to get the same bound for a float64 implementation (torch.optim run in float64; no underflow terms).
"""
import torch

U32 = 2.0 ** -24
U64 = 2.0 ** -53
ETA32 = 2.0 ** -150
ALIGN = 4          # floats: FlatParams pads every slot to 16 bytes


def layout(shapes):
    """FlatParams' rule restated: slot i starts at offsets[i], holds prod(shapes[i]) floats and is padded with zeros to a
    multiple of ALIGN floats. Returns (offsets, total)."""
    offsets, off = [], 0
    for s in shapes:
        n = 1
        for d in tuple(s):
            n *= int(d)
        offsets.append(off)
        off += (n + ALIGN - 1) // ALIGN * ALIGN
    return offsets, off


def advance(t, betas):
    """(step, beta1^step, beta2^step) after one more step; start from (0.0, 1.0, 1.0)."""
    return (t[0] + 1.0, t[1] * betas[0], t[2] * betas[1])


def adam_scalars(t, lr, torch_eps):
    """(step size, factor on the root) in float64 for the step whose counters are t."""
    import math
    if torch_eps:
        return lr / (1.0 - t[1]), 1.0 / math.sqrt(1.0 - t[2])
    return lr * math.sqrt(1.0 - t[2]) / (1.0 - t[1]), 1.0


def ulp32(x):
    """The spacing of fp32 numbers at |x| (float64 tensor in, float64 out; the subnormal spacing below 2^-126)."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))          # |x| = f 2^e, f in [0.5, 1)
    return torch.ldexp(torch.ones_like(x), e - 24)


def _eta(u):
    return ETA32 if u == U32 else 0.0


def _decayed(p, g, weight_decay, u):
    if weight_decay == 0:
        return g, torch.zeros_like(g)
    wp = weight_decay * p
    return g + wp, 3.0 * u * (g.abs() + wp.abs()) + _eta(u)


def _second_moment(v, gw, d_gw, beta, u):
    omb = 1.0 - beta
    new = beta * v + omb * gw * gw
    return new, 4.0 * u * new + 2.0 * omb * gw.abs() * d_gw + 3.0 * _eta(u) * gw.abs().clamp_min(1.0)


def _root(second, d_second, u):
    s = second.sqrt()
    slope = torch.where(second > 0, d_second / (2.0 * s).clamp_min(1e-300), d_second.sqrt())
    return s, u * s + torch.minimum(slope, d_second.sqrt())


def _half_ulp(p, d_upd, u):
    # the subtraction rounds p - (the fp32 update), which lies within d_upd of p': half the spacing at the far end of that
    # interval (it differs from ulp32(p') only where the interval reaches into the next binade)
    return 0.5 * ulp32(p.abs() + d_upd) if u == U32 else u * (p.abs() + d_upd)


def adam(p, g, m, v, vmax, t, lr, betas, eps, weight_decay, amsgrad, torch_eps, u=U32):
    """One Adam step on float64 tensors; t = advance(previous t, betas). Returns ((p', m', v', vmax'), (d_p, d_m, d_v,
    d_vmax)); vmax is returned untouched (bound 0) without amsgrad. Rounding counts: module docstring."""
    beta1, beta2 = betas
    omb1 = 1.0 - beta1
    step, k = adam_scalars(t, lr, torch_eps)
    gw, d_gw = _decayed(p, g, weight_decay, u)
    t1, t2 = beta1 * m, omb1 * gw
    m2 = t1 + t2
    d_m = 3.0 * u * (t1.abs() + t2.abs()) + omb1 * d_gw + 2.0 * _eta(u)
    v2, d_v = _second_moment(v, gw, d_gw, beta2, u)
    if amsgrad:
        vmax2, d_vmax = torch.maximum(vmax, v2), d_v
        second = vmax2
    else:
        vmax2, d_vmax = vmax, torch.zeros_like(vmax)
        second = v2
    s, d_s = _root(second, d_v, u)
    den = s * k + eps
    d_den = k * d_s + u * eps + u * den + (2.0 * u * k * s if k != 1.0 else 0.0)
    assert step <= 1.0
    upd = m2 / den * step
    d_upd = step * (d_m / den + m2.abs() * d_den / (den * den)) + 3.0 * u * upd.abs() + _eta(u) * (1.0 + 1.0 / den)
    p2 = p - upd
    return (p2, m2, v2, vmax2), (_half_ulp(p2, d_upd, u) + d_upd, d_m, d_v, d_vmax)


def rmsprop(p, g, v, lr, alpha, eps, weight_decay, u=U32):
    """One RMSprop step (momentum 0, not centered) on float64 tensors. Returns ((p', v'), (d_p, d_v))."""
    gw, d_gw = _decayed(p, g, weight_decay, u)
    v2, d_v = _second_moment(v, gw, d_gw, alpha, u)
    s, d_s = _root(v2, d_v, u)
    den = s + eps
    d_den = d_s + u * eps + u * den
    assert lr <= 1.0
    upd = lr * gw / den
    d_upd = lr * (d_gw / den + gw.abs() * d_den / (den * den)) + 3.0 * u * upd.abs() + _eta(u) * (1.0 + 1.0 / den)
    p2 = p - upd
    return (p2, v2), (_half_ulp(p2, d_upd, u) + d_upd, d_v)
