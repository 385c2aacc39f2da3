"""The LSTM / GRU cell kernels and the heads kernel at saturated inputs: ladder, float64 references and PER-ELEMENT error bounds.

Plain numpy / torch float64 on the CPU, no GPU import. tests/test_cell_edges_cpu.py tests this module on its own,
tests/test_cell_edges_gpu.py holds the kernels to it.

LADDER     the pre-activation values where the hardware forms of csrc/atr_cell.h change behaviour, each with both signs; C_LADDER
           the same cut at |c| <= 64 for cell states (above that the rounding of f * c alone is an absolute error that makes a
           per-element bound on h meaningless); C_RANGE_ONLY the cell states 1e4 and 3e38, for which only finiteness and sign
           are asked.
draw       every element chosen independently from a ladder; a second half log-uniform in magnitude, random sign.

The two hardware forms (csrc/atr_cell.h, and again as sigm / tanh_fast in csrc/actor_step_hip.hip; __expf(x) is
v_exp_f32(fl(log2e) * x), clang's __clang_hip_math.h):

    sigmoidf_(x) = rcp(1 + exp2(L * -x))              tanhf_(x) = 1 - 2 * rcp(1 + exp2(L * (2 x)))        L = fl(log2 e)

E_SIG, E_TANH: their ABSOLUTE error bounds, derived here from the accuracy of each step. With U = 2^-24 (half an ulp of [1, 2),
one ulp of [1/2, 1)), s = sigmoid(x), t = tanh(x):

  1 the argument. fl(L * y) = y log2(e) (1 + d), |d| <= REL_ARG = |fl(log2 e) / log2 e - 1| + U (the constant's own rounding, one
    multiply; -x and 2 x are exact). exp2 of it is e^y e^(y d): a RELATIVE error |y| REL_ARG of u = e^y. Through s = 1 / (1 + u),
    ds = s (1 - s) du / u, this is s (1 - s) |x| REL_ARG <= K_SIG REL_ARG with K_SIG = max_x s (1 - s) |x| = 0.2239. Through
    t = 1 - 2 / (1 + u), u = e^(2x): dt = (1 - t^2) / 2 * du / u = (1 - t^2) |x| REL_ARG <= K_TANH REL_ARG, K_TANH = 0.4477.
  2 v_exp_f32: 1 ulp (the CDNA ISA guide's figure for V_EXP_F32), a relative error <= 2 U of u: s (1 - s) 2 U <= U / 2 for the
    sigmoid, (1 - t^2) / 2 * 2 U <= U for tanh.
  3 the add 1 + u, rounded to nearest: relative U of the denominator, so relative U of r = 1 / (1 + u) <= 1: U for the sigmoid,
    2 U for tanh (its 2 r).
  4 v_rcp_f32: 1 ulp (the ISA guide's figure for V_RCP_F32). r lies in (0, 1]: an ulp there is at most U (one ulp of [1/2, 1);
    at r = 1 the denominator is exactly 1.0f, whose reciprocal the instruction returns exactly — a value above 1 would also fail
    the range checks the tests make next to every bound). U for the sigmoid, 2 U for tanh.
  5 tanh only: 2 r is exact; 1 - 2 r is exact for 2 r in [1/2, 2] (Sterbenz) and otherwise rounded to nearest with |t| <= 1:
    U / 2.

    E_SIG  = K_SIG  REL_ARG + U / 2 + U + U            = 1.65e-7          (an overflowing exp2 is inf, rcp(inf) = 0: the forms
    E_TANH = K_TANH REL_ARG + U + 2 U + 2 U + U / 2    = 3.61e-7           saturate to 0 / 1 / +-1 exactly; nothing to add)
    (REL_ARG = 7.3e-8: 1.3e-8 of the constant, 6.0e-8 of the multiply.)

The 1-ulp figures are the ISA guide's. A float32 numpy emulation of the two forms (emu_sigmoid / emu_tanh below) over the ladder
and 4M log-uniform points measures 9.3e-8 and 1.8e-7 with exp2 and the reciprocal correctly rounded, and at most 1.24e-7 and 2.49e-7
with each returning the float on the far side of its exact result — the worst a 1-ulp instruction may do
(tests/test_cell_edges_cpu.py). A blunt push of the correctly rounded values by one float, up to 1.5 ulp, measures 1.79e-7 and
3.58e-7: past E_SIG only at x = 16.6, where it turns a reciprocal of 1 - 6e-8 rounded to 1.0 into 1 + 2^-23, three ulps from the
exact result and outside [0, 1].

bound_*    the allowed absolute error per element of every output of a cell forward / backward: E_SIG, E_TANH and U |value| per
           rounded operation (+ ETA = 2^-126 where the result underflows: the other half of float32's rounding model) propagated
           to first order through the kernel's expressions (class Bound: |a| e_b + |b| e_a for a product, e_a + e_b for a sum, the activation's largest slope over [x - e, x + e] times e for an activation of an
           inexact argument), times 2 for what first order leaves out — the second-order terms and the compiler's fma choices.
           Nothing else is added. The float64 value of the same expression comes out of the same pass (class F64), so reference
           and bound cannot drift apart; lstm_bptt_ref / gru_bptt_ref are the same backward expressions over T steps in torch (any
           dtype and device: float64 for the reference, float32 for the rule's floor), and the CPU tests hold all of them to
           nn.LSTMCell / nn.GRUCell autograd.

Every reference is evaluated from the same float32 inputs or stores the kernel reads. Sums the kernel forms in float32 before an
activation (the GRU's ir + hr, the PRE form's (pre + bias) + emb) are formed in float32 in the kernel's order first (f32_sum),
then activated in float64.
"""
import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -126            # the underflow term of float32 rounding: fl(x) = x (1 + d) + e, |d| <= U, |e| <= ETA (flushed or denormal)
LOG2E_F32 = float(np.float32(float.fromhex("0x1.715476p+0")))       # __expf's constant
REL_ARG = abs(LOG2E_F32 / np.log2(np.e) - 1.0) + U


def _sup(fn):
    x = np.linspace(0.0, 8.0, 800001)
    return float(np.max(fn(x)))


K_SIG = _sup(lambda x: x * np.exp(-x) / (1.0 + np.exp(-x)) ** 2)      # max s (1 - s) |x|   (0.2239 at |x| = 1.54)
K_TANH = _sup(lambda x: x * (1.0 - np.tanh(x) ** 2))                   # max (1 - t^2) |x|   (0.4477 at |x| = 0.77)
E_SIG = K_SIG * REL_ARG + 0.5 * U + U + U
E_TANH = K_TANH * REL_ARG + U + 2 * U + 2 * U + 0.5 * U

_POS = [0.0, 2.0 ** -149, 2.0 ** -126, 1e-8, 1e-4, 0.5, 1.0, 4.0, 8.3, 8.4, 16.6, 16.7, 20.0, 44.3, 44.4, 45.0, 88.7, 88.8, 89.0,
        100.0, 1e4, 3e38]
LADDER = np.array([-v for v in reversed(_POS)] + _POS, dtype=np.float32)          # (-0.0 and 0.0 both present)
C_LADDER = LADDER[np.abs(LADDER) <= 64.0]
C_RANGE_ONLY = np.array([-3e38, -1e4, 1e4, 3e38], dtype=np.float32)
assert np.isfinite(LADDER).all() and LADDER.size == 44 and np.signbit(LADDER[21]) and not np.signbit(LADDER[22])


def draw(shape, seed, ladder=LADDER, top=200.0):
    """float32 array: each element independently from `ladder`; a second half (chosen per element) log-uniform in magnitude over
    [1e-8, min(top, max |ladder|)] with random sign — the binades between the ladder's points."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    x = ladder[rng.integers(0, ladder.size, n)].astype(np.float32)
    hi = min(float(top), float(np.abs(ladder).max()))
    mag = np.exp(rng.uniform(np.log(1e-8), np.log(hi), n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return np.where(rng.random(n) < 0.5, mag.astype(np.float32), x).reshape(shape)


def where_on_ladder(x):
    """'8.3' / '-44.4' ... : the ladder point nearest (in log magnitude, same sign) to the scalar x, for the printed tables."""
    x = float(x)
    pts = LADDER.astype(np.float64)
    d = np.abs(np.log(np.abs(pts) + 1e-50) - np.log(abs(x) + 1e-50)) + np.where(np.signbit(pts) == np.signbit(x), 0.0, 1e3)
    return "%.4g (ladder %.4g)" % (x, pts[int(np.argmin(d))])


def f32_sum(*terms):
    """((a + b) + c) ... in float32, as the kernels form a pre-activation from its float32 parts; returned as float32."""
    acc = np.asarray(terms[0], dtype=np.float32)
    with np.errstate(over="ignore"):
        for t in terms[1:]:
            acc = (acc + np.asarray(t, dtype=np.float32)).astype(np.float32)
    return acc


def sigmoid64(x):
    x = np.asarray(x, dtype=np.float64)
    return np.exp(-np.logaddexp(0.0, -x))


def tanh64(x):
    return np.tanh(np.asarray(x, dtype=np.float64))


# ---- float32 emulation of the hardware forms, and of the rewrites the tests must reject ------------------------------------------
def _within_one_ulp(exact, push, exact_stays):
    """`exact` (float64) as a 1-ulp instruction may return it: push = 0 rounds to nearest; +1 / -1 give the float on the upper /
    lower side of the exact value (the farthest result still within one ulp of it). A value that IS a float stays when
    `exact_stays`, else moves one float in push's direction (one ulp off, which "1 ulp" also allows). inf and NaN stay."""
    rn = np.asarray(exact).astype(np.float32)
    if not push:
        return rn
    to = np.float32(np.inf if push > 0 else -np.inf)
    r64 = rn.astype(np.float64)
    move = (r64 < exact) if push > 0 else (r64 > exact)
    if not exact_stays:
        move = move | (r64 == exact)
    return np.where(move & np.isfinite(rn), np.nextafter(rn, to), rn).astype(np.float32)


def _exp2_f32(t, push=0):
    with np.errstate(over="ignore", under="ignore"):
        return _within_one_ulp(np.exp2(np.asarray(t, dtype=np.float32).astype(np.float64)), push, False)


def _rcp_f32(d, push=0):
    with np.errstate(divide="ignore", over="ignore"):
        return _within_one_ulp(1.0 / np.asarray(d, dtype=np.float32).astype(np.float64), push, True)


def _expf_f32(y, push=0):
    """__expf: v_exp_f32(fl(log2 e) * y), the product rounded to float32."""
    with np.errstate(over="ignore", under="ignore"):
        t = (np.float32(LOG2E_F32) * np.asarray(y, dtype=np.float32)).astype(np.float32)
    return _exp2_f32(t, push)


def emu_sigmoid(x, push_exp=0, push_rcp=0, form="hw"):
    """float32 numpy emulation of sigmoidf_ (form 'hw'), or of the rewrite e^x / (1 + e^x) ('ratio')."""
    x = np.asarray(x, dtype=np.float32)
    one = np.float32(1.0)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if form == "hw":
            return _rcp_f32((one + _expf_f32(-x, push_exp)).astype(np.float32), push_rcp)
        if form == "ratio":
            e = _expf_f32(x, push_exp)
            return (e / (one + e).astype(np.float32)).astype(np.float32)
    raise ValueError(form)


def emu_tanh(x, push_exp=0, push_rcp=0, form="hw"):
    """float32 numpy emulation of tanhf_ ('hw'), of the rewrite (e^2x - 1) / (e^2x + 1) ('ratio'), or a tanh of libm accuracy
    ('libm': float64 tanh rounded once)."""
    x = np.asarray(x, dtype=np.float32)
    one, two = np.float32(1.0), np.float32(2.0)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if form == "libm":
            return np.tanh(x.astype(np.float64)).astype(np.float32)
        e = _expf_f32((two * x).astype(np.float32), push_exp)
        if form == "hw":
            r = _rcp_f32((one + e).astype(np.float32), push_rcp)
            return (one - (two * r).astype(np.float32)).astype(np.float32)
        if form == "ratio":
            return ((e - one).astype(np.float32) / (e + one).astype(np.float32)).astype(np.float32)
    raise ValueError(form)


# ---- three arithmetics for ONE set of cell expressions ---------------------------------------------------------------------------
class F64(object):
    """The expressions in float64."""
    def exact(self, x):
        return np.asarray(x, dtype=np.float64)

    def value(self, a):
        return a

    mul = staticmethod(lambda a, b: a * b)
    add = staticmethod(lambda a, b: a + b)
    sub = staticmethod(lambda a, b: a - b)
    mask = staticmethod(lambda k, a: k * a)
    sig = staticmethod(sigmoid64)
    tanh = staticmethod(tanh64)


class Emu32(object):
    """The expressions in float32 numpy, one rounding per operation, with the given emulated activations."""
    def __init__(self, sig=emu_sigmoid, tanh=emu_tanh):
        self.sig, self.tanh = sig, tanh

    def exact(self, x):
        return np.asarray(x, dtype=np.float32)

    def value(self, a):
        return a

    def mul(self, a, b):
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            return (a * b).astype(np.float32)

    def add(self, a, b):
        with np.errstate(over="ignore", invalid="ignore"):
            return (a + b).astype(np.float32)

    def sub(self, a, b):
        with np.errstate(over="ignore", invalid="ignore"):
            return (a - b).astype(np.float32)

    mask = mul


class _V(object):
    __slots__ = ("v", "e")

    def __init__(self, v, e):
        self.v, self.e = v, e


class Bound(object):
    """The expressions in float64 with an absolute error bound carried along, to first order (see the module docstring)."""
    def exact(self, x):
        x = np.asarray(x, dtype=np.float64)
        return _V(x, np.zeros_like(x))

    def value(self, a):
        return a.v

    def mul(self, a, b):
        v = a.v * b.v
        return _V(v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + U * np.abs(v) + ETA)

    def add(self, a, b):
        v = a.v + b.v
        return _V(v, a.e + b.e + U * np.abs(v) + ETA)

    def sub(self, a, b):
        v = a.v - b.v
        return _V(v, a.e + b.e + U * np.abs(v) + ETA)

    def mask(self, k, a):                 # k is 0 or 1: exact
        return _V(k.v * a.v, k.v * a.e)

    @staticmethod
    def _nearest_to_zero(a):
        return np.where(np.abs(a.v) <= a.e, 0.0, np.sign(a.v) * (np.abs(a.v) - a.e))

    def sig(self, a):
        s = sigmoid64(self._nearest_to_zero(a))
        return _V(sigmoid64(a.v), E_SIG + np.minimum(s * (1.0 - s) * a.e, 1.0))

    def tanh(self, a):
        t = tanh64(self._nearest_to_zero(a))
        return _V(tanh64(a.v), E_TANH + np.minimum((1.0 - t * t) * a.e, 2.0))


def lstm_fwd_expr(ops, pi, pf, pg, po, cp, k):
    """cell4 of csrc/atr_cell.h: gate order (i, f, g, o), c' = f (k c) + i g, h' = o tanh(c'); k = 0 where the previous step ended
    the episode (done), else 1."""
    x = ops.exact
    i, f, g, o = ops.sig(x(pi)), ops.sig(x(pf)), ops.tanh(x(pg)), ops.sig(x(po))
    c = ops.add(ops.mul(f, ops.mask(x(k), x(cp))), ops.mul(i, g))
    h = ops.mul(o, ops.tanh(c))
    return dict(i=i, f=f, g=g, o=o, c=c, h=h)


def lstm_bwd_expr(ops, gates, c, cp, dh, ki, activate=False):
    """k_lstm_cell_bwd (csrc/lstm_hip.hip) for a last step (nothing arrives from t + 1), the expressions the one-launch BPTT shares:
    gates = (i, f, g, o) as stored, or with activate=True their float32 pre-activations (the PRE forms re-activate in registers)."""
    x = ops.exact
    if activate:
        i, f, g, o = ops.sig(x(gates[0])), ops.sig(x(gates[1])), ops.tanh(x(gates[2])), ops.sig(x(gates[3]))
    else:
        i, f, g, o = (x(t) for t in gates)
    one, dh = x(1.0), x(dh)
    tc = ops.tanh(x(c))
    dc = ops.mul(ops.mul(dh, o), ops.sub(one, ops.mul(tc, tc)))
    d_o = ops.mul(ops.mul(ops.mul(dh, tc), o), ops.sub(one, o))
    d_i = ops.mul(ops.mul(ops.mul(dc, g), i), ops.sub(one, i))
    d_g = ops.mul(ops.mul(dc, i), ops.sub(one, ops.mul(g, g)))
    d_f = ops.mul(ops.mul(ops.mul(dc, ops.mask(x(ki), x(cp))), f), ops.sub(one, f))
    return dict(di=d_i, df=d_f, dg=d_g, do=d_o, dc0=ops.mul(dc, f))


def gru_fwd_expr(ops, xr, xz, pn, q, khp):
    """gru_cell4 / k_gru_cell_fwd: xr = fl(ir + hr), xz = fl(iz + hz) (float32 sums, f32_sum), pn = i_n, q = k hg_n + b_hn (float32,
    one fma), khp = k h_prev. n = tanh(pn + r q), h' = (1 - z) n + z (k h_prev)."""
    x = ops.exact
    r, z = ops.sig(x(xr)), ops.sig(x(xz))
    n = ops.tanh(ops.add(x(pn), ops.mul(r, x(q))))
    h = ops.add(ops.mul(ops.sub(x(1.0), z), n), ops.mul(z, x(khp)))
    return dict(r=r, z=z, n=n, h=h)


def gru_bwd_expr(ops, r, z, n, q, khp, dh):
    """gru_grad of csrc/gru_hip.hip from the stored (r, z, n, q), khp = k_{t-1} h_{t-1}, dh = the whole gradient of this step's h."""
    x = ops.exact
    r, z, n, q, khp, dh, one = x(r), x(z), x(n), x(q), x(khp), x(dh), x(1.0)
    dn = ops.mul(ops.mul(dh, ops.sub(one, z)), ops.sub(one, ops.mul(n, n)))
    dz = ops.mul(ops.mul(ops.mul(dh, ops.sub(khp, n)), z), ops.sub(one, z))
    dr = ops.mul(ops.mul(ops.mul(dn, q), r), ops.sub(one, r))
    return dict(dr=dr, dz=dz, dn=dn, dq=ops.mul(dn, r), direct=ops.mul(dh, z))


def _ref_and_bound(expr, *args, **kw):
    """{name: (float64 value, allowed absolute error)} of every output of `expr`: one pass of Bound, times 2."""
    out = expr(Bound(), *args, **kw)
    return {k: (v.v, 2.0 * v.e) for k, v in out.items()}


def bound_lstm_fwd(pi, pf, pg, po, cp, k):
    return _ref_and_bound(lstm_fwd_expr, pi, pf, pg, po, cp, k)


def bound_lstm_bwd(gates, c, cp, dh, ki, activate=False):
    return _ref_and_bound(lstm_bwd_expr, gates, c, cp, dh, ki, activate=activate)


def bound_gru_fwd(xr, xz, pn, q, khp):
    return _ref_and_bound(gru_fwd_expr, xr, xz, pn, q, khp)


def bound_gru_bwd(r, z, n, q, khp, dh):
    return _ref_and_bound(gru_bwd_expr, r, z, n, q, khp, dh)


def worst(got, ref, allowed):
    """(largest |got - ref| / allowed, flat index of it, largest |got - ref|); a non-finite `got` counts as infinitely far."""
    got, ref, allowed = (np.asarray(t, dtype=np.float64) for t in (got, ref, allowed))
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
        ratio = np.where(err == 0.0, 0.0, err / allowed)
    i = int(np.argmax(ratio))
    return float(ratio.reshape(-1)[i]), i, float(err.reshape(-1)[i])


# ---- the backward over T steps, in torch (float64: the reference; float32: the rule's floor) --------------------------------------
def split4(x):
    R = x.shape[-1] // 4
    return x[..., :R], x[..., R:2 * R], x[..., 2 * R:3 * R], x[..., 3 * R:]


def lstm_bptt_ref(keep, gates, c_all, h_all, dh, whh, dtype, device, pre=None, act=None, n_act=4):
    """fused._lstm_bptt's results from its stores: keep [T, N], gates [P, T, N, 4R] (activated, or with pre=True float32
    pre-activations activated here in `dtype`), c_all / h_all [P, T + 1, N, R], dh [P, T, N, R], whh [P, 4R, R] (nn layout).
    -> dict(dG [P, T, N, 4R], dh0, dc0 [P, N, R], dW_hh [P, R, 4R] = sum_t (k h_{t-1})^T dG_t, and with act [T, N] (int64) the
    by-action sums S [P, n_act, 4R] of dG)."""
    import torch
    to = lambda t: torch.as_tensor(t).to(device=device, dtype=dtype)
    keep, gates, c_all, h_all, dh, whh = (to(t) for t in (keep, gates, c_all, h_all, dh, whh))
    P, T, N, R4 = gates.shape
    gi, gf, gg, go = split4(gates)
    if pre:
        gi, gf, gg, go = torch.sigmoid(gi), torch.sigmoid(gf), torch.tanh(gg), torch.sigmoid(go)
    kprev = torch.cat([torch.ones_like(keep[:1]), keep[:-1]], 0)
    dG = torch.zeros_like(gates)
    dhn = dcc = None
    for t in range(T - 1, -1, -1):
        d, dcn = dh[:, t], 0.0
        if t < T - 1:
            ko = keep[t].view(1, N, 1)
            d, dcn = d + ko * dhn, ko * dcc
        tc = torch.tanh(c_all[:, t + 1])
        i, f, g, o = gi[:, t], gf[:, t], gg[:, t], go[:, t]
        dc = dcn + d * o * (1.0 - tc * tc)
        dG[:, t] = torch.cat([dc * g * i * (1.0 - i), dc * (kprev[t].view(1, N, 1) * c_all[:, t]) * f * (1.0 - f),
                              dc * i * (1.0 - g * g), d * tc * o * (1.0 - o)], -1)
        dcc = dc * f
        dhn = torch.bmm(dG[:, t], whh)
    hm = (h_all[:, :T] * kprev.view(1, T, N, 1)).reshape(P, T * N, -1)
    out = dict(dG=dG, dh0=dhn, dc0=dcc, dW_hh=torch.bmm(hm.transpose(1, 2), dG.reshape(P, T * N, R4)))
    if act is not None:
        onehot = torch.nn.functional.one_hot(torch.as_tensor(act).to(device).reshape(T * N), n_act).to(dtype)
        out["S"] = torch.matmul(onehot.t(), dG.reshape(P, T * N, R4))
    return out


def gru_bptt_ref(keep, acts, h_all, dh, whh, dtype, device):
    """fused._gru_bptt's results from its stores: acts [P, T, N, 4R] = (r, z, n, q), h_all [P, T + 1, N, R], whh [P, 3R, R] (nn
    layout). -> dict(dG [P, T, N, 4R] = (dr, dz, dn, dq), dh0 [P, N, R], dW_hh [P, R, 3R], db_hh [P, 3R])."""
    import torch
    to = lambda t: torch.as_tensor(t).to(device=device, dtype=dtype)
    keep, acts, h_all, dh, whh = (to(t) for t in (keep, acts, h_all, dh, whh))
    P, T, N, R4 = acts.shape
    R = R4 // 4
    r, z, n, q = split4(acts)
    kprev = torch.cat([torch.ones_like(keep[:1]), keep[:-1]], 0)
    hid = lambda x: torch.cat([x[..., :2 * R], x[..., 3 * R:]], -1)
    dG = torch.zeros_like(acts)
    dhn = None
    for t in range(T - 1, -1, -1):
        d = dh[:, t] if t == T - 1 else dh[:, t] + keep[t].view(1, N, 1) * dhn
        khp = kprev[t].view(1, N, 1) * h_all[:, t]
        dn = d * (1.0 - z[:, t]) * (1.0 - n[:, t] * n[:, t])
        dz = d * (khp - n[:, t]) * z[:, t] * (1.0 - z[:, t])
        dG[:, t] = torch.cat([dn * q[:, t] * r[:, t] * (1.0 - r[:, t]), dz, dn, dn * r[:, t]], -1)
        dhn = d * z[:, t] + torch.bmm(hid(dG[:, t]), whh)
    hm = (h_all[:, :T] * kprev.view(1, T, N, 1)).reshape(P, T * N, R)
    flat = dG.reshape(P, T * N, R4)
    return dict(dG=dG, dh0=dhn, dW_hh=hid(torch.bmm(hm.transpose(1, 2), flat)), db_hh=hid(flat.sum(1)))


# ---- the heads at a peaked policy --------------------------------------------------------------------------------------------------
# (R, rows, A, actor weight factor, ret / gae factor)
HEADS_CASES = ((128, 8195, 4, 40.0, 100.0), (128, 8195, 8, 40.0, 100.0), (64, 777, 4, 40.0, 100.0), (256, 777, 8, 80.0, 1000.0))


HEADS_SEED = 2        # (chosen so that every case meets the conditions tests/test_cell_edges_cpu.py asks of it)


def rows_split(rows):
    for t in range(2, 64):
        if rows % t == 0:
            return t, rows // t
    return rows, 1


def heads_problem(R, rows, A, wfac, rfac, aux, seed=HEADS_SEED):
    """The layout of tests/test_hidden_sizes_gpu.py::test_heads_kernels_match_float64 (two players, a [T, 2, N] action store, ret /
    gae / rew [T, N, 2, 1]) for a TRAINED policy, on the CPU: actor weight x wfac, actor bias N(0, 5), ret / gae x rfac; actions
    drawn from the policy itself except one row in sixteen drawn uniformly (the rows whose log p(a) is far below -80)."""
    import torch
    g = torch.Generator().manual_seed(seed + R + rows + A + (1000 if aux else 0))
    T, N = rows_split(rows)
    lin = lambda o: (torch.empty(o, R).uniform_(-R ** -0.5, R ** -0.5, generator=g), torch.empty(o).uniform_(-R ** -0.5, R ** -0.5, generator=g))
    prm, hs = [], []
    store = torch.empty(T, 2, N, dtype=torch.int64)
    for p in range(2):
        wa, _ = lin(A)
        wa, ba = wa * wfac, torch.randn(A, generator=g) * 5.0
        pl = [wa, ba, *lin(1)] + (list(lin(1)) if (aux and p == 1) else [])
        h = torch.randn(rows, R, generator=g)
        prob = torch.softmax(h.double() @ wa.double().t() + ba.double(), 1)
        a = torch.multinomial(prob, 1, generator=g).reshape(rows)
        uni = torch.randint(0, A, (rows,), generator=g)
        a = torch.where(torch.arange(rows) % 16 == 5, uni, a)
        store[:, p] = a.view(T, N)
        prm.append(pl)
        hs.append(h)
    ret, gae = (torch.randn(T, N, 2, 1, generator=g) * rfac for _ in range(2))
    rew = torch.randn(T, N, 2, 1, generator=g)
    return dict(T=T, N=N, hs=hs, prm=prm, store=store, ret=ret, gae=gae, rew=rew, scale=[1.0 / N, 1.0 / N], scale_aux=1.0 / N,
                w_ent=[0.01, 0.05])
