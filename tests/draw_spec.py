"""Host model of the rollout's action draw, as include/atr_policy.h specifies it (plain numpy, float64, no project import).

One draw per row: a Philox4x32-10 block with

    counter words  (row, counter & 0xffffffff, counter >> 32, 0x5A3D0000 ^ ordinal)
    key words      (seed & 0xffffffff, seed >> 32)

whose first output word x0 gives the uniform u = ((x0 >> 8) + 0.5) / 2**24 (a 2**-24 grid strictly inside (0, 1)); the
action is the first a with u < CDF[a] of softmax(logits), A - 1 if there is none. The Philox below is written from the
Random123 description (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11: two 32x32 -> 64 multiplies per
round by 0xD2511F53 / 0xCD9E8D57, the key bumped by the Weyl constants 0x9E3779B9 / 0xBB67AE85 between rounds).

Because u is an integer function of the key, the draw is predicted EXACTLY, row by row — except where u lies so close to
a CDF boundary that the kernel's float32 softmax may land on the other side. `margin` marks those rows; its width `delta`
(absolute, the CDF running from 0 to 1) is derived here, not tuned:

(a) The kernel's own arithmetic on given float32 logits l_a (csrc/atr_sample.h). With d_a = l_a - max l (<= 0) and
    D = max |d_a|, it forms p_a = __expf(d_a) = exp2(d_a * log2(e)) on the hardware exponential (V_EXP_F32: 1 ulp = 2**-23
    relative). The subtraction rounds d_a by 2**-24 relative, the float32 constant log2(e) and the product add 2 * 2**-24
    relative on the argument: together at most 1.5 * 2**-23 * |d_a| relative on p_a. So p_a carries a relative error
    e_a <= 2**-23 * (1 + 1.5 |d_a|). The largest term is exactly 1 (d = 0), so the true sum S >= 1 and the ABSOLUTE error of
    a cumulative share sum_{b<=a} p_b / S is at most sum_b p_b e_b / S <= 2**-23 * (1 + 1.5 * sum_b p_b |d_b| / S), where
    sum_b p_b |d_b| / S <= min(D, (A - 1) / e) (a weighted mean of |d_b| <= D; and x exp(-x) <= 1 / e for each of the A - 1
    terms below the maximum). Results below 2**-126 flush to zero: an absolute 2**-126, nothing at this scale. The error
    enters through the partial sum and through the total: twice. Both float32 sums (positive terms, at most A of them)
    add (A - 1) * 2**-24 relative each. On the other side of the comparison u * S is formed in float32: (x0 >> 8) + 0.5
    needs 25 bits from 2**23 up (2**-24 relative), the product by the sum rounds once more.
        delta_a = 2 * 2**-23 * (1 + 1.5 * min(D, (A - 1) / e)) + 2 * (A - 1) * 2**-24 + 2 * 2**-24
(b) Where the logits are themselves computed on the device from a float32 hidden row h and the head (w, b), an R-term float32
    dot product in ANY summation order (fused or not) is within R * 2**-24 * sum_j |h_j w_aj| of the exact one, and adding the
    bias rounds once more: eps_a <= (R + 1) * 2**-24 * sum_j |h_j w_aj| + 2**-24 * |b_a|. Logits moved by at most eps move every
    p_a by a factor within exp(+-eps), a cumulative share by at most exp(2 eps) - 1:
        delta_b = 2 * max_a eps_a      (first order; eps is ~1e-5 at most in any case used)
    Where a test makes the logits exact (small-integer rows, weights and biases on a 2**-8 grid: every partial sum is exactly
    representable, whatever the order) delta_b = 0.

delta = SAFETY * (delta_a + delta_b) with SAFETY = 4: the bounds above are first-order and V_EXP_F32's 1 ulp is the
documented figure, not one measured here. The uniform sits on a 2**-24 grid, so the share of rows inside the margin is
about (A - 1) * 2 * delta; the tests hold it to at most CAP = 1e-3 for every case they run.
"""
import numpy as np

SAFETY = 4.0
CAP = 1e-3
ORDINAL_TAG = 0x5A3D0000
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _u64(x):
    if isinstance(x, (int, np.integer)):
        return np.asarray(int(x) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    x = np.asarray(x)
    return x.astype(np.uint64) if x.dtype != np.uint64 else x


def philox4x32_10(counter, key):
    """counter: four uint32 words, key: two; each a scalar or an array (broadcast against each other). Returns the four
    output words as uint32 arrays."""
    c = [_u64(w) & _LO for w in counter]
    k = [_u64(w) & _LO for w in key]
    for r in range(10):
        if r:
            k = [(k[0] + _W0) & _LO, (k[1] + _W1) & _LO]
        p0, p1 = _M0 * c[0], _M1 * c[2]                     # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & _LO, (p0 >> _S32) ^ c[3] ^ k[1], p0 & _LO]
    return [w.astype(np.uint32) for w in np.broadcast_arrays(*c)]


def uniform_bits(seed, row, counter, ordinal):
    """The 24 bits x0 >> 8 of the draw keyed (seed; row, counter, ordinal); ordinal wraps as a uint32."""
    seed, counter = _u64(seed), _u64(counter)
    ordw = (_u64(ordinal) & _LO) ^ np.uint64(ORDINAL_TAG)
    x = philox4x32_10([_u64(row), counter & _LO, counter >> _S32, ordw], [seed & _LO, seed >> _S32])
    return x[0] >> np.uint32(8)


def uniform(seed, row, counter, ordinal):
    return (uniform_bits(seed, row, counter, ordinal).astype(np.float64) + 0.5) / 2.0 ** 24


def cdf(logits64):
    """Inner boundaries CDF[0 .. A-2] of the float64 softmax, [n, A-1]."""
    l = np.asarray(logits64, np.float64)
    p = np.exp(l - l.max(1, keepdims=True))
    return (np.cumsum(p, 1) / p.sum(1, keepdims=True))[:, :-1]


def draw(logits64, u):
    """First a with u < CDF[a], A - 1 if none."""
    return (np.asarray(u)[:, None] >= cdf(logits64)).sum(1).astype(np.int64)


def margin(logits64, u, delta):
    """Rows whose u lies within delta of an inner CDF boundary."""
    return (np.abs(np.asarray(u)[:, None] - cdf(logits64)) <= np.asarray(delta).reshape(-1, 1)).any(1)


def delta_exp(logits64):
    """Term (a) per row, safety factor not applied."""
    l = np.asarray(logits64, np.float64)
    A = l.shape[1]
    D = (l.max(1, keepdims=True) - l).max(1)
    return 2 * 2.0 ** -23 * (1 + 1.5 * np.minimum(D, (A - 1) / np.e)) + 2 * (A - 1) * 2.0 ** -24 + 2 * 2.0 ** -24


def delta_dot(h, w, b):
    """Term (b) per row for logits the device forms from float32 rows h [n, R] and the head w [A, R], b [A]."""
    h, w, b = np.asarray(h, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    R = h.shape[1]
    eps = (R + 1) * 2.0 ** -24 * (np.abs(h) @ np.abs(w).T) + 2.0 ** -24 * np.abs(b)[None, :]
    return 2 * eps.max(1)


def delta_for(logits64, h=None, w=None, b=None):
    d = delta_exp(logits64)
    if h is not None:
        d = d + delta_dot(h, w, b)
    return SAFETY * d


def head_logits(h, w, b):
    return np.asarray(h, np.float64) @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)[None, :]


def check(actions, logits64, u, delta):
    """The rule of every device case. Outside the margin the action must be the model's; inside it, an action a is accepted
    when u lies within delta of a's own interval [CDF[a-1], CDF[a]) (the model's action or the one across the boundary u
    is near). Returns (n, excluded rows, mismatching rows, out-of-range rows)."""
    actions = np.asarray(actions).astype(np.int64).reshape(-1)
    l = np.asarray(logits64, np.float64)
    n, A = l.shape
    u = np.asarray(u, np.float64).reshape(n)
    delta = np.broadcast_to(np.asarray(delta, np.float64), (n,))
    bad_range = (actions < 0) | (actions >= A)
    a = np.clip(actions, 0, A - 1)
    inner = cdf(l)
    lo = np.concatenate([np.full((n, 1), -np.inf), inner], 1)[np.arange(n), a]
    hi = np.concatenate([inner, np.full((n, 1), np.inf)], 1)[np.arange(n), a]
    model = draw(l, u)
    excl = margin(l, u, delta)
    near = (u >= lo - delta) & (u <= hi + delta)
    wrong = np.where(excl, ~near, a != model) | bad_range
    return n, int(excl.sum()), int(wrong.sum()), int(bad_range.sum())


# ---- the logit families of the device tests (shared with the CPU check of the exclusion cap) ----------------------

EXACT_FAMILIES = ("n0.1", "n1", "n8", "equal", "plus60", "neg", "neg_shifted", "spread200", "first_tiny", "last_tiny")
EXACT_A = (2, 3, 4, 5, 8)
EXACT_R = (4, 8, 60, 64, 124, 128, 132, 252, 256)
EXACT_N = 4099
TAIL_N = (1, 63, 64, 65, 300001)
GRID = 256.0                                                 # weights and biases on a 2**-8 grid


def exact_grid_cases():
    """Every (family, A, R, n) of the exact-logit cases."""
    for fam in EXACT_FAMILIES:
        for A in EXACT_A:
            for R in EXACT_R:
                yield fam, A, R, EXACT_N
        for n in TAIL_N:
            yield fam, 4, 128, n


def _fam_id(family):
    return EXACT_FAMILIES.index("neg" if family == "neg_shifted" else family)


def exact_key(family, A, R, n):
    """(seed, counter, ordinal) an exact-logit case draws under ("neg" and "neg_shifted" share theirs)."""
    return 1000 + _fam_id(family), 100000 * A + 100 * R + (n % 97), 0


def plus60_action(A):
    return (A - 1) // 2                                     # never the last one: the fall-through of the CDF walk is A - 1


def exact_case(family, A, R, n, seed=0):
    """(h [n, R] float32, w [A, R] float32, b [A] float32, logits [n, A] float64) with every product and every partial sum
    exact in float32 in any order: each row of h holds four small integers (+-1 .. +-3) at four distinct columns spread over
    the row (all of them when R = 4), w and b are multiples of 2**-8 of modest size. Every row is different up to chance.
    "neg" (all logits in [-120, -100]) and "neg_shifted" are the same rows and heads, exactly 110 apart."""
    rs = np.random.RandomState([int(seed), A, R, n % 65536, _fam_id(family)])
    q4 = R // 4
    offs = np.stack([np.zeros(n, np.int64)] + [q4 * k + rs.randint(0, q4, n) for k in (1, 2, 3)], 1)
    cols = (rs.randint(0, R, (n, 1)) + offs) % R
    vals = rs.randint(1, 4, (n, 4)) * (2 * rs.randint(0, 2, (n, 4)) - 1)
    h = np.zeros((n, R), np.float32)
    h[np.arange(n)[:, None], cols] = vals
    q = lambda x: np.round(np.asarray(x, np.float64) * GRID) / GRID
    scale = {"n0.1": 0.1, "n8": 8.0}.get(family, 1.0)
    w = q(rs.randn(A, R) * scale / 4.3)                      # four terms of variance 14/3 each: logit std ~ scale
    b = q(rs.randn(A) * 0.5 * scale)
    if family == "equal":
        w[:] = w[0]
        b[:] = b[0]
    elif family == "plus60":
        b[plus60_action(A)] = np.ceil(60.0 + 24.0 * np.abs(w).max() + 2 * np.abs(b).max())
    elif family in ("neg", "neg_shifted"):
        w = q(rs.uniform(-0.6, 0.6, (A, R)))
        b = q(rs.uniform(-2, 2, A)) - (110.0 if family == "neg" else 0.0)
    elif family == "spread200":
        b = q(np.linspace(0.0, -200.0, A)[rs.permutation(A)])
    elif family in ("first_tiny", "last_tiny"):
        w = q(rs.randn(A, R) * 0.1 / 4.3)
        b = q(rs.randn(A) * 0.05)
        k = 0 if family == "first_tiny" else A - 1
        w[k] = 0.0
        b[k] = q(-26.0 * np.log(2.0) + np.log(A - 1.0))
    w32, b32 = w.astype(np.float32), b.astype(np.float32)
    logits = head_logits(h, w32, b32)
    assert np.array_equal(w32.astype(np.float64), w) and np.array_equal(b32.astype(np.float64), b)
    assert np.array_equal(logits.astype(np.float32).astype(np.float64), logits) and np.abs(logits).max() < 2.0 ** 15
    return h, w32, b32, logits


def head_family(A, R, seed=0):
    """Actor head of the cell-kernel cases: |w| <= 0.05 / R, so sum_j |h_j w_aj| <= 0.05 for a hidden row (|h| <= 1) and term (b)
    stays near 1e-6 up to R = 256 (the scale of the policies' own heads, whose weight rows have norm 0.01); the spread of the
    distribution comes from the bias."""
    rs = np.random.RandomState([int(seed), A, R, 77])
    return rs.uniform(-0.05 / R, 0.05 / R, (A, R)).astype(np.float32), rs.randn(A).astype(np.float32)


CELL_SEED, CELL_COUNTER = 2 ** 32 + 99, 1                    # (a fresh sampler's counter after begin_block)
CELL_CASES = [(kind, R, A, N) for kind in ("act1", "act2", "step") for R in ((64, 128, 256) if kind != "step" else (128,))
              for A in (4, 8) for N in (257, 4096)]
