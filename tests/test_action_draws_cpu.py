"""The host model of the action draw (tests/draw_spec.py) on its own: its Philox4x32-10 against the Random123 known-answer
vectors and against the oracle's (the env generators' bit-exact counterpart), its draws against the softmax (chi-square),
the distinctness of the uniforms of keys that differ in one field, a float32 re-enactment of the kernel's arithmetic held
to the margin rule, and the exclusion cap of EVERY case tests/test_action_draws_gpu.py runs: the share of rows the margin
takes out of the exact comparison is at most draw_spec.CAP, checked here with the same seeds and keys."""
import numpy as np
import pytest
import torch

import draw_spec as ds
from oracle import oracle as orc


def test_numpy_philox_known_answers_and_the_oracles_philox():
    f = 0xffffffff
    kat = [((0, 0, 0, 0), (0, 0), [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ((f, f, f, f), (f, f), [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, want in kat:
        assert [int(w) for w in ds.philox4x32_10(ctr, key)] == want
        assert orc.philox4x32(key[0], key[1], *ctr) == want
    rs = np.random.RandomState(5)
    words = rs.randint(0, 2 ** 32, size=(6, 4000), dtype=np.uint64)
    got = np.stack(ds.philox4x32_10(words[:4], words[4:]), 1)
    for i in range(words.shape[1]):
        w = [int(x) for x in words[:, i]]
        assert orc.philox4x32(w[4], w[5], w[0], w[1], w[2], w[3]) == [int(x) for x in got[i]], i


def test_uniform_is_the_headers_key_and_strictly_inside_the_unit_interval():
    seed, ctr, ordinal = 2 ** 63 + 12345, 2 ** 40 + 7, 41
    rows = np.arange(1000)
    x0 = ds.philox4x32_10([rows, ctr & 0xffffffff, ctr >> 32, 0x5A3D0000 ^ ordinal], [seed & 0xffffffff, seed >> 32])[0]
    u = ds.uniform(seed, rows, ctr, ordinal)
    assert np.array_equal(u, ((x0 >> 8).astype(np.float64) + 0.5) / 2 ** 24)
    assert u.min() > 0 and u.max() < 1
    # the ordinal wraps as the uint32 the kernels add the player index to
    assert np.array_equal(ds.uniform_bits(seed, rows, ctr, 2 ** 32 + 3), ds.uniform_bits(seed, rows, ctr, 3))


CHI2_1E6 = {1: 23.9, 2: 27.6, 3: 30.7, 4: 33.4, 7: 40.5}        # chi-square quantiles at p = 1e-6 by degrees of freedom


@pytest.mark.parametrize("A", [2, 3, 4, 5, 8])
def test_model_draws_from_the_softmax(A):
    n = 240000
    rs = np.random.RandomState(A)
    logits = np.tile(rs.randn(1, A) * 1.5, (n, 1))
    a = ds.draw(logits, ds.uniform(77 + A, np.arange(n), 3, 9))
    p = np.exp(logits[0] - logits[0].max())
    p /= p.sum()
    counts = np.bincount(a, minlength=A).astype(np.float64)
    chi2 = (((counts - n * p) ** 2) / (n * p)).sum()
    assert a.min() >= 0 and a.max() < A and chi2 < CHI2_1E6[A - 1], (chi2, counts / n, p)


KEY_VARIANTS = {"base": {}, "row": dict(row=2 ** 20), "ordinal": dict(ordinal=1), "counter_lo": dict(counter=1),
                "counter_hi": dict(counter=2 ** 32), "seed_lo": dict(seed=1), "seed_hi": dict(seed=2 ** 32)}


def variant_bits(name, n, seed=2 ** 33 + 5, counter=2 ** 34 + 11, ordinal=6):
    d = KEY_VARIANTS[name]
    return ds.uniform_bits(seed + d.get("seed", 0), np.arange(n) + d.get("row", 0), counter + d.get("counter", 0),
                           ordinal + d.get("ordinal", 0))


def test_keys_that_differ_in_one_field_give_unrelated_uniforms():
    n = 300001
    base = variant_bits("base", n)
    assert len(np.unique(base)) > n - 3 * n * n // 2 ** 25               # rows do not alias (birthday bound x 3)
    for name in KEY_VARIANTS:
        if name != "base":
            same = int((variant_bits(name, n) == base).sum())
            assert same <= 3, (name, same)                               # expectation n / 2**24 = 0.018


def float32_kernel_draw(logits32, bits):
    """csrc/atr_sample.h's draw_action in numpy float32, step by step (libm's exp in place of the hardware's)."""
    f = np.float32
    l = np.asarray(logits32, f)
    p = np.exp((l - l.max(1, keepdims=True)).astype(f)).astype(f)
    acc = np.zeros_like(p)
    s = np.zeros(l.shape[0], f)
    for a in range(l.shape[1]):
        s = (s + p[:, a]).astype(f)
        acc[:, a] = s
    u = (((bits.astype(f) + f(0.5)).astype(f) * f(2.0 ** -24)).astype(f) * s).astype(f)
    hit = u[:, None] < acc
    return np.where(hit.any(1), hit.argmax(1), l.shape[1] - 1)


@pytest.mark.parametrize("family", ds.EXACT_FAMILIES)
def test_a_float32_evaluation_passes_the_margin_rule(family):
    for A in ds.EXACT_A:
        h, w, b, logits = ds.exact_case(family, A, 128, 50021)
        seed, ctr, ordinal = ds.exact_key(family, A, 128, 50021)
        bits = ds.uniform_bits(seed, np.arange(len(h)), ctr, ordinal)
        a32 = float32_kernel_draw(logits.astype(np.float32), bits)
        n, excl, wrong, oor = ds.check(a32, logits, (bits + 0.5) / 2.0 ** 24, ds.delta_for(logits))
        assert wrong == 0 and oor == 0 and excl <= ds.CAP * n, (family, A, n, excl, wrong)
    # ... and the rule is not vacuous: the neighbouring action fails it
    wrong = ds.check((a32 + 1) % A, logits, (bits + 0.5) / 2.0 ** 24, ds.delta_for(logits))[2]
    assert wrong > 0.99 * n - excl


def test_exclusion_cap_of_every_exact_logit_case():
    worst = (-1.0, ())
    for family, A, R, n in ds.exact_grid_cases():
        h, w, b, logits = ds.exact_case(family, A, R, n)
        seed, ctr, ordinal = ds.exact_key(family, A, R, n)
        u = ds.uniform(seed, np.arange(n), ctr, ordinal)
        excl = int(ds.margin(logits, u, ds.delta_for(logits)).sum())
        assert excl <= ds.CAP * n, (family, A, R, n, excl)
        worst = max(worst, (excl / n, (family, A, R, n)))
        if n >= 4099:      # (the rows differ: on a 2**-8 grid of small logits at least dozens of distinct distributions)
            assert len(np.unique(logits - logits[:, :1] if family == "equal" else logits, axis=0)) >= (1 if family == "equal" else 32)
        if family == "plus60":
            k = ds.plus60_action(A)
            assert (logits[:, k] - np.delete(logits, k, 1).max(1) >= 60).all()
            assert (ds.draw(logits, u) == k).all()
        if family == "neg":
            assert logits.min() >= -120 and logits.max() <= -100
            assert np.array_equal(ds.exact_case("neg_shifted", A, R, n)[3], logits + 110.0)
        if family == "spread200":
            assert (logits.max(1) - logits.min(1) >= 170).all()
    print("largest excluded share %.2e at %s" % worst)


def lstm_rows(R, N, seed):
    """torch.nn.LSTMCell hidden rows on the CPU: stand-ins for the rows the device cells write. The cell is built under the
    case's seed as well: its weights come from the process-wide generator, which is seeded anew in every process, so the rows and
    with them the excluded count differed from run to run — about one run in three had a 257-row case with 2 excluded draws
    against a cap of 1. (The caller's generator state is put back.)"""
    g = torch.Generator().manual_seed(seed)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        cell = torch.nn.LSTMCell(256, R)
    with torch.no_grad():
        h, _ = cell(torch.randn(N, 256, generator=g), (torch.randn(N, R, generator=g).tanh(), torch.randn(N, R, generator=g)))
    return h.numpy()


@pytest.mark.parametrize("kind,R,A,N", ds.CELL_CASES)
def test_exclusion_cap_of_the_cell_kernel_cases_on_stand_in_rows(kind, R, A, N):
    """A case's share is taken over all its draws: both heads under the four ordinals the device test uses."""
    excl = 0
    for p in range(2):
        h = lstm_rows(R, N, 11 * R + A + p)
        w, b = ds.head_family(A, R, seed=p)
        logits = ds.head_logits(h, w, b)
        for ordinal in (1, 2, 3, 4):
            u = ds.uniform(ds.CELL_SEED, np.arange(N), ds.CELL_COUNTER, ordinal)
            excl += int(ds.margin(logits, u, ds.delta_for(logits, h, w, b)).sum())
    assert excl <= ds.CAP * N * (4 if kind == "act1" else 4), (kind, R, A, N, excl)


def test_exclusion_cap_at_the_rollout_policies_scale():
    """The rollout cases draw from the model's own actor heads (norm_col_init 0.01: every row of the weight has norm 0.01,
    bias 0) on 128-unit hidden rows: stand-in rows, 20 x 2 x 4096 of them, under a rollout's ordinals."""
    N, T, R, A = 4096, 20, 128, 4
    rs = np.random.RandomState(0)
    w = rs.randn(A, R)
    w = (0.01 * w / np.sqrt((w ** 2).sum(1, keepdims=True))).astype(np.float32)
    b = np.zeros(A, np.float32)
    h = lstm_rows(R, N, 3)
    excl = 0
    for o in range(1, 2 * T + 2):
        logits = ds.head_logits(h, w, b)
        u = ds.uniform(12345, np.arange(N), 7, o)
        excl += int(ds.margin(logits, u, ds.delta_for(logits, h, w, b)).sum())
    assert excl <= ds.CAP * N * (2 * T + 1), excl
