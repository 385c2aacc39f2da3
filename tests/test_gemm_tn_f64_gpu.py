"""The weight-gradient GEMM (csrc/gemm_tn_hip.hip: atr_gemm_tn, atr_gemm_tn_grouped) against float64 over its plan lattice:
the cases of tests/gemm_tn_spec.py, chosen with the host model of the planner so that every chunk size, slice class (whole,
ragged, empty), staging path (DMA, registers) and row group of the staging macros is run (tests/test_gemm_tn_spec_cpu.py
prints and asserts that coverage).

Leg A, integer operands ({-2..2}, row factors {0, 1, 2, -1}): every product and partial sum is an integer below 2^18, so the
fp32 MFMA chain, the split-K partials and the reduction are exact in any order and the result must EQUAL the float64 product.
No tolerance: one wrong, missing or doubled product shows.
Leg B, Gaussian operands: the float64 rule of tests/f64_rule.py per 128 x 128 output tile and per column-sum vector, e(hip) <=
max(4 e(aten32), 1e-6), with the resolution asserted: 10 x the allowed error stays below 1/sqrt(K), one K row's share of a tile.
Guard bands: every operand is the first K rows of an allocation whose 64 further rows hold NaN (column blocks: NaN in the
neighbouring columns too; row factors: a NaN tail), so a row or factor read past its end makes the result non-finite.

Measured on MI355X, leg B (e = ||x - x64|| / ||x64||; ranges over every tile / column-sum vector of the class, all variants):
  class                      product tiles: e(hip)      e(aten32)            column sums: e(hip)      e(aten32)
  16-row, whole, direct      2.27e-7 .. 2.96e-7   1.03e-6 .. 1.04e-6         1.00e-7 .. 1.06e-7   1.03e-7 .. 1.09e-7
  16-row, ragged             2.05e-7 .. 2.32e-7   1.00e-6 .. 1.14e-6         9.82e-8 .. 1.39e-7   1.02e-7 .. 1.61e-7
  32-row, whole, direct      3.06e-7 .. 3.17e-7   1.45e-6 .. 1.66e-6         1.26e-7 .. 1.45e-7   1.43e-7 .. 1.56e-7
  32-row, ragged (K 20481 .. 20511, plain and with row factors)
                             2.93e-7 .. 3.21e-7   1.41e-6 .. 1.63e-6         1.31e-7 .. 1.96e-7   1.50e-7 .. 2.29e-7
  32-row, ragged, K = 20803  3.10e-7 .. 3.18e-7   1.44e-6 .. 1.59e-6         1.41e-7              2.47e-7
  co-run (and the default mode on the same operands)
                             2.29e-7 .. 3.15e-7   1.03e-6 .. 1.69e-6         1.18e-7 .. 1.96e-7   1.34e-7 .. 1.99e-7
  grouped, 5 problems        3.60e-7 .. 4.02e-7   1.44e-6 .. 1.69e-6         2.65e-7 .. 2.88e-7   1.64e-7 .. 2.13e-7
So every e(hip) lies below the rule's floor of 1e-6; what the rule allowed was at most 6.8e-6, and 10 x that is 1/100 of 1/sqrt(K).
Verdict on the kernel header's "tighter error than the library's split-K order": it holds for the products, e(hip) is 0.18 - 0.29
of e(aten32) on every tile measured. It does not extend to the column sums: 0.57 - 1.20 of the library's in single launches, 1.3 -
1.8 in the grouped launch (48 slices of 448 rows each; still a quarter of the floor). The header now says so.

Scratch mutations of the kernel (built apart, loaded through T2D_LIB_PATH, nothing of them committed), against this module and
the kernel-level tests that existed before it (test_fused_stem_gpu -k "gemm_tn or grouped", test_lt_gemm_gpu -k grouped; 15 tests):
  1. rs3 never loaded (the fourth row group's factor stays 1): 34 of this module's 53 tests fail: both legs at every K above
     20480 (the co-run cases there through their comparison with the default mode), all four grouped cases, the C entry at
     K = 20505 and the graph replay. Of the existing tests 3 fail (test_gemm_tn_matches_float64_reference at 20800, 41600, 81920:
     a 0/1 mask missed on a quarter of the rows is far above their bound), 12 pass.
  2. `kc_ < k_end` -> `kc_ + 1 < k_end` on the loads (one row of the third group dropped at the tail): 4 fail, both legs at
     K = 20497 and K = 20504, the two tails that end in the third row group. All 15 existing tests pass: nothing saw it before.
  3. k_gemm_tn_reduce starts at z = 2 (slice 1 left out): 51 fail (the 2 that pass are the misaligned-operand tests, which
     check the library product). All 15 existing tests fail."""
import functools

import pytest
import torch

import f64_rule
import gemm_tn_spec as spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64            # NaN rows behind every operand
SENTINEL = 7.5        # no integer: an exact leg-A value never equals it
PAD = 4096            # sentinel floats around the workspace and the outputs of the directly called entry

CASES = spec.single_cases()


@pytest.fixture(autouse=True)
def _default_plan():
    spec.require_default_plan()


def _band(t, ld=None, col0=0):
    """CPU t [K, C] -> a CUDA view holding it: rows 0:K, columns col0:col0 + C of a [K + GUARD, ld] allocation of NaN."""
    K, C = t.shape
    full = torch.full((K + GUARD, ld or C), float("nan"), device=DEV)
    view = full[:K, col0:col0 + C]
    view.copy_(t)
    return view


def _band1(v):
    """CPU vector v [n] -> the first n elements of a CUDA vector with a NaN tail."""
    full = torch.full((v.numel() + GUARD,), float("nan"), device=DEV)
    full[:v.numel()].copy_(v)
    return full[:v.numel()]


def _operands(leg, seed, K, M, N):
    """CPU float32 x1 [K, M], x2 [K, N], row factors [K] of one leg, from a generator of their own."""
    gen = torch.Generator().manual_seed(seed)
    if leg == "int":
        x1 = torch.randint(-2, 3, (K, M), generator=gen).float()
        x2 = torch.randint(-2, 3, (K, N), generator=gen).float()
        s = torch.tensor([0.0, 1.0, 2.0, -1.0])[torch.randint(0, 4, (K,), generator=gen)]
    else:
        x1, x2 = torch.randn(K, M, generator=gen), torch.randn(K, N, generator=gen)
        s = (torch.rand(K, generator=gen) + 0.5) * (torch.rand(K, generator=gen) > 0.2).float()
    return x1, x2, s


def _refs(x1, x2, s):
    """float64 on the CPU: {variant: (product, column sums or None)}."""
    a, b = x1.double(), x2.double()
    xs = a * s.double().unsqueeze(1)
    scaled = xs.t() @ b
    return {"plain": (a.t() @ b, None), "row_scale": (scaled, None), "row_scale+colsum": (scaled, xs.sum(0))}


def _call(fused, variant, x1, x2, s):
    if variant == "plain":
        return fused.gemm_tn(x1, x2), None
    if variant == "row_scale":
        return fused.gemm_tn(x1, x2, row_scale=s), None
    return fused.gemm_tn(x1, x2, row_scale=s, colsum=True)


@functools.lru_cache(maxsize=None)
def _run(leg, K, M, N, corun):
    """One case through fused.gemm_tn in every variant, twice each; CPU copies of the (small) results only, so that the co-run
    cases find the default mode's results of the same operands here: {variant: dict(c, cs, again, ref, ref_cs, a32, a32_cs)}."""
    from active_tracking_rl_amd import fused
    x1, x2, s = _operands(leg, 1000 * K + M + N + (7 if leg == "int" else 0), K, M, N)
    refs = _refs(x1, x2, s)
    g1, g2, gs = _band(x1), _band(x2), _band1(s)
    assert g1.is_contiguous() and g2.is_contiguous() and g1.data_ptr() % 16 == 0 and g2.data_ptr() % 16 == 0
    out = {}
    with fused.gemm_tn_corun(corun):
        for variant in spec.VARIANTS:
            c, cs = _call(fused, variant, g1, g2, gs)
            c2, cs2 = _call(fused, variant, g1, g2, gs)
            same = torch.equal(c, c2) and (cs is None or torch.equal(cs, cs2))
            out[variant] = dict(c=c.cpu(), cs=None if cs is None else cs.cpu(), again=same, ref=refs[variant][0],
                                ref_cs=refs[variant][1])
    assert fused.lib().atr_gemm_tn_set_corun(0) == 0
    if leg == "gauss":
        xs = g1 * gs.unsqueeze(1)
        out["plain"]["a32"] = (g1.t() @ g2).cpu()
        out["row_scale"]["a32"] = out["row_scale+colsum"]["a32"] = (xs.t() @ g2).cpu()
        out["row_scale+colsum"]["a32_cs"] = xs.sum(0).cpu()
    torch.cuda.synchronize()
    return out


def _tiles(M, N):
    return [(i, j) for i in range(M // 128) for j in range(N // 128)]


def _tile(t, i, j):
    return t[128 * i:128 * (i + 1), 128 * j:128 * (j + 1)]


def _rule_by_tile(table, what, hip, x64, x32):
    for i, j in _tiles(*hip.shape):
        table.rule("%s tile %d,%d" % (what, i, j), _tile(hip, i, j), _tile(x64, i, j), _tile(x32, i, j))


def _finish_with_resolution(table, K):
    """Table.finish(), then the rule's resolution: what it allowed, times 10, is still below one K row's share of a tile."""
    rows = table.finish()
    for what, e_hip, e32 in rows:
        allowed = max(f64_rule.FACTOR * e32, f64_rule.FLOOR)
        assert allowed * 10.0 <= K ** -0.5, (what, allowed, K ** -0.5)
    return rows


@pytest.mark.parametrize("case", CASES, ids=[spec.case_id(c) for c in CASES])
def test_integer_operands_give_the_float64_product_exactly(case):
    """Leg A over the lattice: plain, row factors, row factors + column sums; bit-reproducible; co-run equals default."""
    cls, K, M, N, corun = case
    res = _run("int", K, M, N, corun)
    for variant in spec.VARIANTS:
        r = res[variant]
        what = (cls, K, M, N, corun, variant)
        assert r["c"].shape == (M, N) and bool(torch.isfinite(r["c"]).all()), what
        bad = (r["c"].double() != r["ref"]).nonzero()
        assert bad.numel() == 0, (what, "%d entries differ, first at %s: %s != %s" % (
            bad.shape[0], bad[0].tolist(), float(r["c"][tuple(bad[0])]), float(r["ref"][tuple(bad[0])])))
        if r["ref_cs"] is not None:
            assert bool(torch.isfinite(r["cs"]).all()) and torch.equal(r["cs"].double(), r["ref_cs"]), what
        assert r["again"], what
    if corun:                                       # only the summation order differs: the same bits on exact data
        base = _run("int", K, M, N, False)
        for variant in spec.VARIANTS:
            assert torch.equal(res[variant]["c"], base[variant]["c"]), (K, variant)
        assert torch.equal(res["row_scale+colsum"]["cs"], base["row_scale+colsum"]["cs"])


@pytest.mark.parametrize("case", CASES, ids=[spec.case_id(c) for c in CASES])
def test_gaussian_operands_meet_the_float64_rule(case):
    """Leg B over the lattice, per output tile and column-sum vector (co-run cases: the default mode's result of the same operands
    is held to the rule beside them)."""
    cls, K, M, N, corun = case
    runs = [(corun, _run("gauss", K, M, N, corun))] + ([(False, _run("gauss", K, M, N, False))] if corun else [])
    for mode, res in runs:
        table = f64_rule.Table("[%s] K=%d %dx%d%s" % (cls, K, M, N, " corun" if mode else ""))
        for variant in spec.VARIANTS:
            r = res[variant]
            assert r["again"], (K, variant)
            _rule_by_tile(table, variant, r["c"], r["ref"], r["a32"])
            if r["ref_cs"] is not None:
                table.rule(variant + " colsum", r["cs"], r["ref_cs"], r["a32_cs"])
        _finish_with_resolution(table, K)


def _grouped_case(leg, K):
    """The five problems of spec.GROUPED_PROBLEMS over K rows: CUDA operands in guard bands, float64 references, a bucket."""
    from active_tracking_rl_amd.shared_optim import FlatParams
    params, probs = [], []
    for q, (M, N, n_bias, shift, ld1, col1, ld2, col2) in enumerate(spec.GROUPED_PROBLEMS):
        x1, x2, s = _operands(leg, 77 * K + q + (500 if leg == "int" else 0), K, M, N)
        w = torch.nn.Parameter(torch.zeros(M, N, device=DEV))
        biases = [torch.nn.Parameter(torch.zeros(M, device=DEV)) for _ in range(n_bias)]
        odd = torch.nn.Parameter(torch.zeros(1 + q, device=DEV))         # (leaves padding between the slots)
        params += [w] + biases + [odd]
        scale = torch.ones(K, dtype=torch.float64)
        rs = None
        if shift is not None:
            scale[shift:] = s[:K - shift].double()
            rs = _band1(s[:K - shift])
        xs = x1.double() * scale.unsqueeze(1)
        probs.append(dict(x1=_band(x1, ld1 or None, col1), x2=_band(x2, ld2 or None, col2), w=w, biases=biases, rs=rs,
                          shift=shift or 0, ref=xs.t() @ x2.double(), ref_cs=xs.sum(0), scale=scale.float().to(DEV)))
    bucket = FlatParams(params)
    return bucket, params, probs


def _flush_group(fused, bucket, probs):
    q = fused.DeferredWeightGrads(bucket)
    got = [q.add(p["x1"], p["x2"], p["w"], biases=tuple(p["biases"]), row_scale=p["rs"], shift=p["shift"]) for p in probs]
    assert all(g is not None for g in got)
    q.flush()
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("leg", ["int", "gauss"])
@pytest.mark.parametrize("K", spec.GROUPED_K)
def test_grouped_mixed_launch_at_32_row_chunks(K, leg, monkeypatch):
    """fused.DeferredWeightGrads -> ONE atr_gemm_tn_grouped launch of five problems at a ragged K with 32-row chunks (the kMixed
    instantiation): two bias destinations; row factors with shift 17 and shift 0 (all staged); a 128 x 384 problem without extras
    (its whole slices by DMA); column-block operands (ld1 = 260 at a 16-byte column offset, ld2 = 384). The bucket's padding and
    everything outside the slots keep their sentinel; a second flush gives the same bits."""
    from active_tracking_rl_amd import fused
    bucket, params, probs = _grouped_case(leg, K)
    bucket.grad.fill_(SENTINEL)
    L = fused.lib()
    real, calls = L.atr_gemm_tn_grouped, []

    def spy(*a):
        calls.append(a[1])
        return real(*a)
    monkeypatch.setattr(L, "atr_gemm_tn_grouped", spy)
    got = _flush_group(fused, bucket, probs)
    assert calls == [len(probs)]
    views = {p.data_ptr(): v for p, v in zip(bucket.params, bucket.grad_views())}
    table = f64_rule.Table("[grouped %s] K=%d" % (leg, K))
    for q, (p, (dw, dbs)) in enumerate(zip(probs, got)):
        assert dw.data_ptr() == views[p["w"].data_ptr()].data_ptr() and len(dbs) == len(p["biases"])
        c = dw.cpu()
        assert bool(torch.isfinite(c).all()), q
        outs = [c] + [b.cpu() for b in dbs]
        wants = [p["ref"]] + [p["ref_cs"]] * len(dbs)
        if leg == "int":
            for o, w in zip(outs, wants):
                assert torch.equal(o.double(), w), (q, o.shape)
        else:
            x1 = p["x1"].contiguous() * p["scale"].unsqueeze(1)
            _rule_by_tile(table, "problem %d" % q, c, p["ref"], (x1.t() @ p["x2"].contiguous()).cpu())
            for o in outs[1:]:
                assert bool(torch.isfinite(o).all())
                table.rule("problem %d colsum" % q, o, p["ref_cs"], x1.sum(0).cpu())
    if leg == "gauss":
        _finish_with_resolution(table, K)
    used = torch.zeros_like(bucket.grad, dtype=torch.bool)
    registered = set(p["w"].data_ptr() for p in probs) | set(b.data_ptr() for p in probs for b in p["biases"])
    for prm, off in zip(bucket.params, bucket.offsets):
        if prm.data_ptr() in registered:
            used[off:off + prm.numel()] = True
    assert bool((bucket.grad[~used] == SENTINEL).all()) and int((~used).sum()) > len(probs)
    before = bucket.grad.clone()
    bucket.grad[used] = SENTINEL
    _flush_group(fused, bucket, probs)
    assert torch.equal(before, bucket.grad)


@pytest.mark.parametrize("K", spec.DIRECT_ENTRY_K)
def test_c_entry_writes_exactly_the_regions_the_spec_predicts(K):
    """atr_gemm_tn called directly on integer operands, once per chunk size: workspace, c and colsum sit inside sentinel buffers.
    Every slice's partial product (and column-sum partial) is the float64 product of exactly the rows the spec's plan gives that
    slice (zeros for an empty one); c and colsum are written in full over NaN; the rest of the workspace, the column-sum region of a
    call without column sums included, and everything around the outputs keep the sentinel."""
    from active_tracking_rl_amd import fused
    M, N = 256, 128
    L = fused.lib()
    x1, x2, s = _operands("int", 31 * K, K, M, N)
    g1, g2, gs = _band(x1), _band(x2), _band1(s)
    plan = spec.plan(K, spec.tiles_of(M, N))
    total = spec.workspace_floats([(M, N)], K)
    assert L.atr_gemm_tn_workspace_floats(K, M, N) == total
    for extras in (False, True):
        ws = torch.full((total + PAD,), SENTINEL, device=DEV)
        cbuf = torch.full((PAD + M * N + PAD,), SENTINEL, device=DEV)
        csbuf = torch.full((PAD + M + PAD,), SENTINEL, device=DEV)
        c, cs = cbuf[PAD:PAD + M * N], csbuf[PAD:PAD + M]
        c.fill_(float("nan"))
        cs.fill_(float("nan"))
        assert c.data_ptr() % 16 == 0 and cs.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0
        L.atr_gemm_tn(fused._p(g1), fused._p(g2), fused._p(c), fused._p(ws), K, M, N, fused._pn(gs if extras else None),
                      fused._pn(cs if extras else None), fused._stream(g1))
        torch.cuda.synchronize()
        regions = spec.workspace_regions([(M, N, extras)], K)
        assert regions[0] == (0, plan.slices * M * N) and sum(n for _, n in regions) <= total
        wsc, written = ws.cpu(), 0
        for off, n in regions:
            assert off == written and bool((wsc[off:off + n] != SENTINEL).all()) and bool(torch.isfinite(wsc[off:off + n]).all())
            written += n
        assert bool((wsc[written:] == SENTINEL).all()) and wsc.numel() - written >= PAD
        xs = x1.double() * (s.double().unsqueeze(1) if extras else 1.0)
        part = wsc[:plan.slices * M * N].view(plan.slices, M, N).double()
        for z, (kb, ke, cls) in enumerate(plan.ranges):
            assert torch.equal(part[z], xs[kb:ke].t() @ x2[kb:ke].double()), (K, extras, z, cls)
        assert torch.equal(c.cpu().view(M, N).double(), xs.t() @ x2.double())
        assert bool((cbuf[:PAD] == SENTINEL).all()) and bool((cbuf[PAD + M * N:] == SENTINEL).all())
        if extras:
            cpart = wsc[regions[1][0]:regions[1][0] + regions[1][1]].view(plan.slices, M).double()
            for z, (kb, ke, cls) in enumerate(plan.ranges):
                assert torch.equal(cpart[z], xs[kb:ke].sum(0)), (K, z, cls)
            assert torch.equal(cs.cpu().double(), xs.sum(0))
        else:
            assert bool(torch.isnan(cs).all())
        assert bool((csbuf[:PAD] == SENTINEL).all()) and bool((csbuf[PAD + M:] == SENTINEL).all())


def test_default_and_corun_calls_replay_from_one_graph():
    """One default call (row factors + column sums) and one co-run call (plain) captured in a single chain; the operands are
    refilled in place and the replay equals eager calls on the new data, exactly (the mode is read at capture time)."""
    from active_tracking_rl_amd import fused
    K, M, N = 20505, 128, 128
    old = _operands("int", 5, K, M, N)
    new = _operands("int", 6, K, M, N)
    g1, g2, gs = _band(old[0]), _band(old[1]), _band1(old[2])

    def both():
        c_a, cs_a = fused.gemm_tn(g1, g2, row_scale=gs, colsum=True)
        with fused.gemm_tn_corun(True):
            c_b = fused.gemm_tn(g1, g2)
        return c_a, cs_a, c_b
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()                                          # first use outside the capture (the co-run form's LDS opt-in)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        outs = both()
    assert fused.lib().atr_gemm_tn_set_corun(0) == 0
    for dst, src in zip((g1, g2, gs), new):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in outs]
    eager = both()
    torch.cuda.synchronize()
    refs = _refs(*new)
    for a, b in zip(got, eager):
        assert torch.equal(a, b)
    assert torch.equal(got[0].cpu().double(), refs["row_scale+colsum"][0])
    assert torch.equal(got[1].cpu().double(), refs["row_scale+colsum"][1])
    assert torch.equal(got[2].cpu().double(), refs["plain"][0])


@pytest.mark.parametrize("which", ["x1", "x2"])
def test_misaligned_operand_goes_to_the_library_product(which, monkeypatch):
    """A contiguous [K, 128] view that starts one float into its buffer is not 16-byte aligned: fused.gemm_tn must not hand it to
    the kernel (float4 reads, 16-byte DMA). It computes the library product instead; atr_gemm_tn is not called."""
    from active_tracking_rl_amd import fused
    K, M, N = 4099, 128, 128
    x1, x2, s = _operands("gauss", 11, K, M, N)
    flat = torch.full((K * 128 + 8,), float("nan"), device=DEV)
    off = flat[1:1 + K * 128].view(K, 128)
    off.copy_(x1 if which == "x1" else x2)
    g1, g2 = (off, x2.to(DEV)) if which == "x1" else (x1.to(DEV), off)
    gs = s.to(DEV)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    L = fused.lib()
    real, calls = L.atr_gemm_tn, []

    def spy(*a):
        calls.append(a[4])
        return real(*a)
    monkeypatch.setattr(L, "atr_gemm_tn", spy)
    c, cs = fused.gemm_tn(g1, g2, row_scale=gs, colsum=True)
    assert calls == []
    xs = g1.contiguous() * gs.unsqueeze(1)
    refs = _refs(x1, x2, s)["row_scale+colsum"]
    table = f64_rule.Table("[misaligned %s] K=%d" % (which, K))
    table.rule("product", c, refs[0], xs.t() @ g2)
    table.rule("colsum", cs, refs[1], xs.sum(0))
    _finish_with_resolution(table, K)
    aligned = g1.clone(), g2.clone()                     # the control: the same call on aligned copies does reach the kernel
    fused.gemm_tn(aligned[0], aligned[1], row_scale=gs, colsum=True)
    assert calls == [K]
