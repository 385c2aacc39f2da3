"""tests/gemm_tn_spec.py (the host model of the weight-gradient GEMM's plan) against the built library, its own invariants, and
the coverage it promises for tests/test_gemm_tn_f64_gpu.py. No GPU: the workspace functions and atr_gemm_tn_set_corun touch no
device."""
import pytest

import gemm_tn_spec as spec

LEARNER_K = [10240, 20480, 40960, 81920]
EDGE_K = [1, 15, 16, 17, 30000]
# tile count -> one problem of that many tiles, and a group of that many tiles
SINGLE = {1: (128, 128), 2: (128, 256), 4: (256, 256), 8: (256, 512), 44: (512, 1408)}
GROUPS = {1: [(128, 128)], 2: [(128, 128)] * 2, 4: [(128, 256), (256, 128)], 8: [(256, 128)] * 2 + [(128, 512)],
          44: [(512, 256), (512, 128), (256, 512), (256, 1024), (512, 256)]}


@pytest.fixture(autouse=True)
def _default_plan():
    spec.require_default_plan()


def _grid_K():
    return sorted(set(spec.lattice_K() + LEARNER_K + EDGE_K))


def _lib():
    from active_tracking_rl_amd import build, fused
    build.build()
    return fused.lib()


def _problems(shapes, base=0x100000):
    """A GemmTnProblem array for [(M, N), ...] with made-up, 16-byte aligned host addresses (never dereferenced)."""
    from active_tracking_rl_amd import fused
    arr = (fused.GemmTnProblem * len(shapes))()
    for q, (M, N) in enumerate(shapes):
        arr[q].x1, arr[q].x2, arr[q].c = base, base + 0x1000, base + 0x2000
        arr[q].M, arr[q].N = M, N
    return arr


def test_spec_reproduces_the_issue_example():
    p = spec.plan(20481, 1)
    assert (p.chunk_rows, p.slices, p.chunks_per_slice) == (32, 216, 3)
    assert p.ragged_index() == 213 and p.ranges[213][:2] == (20448, 20481) and p.classes()[214:] == ["empty", "empty"]


def test_spec_against_the_library_workspace_sizes():
    L = _lib()
    was = L.atr_gemm_tn_set_corun(0)
    try:
        for corun in (False, True):
            L.atr_gemm_tn_set_corun(1 if corun else 0)
            for K in _grid_K():
                for tiles in sorted(SINGLE):
                    M, N = SINGLE[tiles]
                    assert spec.tiles_of(M, N) == tiles == sum(spec.tiles_of(*s) for s in GROUPS[tiles])
                    assert L.atr_gemm_tn_workspace_floats(K, M, N) == spec.workspace_floats([(M, N)], K, corun), (K, tiles, corun)
                    got = L.atr_gemm_tn_grouped_workspace_floats(_problems(GROUPS[tiles]), len(GROUPS[tiles]), K)
                    assert got == spec.workspace_floats(GROUPS[tiles], K, corun), (K, tiles, corun)
    finally:
        L.atr_gemm_tn_set_corun(was)
    assert L.atr_gemm_tn_set_corun(was) == was


def test_spec_plans_partition_K():
    for corun in (False, True):
        for K in _grid_K():
            for tiles in sorted(SINGLE):
                p = spec.plan(K, tiles, corun)
                what = (K, tiles, corun)
                assert p.slices % 8 == 0 and 8 <= p.slices <= 512 and len(p.ranges) == p.slices, what
                assert p.chunk_rows == (16 if corun or K <= 20480 else 32), what
                cls = p.classes()
                live = [r for r in p.ranges if r[2] != "empty"]
                assert live[0][0] == 0 and live[-1][1] == K, what                   # [0, K) ...
                assert all(a[1] == b[0] for a, b in zip(live, live[1:])), what      # ... without gaps or overlap
                assert all(kb < ke for kb, ke, _ in live), what
                assert cls.count("ragged") <= 1 and (cls.count("ragged") == 1) == (K % p.chunk_rows != 0), what
                assert cls[:len(live)] == [r[2] for r in live], what                # empty slices only after the last live one
                if "ragged" in cls:
                    assert cls.index("ragged") == len(live) - 1, what
                assert all((ke - kb) % p.chunk_rows == 0 for kb, ke, c in p.ranges if c == "whole"), what


def _rows(cls, K, M, N, corun):
    """Table rows of one (K, M, N) case, one per variant: (label, plan, paths of the single problem)."""
    out = []
    for variant in spec.VARIANTS:
        rs = variant != "plain"
        p = spec.plan(K, spec.tiles_of(M, N), corun)
        out.append((variant, p, spec.paths(K, [(M, N, rs)], corun)[0]))
    return out


def test_coverage_of_the_gpu_lattice(capsys):
    """Every class of the GPU module's table is reached by at least one of its cases according to the spec; prints the table."""
    table, hit = [], {}
    for cls, K, M, N, corun in spec.single_cases():
        rows = _rows(cls, K, M, N, corun)
        assert rows[1][2] == rows[2][2]                             # column sums do not change a workgroup's path
        table.append(("%s %dx%d%s" % (K, M, N, " corun" if corun else ""), rows[0][1], [rows[0][2], rows[1][2]]))
        for variant, p, paths in rows:
            tail = K % p.chunk_rows
            group = (tail + 7) // 8 if tail else 0                  # the row group (1-based) the tail ends in; 0: whole chunks
            hit.setdefault((p.chunk_rows, corun, variant != "plain"), []).append((K, group, p.empty_count(), tuple(paths)))
    for K in spec.GROUPED_K:
        probs = [(M, N, shift is not None) for M, N, _, shift, _, _, _, _ in spec.GROUPED_PROBLEMS]
        p = spec.plan(K, sum(spec.tiles_of(M, N) for M, N, _ in probs))
        table.append(("%s grouped x%d" % (K, len(probs)), p, spec.paths(K, probs)))
    with capsys.disabled():
        print("\n%-20s %5s %6s %6s %6s %5s  %s" % ("case", "chunk", "slices", "chunks", "ragged", "empty",
                                                  "slice class:path (single cases: plain | with row factors; grouped: per problem)"))
        short = {"whole": "w", "ragged": "r", "empty": "e"}
        for what, p, paths in table:
            print("%-20s %5d %6d %6d %6s %5d  %s" % (what, p.chunk_rows, p.slices, p.chunks_per_slice, p.ragged_index(),
                                                    p.empty_count(),
                                                    " | ".join(" ".join("%s:%s" % (short[c], x) for c, x in pp) for pp in paths)))
    dma, staged = ("whole", "dma"), ("whole", "staged")
    # 16-row, whole, direct: no staged workgroup at all; once with empty slices
    c = [x for x in hit[(16, False, False)] if x[1] == 0]
    assert c and all("staged" not in [q[1] for q in x[3]] for x in c) and any(x[2] > 0 for x in c)
    # 16-row, ragged: everything staged, the tail ends in each of the two row groups
    c = [x for x in hit[(16, False, False)] + hit[(16, False, True)] if x[1] != 0]
    assert set(x[1] for x in c) == {1, 2} and all("dma" not in [q[1] for q in x[3]] for x in c)
    # 32-row, whole, direct; once with empty slices
    c = [x for x in hit[(32, False, False)] if x[1] == 0]
    assert c and all("staged" not in [q[1] for q in x[3]] for x in c) and any(x[2] > 0 for x in c)
    # 32-row, ragged, no row factors: one problem takes BOTH paths; the tail ends in each of the four row groups; and once the
    # ragged slice is not the launch's last one
    c = [x for x in hit[(32, False, False)] if x[1] != 0]
    assert set(x[1] for x in c) == {1, 2, 3, 4} and any(x[2] > 0 for x in c)
    assert all(dma in x[3] and ("ragged", "staged") in x[3] for x in c)
    # 32-row, row factors: all staged, ragged (each row group again) and whole
    c = hit[(32, False, True)]
    assert set(x[1] for x in c) >= {1, 2, 3, 4} and all(staged in x[3] and dma not in x[3] for x in c) and any(x[2] > 0 for x in c)
    # co-run: 16-row chunks at every K, also above the default mode's threshold, with many empty slices at the small K
    c = hit[(16, True, False)] + hit[(16, True, True)]
    assert any(x[0] > 20480 for x in c) and any(x[2] >= 64 for x in c) and all(x[1] != 0 for x in c)
    assert (32, True, False) not in hit and (32, True, True) not in hit
    # the grouped launch: 32-row chunks, mixed, ragged; the problem without extras moves its whole slices by DMA, the
    # row_scale problems stage everything; empty slices at the second K
    for K in spec.GROUPED_K:
        probs = [(M, N, shift is not None) for M, N, _, shift, _, _, _, _ in spec.GROUPED_PROBLEMS]
        p = spec.plan(K, sum(spec.tiles_of(M, N) for M, N, _ in probs))
        assert p.chunk_rows == 32 and p.ragged_index() is not None and spec.group_is_mixed(K, True)
        for (M, N, rs), pp in zip(probs, spec.paths(K, probs)):
            assert (dma in pp) == (not rs) and ("ragged", "staged") in pp
    assert spec.plan(spec.GROUPED_K[1], 10).empty_count() > 0
    assert len(spec.GROUPED_PROBLEMS) == 5 and sum(spec.tiles_of(g[0], g[1]) for g in spec.GROUPED_PROBLEMS) == 10
    # the directly called C entry: one K per chunk size, both ragged
    assert sorted(spec.chunk_rows(K) for K in spec.DIRECT_ENTRY_K) == [16, 32]
    assert all(K % spec.chunk_rows(K) for K in spec.DIRECT_ENTRY_K)


def test_path_follows_the_kernels_direct_expression():
    for kc in (16, 32):
        for rs in (False, True):
            for cls in ("whole", "ragged", "empty"):
                assert spec.path(rs, cls, kc, False) == "dma"           # kMixed = false: the staged path is compiled out
                want = "dma" if (kc == 32 and not rs and cls == "whole") else "staged"
                assert spec.path(rs, cls, kc, True) == want
    assert not spec.group_is_mixed(20512, False) and spec.group_is_mixed(20512, True) and spec.group_is_mixed(20513, False)
    assert not spec.group_is_mixed(20496, False, corun=True) and spec.group_is_mixed(20496, False)


@pytest.mark.parametrize("field", ["x1", "x2", "c", "colsum0", "colsum1"])
def test_workspace_functions_refuse_misaligned_pointers(field):
    """group_tiles refuses an operand or destination that is not 16-byte aligned exactly as it refuses M % 128 != 0 (-1): the
    kernel reads x1 / x2 and writes c 16 bytes at a time. row_scale is read one float at a time and may sit anywhere."""
    L = _lib()
    K = 20505
    good = _problems([(128, 256), (256, 128)])
    good[1].colsum0, good[1].colsum1 = 0x300000, 0x300400
    good[0].row_scale = 0x400004
    want = spec.workspace_floats([(128, 256), (256, 128)], K)
    assert L.atr_gemm_tn_grouped_workspace_floats(good, 2, K) == want
    bad_shape = _problems([(128, 256), (130, 128)])
    assert L.atr_gemm_tn_grouped_workspace_floats(bad_shape, 2, K) == -1
    for off in (4, 8, 12):
        bad = _problems([(128, 256), (256, 128)])
        bad[1].colsum0, bad[1].colsum1 = 0x300000, 0x300400
        setattr(bad[1], field, getattr(bad[1], field) + off)
        assert L.atr_gemm_tn_grouped_workspace_floats(bad, 2, K) == -1, (field, off)
    # the single-problem query stands in an aligned dummy for the pointers and keeps answering
    assert L.atr_gemm_tn_workspace_floats(K, 128, 256) == spec.workspace_floats([(128, 256)], K)
    assert L.atr_gemm_tn_workspace_floats(K, 130, 256) == -1
