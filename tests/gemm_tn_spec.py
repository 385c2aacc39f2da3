"""A host model of the weight-gradient GEMM's launch plan (csrc/gemm_tn_hip.hip: tn_kc, tn_wg_per_cu_now, gemm_tn_plan, the
kernel's `direct` expression) in plain Python, and the case lattice of tests/test_gemm_tn_f64_gpu.py chosen with it.

The model is of the DEFAULT plan: the library's tuning knobs must be unset (require_default_plan). tests/test_gemm_tn_spec_cpu.py
holds it to the built library's workspace functions, which return what the same planner decides."""
import os

TILE = 128
SMALL_K = 20 * 1024 + 1            # kSmallK: 16-row chunks below, 32-row chunks from here on (default mode)
MAX_PROBLEMS = 8
KNOBS = ("ATR_GEMM_TN_KC", "ATR_GEMM_TN_SLICES", "ATR_GEMM_TN_LDS_PAD")


def require_default_plan():
    """The spec and the tests that use it describe the default plan: fail (not skip) when a tuning knob is set."""
    found = [k for k in KNOBS if k in os.environ]
    assert not found, "unset %s: the gemm_tn spec and its tests model the library's default plan" % ", ".join(found)


def chunk_rows(K, corun=False):
    """tn_kc: rows of K per staged chunk."""
    if corun:
        return 16
    return 16 if K < SMALL_K else 32


def wg_per_cu(kc, corun=False):
    """tn_wg_per_cu_now: co-resident workgroups per CU the planner counts on."""
    if corun:
        return 1
    return 2 if kc == 32 else 3 if kc == 24 else 4


def tiles_of(M, N):
    return (M // TILE) * (N // TILE)


class Plan(object):
    """chunk_rows, slices, chunks_per_slice, and per slice (k_begin, k_end, cls) with cls in {"whole", "ragged", "empty"}: the
    rows [k_begin, k_end) a workgroup of that slice multiplies (both clamped to K, so an empty slice is (K, K))."""

    def __init__(self, K, kc, slices, cps):
        self.K, self.chunk_rows, self.slices, self.chunks_per_slice = K, kc, slices, cps
        self.ranges = []
        for s in range(slices):
            kb = min(s * cps * kc, K)
            ke = min((s + 1) * cps * kc, K)
            cls = "empty" if ke <= kb else "ragged" if (ke - kb) % kc else "whole"
            self.ranges.append((kb, ke, cls))

    def classes(self):
        return [r[2] for r in self.ranges]

    def ragged_index(self):
        idx = [i for i, r in enumerate(self.ranges) if r[2] == "ragged"]
        return idx[0] if idx else None

    def empty_count(self):
        return sum(1 for r in self.ranges if r[2] == "empty")


def plan(K, tiles, corun=False):
    """gemm_tn_plan for `tiles` output tiles in all (the same arithmetic in the same order, doubles on both sides)."""
    kc = chunk_rows(K, corun)
    per_cu = wg_per_cu(kc, corun)
    chunks = (K + kc - 1) // kc
    eff_pair, eff_solo = 0.85, 0.6
    best, best_cost = 8, 1e30
    for s in range(8, 513, 8):
        if s > chunks and s > 8:
            break
        cps, wgs = (chunks + s - 1) // s, tiles * s
        rows = float(cps) * kc + 64.0
        rnd = 256 * per_cu
        full = wgs // rnd
        rem = wgs - full * rnd
        cost = float(full) * per_cu * rows / eff_pair
        if rem > 256:
            cost += float((rem + 255) // 256) * rows / eff_pair
        elif rem > 0:
            cost += rows / eff_solo
        if cost < best_cost - 1e-9:
            best_cost, best = cost, s
    return Plan(K, kc, best, (chunks + best - 1) // best)


def workspace_floats(problems, K, corun=False):
    """atr_gemm_tn_grouped_workspace_floats for problems [(M, N), ...]: room for the partials and the column-sum partials of
    every problem, whether it asks for column sums or not."""
    s = plan(K, sum(tiles_of(M, N) for M, N in problems), corun).slices
    return sum(s * M * N + s * M for M, N in problems)


def workspace_regions(problems, K, corun=False):
    """What a launch writes of its workspace, for problems [(M, N, has_colsum), ...]: [(offset, length), ...] in floats, packed from
    offset 0 in problem order (partials, then the column-sum partials of a problem that has a destination for them)."""
    s = plan(K, sum(tiles_of(M, N) for M, N, _ in problems), corun).slices
    out, off = [], 0
    for M, N, cs in problems:
        out.append((off, s * M * N))
        off += s * M * N
        if cs:
            out.append((off, s * M))
            off += s * M
    return out


def group_is_mixed(K, any_row_scale, corun=False):
    """Whether the launch is the kMixed = true instantiation (some workgroup may need the register-staged path)."""
    return bool(any_row_scale) or K % chunk_rows(K, corun) != 0


def path(problem_has_row_scale, slice_class, chunk_rows, group_is_mixed):
    """The kernel's `direct` expression: "dma" (operands straight into LDS) or "staged" (through registers: row factors, ragged
    and empty slices of a mixed launch, and every workgroup of a mixed launch with 16-row chunks)."""
    if not group_is_mixed:
        return "dma"
    if chunk_rows == 32 and not problem_has_row_scale and slice_class == "whole":
        return "dma"
    return "staged"


def paths(K, problems, corun=False):
    """Per problem [(M, N, has_row_scale), ...] of one launch: the set of (slice class, path) its workgroups take."""
    p = plan(K, sum(tiles_of(M, N) for M, N, _ in problems), corun)
    mixed = group_is_mixed(K, any(rs for _, _, rs in problems), corun)
    return [sorted(set((c, path(rs, c, p.chunk_rows, mixed)) for c in p.classes())) for _, _, rs in problems]


# ---- the case lattice of tests/test_gemm_tn_f64_gpu.py -------------------------------------------------------------------------
# class -> [(K, M, N), ...]; every case runs plain, with row factors, and with row factors + column sums (VARIANTS), so the
# "no row factors" and "row_scale" classes of 32-row ragged K are the plain and the scaled variants of the same K values.
CLASSES = {
    "16-row whole direct": [(4096, 128, 128), (4160, 128, 128)],
    "16-row ragged": [(4097, 128, 128), (4103, 256, 128), (4104, 128, 128), (4105, 128, 256), (4111, 128, 128)],
    "32-row whole direct": [(20512, 128, 128), (20800, 128, 256)],
    "32-row ragged plain": [(20481, 128, 128), (20487, 128, 128), (20488, 256, 128), (20489, 128, 128), (20496, 128, 128),
                            (20497, 128, 256), (20504, 128, 128), (20505, 128, 384), (20511, 128, 128)],
    "32-row ragged row_scale": [(20481, 128, 128), (20505, 128, 384), (20803, 256, 128)],
    "co-run": [(4099, 128, 128), (20481, 128, 128), (20505, 128, 384)],
}
VARIANTS = ("plain", "row_scale", "row_scale+colsum")
GROUPED_K = (20505, 20803)
# the grouped launch's five problems: (M, N, biases, row_scale shift or None, ld1, col1, ld2, col2); ld = 0: dense operand
GROUPED_PROBLEMS = [
    (256, 128, 2, None, 0, 0, 0, 0),
    (128, 256, 0, 17, 0, 0, 0, 0),
    (128, 256, 0, 0, 0, 0, 0, 0),
    (128, 384, 0, None, 0, 0, 0, 0),
    (128, 128, 1, None, 260, 4, 384, 0),
]
DIRECT_ENTRY_K = (4103, 20505)     # the C entry called directly, one K per chunk size (sentinels around workspace and outputs)


def single_cases():
    """[(class, K, M, N, corun)] without repeats: the (K, M, N, corun) points the GPU module runs through fused.gemm_tn."""
    seen, out = set(), []
    for cls, cases in CLASSES.items():
        corun = cls == "co-run"
        for K, M, N in cases:
            if (K, M, N, corun) not in seen:
                seen.add((K, M, N, corun))
                out.append((cls, K, M, N, corun))
    return out


def case_id(case):
    return "K%d-%dx%d%s" % (case[1], case[2], case[3], "-corun" if case[4] else "")


def lattice_K():
    return sorted(set(K for cases in CLASSES.values() for K, _, _ in cases) | set(GROUPED_K))
