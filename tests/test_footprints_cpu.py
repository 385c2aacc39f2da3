"""CPU-side checks of footprints: the rule of include/atr_footprints.h as tests/footprints_spec.py states it (what is never painted,
the record rule case by case, the trail's length, a walk away from a standing tracker); csrc/atr_footprint_rule.h through a
stand-alone host program built with the address and undefined-behaviour sanitizers, table for table against the spec; the header
against the built library and footprints.FOOTPRINT_PROTOTYPES; every refusal that comes before the handle is looked at; the flags
of both parsers; the refusals of create_env and VecEnv."""
import argparse
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import footprints_spec as sp
from conftest import ROOT
from test_abi_cpu import _header_functions, _header_structs, _header_symbols, _py_class

PARTIAL = "Track2D-BlockPartialPZR-v0"
E = sp.EMPTY


def _open_map(side=20):
    return np.zeros((side, side), np.uint8)


def _pos(tracker, target):
    return np.array([[tracker, target]], np.int64)


# -- the spec's own properties ---------------------------------------------------------------------------------------------------

def test_what_is_never_painted():
    """A map with a wall segment, the tracker at (1, 8) — so that rows of padding are in its window — and a target trail that
    holds the tracker's own cell, a wall cell, the target's current cell (it walked back onto its print), a cell the field of
    view wrote as 5, a cell outside the map's window and two free cells, one of them twice: only the free cells become 6."""
    grid = _open_map()
    grid[3, 5:12] = 1
    pos = _pos((1, 8), (4, 9))
    w = sp.windows_of(grid, pos)
    assert w[0, 0, 6, 6] == 2 and w[0, 0, 9, 7] == 4 and (w[0, 0, :5] == 1).all() and w[0, 0, 8, 6] == 1
    w[0, 0, 10, 3] = 5                                         # (5, 5) reads "unseen"
    trail = sp.new_trail(1, 8)
    trail[0, 1] = [sp.cell(4, 9), sp.cell(1, 8), sp.cell(3, 8), sp.cell(4, 9), sp.cell(5, 5), sp.cell(1, 16), sp.cell(5, 9),
                   sp.cell(5, 9), sp.cell(2, 7)]
    out = sp.paint(w, trail, pos, 1)
    changed = np.argwhere(out != w)
    assert sorted(map(tuple, changed)) == [(0, 0, 7, 5), (0, 0, 10, 7)] and (out[out != w] == 6).all()
    can = sp.paintable(trail, pos, 1)
    assert can[0, 0, 6, 6] and can[0, 0, 8, 6] and can[0, 0, 9, 7] and can[0, 0, 10, 3] and int(can.sum()) == 6
    assert not can[0, 1].any() and np.array_equal(out[0, 1], w[0, 1])           # roles = 1: window 1 is left alone
    # a print in the padding: the tracker's window row 4 is map row -1, which no trail entry can name; column -1 likewise
    edge = _pos((0, 0), (0, 3))
    we = sp.windows_of(grid, edge)
    te = sp.new_trail(1, 3)
    te[0, 1] = [sp.cell(0, 3), sp.cell(0, 2), sp.cell(0, 1), E]
    oe = sp.paint(we, te, edge, 3)
    assert (oe[0, 0, :6] == 1).all() and (oe[0, 0, :, :6] == 1).all() and oe[0, 0, 6, 7] == 6 and oe[0, 0, 6, 8] == 6
    # which cells can be painted depends on positions and trail alone; which are painted on the window reading 0
    zeros = np.zeros_like(w)
    assert np.array_equal(sp.paint(zeros, trail, pos, 1) == 6, can)
    assert np.array_equal(sp.paint(np.full_like(w, 5), trail, pos, 3), np.full_like(w, 5))
    assert np.array_equal(sp.paint(zeros, trail, pos, 1, value=9) == 9, can)
    wf = w.astype(np.float32)
    assert np.array_equal(sp.paint(wf, trail, pos, 1), out.astype(np.float32)) and sp.paint(wf, trail, pos, 1).dtype == np.float32


def test_roles_choose_the_window():
    pos = _pos((8, 8), (8, 10))
    w = sp.windows_of(_open_map(), pos)
    trail = sp.new_trail(1, 2)
    trail[0, 0] = [sp.cell(8, 8), sp.cell(9, 8), E]               # the tracker came from below
    trail[0, 1] = [sp.cell(8, 10), sp.cell(8, 11), sp.cell(8, 12)]  # the target from the right
    for roles in (1, 2, 3):
        out = sp.paint(w, trail, pos, roles)
        assert ((out[0, 0] == 6).sum(), (out[0, 1] == 6).sum()) == ((2, 0), (0, 1), (2, 1))[roles - 1]
    out = sp.paint(w, trail, pos, 3)
    assert out[0, 0, 6, 9] == 6 and out[0, 0, 6, 10] == 6 and out[0, 1, 7, 4] == 6


def test_record_rule_case_by_case():
    a, b, c, d = sp.cell(5, 3), sp.cell(4, 3), sp.cell(3, 3), sp.cell(2, 3)
    trail = np.array([[[b, c, d, E], [E, E, E, E]], [[a, b, E, c], [a, a, a, a]]], np.uint16)
    pos = np.array([[(5, 3), (5, 3)], [(5, 3), (6, 3)]])
    n = sp.cell(6, 3)
    assert np.array_equal(sp.record(trail, pos, sp.PEEK), trail) and np.array_equal(sp.record(trail, pos, sp.PEEK, [1, 1]), trail)
    # a move shifts (an EMPTY entry 0 shifts in like any other), a stay / bump changes nothing
    assert sp.record(trail, pos, sp.STEP).tolist() == [[[a, b, c, d], [a, E, E, E]], [[a, b, E, c], [n, a, a, a]]]
    assert sp.record(trail, pos, sp.STEP, [0, 0]).tolist() == sp.record(trail, pos, sp.STEP).tolist()
    # done restarts that env's rows from the current cell; 255 is as set as 1
    assert sp.record(trail, pos, sp.STEP, [1, 0]).tolist() == [[[a, E, E, E], [a, E, E, E]], [[a, b, E, c], [n, a, a, a]]]
    assert sp.record(trail, pos, sp.STEP, [0, 255]).tolist() == [[[a, b, c, d], [a, E, E, E]], [[a, E, E, E], [n, E, E, E]]]
    # BEGIN does not look at done
    for done in (None, [0, 0], [1, 0]):
        assert sp.record(trail, pos, sp.BEGIN, done).tolist() == [[[a, E, E, E], [a, E, E, E]], [[a, E, E, E], [n, E, E, E]]]
    assert sp.record(trail, pos, sp.STEP).dtype == np.uint16


@pytest.mark.parametrize("k", [1, 2, 4, 63])
def test_after_k_plus_one_moves_the_first_print_is_gone(k):
    trail = sp.new_trail(1, k)
    walk = [(10, c) for c in range(1, k + 4)]
    trail = sp.record(trail, _pos(walk[0], (0, 0)), sp.BEGIN)
    for i, at in enumerate(walk[1:], 1):
        trail = sp.record(trail, _pos(at, (0, 0)), sp.STEP)
        prints = [int(x) for x in trail[0, 0, 1:] if x != E]
        assert prints == [sp.cell(*walk[j]) for j in range(i - 1, max(i - 1 - k, -1), -1)], (k, i)
        assert (sp.cell(*walk[0]) in prints) == (i <= k)
    assert (trail[0, 1] == [sp.cell(0, 0)] + [E] * k).all()        # the target never moved


@pytest.mark.parametrize("k", [1, 3, 5, 8])
def test_a_target_walking_straight_away_from_a_standing_tracker(k):
    """Empty map, the tracker standing at (10, 4), the target next to it at (10, 5); the trail starts all EMPTY and every step is
    a STEP call. After m steps to the right the target stands on column 5 + m and has left prints on columns 6 .. 4 + m, the
    newest K of them kept (its start cell was never recorded: the first call only filled entry 0). The tracker's window reaches
    column 10, so window 0 shows exactly min(m - 1, K, 5) cells of 6 for m = 1 .. 6 (past that the target's newest prints lie
    outside the window as well); window 1 shows none under roles = 1, and the tracker, which never moves, leaves none at all."""
    grid = _open_map(30)
    trail = sp.new_trail(1, k)
    for m in range(1, 7):
        pos = _pos((10, 4), (10, 5 + m))
        w = sp.windows_of(grid, pos)
        out, trail = sp.call(w, trail, pos, sp.STEP, roles=1)
        assert int((out[0, 0] == 6).sum()) == min(m - 1, k, 5) == int((out != w).sum()), (k, m)
        assert np.array_equal(out[0, 1], w[0, 1]) and (trail[0, 0, 1:] == E).all()
        both, _ = sp.call(w, trail, pos, sp.PEEK, roles=3)
        assert np.array_equal(both, out)


# -- csrc/atr_footprint_rule.h through a sanitizer-built host program ------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the host program needs g++"
    exe = str(tmp_path_factory.mktemp("footprints_host") / "footprints_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "active_tracking_rl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "footprints_host.cpp"), "-o", exe])
    return exe


def _rc(cell):
    return (cell & 255, cell >> 8)


def test_host_program_record_table_equals_the_spec(host_program):
    rows = subprocess.check_output([host_program, "record"], text=True).split("\n")
    assert rows[-1] == "" and len(rows) - 1 == 3 * 4 * 4 * 6
    kinds = set()
    for row in rows[:-1]:
        f = row.split()
        assert f[0] == "rec" and len(f) == 12
        mode, done, cur = int(f[1]), None if f[2] == "x" else [int(f[2])], int(f[3])
        old, new = [int(x) for x in f[4:8]], [int(x) for x in f[8:12]]
        want = sp.record(np.array([[old, old]], np.uint16), [[_rc(cur), _rc(cur)]], mode, done)
        assert want[0, 0].tolist() == new == want[0, 1].tolist(), row
        kinds.add((mode, f[2], new == old, new[1:] == [E] * 3))
    assert len(kinds) >= 12


def test_host_program_paint_table_equals_the_spec(host_program):
    rows = subprocess.check_output([host_program, "paint"], text=True).split("\n")
    assert rows[-1] == "" and len(rows) > 6 * 100
    seen = unseen = 0
    for row in rows[:-1]:
        tag, pr, viewer, got = row.split()
        assert tag == "cell"
        pr, viewer, got = int(pr), int(viewer), int(got)
        trail = np.array([[[E, E], [E, pr]]], np.uint16)
        can = sp.paintable(trail, [[_rc(viewer), (0, 0)]], 1)
        want = np.flatnonzero(can[0, 0].reshape(-1))
        assert (want.tolist() == [got]) if got >= 0 else (want.size == 0), row
        assert not can[0, 1].any()
        seen += got >= 0
        unseen += got < 0
    assert seen > 400 and unseen > 400        # (both verdicts occur in plenty: the table is no one-sided check)
    rows = subprocess.check_output([host_program, "pos"], text=True).split("\n")
    assert len(rows) - 1 == 10
    for row in rows[:-1]:
        tag, word, p, got = row.split()
        word, p = int(word), int(p)
        r, c = ((word & 255, word >> 8 & 255), (word >> 16 & 255, word >> 24))[p]
        assert tag == "pos" and int(got) == sp.cell(r, c), row


# -- the ABI -----------------------------------------------------------------------------------------------------------------------

def _fp_header():
    """include/atr_footprints.h without comments and preprocessor lines."""
    txt = open(os.path.join(ROOT, "include", "atr_footprints.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    return "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", txt).split("\n") if not ln.lstrip().startswith("#"))


def test_header_prototypes_and_exports_agree():
    """The header's one function is exported by the built library and bound by FOOTPRINT_PROTOTYPES with the header's parameter
    count and classes; the constants are the module's and the spec's; the source and both headers are in the build, the kernel
    under its no-scratch check; the tables that were there before are what they were; the policy table and the env's symbol list
    do not know the entry point."""
    from active_tracking_rl_amd import build, footprints, fused, occlusion, vec_env
    build.build()
    assert os.path.join("..", "..", "include", "atr_footprints.h") in build.HEADERS and "atr_footprint_rule.h" in build.HEADERS
    assert "footprints_hip.hip" in build.SOURCES and build.NO_SCRATCH_FOOTPRINTS == {"footprints_hip.hip": "k_footprints"}
    assert build.NO_SCRATCH_FOV == {"fov_hip.hip": "k_fov"} and build.NO_SCRATCH_OCCLUSION == {"occlusion_hip.hip": "k_occlude"}
    assert build.NO_SCRATCH == {"track2d_hip.hip": "k_gru_step"}
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    funcs = _header_functions(_fp_header())
    assert sorted(funcs) == ["atr_footprint_windows"] == sorted(footprints.FOOTPRINT_PROTOTYPES)
    assert sorted(funcs) == _header_symbols("atr_footprints.h", "atr_") and _header_structs(_fp_header()) == {}
    for name, (res, params) in funcs.items():
        assert hasattr(lib, name), name
        restype, argtypes = footprints.FOOTPRINT_PROTOTYPES[name]
        assert _py_class(restype) == res == ctypes.c_int, name
        assert len(argtypes) == len(params) == 12, name
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _py_class(a) == c, (name, i)
    params = funcs["atr_footprint_windows"][1]
    assert [i for i, c in enumerate(params) if c is ctypes.c_longlong] == [3, 4]
    assert [i for i, c in enumerate(params) if c == "ptr"] == [0, 1, 5, 9, 11]
    assert "atr_footprint_windows" not in fused.ATR_PROTOTYPES and "atr_footprint_windows" not in vec_env.ABI_SYMBOLS
    assert footprints.window_grid is occlusion.window_grid
    txt = open(os.path.join(ROOT, "include", "atr_footprints.h")).read()
    const = lambda name: int(re.search(r"#define\s+ATR_FOOTPRINT_%s\s+(\d+)" % name, txt).group(1))
    assert [const(n) for n in ("WINDOW", "SIDE", "CENTRE", "EMPTY", "VALUE", "MAX_K", "PEEK", "STEP", "BEGIN")] == \
        [footprints.WINDOW, footprints.SIDE, sp.CENTRE, footprints.EMPTY, footprints.VALUE, footprints.MAX_K, footprints.PEEK,
         footprints.STEP, footprints.BEGIN] == \
        [sp.WINDOW, sp.SIDE, 6, sp.EMPTY, sp.VALUE, sp.MAX_K, sp.PEEK, sp.STEP, sp.BEGIN] == [169, 13, 6, 0xFFFF, 6, 63, 0, 1, 2]
    assert footprints.ROLES == {"tracker": 1, "target": 2, "both": 3}
    rule = open(os.path.join(ROOT, "active_tracking_rl_amd", "csrc", "atr_footprint_rule.h")).read()
    assert "hip_runtime" not in rule
    src = open(os.path.join(ROOT, "active_tracking_rl_amd", "csrc", "footprints_hip.hip")).read()
    assert "static_assert" in src and "atr_footprint_rule.h" in src and "__shared__" not in src and "atomic" not in src


def test_binding_checks_status_and_refuses_before_the_handle():
    """lib() binds the table with an errcheck that raises with the entry point's name and the library's text; every handle-free
    refusal of the header is reached with h = NULL and one bad argument, in the header's order; all-good arguments with h = NULL
    give the null-handle text (this test runs without a device, on addresses that are never read)."""
    from active_tracking_rl_amd import build, footprints
    build.build()
    L = footprints.lib()
    for name, (restype, argtypes) in footprints.FOOTPRINT_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
        assert f.errcheck(0, None, ()) == 0
        with pytest.raises(RuntimeError, match=r"^%s failed \(-1\): " % name):
            f.errcheck(-1, None, ())
    p, q = 1 << 20, 1 << 24        # any non-null, aligned addresses: a refused call never reads them
    ok = dict(h=None, obs=p, is_u8=True, se=338, sp=169, trail=q, k=4, roles=1, mode=1, done=q + 4096, value=6, stream=None)
    cases = [(dict(obs=0), "null pointer"), (dict(trail=0), "null pointer"), (dict(obs=0, trail=0, k=0), "null pointer"),
             (dict(k=0), r"k 0 outside 1 \.\. 63"), (dict(k=64), r"k 64 outside 1 \.\. 63"), (dict(k=-1, roles=0), r"k -1 outside"),
             (dict(roles=0), r"roles 0 outside 1 \.\. 3"), (dict(roles=4), r"roles 4 outside 1 \.\. 3"),
             (dict(roles=-1, mode=3), r"roles -1 outside"),
             (dict(mode=-1), r"mode -1 outside 0 \.\. 2"), (dict(mode=3), r"mode 3 outside 0 \.\. 2"),
             (dict(mode=3, value=256), r"mode 3 outside"),
             (dict(value=-1), r"value -1 outside 0 \.\. 255"), (dict(value=256), r"value 256 outside 0 \.\. 255"),
             (dict(value=256, se=-1), r"value 256 outside"),
             (dict(se=-338), "negative element stride"), (dict(sp=-1), "negative element stride"),
             (dict(sp=-1, obs=p + 2, is_u8=False), "negative element stride"),
             (dict(obs=p + 2, is_u8=False), "not 4-byte aligned"), (dict(obs=p + 1, is_u8=False, trail=q + 1), "not 4-byte aligned"),
             (dict(trail=q + 1), "not 2-byte aligned"), (dict(trail=q + 3, obs=p + 3), "not 2-byte aligned"),
             (dict(), "null handle"), (dict(is_u8=False, done=0, mode=0, roles=3, k=63, value=0, se=0, sp=0), "null handle"),
             (dict(obs=p + 3, k=1, mode=2, value=255), "null handle")]
    for change, text in cases:
        with pytest.raises(RuntimeError, match=r"^atr_footprint_windows failed \(-1\): atr_footprint_windows: .*%s" % text):
            footprints.footprint_windows(**dict(ok, **change))


def test_the_tensor_checks():
    """mark_ refuses a host tensor (there is no host path); count_of and roles_of take what the header allows and nothing else."""
    import torch
    from active_tracking_rl_amd import footprints
    with pytest.raises(RuntimeError, match="there is no host path"):
        footprints.mark_(torch.zeros(2, 2, 13, 13, dtype=torch.uint8), torch.zeros(2, 2, 5, dtype=torch.uint16), None, 1)
    with pytest.raises(RuntimeError, match="there is no host path"):
        footprints.mark_(np.zeros((2, 2, 13, 13), np.uint8), np.zeros((2, 2, 5), np.uint16), None, 1)
    assert [footprints.count_of(k) for k in (1, 4, 63)] == [1, 4, 63]
    for bad in (0, 64, -1, True, 4.0, "4", None, (4,)):
        with pytest.raises(ValueError, match="footprints must be a trail length K in 1 .. 63"):
            footprints.count_of(bad)
    assert [footprints.roles_of(w) for w in ("tracker", "target", "both")] == [1, 2, 3]
    for bad in ("Tracker", "all", 1, None):
        with pytest.raises(ValueError, match="footprints_for must be one of"):
            footprints.roles_of(bad)
    t = footprints.new_trail(3, 4, "cpu")
    assert t.dtype == torch.uint16 and tuple(t.shape) == (3, 2, 5) and (t.numpy() == E).all() and t.is_contiguous()


# -- flags and refusals ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("script", ["main.py", "gym_eval.py"])
def test_both_parsers_list_the_flags(script):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0
    for flag in ("--footprints K", "--footprints-for WHO"):
        assert flag in r.stdout, flag
    assert "default: tracker" in " ".join(r.stdout.split())


@pytest.mark.parametrize("script,argv,text", [
    ("main.py", ["--footprints", "4", "--tracking-stats"], "--tracking-stats / --sight-stats"),
    ("main.py", ["--footprints", "4", "--sight-stats"], "--tracking-stats / --sight-stats"),
    ("main.py", ["--footprints", "4", "--render"], "cannot be combined with --render"),
    ("main.py", ["--footprints-for", "both"], "--footprints-for needs --footprints"),
    ("main.py", ["--footprints-for", "tracker"], "--footprints-for needs --footprints"),
    ("main.py", ["--footprints", "0"], "invalid choice"),
    ("main.py", ["--footprints", "64"], "invalid choice"),
    ("main.py", ["--footprints", "4", "--footprints-for", "all"], "invalid choice"),
    ("main.py", ["--footprints", "4", "--footprints-for", "both", "--env-base", "Track2D-BlockPartialNav-v0"],
     "the scripted target of --env-base Track2D-BlockPartialNav-v0 reads no window"),
    ("main.py", ["--footprints", "4", "--footprints-for", "target", "--env", "Track2D-MazePartialRam-v0"],
     "the scripted target of --env Track2D-MazePartialRam-v0 reads no window"),
    ("gym_eval.py", ["--footprints", "4", "--footprints-for", "both", "--env", "Track2D-BlockPartialNav-v0"],
     "the scripted target of Track2D-BlockPartialNav-v0 reads no window"),
    ("gym_eval.py", ["--footprints", "4", "--render"], "cannot be combined with --render"),
    ("gym_eval.py", ["--footprints-for", "target"], "--footprints-for needs --footprints"),
    ("gym_eval.py", ["--footprints", "64"], "invalid choice"),
])
def test_parsers_refuse(script, argv, text):
    """The refused combinations end the command in the parser, before a device is looked for (this test runs without one)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and text in r.stderr, r.stderr[-400:]


def test_default_args_and_create_env_refusals():
    """train.default_args carries the two settings; create_env refuses --footprints on a whole-map id, with traces and on the
    batched rng='numpy' envs, and --footprints-for alone; VecEnv and Track2DEnv refuse a whole-map id, traces, a bad K or role,
    and a painted window for a scripted target themselves — all before a device is touched (this test runs without one)."""
    from active_tracking_rl_amd import environment
    from active_tracking_rl_amd.train import default_args
    d = default_args()
    assert d.footprints is None and d.footprints_for == "tracker" and default_args(footprints=4).footprints == 4
    args = argparse.Namespace(footprints=4, footprints_for="tracker", stack_frames=1, seed=1, gpu_ids=[0])
    for n in (4, 1):
        with pytest.raises(ValueError, match="--footprints needs the 13 x 13 windows"):
            environment.create_env("Track2D-BlockFullPZR-v0", args, num_envs=n)
        with pytest.raises(NotImplementedError, match="--footprints with episode traces"):
            environment.create_env(PARTIAL, args, num_envs=n, traces=True)
    for rng in ("numpy", "numpy-device"):
        with pytest.raises(NotImplementedError, match="--footprints is not wired to the batched rng='numpy' envs"):
            environment.create_env(PARTIAL, args, num_envs=4, rng=rng)
    with pytest.raises(ValueError, match="--footprints-for needs --footprints"):
        environment.create_env(PARTIAL, argparse.Namespace(footprints=None, footprints_for="both", stack_frames=1, seed=1,
                                                           gpu_ids=[0]), num_envs=4)
    with pytest.raises(ValueError, match="footprints=4 needs the 13 x 13 windows"):
        environment.VecEnv("Track2D-MazeFullNav-v0", 4, footprints=4)
    with pytest.raises(ValueError, match="footprints=4 needs the 13 x 13 windows"):
        environment.Track2DEnv("Track2D-BlockFullPZR-v0", footprints=4)
    with pytest.raises(NotImplementedError, match="traces=True"):
        environment.VecEnv(PARTIAL, 4, footprints=4, traces=True, auto_reset=False)
    with pytest.raises(NotImplementedError, match="traces=True"):
        environment.Track2DEnv(PARTIAL, footprints=4, traces=True)
    for bad in (0, 64, True, "4"):
        with pytest.raises(ValueError, match="footprints must be a trail length K"):
            environment.VecEnv(PARTIAL, 4, footprints=bad)
    with pytest.raises(ValueError, match="footprints_for must be one of"):
        environment.VecEnv(PARTIAL, 4, footprints=4, footprints_for="all")
    with pytest.raises(ValueError, match="footprints_for='both' needs footprints=K"):
        environment.VecEnv(PARTIAL, 4, footprints_for="both")
    for env_id in ("Track2D-BlockPartialRam-v0", "Track2D-BlockPartialNav-v0", "Track2D-MazePartialRPF-v0"):
        for who in ("target", "both"):
            with pytest.raises(ValueError, match="scripted"):
                environment.VecEnv(env_id, 4, footprints=4, footprints_for=who)
            with pytest.raises(ValueError, match="scripted"):
                environment.Track2DEnv(env_id, footprints=4, footprints_for=who, rng="numpy" if "RPF" not in env_id else "philox")


def test_without_the_option_nothing_is_launched(monkeypatch):
    """VecEnv._mark with footprints off hands the tensor back untouched and never reaches the binding; with it on it hands the
    binding the windows, the env's trail, the core, the mode, the core's done where the core auto-resets, and the env's roles;
    fused_step_out declines."""
    from active_tracking_rl_amd import environment, footprints

    calls = []
    monkeypatch.setattr(footprints, "mark_", lambda *a: calls.append(a))
    env = object.__new__(environment.VecEnv)
    env.footprints = None
    obs = object()
    assert env._mark(obs, 2) is obs and env._mark(obs, 1, "done") is obs and env._mark(obs, 0) is obs
    assert calls == []

    class Core(object):
        auto_reset = True
        supports_u8 = True
    env.footprints, env._trail, env._footprint_roles, env.core = 4, "trail", 3, Core()
    assert env._mark(obs, 2) is obs and env._mark(obs, 1, "done") is obs and env._mark(obs, 0) is obs
    Core.auto_reset = False
    assert env._mark(obs, 1, "done") is obs
    assert calls == [(obs, "trail", env.core, 2, None, 3), (obs, "trail", env.core, 1, "done", 3), (obs, "trail", env.core, 0, None, 3),
                     (obs, "trail", env.core, 1, None, 3)]
    env.stack_frames, env.rescale, env.occlusion, env.fov, env.obs_u8 = 1, False, False, None, True
    assert env.fused_step_out(("o", "r", "d")) is None
