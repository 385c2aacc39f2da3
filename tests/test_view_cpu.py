"""Player views (include/atr_view.h) without a device: the numpy spec's two forms against each other, the header's macros and the
golden palette, the rule's properties, csrc/atr_view_rule.h through a sanitizer-built host program, the ABI, every handle-free
refusal in the header's order, the flags and the refusals of the layers."""
import argparse
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import view_spec as sp
from conftest import ROOT
from test_abi_cpu import _header_functions, _header_structs, _header_symbols, _py_class

PARTIAL = "Track2D-BlockPartialPZR-v0"
NAV = "Track2D-BlockPartialNav-v0"
VALUES = np.array([0, 0, 0, 1, 1, 2, 4, 5, 5, 6, 7, 8, 3, 9, 255], np.uint8)


def _frames(n, seed=0, steps=7):
    """n oracle envs (Block and Maze in turn, so that sides 82 and 81 both occur) stepped a few times: maps [n, 82, 82], side,
    pos [n, 2, 2] and the windows [n, 2, 13, 13] the oracle hands out (no pass on)."""
    from oracle import oracle as orc
    rng = np.random.RandomState(seed)
    maps, side, pos, wins = np.zeros((n, 82, 82), np.uint8), np.zeros(n, np.int32), np.zeros((n, 2, 2), np.int32), []
    for i in range(n):
        env = orc.OracleEnv(("Block", "Maze")[i % 2], "PZR", 0, 500, orc.RNG_PHILOX, 5 + seed, i)
        env.reset()
        for _ in range(steps):
            env.step(rng.randint(0, 4, 2))
        s = env.side
        maps[i, :s, :s], side[i], pos[i] = env.maze, s, env.state()["pos"]
        wins.append(env.obs())
    return maps, side, pos, np.stack(wins)


@pytest.fixture(scope="module")
def frames():
    return _frames(6)


def _random_windows(n, seed):
    return VALUES[np.random.RandomState(seed).randint(0, len(VALUES), (n, 2, 13, 13))]


def test_loops_and_arrays_state_one_rule(frames):
    """frame_cells / frame_rgb (loops) and view_cells / view_rgb (arrays) give the same bytes: oracle windows and random ones with
    every value, both viewers, every `turned`, facings over 0 .. 3 and NONE, byte and float windows with 0.5 and NaN."""
    maps, side, pos, wins = frames
    n = len(side)
    facing = np.array([[0, 1], [2, 3], [sp.NONE, 0], [3, sp.NONE], [1, 2], [7, 200]], np.uint8)[:n]
    fl = _random_windows(n, 3).astype(np.float32)
    fl[:, :, 2, 3], fl[:, :, 9, 1] = 0.5, np.nan
    for k, windows in enumerate((wins, _random_windows(n, 1), fl)):
        for viewer in (0, 1):
            for turned in range(4):
                cells, wc = sp.view_cells(maps, side, pos, windows, facing, turned, viewer)
                assert cells.dtype == wc.dtype == np.uint8 and cells.shape == (n, 82, 82) and wc.shape == (n, 2, 13, 13)
                for i in range(n):
                    c1, w1 = sp.frame_cells(maps[i], side[i], pos[i], windows[i], facing[i], turned, viewer)
                    assert np.array_equal(c1, cells[i]) and np.array_equal(w1, wc[i]), (k, viewer, turned, i)
                if k == 2:
                    assert (wc[:, :, 2, 3] == 15).all() and (wc[:, :, 9, 1] == 15).all()
    cells, wc = sp.view_cells(maps, side, pos, _random_windows(n, 1), facing, 1, 0)
    for scale, pitch in ((1, 736), (2, 1456), (3, 2192)):
        img = sp.view_rgb(cells[:2], wc[:2], scale, pitch)
        for i in range(2):
            assert np.array_equal(img[i], sp.frame_rgb(cells[i], wc[i], scale, pitch)), (scale, i)
        assert not img[:, :, 726 * scale:].any()


def _macros():
    txt = open(os.path.join(ROOT, "include", "atr_view.h")).read()
    return {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+ATR_VIEW_(\w+)\s+(0[xX][0-9A-Fa-f]+|\d+)", txt)}


def test_header_macros_spec_and_golden_palette_agree():
    """The header's constants are the spec's and the module's; its colours are the spec's; 0, 1, 2, 4 and 6 are the reference's
    palette as recorded in tests/golden/traces.npz; all colours that can appear are pairwise distinct."""
    from active_tracking_rl_amd import view
    m = _macros()
    assert [m[k] for k in ("UNKNOWN", "OUTSIDE", "HIDDEN", "BAND_HIDDEN", "BAND_BEYOND", "CELLS_H", "CELLS_W", "WINDOW", "MAX_SCALE")] == \
        [sp.UNKNOWN, sp.OUTSIDE, sp.HIDDEN, sp.BAND_HIDDEN, sp.BAND_BEYOND, sp.CELLS_H, sp.CELLS_W, sp.WINDOW, 8] == \
        [view.UNKNOWN, view.OUTSIDE, view.HIDDEN, view.BAND_HIDDEN, view.BAND_BEYOND, view.CELLS_H, view.CELLS_W, view.WINDOW,
         view.MAX_SCALE] == [15, 255, 5, 16, 32, 82, 242, 169, 8]
    names = {0: "FREE", 1: "WALL", 2: "TRACKER", 4: "TARGET", 5: "UNSEEN", 6: "PRINT", 7: "MEM_WALL", 8: "MEM_FREE", 15: "UNKNOWN"}
    assert {v: m["RGB_" + n] for v, n in names.items()} == sp.RGB == \
        {0: 0xFFFFFF, 1: 0x000000, 2: 0xFF0000, 4: 0x0000FF, 5: 0x505050, 6: 0x00FFFF, 7: 0x303060, 8: 0xC0C0E8, 15: 0xFF00FF}
    assert m["RGB_BACKGROUND"] == sp.BACKGROUND == 0x808080
    g = np.load(os.path.join(ROOT, "tests", "golden", "traces.npz"))
    golden = {int(v): tuple(int(x) for x in rgb) for v, rgb in zip(g["palette_values"], g["palette"])}
    assert sorted(golden) == [0, 1, 2, 4, 6]
    for v, rgb in golden.items():
        assert sp.channels(sp.RGB[v]) == rgb == sp.code_rgb(v) == tuple(sp.PALETTE[v]), v
    # the band arithmetic, written out
    assert sp.code_rgb(16 + 0) == (191, 191, 191) and sp.code_rgb(16 + 1) == (64, 64, 64)
    assert sp.code_rgb(16 + 2) == tuple((c + 128) >> 1 for c in golden[2]) == (64, 64, 191)
    assert sp.code_rgb(32 + 4) == tuple((c + 384) >> 2 for c in golden[4]) == (159, 96, 96)
    assert sp.code_rgb(32 + 0) == (159, 159, 159) and sp.code_rgb(32 + 1) == (96, 96, 96)
    codes = [0, 1, 2, 4, 5, 6, 7, 8, 15] + [16 + t for t in (0, 1, 2, 4)] + [32 + t for t in (0, 1, 2, 4)] + [255]
    colours = [sp.code_rgb(c) for c in codes]
    assert len(set(colours)) == len(codes) == 18
    for c in range(256):        # everything that is no code is the background
        if c not in codes:
            assert sp.code_rgb(c) == (128, 128, 128), c


def test_without_a_pass_the_window_is_band_zero_and_true(frames):
    """Windows straight from the oracle: every in-window map cell is in band 0 and equals the truth, except the viewer's own cell
    when the players share it, which shows the viewer's value; everything else is 32 + T or 255."""
    maps, side, pos, wins = frames
    from oracle import oracle as orc
    pos, wins = pos.copy(), wins.copy()
    pos[1, 1] = pos[1, 0]                           # one co-located pair, its windows from the oracle as well
    env = orc.OracleEnv("Maze", "PZR", 0, 500, orc.RNG_PHILOX, 5, 1)
    env.reset()
    env.inject(maps[1, :side[1], :side[1]], pos[1])
    wins[1] = env.obs()
    assert wins[1, 0, 6, 6] == 2 and wins[1, 1, 6, 6] == 4 and not (wins[1, 0] == 4).any() and not (wins[1, 1] == 2).any()
    for viewer in (0, 1):
        cells, wc = sp.view_cells(maps, side, pos, wins, None, 0, viewer)
        assert np.array_equal(wc, wins)
        seen = 0
        for i in range(len(side)):
            for r in range(82):
                for c in range(82):
                    if r >= side[i] or c >= side[i]:
                        assert cells[i, r, c] == 255
                        continue
                    t = sp.truth(maps[i], side[i], pos[i], r, c)
                    if max(abs(r - pos[i, viewer, 0]), abs(c - pos[i, viewer, 1])) > 6:
                        assert cells[i, r, c] == 32 + t
                    elif (r, c) == tuple(pos[i, viewer]):
                        assert cells[i, r, c] == (2, 4)[viewer]
                        seen += 1
                    else:
                        assert cells[i, r, c] == t, (viewer, i, r, c)
                        seen += 1
        assert seen > 100 * len(side)


def test_an_all_hidden_window_shows_the_dimmed_truth(frames):
    maps, side, pos, wins = frames
    hidden = np.full_like(wins, 5)
    for viewer in (0, 1):
        cells, wc = sp.view_cells(maps, side, pos, hidden, None, 0, viewer)
        assert (wc == 5).all()
        for i in range(len(side)):
            pr, pc = pos[i, viewer]
            for r in range(max(0, pr - 6), min(side[i], pr + 7)):
                for c in range(max(0, pc - 6), min(side[i], pc + 7)):
                    assert cells[i, r, c] == 16 + sp.truth(maps[i], side[i], pos[i], r, c)
        assert not ((cells < 16) | ((cells >= 48) & (cells != 255))).any()


def test_projecting_a_turned_window_equals_projecting_the_absolute_one(frames):
    """E[cell] = W[src_cell(h, cell)] (the egocentric pass): the map panel of (E, turned) is the map panel of (W, not turned), for
    h = 0 .. 3 and NONE; the window panel keeps E."""
    import ego_spec
    maps, side, pos, _ = frames
    n = len(side)
    w_abs = _random_windows(n, 9)
    for viewer in (0, 1):
        want, _ = sp.view_cells(maps, side, pos, w_abs, None, 0, viewer)
        for facing in (0, 1, 2, 3, sp.NONE):
            h = sp.heading_of(facing)
            turned = w_abs.copy()
            for e in range(n):                      # (the egocentric pass's own spec makes the turned window)
                turned[e, viewer] = ego_spec.view(w_abs[e, viewer], facing)
            fac = np.full((n, 2), facing, np.uint8)
            fac[:, 1 - viewer] = 1                  # (the other player's facing is not read)
            got, wc = sp.view_cells(maps, side, pos, turned, fac, 1 << viewer, viewer)
            assert np.array_equal(got, want), (viewer, facing)
            assert np.array_equal(wc, sp.window_codes(turned))
            if h != 0:
                assert not np.array_equal(sp.view_cells(maps, side, pos, turned, fac, 0, viewer)[0], want)


def test_unknown_values_become_fifteen(frames):
    maps, side, pos, _ = frames
    n = len(side)
    for bad in (3, 9, 10, 14, 16, 200, 255):
        cells, wc = sp.view_cells(maps, side, pos, np.full((n, 2, 13, 13), bad, np.uint8), None, 0, 0)
        assert (wc == 15).all() and set(np.unique(cells[cells < 32])) == {15} and (cells == 15).sum() >= 49 * n
    for bad in (0.5, np.nan, -1.0, 1e-3, np.inf, 4.0000005):
        _, wc = sp.view_cells(maps, side, pos, np.full((n, 2, 13, 13), bad, np.float32), None, 0, 1)
        assert (wc == 15).all(), bad
    assert [sp.known(v) for v in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 255)] == [0, 1, 2, 15, 4, 5, 6, 7, 8, 15, 15, 15]
    assert sp.known(np.float32(-0.0)) == 0 and sp.known(np.float32(7.0)) == 7


# -- csrc/atr_view_rule.h through a sanitizer-built host program -------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the host program needs g++"
    exe = str(tmp_path_factory.mktemp("view_host") / "view_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "active_tracking_rl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "view_host.cpp"), "-o", exe])
    return exe


def test_host_program_codes_equal_the_spec(host_program):
    rows = [r.split() for r in subprocess.check_output([host_program, "codes"], text=True).split("\n")[:-1]]
    kn = [r for r in rows if r[0] == "known"]
    assert [int(r[1]) for r in kn] == list(range(-2, 301))
    for r in kn:
        assert int(r[2]) == sp.known(int(r[1])), r
    kf = [r for r in rows if r[0] == "knownf"]
    assert len(kf) == 20
    for r in kf:
        assert int(r[2]) == sp.known(np.float32(float.fromhex(r[1]))), r
    assert sum(int(r[2]) == 15 for r in kf) == 11
    tr = [[int(x) for x in r[1:]] for r in rows if r[0] == "truth"]
    assert len(tr) == 8
    for bit, a, b, t in tr:
        assert t == (4 if b else 2 if a else bit)
    cd = [[int(x) for x in r[1:]] for r in rows if r[0] == "code"]
    assert len(cd) == 2 * 4 * 16 and len(rows) == len(kn) + len(kf) + 8 + len(cd)
    seen = set()
    for inside, t, w, code in cd:
        want = 32 + t if not inside else 16 + t if w == 5 else w
        assert code == want, (inside, t, w)
        seen.add((inside, t, w))
    assert seen == {(i, t, w) for i in (0, 1) for t in (0, 1, 2, 4) for w in (0, 1, 2, 4, 5, 6, 7, 8, 15)}


def test_host_program_colours_equal_the_spec(host_program):
    rows = [r.split() for r in subprocess.check_output([host_program, "colours"], text=True).split("\n")[:-1]]
    assert [int(r[1]) for r in rows] == list(range(256)) and all(r[0] == "rgb" for r in rows)
    for r in rows:
        assert sp.channels(int(r[2], 16)) == sp.code_rgb(int(r[1])), r


def test_host_program_unturn_is_the_egocentric_cell_map(host_program):
    rows = [r.split() for r in subprocess.check_output([host_program, "unturn"], text=True).split("\n")[:-1]]
    assert len(rows) == 2 * 4 * 169
    for _, turned, h, cell, dst in rows:
        turned, h, cell, dst = int(turned), int(h), int(cell), int(dst)
        assert dst == (sp.src_cell(h, cell) if turned else cell)
    import ego_spec
    for h in range(4):
        for i in range(169):
            r, c = ego_spec.source(h, i // 13, i % 13)
            assert r * 13 + c == sp.src_cell(h, i)


# -- the ABI -----------------------------------------------------------------------------------------------------------------------

def _vw_header():
    """include/atr_view.h without comments and preprocessor lines."""
    txt = open(os.path.join(ROOT, "include", "atr_view.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    return "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", txt).split("\n") if not ln.lstrip().startswith("#"))


def test_header_prototypes_and_exports_agree():
    """The header's two functions are exported by the built library and bound by VIEW_PROTOTYPES with the header's parameter
    counts and classes; the source and both headers are in the build, the kernels under their no-scratch check; the pinned
    headers and tables do not know the entry points; the rule header has no HIP dependence."""
    from active_tracking_rl_amd import build, fused, vec_env, view
    build.build()
    assert os.path.join("..", "..", "include", "atr_view.h") in build.HEADERS and "atr_view_rule.h" in build.HEADERS
    assert "view_hip.hip" in build.SOURCES and build.NO_SCRATCH_VIEW == {"view_hip.hip": "k_view"}
    assert build.NO_SCRATCH_NOISE == {"noise_hip.hip": "k_noise"} and build.NO_SCRATCH_RENDER == {"render_hip.hip": "k_"}
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    funcs = _header_functions(_vw_header())
    assert sorted(funcs) == ["atr_view_cells", "atr_view_rgb"] == sorted(view.VIEW_PROTOTYPES)
    assert sorted(funcs) == _header_symbols("atr_view.h", "atr_") and _header_structs(_vw_header()) == {}
    for name, (res, params) in funcs.items():
        assert hasattr(lib, name), name
        restype, argtypes = view.VIEW_PROTOTYPES[name]
        assert _py_class(restype) == res == ctypes.c_int, name
        assert len(argtypes) == len(params) == {"atr_view_cells": 13, "atr_view_rgb": 14}[name], name
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _py_class(a) == c, (name, i)
    assert [i for i, c in enumerate(funcs["atr_view_cells"][1]) if c == "ptr"] == [0, 1, 5, 7, 10, 11, 12]
    assert [i for i, c in enumerate(funcs["atr_view_rgb"][1]) if c == "ptr"] == [0, 1, 5, 7, 11, 13]
    for name in funcs:
        assert name not in fused.ATR_PROTOTYPES and name not in vec_env.ABI_SYMBOLS
    for pinned in ("track2d.h", "atr_policy.h", "track2d_trace.h"):
        assert "atr_view" not in open(os.path.join(ROOT, "include", pinned)).read()
    rule = open(os.path.join(ROOT, "active_tracking_rl_amd", "csrc", "atr_view_rule.h")).read()
    assert "hip_runtime" not in rule and "atr_ego_rule.h" in rule
    src = open(os.path.join(ROOT, "active_tracking_rl_amd", "csrc", "view_hip.hip")).read()
    assert "static_assert" in src and "atr_view_rule.h" in src and "__shared__" in src
    assert src.count("atomic") == 1 and "atomicOr(a.faults, T2D_FAULT_RENDER_ID)" in src
    assert "hipMalloc" not in src and "Synchronize" not in src
    assert view.min_pitch(1) == 736 and view.min_pitch(4) == 2912 and view.min_pitch(8) == 5808


def test_binding_checks_status_and_refuses_before_the_handle():
    """lib() binds the table with an errcheck that raises with the entry point's name and the library's text; every handle-free
    refusal of the header is reached with h = NULL and one bad argument, and with a later bad argument beside it the earlier one
    is named: the header's order; all-good arguments with h = NULL give the null-handle text (this test runs without a device, on
    addresses that are never read)."""
    from active_tracking_rl_amd import build, view
    build.build()
    L = view.lib()
    for name, (restype, argtypes) in view.VIEW_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
        assert f.errcheck(0, None, ()) == 0
        with pytest.raises(RuntimeError, match=r"^%s failed \(-1\): " % name):
            f.errcheck(-1, None, ())
    p, q, ids, fac = 1 << 20, 1 << 24, 1 << 22, 1 << 23        # non-null, aligned addresses: a refused call never reads them
    shared = [(dict(obs=0), "null obs"), (dict(obs=0, env_ids=0), "null obs"),
              (dict(env_ids=0), "null env_ids"), (dict(env_ids=0, count=0), "null env_ids"),
              ("no_output", "null output buffer"),
              (dict(count=0), r"count 0 outside \[1, 65535\]"), (dict(count=65536, viewer=2), r"count 65536 outside"),
              (dict(count=-1), r"count -1 outside"),
              (dict(viewer=2), r"viewer 2 outside 0 \.\. 1"), (dict(viewer=-1, turned=4), r"viewer -1 outside"),
              (dict(turned=4), r"turned 4 outside 0 \.\. 3"), (dict(turned=-1, facing=0), r"turned -1 outside"),
              (dict(turned=1, facing=0), r"turned 1 needs the facing bytes"), (dict(turned=3, facing=0, se=-1), r"turned 3 needs"),
              (dict(se=-338), "negative element stride"), (dict(sp=-1, obs=p + 2, is_u8=False), "negative element stride"),
              (dict(obs=p + 2, is_u8=False), "float32 windows not 4-byte aligned"),
              ("float_then_output", "float32 windows not 4-byte aligned"),
              (dict(), "null handle"), (dict(obs=p + 3, se=0, sp=0, turned=0, facing=0, viewer=1, count=65535), "null handle"),
              (dict(is_u8=False, turned=3), "null handle")]
    ok_c = dict(h=None, obs=p, is_u8=True, se=338, sp=169, facing=fac, turned=1, env_ids=ids, count=3, viewer=0, cells=q,
                windows=q + 64, stream=None)
    own_c = [(dict(cells=q + 2), "cells buffer .* is not 4-byte aligned"), (dict(cells=q + 1, windows=0), "is not 4-byte aligned"),
             (dict(cells=0), "null handle"), (dict(windows=0), "null handle"), (dict(cells=0, windows=q + 1), "null handle")]
    for change, text in shared + own_c:
        if change == "no_output":
            change = dict(cells=0, windows=0, count=0)
        elif change == "float_then_output":
            change = dict(obs=p + 1, is_u8=False, cells=q + 2)
        with pytest.raises(RuntimeError, match=r"^atr_view_cells failed \(-1\): atr_view_cells: .*%s" % text):
            view.view_cells_raw(**dict(ok_c, **change))
    ok_r = dict(h=None, obs=p, is_u8=True, se=338, sp=169, facing=fac, turned=1, env_ids=ids, count=3, viewer=0, scale=4, rgb=q,
                pitch=2912, stream=None)
    own_r = [(dict(scale=0), r"scale 0 outside \[1, 8\]"), (dict(scale=9, pitch=8), r"scale 9 outside \[1, 8\]"),
             (dict(pitch=2896), r"pitch 2896 must be a multiple of 16 and at least 2904"),
             (dict(pitch=2920), r"pitch 2920 must be a multiple of 16"), (dict(pitch=2904, rgb=q + 4), r"pitch 2904 must be"),
             (dict(scale=1, pitch=720), r"pitch 720 must be a multiple of 16 and at least 726"),
             (dict(rgb=q + 8), "frame buffer .* is not 16-byte aligned"), (dict(rgb=q + 1), "is not 16-byte aligned"),
             (dict(scale=8, pitch=5808), "null handle"), (dict(scale=1, pitch=736), "null handle"), (dict(pitch=4096), "null handle")]
    for change, text in shared + own_r:
        if change == "no_output":
            change = dict(rgb=0, count=0)
        elif change == "float_then_output":
            change = dict(obs=p + 1, is_u8=False, scale=0)
        with pytest.raises(RuntimeError, match=r"^atr_view_rgb failed \(-1\): atr_view_rgb: .*%s" % text):
            view.view_rgb_raw(**dict(ok_r, **change))


def test_the_tensor_checks():
    """view_cells / view_rgb refuse a host tensor (there is no host path); viewer_of takes 0, 1 and the two names."""
    import torch
    from active_tracking_rl_amd import view
    for f in (view.view_cells, view.view_rgb):
        with pytest.raises(RuntimeError, match="there is no host path"):
            f(torch.zeros(2, 2, 13, 13, dtype=torch.uint8), None, [0])
        with pytest.raises(RuntimeError, match="there is no host path"):
            f(np.zeros((2, 2, 13, 13), np.uint8), None, [0])
    assert [view.viewer_of(v) for v in (0, 1, "tracker", "target")] == [0, 1, 0, 1]
    for bad in (2, -1, "both", None, True, 0.5):
        with pytest.raises(ValueError, match="viewer must be"):
            view.viewer_of(bad)


# -- flags and refusals ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("script", ["main.py", "gym_eval.py"])
def test_both_parsers_list_the_flags(script):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0
    for flag in ("--view [WHO]", "--view-dir DIR", "--view-eps K", "--view-scale S"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("script,argv,text", [
    ("main.py", ["--view", "--render"], "--view cannot be combined with --render"),
    ("main.py", ["--view", "target", "--render"], "--view cannot be combined with --render"),
    ("main.py", ["--view", "both"], "invalid choice"),
    ("main.py", ["--view", "--env-base", "Track2D-BlockFullPZR-v0"], "observes the whole map"),
    ("gym_eval.py", ["--view", "--render"], "--view cannot be combined with --render"),
    ("gym_eval.py", ["--view", "tracker", "--occlusion", "--render"], "--view cannot be combined with --render"),
    ("gym_eval.py", ["--view", "all"], "invalid choice"),
    ("gym_eval.py", ["--view", "--env", "Track2D-BlockFullPZR-v0"], "observes the whole map"),
    # the refusals of --render stay as they were
    ("gym_eval.py", ["--fov", "90", "--render"], "--fov cannot be combined with --render"),
    ("main.py", ["--noise-ghost", "0.1", "--render"], "cannot be combined with --render"),
])
def test_parsers_refuse(script, argv, text):
    """The refused combinations end the command in the parser, before a device is looked for (this test runs without one)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and text in r.stderr, r.stderr[-400:]


def test_parser_defaults():
    """--view is None by default, 'tracker' as the bare flag; it combines with every observation flag."""
    code = ("import sys; sys.argv = ['x']; import {0} as m; a = m.parser.parse_args([]); "
            "assert a.view is None and a.view_dir is None and a.view_eps == 4 and a.view_scale == 4; "
            "b = m.parser.parse_args(['--view']); assert b.view == 'tracker'; "
            "c = m.parser.parse_args(['--view', 'target', '--view-dir', 'd', '--view-eps', '2', '--view-scale', '8', '--occlusion', "
            "'--fov', '90', '--footprints', '4', '--map-memory', '--noise-miss', '0.1', '--egocentric']); "
            "assert (c.view, c.view_dir, c.view_eps, c.view_scale) == ('target', 'd', 2, 8); print('ok')")
    for mod in ("main", "gym_eval"):
        r = subprocess.run([sys.executable, "-c", code.format(mod)], capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-600:]


def test_default_args_and_layer_refusals():
    """train.default_args carries the four settings; create_env defaults views to bool(args.view) and refuses a whole-map id,
    traces and the batched rng='numpy' envs; VecEnv and Track2DEnv refuse a whole-map id and traces themselves; evaluate refuses
    both drawing modes at once — all before a device is touched (this test runs without one)."""
    from active_tracking_rl_amd import environment
    from active_tracking_rl_amd import test as test_mod
    from active_tracking_rl_amd.train import default_args
    d = default_args()
    assert d.view is None and d.view_dir is None and d.view_eps == 4 and d.view_scale == 4
    assert default_args(view="target").view == "target"
    ns = lambda **kw: argparse.Namespace(**dict(dict(view="tracker", stack_frames=1, seed=1, gpu_ids=[0]), **kw))
    for n in (4, 1):
        with pytest.raises(ValueError, match="--view needs the 13 x 13 windows"):
            environment.create_env("Track2D-BlockFullPZR-v0", ns(), num_envs=n)
        with pytest.raises(ValueError, match="--view needs the 13 x 13 windows"):
            environment.create_env("Track2D-BlockFullPZR-v0", ns(view=None), num_envs=n, views=True)
        with pytest.raises(ValueError, match="one drawing mode per env"):
            environment.create_env(PARTIAL, ns(), num_envs=n, traces=True)
        with pytest.raises(ValueError, match="one drawing mode per env"):
            environment.create_env(PARTIAL, ns(render=True), num_envs=n)
    for rng in ("numpy", "numpy-device"):
        with pytest.raises(NotImplementedError, match="--view is not wired to the batched rng='numpy' envs"):
            environment.create_env(PARTIAL, ns(), num_envs=4, rng=rng)
    with pytest.raises(ValueError, match="views=True needs the 13 x 13 windows"):
        environment.VecEnv("Track2D-MazeFullNav-v0", 4, views=True)
    with pytest.raises(ValueError, match="views=True needs the 13 x 13 windows"):
        environment.Track2DEnv("Track2D-BlockFullPZR-v0", views=True)
    with pytest.raises(ValueError, match="views=True with traces=True: one drawing mode per env"):
        environment.VecEnv(PARTIAL, 4, views=True, traces=True, auto_reset=False)
    with pytest.raises(ValueError, match="views=True with traces=True: one drawing mode per env"):
        environment.Track2DEnv(PARTIAL, views=True, traces=True)
    # the later passes' refusals of traces stay as they were, views or not
    with pytest.raises(NotImplementedError, match="traces=True"):
        environment.VecEnv(PARTIAL, 4, sensor_noise={"miss": 0.1}, traces=True, auto_reset=False)
    with pytest.raises(ValueError, match="one drawing mode each"):
        test_mod.evaluate(None, NAV, default_args(), "cpu", 2, heuristic_tracker="pursuit", render_dir="a", view_dir="b")


def test_views_default_off_and_create_env_passes_the_flag(monkeypatch):
    """create_env: views=None means bool(args.view); an explicit views wins (a training env passes False); auto_reset reaches the
    VecEnv. Read off the arguments of envs that are never made."""
    from active_tracking_rl_amd import environment
    seen = []

    class Stop(Exception):
        pass

    def vec(*a, **k):
        seen.append(("vec", k.get("views"), k.get("auto_reset")))
        raise Stop()

    def one(*a, **k):
        seen.append(("one", k.get("views")))
        raise Stop()
    monkeypatch.setattr(environment, "VecEnv", vec)
    monkeypatch.setattr(environment, "Track2DEnv", one)
    ns = lambda **kw: argparse.Namespace(**dict(dict(stack_frames=1, seed=1, gpu_ids=[0]), **kw))
    for args, kw in ((ns(), {}), (ns(view=None), {}), (ns(view="target"), {}), (ns(view="tracker"), dict(views=False)),
                     (ns(), dict(views=True, auto_reset=False))):
        for n in (4, 1):
            with pytest.raises(Stop):
                environment.create_env(PARTIAL, args, num_envs=n, **kw)
    assert seen == [("vec", False, None), ("one", False), ("vec", False, None), ("one", False), ("vec", True, None), ("one", True),
                    ("vec", False, None), ("one", False), ("vec", True, False), ("one", True)]


def test_without_the_option_nothing_is_kept_or_launched(monkeypatch):
    """VecEnv._viewed with views off hands the tensor back, keeps nothing and does not import the module; view_cells / view_rgb
    then refuse. With views on it keeps the reference and the two methods hand the binding the kept windows, the core, the ids,
    the facings and the turned bits of the egocentric players."""
    code = ("import sys; from active_tracking_rl_amd import environment; "
            "env = object.__new__(environment.VecEnv); env.views = False; env._view_obs = None; o = object(); "
            "assert env._viewed(o) is o and env._view_obs is None; "
            "assert 'active_tracking_rl_amd.view' not in sys.modules; print('clean')")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "clean", r.stderr[-400:]

    from active_tracking_rl_amd import environment, view
    calls = []
    monkeypatch.setattr(view, "view_cells", lambda *a, **k: calls.append(("cells", a, k)))
    monkeypatch.setattr(view, "view_rgb", lambda *a, **k: calls.append(("rgb", a, k)))
    env = object.__new__(environment.VecEnv)
    env.views, env._view_obs = False, None
    obs = object()
    assert env._viewed(obs) is obs and env._view_obs is None
    for f in (env.view_cells, env.view_rgb):
        with pytest.raises(NotImplementedError, match="needs an env created with views=True"):
            f([0])
    assert calls == []
    env.views, env._ego_roles, env._facing, env.core = True, 0, None, "core"
    with pytest.raises(RuntimeError, match="call reset"):
        env.view_cells([0])
    assert env._viewed(obs) is obs and env._view_obs is obs
    env.view_cells([1, 0], viewer=1)
    env._ego_roles, env._facing = 3, "facing"
    env.view_rgb([2], scale=3, viewer="target", pitch=2192)
    assert calls == [("cells", (obs, "core", [1, 0]), dict(viewer=1, out=None, facing=None, turned=0)),
                     ("rgb", (obs, "core", [2]), dict(scale=3, viewer="target", pitch=2192, out=None, facing="facing", turned=3))]
    # __init__ without the option keeps nothing
    class Stop(Exception):
        pass

    def no_handle(*a, **k):
        raise Stop()
    monkeypatch.setattr(environment, "VecTrack2D", no_handle)
    for kw, want in ((dict(), False), (dict(views=True), True), (dict(views=True, egocentric="tracker", occlusion=True), True)):
        e = object.__new__(environment.VecEnv)
        with pytest.raises(Stop):
            e.__init__(PARTIAL, 4, **kw)
        assert e.views is want and e._view_obs is None
