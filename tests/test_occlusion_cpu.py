"""CPU-side checks of the occluded observations: the rule of include/atr_occlusion.h as tests/occlusion_spec.py states it (the two
fixtures cell for cell, what never hides, what blocks, the 56 offsets whose two lines differ, the symmetry between the two players on
random maps); the header against the built library and occlusion.OCCLUSION_PROTOTYPES; every refusal that comes before a device is
touched; the leading strides the binding accepts; the flag of both parsers; create_env's refusals."""
import argparse
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import occlusion_spec as sp
from conftest import ROOT
from test_abi_cpu import _header_functions, _header_structs, _header_symbols, _py_class


def _window(walls=(), fill=0):
    w = np.full((13, 13), fill, np.uint8)
    for r, c in walls:
        w[r, c] = 1
    return w


def test_a_single_wall_hides_the_cells_behind_it():
    """A wall at (6, 8) in an otherwise empty window hides exactly eight cells; the wall itself stays 1."""
    w = _window([(6, 8)])
    want = {(5, 11), (5, 12), (6, 9), (6, 10), (6, 11), (6, 12), (7, 11), (7, 12)}
    hid = sp.hidden_cells(w)
    assert {(r, c) for r in range(13) for c in range(13) if hid[r, c]} == want
    out = sp.occlude(w)
    for r in range(13):
        for c in range(13):
            assert out[r, c] == (5 if (r, c) in want else w[r, c]), (r, c)
    assert out[6, 8] == 1 and out.dtype == np.uint8


def test_eight_walls_round_the_centre_hide_everything_else():
    ring = [(r, c) for r in (5, 6, 7) for c in (5, 6, 7) if (r, c) != (6, 6)]
    w = _window(ring)
    w[6, 6] = 2
    out = sp.occlude(w)
    assert (out == 5).sum() == 160 and out[6, 6] == 2 and all(out[r, c] == 1 for r, c in ring)
    assert sp.hidden_cells(w).sum() == 160


def test_an_empty_window_is_unchanged_and_the_value_is_the_callers():
    for fill in (0, 2, 4, 5, 255):
        w = _window(fill=fill)
        assert np.array_equal(sp.occlude(w), w) and not sp.hidden_cells(w).any()
    w = _window([(6, 8)]).astype(np.float32)
    out = sp.occlude(w, hidden=9)
    assert out.dtype == np.float32 and (out == 9).sum() == 8 and (out == 5).sum() == 0


def test_cells_next_to_the_centre_are_never_hidden():
    """The centre and the cells with m <= 1 have no line cell: under any walls (all of them included) they stay."""
    near = [(r, c) for r in (5, 6, 7) for c in (5, 6, 7)]
    rs = np.random.RandomState(3)
    windows = [np.ones((13, 13), np.uint8)] + [(rs.random_sample((13, 13)) < d).astype(np.uint8) for d in (0.2, 0.5, 0.8) for _ in range(20)]
    for w in windows:
        hid = sp.hidden_cells(w)
        assert not any(hid[r, c] for r, c in near)
        out = sp.occlude(w)
        assert all(out[r, c] == w[r, c] for r, c in near)
    assert sp.hidden_cells(np.ones((13, 13), np.uint8)).sum() == 160


def test_only_the_value_one_blocks():
    """0, 2, 4, 5 and 255 on both lines of every cell do not hide it; a 1 on both does."""
    for v in (0, 2, 4, 5, 255):
        w = _window(fill=v)
        assert not sp.hidden_cells(w).any() and np.array_equal(sp.occlude(w), w), v
    for dr, dc in sp.OFFSETS:
        if max(abs(dr), abs(dc)) < 2:
            continue
        for v in (0, 2, 4, 5, 255, 1):
            w = _window()
            for r, c in sp.near_line(dr, dc) + sp.far_line(dr, dc):
                w[r, c] = v
            assert sp.hidden_cells(w)[6 + dr, 6 + dc] == (v == 1), (dr, dc, v)
    # a float window: 1.0 blocks, 0.999 and 1.001 do not
    w = _window().astype(np.float32)
    w[6, 8] = 1.001
    assert not sp.hidden_cells(w).any()
    w[6, 8] = 1.0
    assert sp.hidden_cells(w).sum() == 8


def test_both_lines_must_hold_a_wall():
    """Offset (2, 1): the near line is (7, 7), the far line (7, 6). A wall on one of them alone hides nothing at (8, 7)."""
    assert sp.near_line(2, 1) == [(7, 7)] and sp.far_line(2, 1) == [(7, 6)]
    assert not sp.hidden_cells(_window([(7, 7)]))[8, 7] and not sp.hidden_cells(_window([(7, 6)]))[8, 7]
    assert sp.hidden_cells(_window([(7, 7), (7, 6)]))[8, 7]


def test_the_two_lines_differ_for_56_offsets_and_stay_inside_the_window():
    differ = 0
    for dr, dc in sp.OFFSETS:
        a, b = sp.near_line(dr, dc), sp.far_line(dr, dc)
        m = max(abs(dr), abs(dc))
        assert len(a) == len(b) == m - 1
        for r, c in a + b:
            assert 0 <= r < 13 and 0 <= c < 13 and (r, c) != (6, 6) and (r, c) != (6 + dr, 6 + dc)
        differ += sorted(a) != sorted(b)
    assert differ == 56
    # the near line is the line of the sight statistics
    import sight_spec
    for dr, dc in sp.OFFSETS:
        assert sp.near_line(dr, dc) == sight_spec.line(dr, dc)


def test_the_tabulated_form_is_the_loop():
    for density, seed in ((0.05, 1), (0.15, 2), (0.4, 3)):
        w = sp.random_windows(40, density, seed)
        out = sp.occlude(w)
        for i in range(len(w)):
            want = w[i].copy()
            want[sp.hidden_cells(w[i])] = 5
            assert np.array_equal(out[i], want), (density, i)
        as_float = sp.occlude(w.astype(np.float32))
        assert as_float.dtype == np.float32 and np.array_equal(as_float, out.astype(np.float32))


def test_the_tracker_sees_the_target_exactly_when_the_target_sees_the_tracker():
    """2400 random (map, T, G): 20 x 20 maps at wall densities 0.05, 0.15 and 0.3, T anywhere (its window reaches over the border
    into the padding for most positions, and a third of the cases put T on the border itself), G free inside T's window. G's cell
    in T's window is hidden exactly when T's cell in G's window is. Not one disagreement."""
    rs = np.random.RandomState(11)
    disagreements = hidden = border = 0
    for case in range(2400):
        density = (0.05, 0.15, 0.3)[case % 3]
        grid = (rs.random_sample((20, 20)) < density).astype(np.uint8)
        if case % 3 == 0:                 # T on the map's border
            t = [(0, rs.randint(20)), (19, rs.randint(20)), (rs.randint(20), 0), (rs.randint(20), 19)][rs.randint(4)]
        else:
            t = (rs.randint(20), rs.randint(20))
        while True:
            dr, dc = rs.randint(-6, 7), rs.randint(-6, 7)
            g = (t[0] + dr, t[1] + dc)
            if (dr, dc) != (0, 0) and 0 <= g[0] < 20 and 0 <= g[1] < 20:
                break
        grid[t], grid[g] = 0, 0
        border += min(t[0], t[1], 19 - t[0], 19 - t[1]) < 6
        w0 = sp.window_of(grid, *t)
        w1 = sp.window_of(grid, *g)
        w0[6, 6], w0[6 + dr, 6 + dc] = 2, 4
        w1[6, 6], w1[6 - dr, 6 - dc] = 4, 2
        a = sp.hidden_cells(w0)[6 + dr, 6 + dc]
        b = sp.hidden_cells(w1)[6 - dr, 6 - dc]
        disagreements += a != b
        hidden += a
    assert disagreements == 0
    assert hidden > 200 and border > 1200          # (both verdicts occur; most windows reach into the padding)


def _occlusion_header():
    """include/atr_occlusion.h without comments and preprocessor lines."""
    txt = open(os.path.join(ROOT, "include", "atr_occlusion.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    return "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", txt).split("\n") if not ln.lstrip().startswith("#"))


def test_header_prototypes_and_exports_agree():
    """The header's one function is exported by the built library and bound by OCCLUSION_PROTOTYPES with the header's parameter
    count and classes; the constants are the module's and the spec's; the source is in the build and under its no-scratch check;
    the 54-function policy table and the env's symbol list do not know it."""
    from active_tracking_rl_amd import build, fused, occlusion, vec_env
    build.build()
    assert os.path.join("..", "..", "include", "atr_occlusion.h") in build.HEADERS
    assert "occlusion_hip.hip" in build.SOURCES and build.NO_SCRATCH_OCCLUSION == {"occlusion_hip.hip": "k_occlude"}
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    funcs = _header_functions(_occlusion_header())
    assert sorted(funcs) == ["atr_occlude_windows"] == sorted(occlusion.OCCLUSION_PROTOTYPES)
    assert sorted(funcs) == _header_symbols("atr_occlusion.h", "atr_") and _header_structs(_occlusion_header()) == {}
    for name, (res, params) in funcs.items():
        assert hasattr(lib, name), name
        restype, argtypes = occlusion.OCCLUSION_PROTOTYPES[name]
        assert _py_class(restype) == res == ctypes.c_int, name
        assert len(argtypes) == len(params) == 9, name
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _py_class(a) == c, (name, i)
    assert [i for i, c in enumerate(funcs["atr_occlude_windows"][1]) if c is ctypes.c_longlong] == [3, 4, 5, 6]
    assert "atr_occlude_windows" not in fused.ATR_PROTOTYPES and "atr_occlude_windows" not in vec_env.ABI_SYMBOLS
    txt = open(os.path.join(ROOT, "include", "atr_occlusion.h")).read()
    const = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, txt).group(1))
    assert [const("ATR_OCCLUDE_" + n) for n in ("WINDOW", "SIDE", "CENTRE", "WALL", "HIDDEN")] == \
        [occlusion.WINDOW, occlusion.SIDE, sp.CENTRE, occlusion.WALL, occlusion.HIDDEN] == \
        [sp.WINDOW, sp.SIDE, 6, sp.WALL, sp.HIDDEN] == [169, 13, 6, 1, 5]
    assert const("ATR_OCCLUDE_MAX_WINDOWS") == occlusion.MAX_WINDOWS == (1 << 31) - 1


def test_binding_checks_status_and_refuses_before_any_device():
    """lib() binds the table with an errcheck that raises with the entry point's name and the library's text; every refusal of
    the header comes from the argument checks, before anything touches a device (this test runs without one, on addresses that
    are never read)."""
    from active_tracking_rl_amd import build, occlusion
    build.build()
    L = occlusion.lib()
    for name, (restype, argtypes) in occlusion.OCCLUSION_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
        assert f.errcheck(0, None, ()) == 0
        with pytest.raises(RuntimeError, match=r"^%s failed \(-1\): " % name):
            f.errcheck(-1, None, ())
    p = 1 << 20        # any non-null, aligned address: a refused call never reads it
    ok = dict(src=p, dst=p, is_u8=True, n_env=8, n_win=2, se=338, sp=169, hidden=5, stream=None)
    span = 7 * 338 + 169 + 169        # bytes from the first cell to the last of the 8 x 2 byte windows
    cases = [(dict(src=0), "null pointer"), (dict(dst=0), "null pointer"), (dict(src=0, dst=0), "null pointer"),
             (dict(n_env=0), "n_env > 0"), (dict(n_env=-1), "n_env > 0"), (dict(n_win=0), "n_win > 0"), (dict(n_win=-2), "n_win > 0"),
             (dict(n_env=1 << 31, n_win=1), "above"), (dict(n_env=1 << 16, n_win=1 << 15), "above"),
             (dict(n_env=1 << 62, n_win=1 << 62), "above"),
             (dict(se=-338), "negative element stride"), (dict(sp=-1), "negative element stride"),
             (dict(hidden=-1), r"outside 0 \.\. 255"), (dict(hidden=256), r"outside 0 \.\. 255"),
             (dict(src=p + 2, dst=p + 2, is_u8=False), "not 4-byte aligned"),
             (dict(src=p, dst=p + (1 << 16) + 1, is_u8=False), "not 4-byte aligned"),
             (dict(dst=p + 1), "byte ranges overlap"), (dict(dst=p + span - 1), "byte ranges overlap"),
             (dict(dst=p - span + 1), "byte ranges overlap"), (dict(dst=p + 4 * span - 4, is_u8=False), "byte ranges overlap"),
             (dict(dst=p + 4, n_env=1, n_win=1 << 20, se=0, sp=1 << 40), "byte ranges overlap")]
    for change, text in cases:
        with pytest.raises(RuntimeError, match=r"^atr_occlude_windows failed \(-1\): atr_occlude_windows: .*%s" % text):
            occlusion.occlude_windows(**dict(ok, **change))


def test_window_grid_and_the_tensor_checks():
    """The leading dimensions of a tensor as the two strides of the ABI; what they cannot express, and windows that would
    overlap, are ValueErrors; a host tensor is refused (there is no host path)."""
    import torch
    from active_tracking_rl_amd import occlusion
    g = occlusion.window_grid
    assert g((), ()) == (1, 1, 0, 0)
    assert g((7,), (169,)) == (1, 7, 0, 169)
    assert g((4096, 2), (338, 169)) == (1, 8192, 0, 169)                      # dense: one walk
    assert g((21, 4096, 2), (4096 * 338, 338, 169)) == (1, 21 * 8192, 0, 169)
    assert g((5, 2), (3380, 169)) == (5, 2, 3380, 169)                        # a slice of a larger store
    assert g((5, 1, 2, 1, 1), (3380, 338, 169, 169, 169)) == (5, 2, 3380, 169)
    assert g((3, 5, 2), (16900, 3380, 169)) == (15, 2, 3380, 169)
    assert g((5, 1), (400, 7)) == (1, 5, 0, 400)
    assert g((2, 5), (169, 338)) == (2, 5, 169, 338)                          # (permuted: the window index walks the larger stride)
    with pytest.raises(ValueError, match="more than the two strides"):
        g((3, 5, 2), (20000, 3380, 169))
    for shape, strides in (((4,), (168,)), ((4, 2), (338, 100)), ((4, 2), (0, 169)), ((4, 2), (300, 169))):
        with pytest.raises(ValueError, match="windows overlap"):
            g(shape, strides)
    with pytest.raises(RuntimeError, match="there is no host path"):
        occlusion.occlude_(torch.zeros(2, 13, 13, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="there is no host path"):
        occlusion.occlude_(np.zeros((2, 13, 13), np.uint8))


@pytest.mark.parametrize("script", ["main.py", "gym_eval.py"])
def test_both_parsers_list_the_flag(script):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "--occlusion" in r.stdout


def test_default_args_and_create_env_refusals():
    """train.default_args carries occlusion=False; create_env refuses --occlusion on a whole-map id (ValueError) and on the
    batched rng='numpy' envs (NotImplementedError), and VecEnv refuses the whole-map id itself — all before a device is touched
    (this test runs without one)."""
    from active_tracking_rl_amd import environment
    from active_tracking_rl_amd.train import default_args
    assert default_args().occlusion is False and default_args(occlusion=True).occlusion is True
    args = argparse.Namespace(occlusion=True, stack_frames=1, seed=1, gpu_ids=[0])
    with pytest.raises(ValueError, match="--occlusion needs the 13 x 13 windows"):
        environment.create_env("Track2D-BlockFullPZR-v0", args, num_envs=4)
    with pytest.raises(ValueError, match="--occlusion needs the 13 x 13 windows"):
        environment.create_env("Track2D-BlockFullPZR-v0", args, num_envs=1)
    for rng in ("numpy", "numpy-device"):
        with pytest.raises(NotImplementedError, match="--occlusion is not wired to the batched rng='numpy' envs"):
            environment.create_env("Track2D-BlockPartialPZR-v0", args, num_envs=4, rng=rng)
    with pytest.raises(ValueError, match="occlusion=True needs the 13 x 13 windows"):
        environment.VecEnv("Track2D-MazeFullNav-v0", 4, occlusion=True)
    with pytest.raises(ValueError, match="occlusion=True needs the 13 x 13 windows"):
        environment.Track2DEnv("Track2D-BlockFullPZR-v0", occlusion=True)


def test_without_the_flag_nothing_is_launched(monkeypatch):
    """VecEnv._occlude with occlusion off hands the tensor back untouched and never reaches the binding."""
    from active_tracking_rl_amd import environment, occlusion

    def boom(*a, **k):
        raise AssertionError("occlude_ called with occlusion off")
    monkeypatch.setattr(occlusion, "occlude_", boom)
    env = object.__new__(environment.VecEnv)
    env.occlusion = False
    obs = object()
    assert env._occlude(obs) is obs
    env.occlusion = True
    with pytest.raises(AssertionError, match="occlusion off"):
        env._occlude(obs)
