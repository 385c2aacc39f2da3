"""CPU-side checks of the episode traces and the renderer (include/track2d_trace.h): the host model tests/render_spec.py
against the reference's own record (tests/golden/traces.npz, captured by tests/golden/make_golden_traces.py), the ctypes
table against the header, the PNG writer and the --render flags. The device is held to the same fixture and the same model
in tests/test_traces_gpu.py."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest

import render_spec as rs
from conftest import ROOT


@pytest.fixture(scope="module")
def fixture():
    return rs.load_fixture()


def test_fixture_exercises_the_paint_rules(fixture):
    """The record itself proves it contains a tracker painted 6, a target painted 6, a co-located step and a wall bump; it has a
    side-81 map, an episode that ends, and the five palette entries."""
    eps, palette, coverage = fixture
    assert len(eps) == 4 and all(len(ep["actions"]) <= 40 for ep in eps)
    assert (np.asarray(coverage) >= 1).all()
    assert [ep["side"] for ep in eps] == [82, 82, 81, 82]
    assert eps[3]["done"][-1] == 1 and not eps[3]["done"][:-1].any()
    assert sorted(palette) == [0, 1, 2, 4, 6] and len(set(palette.values())) == 5 and rs.BACKGROUND not in palette.values()
    seen = dict(tracker6=0, target6=0, colocated=0, bump=0)
    for ep in eps:
        prev = [list(map(int, p)) for p in ep["init"]]
        for t in range(len(ep["actions"])):
            cur = [list(map(int, p)) for p in ep["pos"][t]]
            head = [list(map(int, p)) for p in ep["traces"][: t + 1]]
            seen["tracker6"] += cur[0] in head and ep["cells"][t][cur[0][0], cur[0][1]] == 6
            seen["target6"] += cur[1] in head and ep["cells"][t][cur[1][0], cur[1][1]] == 6
            seen["colocated"] += cur[0] == cur[1]
            seen["bump"] += (cur[0] == prev[0]) + (cur[1] == prev[1])
            prev = cur
    assert all(v >= 1 for v in seen.values()), seen


def test_spec_reproduces_the_reference_record(fixture):
    """From (map, spawns, actions) alone the host model gives the reference's traces, traces_relative, painted cells,
    unpainted observation and tracker window at every step."""
    eps, _, _ = fixture
    for ep in eps:
        pos = rs.positions(ep["maze"], ep["init"], ep["actions"])
        T = len(ep["actions"])
        assert np.array_equal(np.array(pos[1:], np.int32), ep["pos"]), ep["name"]
        assert rs.traces(pos, T) == ep["traces"].tolist()
        assert np.array_equal(np.array(rs.traces_relative(pos, 0)), ep["rel0"])
        assert np.array_equal(rs.cells(ep["maze"], pos, 0), ep["cells0"]) and np.array_equal(ep["cells0"], ep["full0"])
        assert np.array_equal(rs.partial(ep["maze"], pos, 0), ep["partial0"])
        for t in range(1, T + 1):
            tag = (ep["name"], t)
            assert rs.traces(pos, t) == ep["traces"][: t + 1].tolist(), tag
            assert np.array_equal(np.array(rs.traces_relative(pos, t)), ep["rel"][t - 1]), tag
            assert np.array_equal(rs.cells(ep["maze"], pos, t), ep["cells"][t - 1]), tag
            assert np.array_equal(rs.cells(ep["maze"], pos, t, trace=False), ep["full"][t - 1]), tag
            assert np.array_equal(rs.partial(ep["maze"], pos, t), ep["partial"][t - 1]), tag
        if ep["side"] == 81:
            assert (ep["cells"][:, 81, :] == rs.OUTSIDE).all() and (ep["cells"][:, :, 81] == rs.OUTSIDE).all()
            assert (ep["cells"][:, :81, :81] != rs.OUTSIDE).all()


@pytest.mark.parametrize("scale", [1, 3])
def test_spec_rgb_is_the_palette_of_the_cells_upscaled(fixture, scale):
    eps, palette, _ = fixture
    up = lambda img, k: np.repeat(np.repeat(img, k, axis=0), k, axis=1)
    bg = np.array(rs.BACKGROUND, np.uint8)
    for ep in eps:
        for t in (0, len(ep["actions"]) // 2, len(ep["actions"]) - 1):
            cells, part = ep["cells"][t], ep["partial"][t]
            img = rs.rgb(cells, part, palette, scale)
            assert img.shape == (82 * scale, 162 * scale, 3) and img.dtype == np.uint8
            want = np.zeros((82, 82, 3), np.uint8)
            for r in range(82):
                for c in range(82):
                    want[r, c] = palette[int(cells[r, c])] if int(cells[r, c]) in palette else bg
            assert np.array_equal(img[:, : 82 * scale], up(want, scale))
            assert (img[:, 82 * scale: 84 * scale] == bg).all() and (img[78 * scale:, 84 * scale:] == bg).all()
            win = np.array([[palette[int(v)] for v in row] for row in part], np.uint8)
            assert np.array_equal(img[: 78 * scale, 84 * scale:], up(win, 6 * scale))


def _trace_header_functions():
    txt = open(os.path.join(ROOT, "include", "track2d_trace.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = "\n".join(ln for ln in txt.split("\n") if not ln.lstrip().startswith("#"))
    out = {}
    for m in re.finditer(r"\bint\s+(t2d_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", txt):
        kinds = ""
        for p in m.group(2).split(","):
            decl = re.sub(r"\w+$", "", p.strip())                       # every parameter is named
            kinds += "p" if "*" in decl else {"int": "i"}[" ".join(w for w in decl.split() if w != "const")]
        out[m.group(1)] = kinds
    return out


def test_ctypes_table_matches_the_header_and_the_library_exports_it():
    from active_tracking_rl_amd import build, vec_env
    fns = _trace_header_functions()
    assert sorted(fns) == ["t2d_render_cells", "t2d_render_rgb", "t2d_trace_append", "t2d_trace_attach", "t2d_trace_begin",
                           "t2d_trace_get"]
    assert fns == vec_env.TRACE_ABI
    txt = open(os.path.join(ROOT, "include", "track2d_trace.h")).read()
    assert int(re.search(r"#define T2D_RENDER_TRACE (\d+)", txt).group(1)) == vec_env.RENDER_TRACE
    assert int(re.search(r"#define T2D_FAULT_RENDER_ID (\d+)u", txt).group(1)) == vec_env.FAULT_RENDER_ID
    assert "auto_reset = 1" in txt                                      # the header says why attach refuses such a handle
    build.build()
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    for name in fns:
        assert hasattr(lib, name), name
    L = vec_env.load_library()
    for name, kinds in fns.items():
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int
        assert ["p" if a is ctypes.c_void_p else "i" for a in fn.argtypes] == list(kinds), name
        assert all(a in (ctypes.c_void_p, ctypes.c_int) for a in fn.argtypes)


def test_write_png_decodes_back(tmp_path):
    from active_tracking_rl_amd.utils import write_png
    g = np.random.RandomState(3)
    for shape in ((1, 1, 3), (7, 5, 3), (82, 162, 3)):
        a = g.randint(0, 256, size=shape).astype(np.uint8)
        path = str(tmp_path / ("a%d.png" % shape[0]))
        write_png(path, a)
        data = open(path, "rb").read()
        assert np.array_equal(rs.decode_png(data), a)
        assert data[12:16] == b"IHDR" and data[-8:-4] == b"IEND" and data[-4:] == zlib.crc32(b"IEND").to_bytes(4, "big")
    with pytest.raises(ValueError):
        write_png(str(tmp_path / "bad.png"), np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError):
        write_png(str(tmp_path / "bad.png"), np.zeros((4, 4, 3), np.float32))


def test_cli_parsers_take_the_render_flags():
    import importlib.util

    def load(name):
        spec = importlib.util.spec_from_file_location("_cli_" + name, os.path.join(ROOT, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod.parser

    p = load("gym_eval")
    a = p.parse_args([])
    assert (a.render, a.render_dir, a.render_eps, a.render_scale) == (False, None, 4, 4)
    a = p.parse_args(["--render", "--render-dir", "out/frames", "--render-eps", "2", "--render-scale", "3"])
    assert (a.render, a.render_dir, a.render_eps, a.render_scale) == (True, "out/frames", 2, 3)
    assert "not supported" not in p.format_help()
    m = load("main")
    a = m.parse_args(["--render", "--render-eps", "1"])
    assert a.render and a.render_eps == 1 and a.render_scale == 4
    assert "not supported" not in m.format_help()


def test_traces_need_the_gym_protocol():
    """traces=True implies auto_reset=False; asking for both is refused before anything touches a device."""
    from active_tracking_rl_amd.environment import VecEnv
    with pytest.raises(ValueError, match="auto_reset"):
        VecEnv("Track2D-BlockPartialPZR-v0", 2, traces=True, auto_reset=True)
