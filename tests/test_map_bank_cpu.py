"""CPU-side checks of map banks: the two file formats round trip, .fit, every refusal the Python side makes (the library's
reasons in the library's words), the .txt marks, include/track2d_bank.h against the built library and
map_bank.BANK_PROTOTYPES, the selection rule's plain-Python statement against itself, the flags of the parsers."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import map_bank_spec as sp
from conftest import ROOT
from test_abi_cpu import _header_symbols

from active_tracking_rl_amd import map_bank
from active_tracking_rl_amd.map_bank import MapBank


def room(side=9, walls=()):
    m = np.ones((side, side), np.uint8)
    m[1:-1, 1:-1] = 0
    for r, c in walls:
        m[r, c] = 1
    return m


def test_npz_round_trip_with_and_without_spawns(tmp_path):
    maps = np.stack([room(), room(walls=[(3, 3), (4, 4)])])
    spawns = np.array([[1, 1, 2, 2], [-1, -1, -1, -1]], np.int32)
    for s in (None, spawns):
        p = MapBank(maps, s).save(str(tmp_path / ("b%d.npz" % (s is not None))))
        back = MapBank.load(p)
        assert np.array_equal(back.maps, maps) and back.maps.dtype == np.uint8 and back.count == 2 and back.side == 9
        assert (back.spawns is None) if s is None else (np.array_equal(back.spawns, s) and back.spawns.dtype == np.int32)
        with np.load(p) as z:
            assert sorted(z.files) == (["maps"] if s is None else ["maps", "spawns"])


def test_txt_round_trip_and_marks(tmp_path):
    maps = np.stack([room(7), room(7, walls=[(2, 2)]), room(7)])
    spawns = np.array([[1, 1, 5, 5], [-1, -1, -1, -1], [3, 2, 1, 4]], np.int32)
    p = MapBank(maps, spawns).save(str(tmp_path / "b.txt"))
    back = MapBank.load(p)
    assert np.array_equal(back.maps, maps) and np.array_equal(back.spawns, spawns)
    plain = MapBank.load(MapBank(maps).save(str(tmp_path / "plain.txt")))
    assert np.array_equal(plain.maps, maps) and plain.spawns is None
    # every character the format knows: '#' / '1' walls, '.', '0', ' ' free, T / G free cells with a spawn row, ';' comments
    text = "; a comment\n#####\n#T 0#\n#.1.#\n#..G#\n11111\n\n\n; another\n#####\n#...#\n#...#\n#...#\n#####\n"
    b = MapBank.from_text(text)
    want = room(5)
    want[2, 2] = 1
    assert b.count == 2 and np.array_equal(b.maps[0], want) and np.array_equal(b.maps[1], room(5))
    assert b.spawns.tolist() == [[1, 1, 3, 3], [-1, -1, -1, -1]]


def test_txt_refusals():
    with pytest.raises(ValueError, match="ragged"):
        MapBank.from_text("#####\n#...#\n#..#\n#...#\n#####\n")
    with pytest.raises(ValueError, match="needs both"):
        MapBank.from_text("#####\n#T..#\n#...#\n#...#\n#####\n")
    with pytest.raises(ValueError, match="needs both"):
        MapBank.from_text("#####\n#G..#\n#...#\n#...#\n#####\n")
    with pytest.raises(ValueError, match="more than one"):
        MapBank.from_text("#####\n#T.T#\n#..G#\n#...#\n#####\n")
    with pytest.raises(ValueError, match="character"):
        MapBank.from_text("#####\n#.x.#\n#...#\n#...#\n#####\n")
    with pytest.raises(ValueError, match="not square"):
        MapBank.from_text("#####\n#...#\n#####\n")
    with pytest.raises(ValueError, match="different sides"):
        MapBank.from_text("#####\n#...#\n#...#\n#...#\n#####\n\n####\n#..#\n#..#\n####\n")
    with pytest.raises(ValueError, match="no map"):
        MapBank.from_text("; nothing\n\n")
    with pytest.raises(ValueError, match="cannot say"):
        MapBank(room(5)[None], np.array([[1, 1, 1, 1]])).to_text()
    with pytest.raises(ValueError, match="neither"):
        MapBank(room(5)).save("bank.json")
    with pytest.raises(ValueError, match="neither"):
        MapBank.load("bank.json")


def test_fit_pads_with_walls_bottom_and_right():
    b = MapBank(np.stack([room(9), room(9, walls=[(4, 4)])]), np.array([[1, 1, 7, 7], [-1, -1, -1, -1]]))
    for side in (81, 82):
        f = b.fit(side)
        assert f.side == side and f.count == 2 and np.array_equal(f.maps[:, :9, :9], b.maps)
        assert f.maps[:, 9:, :].all() and f.maps[:, :, 9:].all() and np.array_equal(f.spawns, b.spawns)
        assert all(sp.map_ok(m) for m in f.maps)
    assert b.fit(9) is b
    with pytest.raises(ValueError, match="larger than"):
        MapBank(room(82)).fit(81)
    with pytest.raises(ValueError, match="side 83"):
        MapBank(room(83))


def test_python_refusals_carry_the_library_reasons():
    ok = room()
    with pytest.raises(ValueError, match=r"map 1: cell \(2, 3\) is 2, not 0 / 1"):
        bad = room()
        bad[2, 3] = 2
        MapBank(np.stack([ok, bad]))
    with pytest.raises(ValueError, match=r"cell \(2, 3\) is -1, not 0 / 1"):
        bad = room().astype(np.int64)
        bad[2, 3] = -1
        MapBank(bad)
    with pytest.raises(ValueError, match=r"cell \(2, 3\) is 256, not 0 / 1"):         # (not folded to 0 by a uint8 cast)
        bad = room().astype(np.int64)
        bad[2, 3] = 256
        MapBank(bad)
    for r, c in ((0, 4), (8, 4), (4, 0), (4, 8), (0, 0), (8, 8)):
        bad = room()
        bad[r, c] = 0
        assert not sp.map_ok(bad)
        with pytest.raises(ValueError, match=r"map 0: border cell \(%d, %d\) is not a wall" % (r, c)):
            MapBank(bad)
    two = np.ones((9, 9), np.uint8)
    two[4, 4] = two[4, 5] = 0
    assert not sp.map_ok(two)
    with pytest.raises(ValueError, match=r"map 0: 2 free cell\(s\), at least 3 are needed"):
        MapBank(two)
    three = two.copy()
    three[4, 6] = 0
    assert sp.map_ok(three) and MapBank(three).count == 1
    for row, why in (([1, 1, -1, -1], "neither all -1 nor inside the map"), ([1, 1, 9, 1], "neither all -1 nor inside the map"),
                     ([0, 0, 1, 1], "places an agent on a wall"), ([1, 1, 8, 8], "places an agent on a wall")):
        assert not sp.spawn_ok(ok, row)
        with pytest.raises(ValueError, match="map 0: spawn row .* " + why):
            MapBank(ok, np.array([row]))
    assert MapBank(ok, np.array([[3, 3, 3, 3]])).spawns.tolist() == [[3, 3, 3, 3]] and sp.spawn_ok(ok, [3, 3, 3, 3])
    with pytest.raises(ValueError, match=r"spawns must be integers \[1, 4\]"):
        MapBank(ok, np.zeros((2, 4), np.int32))
    with pytest.raises(ValueError, match="spawns must be integers"):
        MapBank(ok, np.zeros((1, 4), np.float32))
    with pytest.raises(ValueError, match=r"\[K, S, S\]"):
        MapBank(np.zeros((2, 5, 6), np.uint8))
    with pytest.raises(ValueError, match="must be integers"):
        MapBank(room().astype(np.float32))
    with pytest.raises(ValueError, match="count 0 outside"):
        MapBank(np.zeros((0, 9, 9), np.uint8))
    with pytest.raises(ValueError, match="expected 'cycle' or 'random'"):
        map_bank.select_code("shuffle")
    assert map_bank.select_code("cycle") == sp.CYCLE == 0 and map_bank.select_code("random") == sp.RANDOM == 1


def test_header_functions_are_exported_and_bound():
    """Every function include/track2d_bank.h declares is exported by the built library and has a BANK_PROTOTYPES entry with the
    header's parameter count; none of them leaked into the pinned symbol tables."""
    from active_tracking_rl_amd import build, vec_env
    build.build()
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    txt = open(os.path.join(ROOT, "include", "track2d_bank.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    decl = {m.group(1): [p for p in m.group(2).split(",") if p.strip() not in ("", "void")]
            for m in re.finditer(r"\bint\s+(t2d_map_bank_[a-z_]+)\s*\(([^()]*)\)\s*;", txt)}
    assert sorted(decl) == ["t2d_map_bank_attach", "t2d_map_bank_count", "t2d_map_bank_index"] == sorted(map_bank.BANK_PROTOTYPES)
    for name, params in decl.items():
        assert hasattr(lib, name), name
        restype, argtypes = map_bank.BANK_PROTOTYPES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        assert name not in vec_env.ABI_SYMBOLS
    assert not [s for s in _header_symbols() if "map_bank" in s]
    consts = dict(re.findall(r"#define\s+(T2D_BANK_[A-Z_]+)\s+(\d+)", txt))
    assert int(consts["T2D_BANK_CYCLE"]) == map_bank.CYCLE and int(consts["T2D_BANK_RANDOM"]) == map_bank.RANDOM
    assert int(consts["T2D_BANK_MAX_MAPS"]) == map_bank.MAX_MAPS == sp.MAX_MAPS


def test_selection_rule_spec():
    """The plain-Python rule: CYCLE wraps in 64 bits, RANDOM stays below K, draws nothing at K = 1, rejects at K = 3 and is a
    pure function of (seed, genv, ep)."""
    assert sp.index(sp.CYCLE, 1, 0xFFFFFFFF, 0xFFFFFFFF, 7) == (2 * 0xFFFFFFFF) % 7
    assert [sp.index(sp.CYCLE, 9, 1000 + e, 1, 3) for e in range(4)] == [2, 0, 1, 2]
    assert sp.index(sp.RANDOM, 5, 1234, 9, 1) == 0 and sp.rejections(5, 1234, 9, 1) == 0
    idx = [sp.index(sp.RANDOM, 5, 1000 + e, ep, 3) for e in range(16) for ep in range(1, 9)]
    assert set(idx) == {0, 1, 2}
    assert any(sp.rejections(5, 1000 + e, ep, 3) > 0 for e in range(16) for ep in range(1, 9))
    assert all(sp.rejections(5, 1000 + e, 1, 4) == 0 for e in range(16))          # (a power of two never rejects)
    assert sp.index(sp.RANDOM, 5, 1000, 2, 5) == sp.index(sp.RANDOM, 5, 1000, 2, 5)
    for select in (sp.CYCLE, sp.RANDOM):           # the array form is the scalar rule, env by env
        for count in (1, 2, 3, 5, 64):
            eps = [1 + (e * 7) % 5 for e in range(40)]
            want = [sp.index(select, 0x1234567890, 1000 + e, ep, count) for e, ep in enumerate(eps)]
            assert sp.indices(select, 0x1234567890, 1000, eps, count).tolist() == want
    # the stream's words: component (i & 3) of the block (i >> 2), keyed by the seed's halves
    from draw_spec import philox4x32_10
    blk = philox4x32_10((1, 7, 1003, 0), (0x89ABCDEF, 0x01234567))
    assert [sp.map_word(0x0123456789ABCDEF, 1003, 7, 4 + j) for j in range(4)] == [int(w) for w in blk]


def test_per_map_summary_groups_episodes():
    from active_tracking_rl_amd.test import per_map_summary
    rows = per_map_summary([2, 0, 2, 0], np.array([[1., -1.], [3., -3.], [5., -5.], [7., -7.]]), [500, 10, 100, 30])
    assert [r["map"] for r in rows] == [0, 2] and [r["episodes"] for r in rows] == [2, 2]
    assert rows[0]["eps_len"] == 20.0 and rows[1]["eps_len"] == 300.0 and rows[1]["success_rate"] == 0.5
    assert rows[0]["reward"].tolist() == [5.0, -5.0]


def test_eval_args_serves_the_eval_bank_in_cycle_order():
    import argparse
    from active_tracking_rl_amd.environment import eval_args
    plain = argparse.Namespace(seed=1)
    assert eval_args(plain) is plain
    a = eval_args(argparse.Namespace(map_bank="train.npz", bank_select="random", eval_map_bank=None))
    assert a.map_bank is None
    b = eval_args(argparse.Namespace(map_bank="train.npz", bank_select="random", eval_map_bank="held_out.npz"))
    assert b.map_bank == "held_out.npz" and b.bank_select == "cycle"


def test_cli_help_runs():
    r = subprocess.run([sys.executable, "-m", "active_tracking_rl_amd.map_bank", "--help"], capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "make" in r.stdout, r.stderr
    r = subprocess.run([sys.executable, "-m", "active_tracking_rl_amd.map_bank", "make", "--help"], capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0 and all(f in r.stdout for f in ("--env", "--count", "--seed", "--out")), r.stderr


@pytest.mark.parametrize("script, flags", [("main.py", ("--map-bank", "--bank-select", "--eval-map-bank")),
                                           ("gym_eval.py", ("--map-bank",))])
def test_parsers_have_the_flags(script, flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
    for f in flags:
        assert f in r.stdout, f
