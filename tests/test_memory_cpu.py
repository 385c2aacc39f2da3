"""CPU-side checks of map memory: the rule of include/atr_memory.h as tests/memory_spec.py states it (idempotent recording, a visible
cell never changes, no bit outside the square, a clear empties both tiles, a player's tile depends on its own window only);
csrc/atr_memory_rule.h through a stand-alone host program built with the address and undefined-behaviour sanitizers, table for
table against the spec; the header against the built library and memory.MEMORY_PROTOTYPES; every refusal that comes before the
handle is looked at, in the header's order; the flags of both parsers; the refusals of create_env and VecEnv."""
import argparse
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import memory_spec as sp
from conftest import ROOT
from test_abi_cpu import _header_functions, _header_structs, _header_symbols, _py_class

PARTIAL = "Track2D-BlockPartialPZR-v0"
S = 20


def _case(seed, n=3, side=S):
    """(windows [n, 2, 13, 13] over {0, 1, 2, 4, 5, 6}, walls [n, side, side], pos [n, 2, 2] with corners and edges, sides [n])."""
    rs = np.random.RandomState(seed)
    walls = rs.random_sample((n, side, side)) < 0.3
    pos = rs.randint(0, side, (n, 2, 2))
    pos[0, 0], pos[0, 1] = (0, 0), (side - 1, side - 1)
    return sp.random_windows(n, seed + 1), walls, pos, np.full(n, side)


# -- the spec's own properties ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_recording_is_idempotent_and_a_visible_cell_never_changes(seed):
    w, walls, pos, sides = _case(seed)
    out, seen = sp.call(w, sp.new_seen(3, S), walls, pos, sides, sp.BEGIN)
    assert seen.any() and np.array_equal(out, w)          # (an empty memory: what is hidden now was never seen, nothing painted)
    again, seen2 = sp.call(w, seen, walls, pos, sides, sp.KEEP)
    assert np.array_equal(seen2, seen) and np.array_equal(again, out)
    # a call on the painted windows changes neither
    w2 = sp.random_windows(3, seed + 50)
    out2, seen3 = sp.call(w2, seen, walls, pos, sides, sp.STEP, [0, 0, 0])
    assert np.array_equal(out2[w2 != 5], w2[w2 != 5]) and set(np.unique(out2[w2 == 5])) <= {5, 7, 8}
    assert (out2 == 7).any() and (out2 == 8).any() and (out2[w2 == 5] == 5).any()
    out3, seen4 = sp.call(out2, seen3, walls, pos, sides, sp.KEEP)
    assert np.array_equal(out3, out2) and np.array_equal(seen4, seen3)
    # nothing is forgotten without a clear; the centre is recorded like any other cell
    assert (seen3 >= seen).all() and all(seen3[e, p, pos[e, p, 0], pos[e, p, 1]] == (w2[e, p, 6, 6] != 5 or w[e, p, 6, 6] != 5)
                                         for e in range(3) for p in range(2))
    # 7 where the map has a wall, 8 where it has none
    for e, p, wr, wc in np.argwhere(out2 != w2):
        r, c = pos[e, p, 0] - 6 + wr, pos[e, p, 1] - 6 + wc
        assert 0 <= r < S and 0 <= c < S and seen3[e, p, r, c] and out2[e, p, wr, wc] == (7 if walls[e, r, c] else 8)
    # float windows hold the same integers
    outf, seenf = sp.call(w2.astype(np.float32), seen, walls, pos, sides, sp.STEP)
    assert outf.dtype == np.float32 and np.array_equal(outf, out2.astype(np.float32)) and np.array_equal(seenf, seen3)


def test_no_bit_outside_the_square_and_outside_cells_stay_hidden():
    w, walls, pos, sides = _case(7, side=S)
    big = sp.new_seen(3, sp.MAX_SIDE)
    wide = np.zeros((3, sp.MAX_SIDE, sp.MAX_SIDE), bool)
    wide[:, :S, :S] = walls
    out, seen = sp.call(np.zeros_like(w), big, wide, pos, sides, sp.BEGIN)     # everything visible
    assert not seen[:, :, S:].any() and not seen[:, :, :, S:].any()
    assert seen[0, 0, :7, :7].all() and int(seen[0, 0].sum()) == 49 and int(seen[0, 1].sum()) == 49     # the corners' windows
    tiles = sp.pack(seen)
    back, stray = sp.unpack(tiles, S)
    assert not stray and np.array_equal(back, seen[:, :, :S, :S]) and not tiles[:, :, 3 * S:].any()
    allseen = np.ones_like(big)
    hidden = np.full_like(w, 5)
    painted = sp.paint(hidden, allseen, wide, pos, sides)
    assert (painted[0, 0, :6] == 5).all() and (painted[0, 0, :, :6] == 5).all() and (painted[0, 0, 6:, 6:] != 5).all()
    assert (painted[0, 1, 7:] == 5).all() and (painted[0, 1, :, 7:] == 5).all() and (painted[0, 1, :7, :7] != 5).all()


def test_a_clear_empties_both_tiles_and_roles_choose_the_player():
    w, walls, pos, sides = _case(11)
    full = np.ones((3, 2, S, S), bool)
    assert np.array_equal(sp.clear(full, sp.KEEP, [1, 1, 1]), full) and np.array_equal(sp.clear(full, sp.STEP), full)
    c = sp.clear(full, sp.STEP, [0, 255, 1])
    assert c[0].all() and not c[1].any() and not c[2].any()
    for done in (None, [0, 0, 0], [1, 0, 0]):
        assert not sp.clear(full, sp.BEGIN, done).any()
    for roles in (1, 2):
        c = sp.clear(full, sp.BEGIN, None, roles)
        assert not c[:, roles - 1].any() and c[:, 2 - roles].all()
        out, seen = sp.call(w, full, walls, pos, sides, sp.BEGIN, None, roles)
        assert seen[:, 2 - roles].all() and np.array_equal(out[:, 2 - roles], w[:, 2 - roles])
    _, a = sp.call(w, sp.new_seen(3, S), walls, pos, sides, sp.BEGIN)
    # each player's memory is fed only by its own window: changing player 1's window leaves tile 0 as it was
    w2 = w.copy()
    w2[:, 1] = sp.random_windows(3, 99)[:, 1]
    _, b = sp.call(w2, sp.new_seen(3, S), walls, pos, sides, sp.BEGIN)
    assert np.array_equal(a[:, 0], b[:, 0]) and not np.array_equal(a[:, 1], b[:, 1])
    # players are never remembered: a hidden cell under the other player reads 7 or 8
    grid = np.zeros((1, S, S), bool)
    p1 = np.array([[(8, 8), (8, 10)]])
    win = np.zeros((1, 2, 13, 13), np.uint8)
    win[0, 0, 6, 6], win[0, 0, 6, 8] = 2, 4
    _, seen = sp.call(win, sp.new_seen(1, S), grid, p1, [S], sp.BEGIN)
    win[0, 0, 6, 8] = 5
    out, _ = sp.call(win, seen, grid, p1, [S], sp.STEP)
    assert out[0, 0, 6, 8] == 8


def test_the_model_carries_the_sets_step_by_step():
    w, walls, pos, sides = _case(13)
    m = sp.Model(3, 3)
    first = m.begin(np.zeros_like(w), walls, pos, sides)
    assert np.array_equal(first, np.zeros_like(w)) and m.seen.shape == (3, 2, sp.MAX_SIDE, sp.MAX_SIDE)
    kept = m.keep(np.full_like(w, 5), walls, pos, sides)
    stepped = m.step(np.full_like(w, 5), walls, pos, sides, np.array([0, 1, 0], np.uint8))
    assert (kept[1] != 5).any() and (stepped[1] == 5).all() and np.array_equal(stepped[0], kept[0]) and not m.seen[1].any()


def test_tensor_unpack_equals_the_spec():
    import torch
    from active_tracking_rl_amd import memory
    rs = np.random.RandomState(3)
    seen = rs.random_sample((3, 2, 82, 82)) < 0.4
    tiles = sp.pack(seen)
    t = torch.from_numpy(tiles.view(np.int32)).view(torch.uint32)
    for side in (82, 81, 33, 1):
        got = memory.unpack(t, side)
        assert got.dtype == torch.bool and tuple(got.shape) == (3, 2, side, side)
        assert np.array_equal(got.numpy(), seen[:, :, :side, :side])
    for bad in (0, 83):
        with pytest.raises(ValueError, match="side must be 1 .. 82"):
            memory.unpack(t, bad)
    with pytest.raises(ValueError, match="seen must be a uint32"):
        memory.unpack(t.view(torch.int32), 82)
    z = memory.new_seen(3, "cpu")
    assert z.dtype == torch.uint32 and tuple(z.shape) == (3, 2, 256) and z.is_contiguous() and not z.view(torch.int32).any()


# -- csrc/atr_memory_rule.h through a sanitizer-built host program ---------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the host program needs g++"
    exe = str(tmp_path_factory.mktemp("memory_host") / "memory_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "active_tracking_rl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "memory_host.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("side", [81, 82])
def test_host_program_place_row_equals_the_spec(host_program, side):
    """Every 13-bit mask at every pc in 0 .. side - 1: the negative shift (pc < 6), both word seams (31 | 32, 63 | 64) and the clip
    at the right edge are all in there; the scalar spec agrees with the table on the seams and on a sample."""
    out = subprocess.check_output([host_program, "place", str(side)], text=True)
    got = np.array(out.split(), dtype=np.uint64).astype(np.uint32).reshape(side, 1 << 13, 3)
    want = sp.place_table(side)
    assert np.array_equal(got, want)
    rs = np.random.RandomState(side)
    picks = [(m, pc) for pc in (0, 5, 6, 26, 31, 32, 37, 38, 58, 63, 64, 69, 70, side - 7, side - 6, side - 1) for m in (0x1FFF, 0x1001, 0x0AAA)]
    picks += [(int(rs.randint(0, 1 << 13)), int(rs.randint(0, side))) for _ in range(500)]
    for m, pc in picks:
        assert sp.place_row(m, pc, side) == want[pc, m].tolist(), (m, pc)
    assert (want[:, :, 2] >> np.uint32(side - 64)).max() == 0 and (want[side - 1, 0x1FFF] != 0).sum() == 1
    assert want[0, 0x1FFF, 0] == 0x7F and want[32, 0x1FFF].tolist() == [0xFC000000, 0x7F, 0] and want[64, 0x1FFF, 1] == 0xFC000000


def test_host_program_tables_equal_the_spec(host_program):
    rows = subprocess.check_output([host_program, "slice"], text=True).split("\n")
    assert rows[-1] == "" and len(rows) - 1 == 9 * 13
    for row in rows[:-1]:
        tag, m0, m1, m2, wr, bits = row.split()
        assert tag == "slice" and int(bits) == sp.row_bits(int(m0), int(m1), int(m2), int(wr)), row
    rows = subprocess.check_output([host_program, "verdict"], text=True).split("\n")
    assert len(rows) - 1 == 32
    results = set()
    for row in rows[:-1]:
        tag, hidden, inside, seen, wall, wv, fv, got = row.split()
        hidden, inside, seen, wall, wv, fv, got = (int(x) for x in (hidden, inside, seen, wall, wv, fv, got))
        # one cell through the spec: the player at (6, 6) of a 13 x 13 map, or of a 12 x 12 one, which cell (12, 12) is outside of
        side = 13 if inside else 12
        w = np.zeros((1, 2, 13, 13), np.uint8)
        w[0, 0, 12, 12] = 5 if hidden else 0
        s = np.zeros((1, 2, 13, 13), bool)
        s[0, 0, 12, 12] = seen
        walls = np.zeros((1, 13, 13), bool)
        walls[0, 12, 12] = wall
        out = sp.paint(w, s, walls, [[(6, 6), (0, 0)]], [side], 1, 5, wv, fv)
        cell = int(out[0, 0, 12, 12])
        assert tag == "verdict" and (cell == got if got >= 0 else cell == w[0, 0, 12, 12]), row
        assert (got >= 0) == bool(hidden and inside and seen), row
        results.add(got)
    assert results == {-1, 7, 8, 200, 0}
    rows = subprocess.check_output([host_program, "clears"], text=True).split("\n")
    assert len(rows) - 1 == 12
    for row in rows[:-1]:
        tag, mode, done, got = row.split()
        want = not sp.clear(np.ones((1, 2, 2, 2), bool), int(mode), None if done == "x" else [int(done)]).any()
        assert tag == "clears" and int(got) == int(want), row
    rows = subprocess.check_output([host_program, "pos"], text=True).split("\n")
    assert len(rows) - 1 == 10
    for row in rows[:-1]:
        tag, word, p, r, c = row.split()
        word, p = int(word), int(p)
        assert tag == "pos" and (int(r), int(c)) == ((word & 255, word >> 8 & 255), (word >> 16 & 255, word >> 24))[p], row


# -- the ABI -----------------------------------------------------------------------------------------------------------------------

def _mem_header():
    """include/atr_memory.h without comments and preprocessor lines."""
    txt = open(os.path.join(ROOT, "include", "atr_memory.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    return "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", txt).split("\n") if not ln.lstrip().startswith("#"))


def test_header_prototypes_and_exports_agree():
    """The header's one function is exported by the built library and bound by MEMORY_PROTOTYPES with the header's parameter count
    and classes; the constants are the module's and the spec's; the source and both headers are in the build, the kernel under its
    no-scratch check; the policy table and the env's symbol list do not know the entry point."""
    from active_tracking_rl_amd import build, fused, memory, occlusion, vec_env
    build.build()
    assert os.path.join("..", "..", "include", "atr_memory.h") in build.HEADERS and "atr_memory_rule.h" in build.HEADERS
    assert "memory_hip.hip" in build.SOURCES and build.NO_SCRATCH_MEMORY == {"memory_hip.hip": "k_memory"}
    assert build.NO_SCRATCH_FOOTPRINTS == {"footprints_hip.hip": "k_footprints"} and build.NO_SCRATCH_EGO == {"ego_hip.hip": "k_ego"}
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    funcs = _header_functions(_mem_header())
    assert sorted(funcs) == ["atr_memory_windows"] == sorted(memory.MEMORY_PROTOTYPES)
    assert sorted(funcs) == _header_symbols("atr_memory.h", "atr_") and _header_structs(_mem_header()) == {}
    for name, (res, params) in funcs.items():
        assert hasattr(lib, name), name
        restype, argtypes = memory.MEMORY_PROTOTYPES[name]
        assert _py_class(restype) == res == ctypes.c_int, name
        assert len(argtypes) == len(params) == 13, name
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _py_class(a) == c, (name, i)
    params = funcs["atr_memory_windows"][1]
    assert [i for i, c in enumerate(params) if c is ctypes.c_longlong] == [3, 4]
    assert [i for i, c in enumerate(params) if c == "ptr"] == [0, 1, 5, 8, 12]
    assert "atr_memory_windows" not in fused.ATR_PROTOTYPES and "atr_memory_windows" not in vec_env.ABI_SYMBOLS
    assert memory.window_grid is occlusion.window_grid
    txt = open(os.path.join(ROOT, "include", "atr_memory.h")).read()
    const = lambda name: int(re.search(r"#define\s+ATR_MEMORY_%s\s+(\d+)" % name, txt).group(1))
    names = ("WINDOW", "SIDE", "CENTRE", "TILE_WORDS", "ROW_WORDS", "MAX_SIDE", "HIDDEN", "WALL", "FREE", "KEEP", "STEP", "BEGIN")
    assert [const(n) for n in names] == \
        [memory.WINDOW, memory.SIDE, sp.CENTRE, memory.TILE_WORDS, memory.ROW_WORDS, memory.MAX_SIDE, memory.HIDDEN, memory.WALL,
         memory.FREE, memory.KEEP, memory.STEP, memory.BEGIN] == \
        [sp.WINDOW, sp.SIDE, 6, sp.TILE_WORDS, sp.ROW_WORDS, sp.MAX_SIDE, sp.HIDDEN, sp.WALL, sp.FREE, sp.KEEP, sp.STEP, sp.BEGIN] == \
        [169, 13, 6, 256, 3, 82, 5, 7, 8, 0, 1, 2]
    assert memory.ROLES == {"tracker": 1, "target": 2, "both": 3}
    rule = open(os.path.join(ROOT, "active_tracking_rl_amd", "csrc", "atr_memory_rule.h")).read()
    assert "hip_runtime" not in rule
    src = open(os.path.join(ROOT, "active_tracking_rl_amd", "csrc", "memory_hip.hip")).read()
    assert "static_assert" in src and "atr_memory_rule.h" in src and "t2d::kTileWords" in src and "t2d::kRowWords" in src
    assert "atomic" not in src.replace("No atomics", "").replace("__ATOMIC_RELEASE", "").replace("__ATOMIC_ACQUIRE", "")
    assert "__syncthreads" not in src


def test_binding_checks_status_and_refuses_before_the_handle():
    """lib() binds the table with an errcheck that raises with the entry point's name and the library's text; every handle-free
    refusal of the header is reached with h = NULL and one bad argument, and where two arguments are bad the earlier one in the
    header's order speaks; all-good arguments with h = NULL give the null-handle text (this test runs without a device, on
    addresses that are never read)."""
    from active_tracking_rl_amd import build, memory
    build.build()
    L = memory.lib()
    for name, (restype, argtypes) in memory.MEMORY_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
        assert f.errcheck(0, None, ()) == 0
        with pytest.raises(RuntimeError, match=r"^%s failed \(-1\): " % name):
            f.errcheck(-1, None, ())
    p, q = 1 << 20, 1 << 24        # any non-null, aligned addresses: a refused call never reads them
    ok = dict(h=None, obs=p, is_u8=True, se=338, sp=169, seen=q, roles=1, mode=1, done=q + 8192, hidden=5, wall_value=7,
              free_value=8, stream=None)
    cases = [(dict(obs=0), "null pointer"), (dict(seen=0), "null pointer"), (dict(obs=0, seen=0, roles=0), "null pointer"),
             (dict(roles=0), r"roles 0 outside 1 \.\. 3"), (dict(roles=4), r"roles 4 outside 1 \.\. 3"),
             (dict(roles=-1, mode=3), r"roles -1 outside"),
             (dict(mode=-1), r"mode -1 outside 0 \.\. 2"), (dict(mode=3), r"mode 3 outside 0 \.\. 2"),
             (dict(mode=3, hidden=256), r"mode 3 outside"),
             (dict(hidden=-1), r"value outside 0 \.\. 255 \(hidden -1"), (dict(hidden=256), r"value outside 0 \.\. 255"),
             (dict(wall_value=256), r"value outside 0 \.\. 255 .*wall_value 256"),
             (dict(wall_value=-1), r"value outside 0 \.\. 255"), (dict(free_value=256), r"value outside 0 \.\. 255 .*free_value 256"),
             (dict(free_value=-1), r"value outside 0 \.\. 255"),
             (dict(free_value=256, wall_value=5), r"value outside 0 \.\. 255"),
             (dict(wall_value=5), "equal to hidden 5"), (dict(free_value=5), "equal to hidden 5"),
             (dict(hidden=8), "equal to hidden 8"), (dict(hidden=7, se=-1), "equal to hidden 7"),
             (dict(se=-338), "negative element stride"), (dict(sp=-1), "negative element stride"),
             (dict(sp=-1, obs=p + 2, is_u8=False), "negative element stride"),
             (dict(obs=p + 2, is_u8=False), "not 4-byte aligned"), (dict(obs=p + 1, is_u8=False, seen=q + 4), "not 4-byte aligned"),
             (dict(seen=q + 4), "not 16-byte aligned"), (dict(seen=q + 8), "not 16-byte aligned"), (dict(seen=q + 1, obs=p + 3), "not 16-byte aligned"),
             (dict(), "null handle"),
             (dict(is_u8=False, done=0, mode=0, roles=3, hidden=0, wall_value=255, free_value=1, se=0, sp=0), "null handle"),
             (dict(obs=p + 3, mode=2, wall_value=8, free_value=8), "null handle")]
    for change, text in cases:
        with pytest.raises(RuntimeError, match=r"^atr_memory_windows failed \(-1\): atr_memory_windows: .*%s" % text):
            memory.memory_windows(**dict(ok, **change))


def test_the_tensor_checks():
    """remember_ refuses a host tensor (there is no host path); roles_of takes the three names and nothing else."""
    import torch
    from active_tracking_rl_amd import memory
    with pytest.raises(RuntimeError, match="there is no host path"):
        memory.remember_(torch.zeros(2, 2, 13, 13, dtype=torch.uint8), memory.new_seen(2, "cpu"), None, 1)
    with pytest.raises(RuntimeError, match="there is no host path"):
        memory.remember_(np.zeros((2, 2, 13, 13), np.uint8), np.zeros((2, 2, 256), np.uint32), None, 1)
    assert [memory.roles_of(w) for w in ("tracker", "target", "both")] == [1, 2, 3]
    for bad in ("Tracker", "all", 1, None, True):
        with pytest.raises(ValueError, match="map_memory must be one of"):
            memory.roles_of(bad)


# -- flags and refusals ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("script", ["main.py", "gym_eval.py"])
def test_both_parsers_list_the_flag(script):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "--map-memory [WHO]" in r.stdout
    assert "Needs --occlusion or --fov" in " ".join(r.stdout.split())


@pytest.mark.parametrize("script,argv,text", [
    ("main.py", ["--map-memory"], "--map-memory needs --occlusion or --fov"),
    ("main.py", ["--map-memory", "tracker", "--footprints", "4"], "--map-memory needs --occlusion or --fov"),
    ("main.py", ["--map-memory", "--occlusion", "--tracking-stats"], "--tracking-stats / --sight-stats"),
    ("main.py", ["--map-memory", "--fov", "90", "--sight-stats"], "--tracking-stats / --sight-stats"),
    ("main.py", ["--map-memory", "--occlusion", "--render"], "cannot be combined with --render"),
    ("main.py", ["--map-memory", "all", "--occlusion"], "invalid choice"),
    ("main.py", ["--map-memory", "both", "--occlusion", "--env-base", "Track2D-BlockPartialNav-v0"],
     "the scripted target of --env-base Track2D-BlockPartialNav-v0 reads no window"),
    ("main.py", ["--map-memory", "target", "--occlusion", "--env", "Track2D-MazePartialRam-v0"],
     "the scripted target of --env Track2D-MazePartialRam-v0 reads no window"),
    ("main.py", ["--map-memory", "--occlusion", "--env", "Track2D-BlockFullPZR-v0"], "--env Track2D-BlockFullPZR-v0 observes the whole map"),
    ("main.py", ["--map-memory", "--occlusion", "--env-base", "Track2D-MazeFullNav-v0"],
     "--env-base Track2D-MazeFullNav-v0 observes the whole map"),
    ("gym_eval.py", ["--map-memory"], "--map-memory needs --occlusion or --fov"),
    ("gym_eval.py", ["--map-memory", "both", "--fov", "90", "--env", "Track2D-BlockPartialNav-v0"],
     "the scripted target of Track2D-BlockPartialNav-v0 reads no window"),
    ("gym_eval.py", ["--map-memory", "--occlusion", "--render"], "cannot be combined with --render"),
    ("gym_eval.py", ["--map-memory", "--occlusion", "--env", "Track2D-BlockFullPZR-v0"], "observes the whole map"),
    ("gym_eval.py", ["--map-memory", "everyone", "--occlusion"], "invalid choice"),
])
def test_parsers_refuse(script, argv, text):
    """The refused combinations end the command in the parser, before a device is looked for (this test runs without one)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and text in r.stderr, r.stderr[-400:]


def test_default_args_and_create_env_refusals():
    """train.default_args carries the setting; create_env refuses --map-memory on a whole-map id, without --occlusion / --fov, with
    traces and on the batched rng='numpy' envs; VecEnv and Track2DEnv refuse a whole-map id, traces, a bad role, a missing
    occlusion / fov and a remembering scripted target themselves — all before a device is touched (this test runs without one)."""
    from active_tracking_rl_amd import environment
    from active_tracking_rl_amd.train import default_args
    assert default_args().map_memory is None and default_args(map_memory=True).map_memory is True
    ns = lambda **kw: argparse.Namespace(stack_frames=1, seed=1, gpu_ids=[0], **kw)
    for n in (4, 1):
        with pytest.raises(ValueError, match="--map-memory needs the 13 x 13 windows"):
            environment.create_env("Track2D-BlockFullPZR-v0", ns(map_memory=True), num_envs=n)
        with pytest.raises(ValueError, match="--map-memory needs --occlusion or --fov"):
            environment.create_env(PARTIAL, ns(map_memory="both"), num_envs=n)
        with pytest.raises(ValueError, match="--map-memory needs --occlusion or --fov"):
            environment.create_env(PARTIAL, ns(map_memory=True, footprints=4, egocentric=True), num_envs=n)
        with pytest.raises(NotImplementedError, match="--map-memory with episode traces"):
            environment.create_env(PARTIAL, ns(map_memory=True, occlusion=True), num_envs=n, traces=True)
    for rng in ("numpy", "numpy-device"):
        with pytest.raises(NotImplementedError, match="--map-memory is not wired to the batched rng='numpy' envs"):
            environment.create_env(PARTIAL, ns(map_memory=True, occlusion=False, fov=90, footprints=None, egocentric=None),
                                   num_envs=4, rng=rng)
    with pytest.raises(ValueError, match="map_memory=True needs the 13 x 13 windows"):
        environment.VecEnv("Track2D-MazeFullNav-v0", 4, map_memory=True)
    with pytest.raises(ValueError, match="map_memory='tracker' needs the 13 x 13 windows"):
        environment.Track2DEnv("Track2D-BlockFullPZR-v0", map_memory="tracker")
    for kw in (dict(), dict(footprints=4), dict(egocentric=True), dict(occlusion=False, fov=None)):
        with pytest.raises(ValueError, match="needs occlusion=True or fov="):
            environment.VecEnv(PARTIAL, 4, map_memory=True, **kw)
        with pytest.raises(ValueError, match="needs occlusion=True or fov="):
            environment.Track2DEnv(PARTIAL, map_memory="both", **kw)
    with pytest.raises(NotImplementedError, match="traces=True"):
        environment.VecEnv(PARTIAL, 4, map_memory=True, occlusion=True, traces=True, auto_reset=False)
    with pytest.raises(NotImplementedError, match="traces=True"):
        environment.Track2DEnv(PARTIAL, map_memory=True, occlusion=True, traces=True)
    for bad in ("all", "Tracker", 1, 3):
        with pytest.raises(ValueError, match="map_memory must be one of"):
            environment.VecEnv(PARTIAL, 4, map_memory=bad, occlusion=True)
    for env_id in ("Track2D-BlockPartialRam-v0", "Track2D-BlockPartialNav-v0", "Track2D-MazePartialRPF-v0"):
        for who in ("target", "both"):
            with pytest.raises(ValueError, match="scripted"):
                environment.VecEnv(env_id, 4, map_memory=who, occlusion=True)
            with pytest.raises(ValueError, match="scripted"):
                environment.Track2DEnv(env_id, map_memory=who, occlusion=True, rng="numpy" if "RPF" not in env_id else "philox")


def test_without_the_option_nothing_is_launched(monkeypatch):
    """VecEnv._remember with map memory off hands the tensor back untouched and never reaches the binding; with it on it hands the
    binding the windows, the env's tiles, the core, the mode, the core's done where the core auto-resets, and the env's roles;
    fused_step_out declines on memory alone; seen_cells needs the option."""
    from active_tracking_rl_amd import environment, memory

    calls = []
    monkeypatch.setattr(memory, "remember_", lambda *a: calls.append(a))
    env = object.__new__(environment.VecEnv)
    env._memory_roles, env._seen = 0, None
    obs = object()
    assert env._remember(obs, 2) is obs and env._remember(obs, 1, "done") is obs and env._remember(obs, 0) is obs
    assert calls == []
    with pytest.raises(ValueError, match="created without map_memory"):
        env.seen_cells()

    class Core(object):
        auto_reset = True
        supports_u8 = True
    env._memory_roles, env._seen, env.core = 3, "seen", Core()
    assert env._remember(obs, 2) is obs and env._remember(obs, 1, "done") is obs and env._remember(obs, 0) is obs
    Core.auto_reset = False
    assert env._remember(obs, 1, "done") is obs
    assert calls == [(obs, "seen", env.core, 2, None, 3), (obs, "seen", env.core, 1, "done", 3), (obs, "seen", env.core, 0, None, 3),
                     (obs, "seen", env.core, 1, None, 3)]
    assert (environment.VecEnv._MEM_KEEP, environment.VecEnv._MEM_STEP, environment.VecEnv._MEM_BEGIN) == \
        (memory.KEEP, memory.STEP, memory.BEGIN)
    env.stack_frames, env.rescale, env.occlusion, env.fov, env.obs_u8 = 1, False, False, None, True
    env.footprints, env._ego_roles = None, 0
    assert env.fused_step_out(("o", "r", "d")) is None
