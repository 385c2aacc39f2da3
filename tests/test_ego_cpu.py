"""CPU-side checks of the egocentric view: the rule of include/atr_ego.h as tests/ego_spec.py states it (the tables are permutations
and inverses, forward is the heading, the four rot90 identities, the cell a relative action moves towards); csrc/atr_ego_rule.h
through a stand-alone host program built with the address and undefined-behaviour sanitizers, line for line against the spec; the
header against the built library and ego.EGO_PROTOTYPES; every refusal that comes before a device is touched; the flags of both
parsers; the refusals of create_env, VecEnv and Track2DEnv; relative_actions' lookup on host tensors."""
import argparse
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ego_spec as sp
from conftest import ROOT
from test_abi_cpu import _header_functions, _header_structs, _header_symbols, _py_class

PARTIAL = "Track2D-BlockPartialPZR-v0"
RAM = "Track2D-BlockPartialRam-v0"
OPPOSITE = {0: 1, 1: 0, 2: 3, 3: 2}


def _distinct(seed=0):
    """A [13, 13] window whose 169 cells are all different."""
    return np.random.RandomState(seed).permutation(169).reshape(13, 13)


# -- the spec's own properties ---------------------------------------------------------------------------------------------------

def test_the_tables_are_permutations_and_inverses():
    assert sp.ABS == ((0, 1, 2, 3), (1, 0, 3, 2), (2, 3, 1, 0), (3, 2, 0, 1))
    assert sp.REL == ((0, 1, 2, 3), (1, 0, 3, 2), (3, 2, 0, 1), (2, 3, 1, 0))
    for h in range(4):
        assert sorted(sp.ABS[h]) == [0, 1, 2, 3] == sorted(sp.REL[h])
        for k in range(4):
            assert sp.REL[h][sp.ABS[h][k]] == k and sp.ABS[h][sp.REL[h][k]] == k
        assert sp.ABS[h][sp.FORWARD] == h and sp.ABS[h][sp.BACK] == OPPOSITE[h]
        # left and right are each other's opposite, and a right-handed pair with forward: (ur, uc) x (lr, lc) = +1 for "left"
        left, right = sp.MOVES[sp.ABS[h][sp.LEFT]], sp.MOVES[sp.ABS[h][sp.RIGHT]]
        assert left == tuple(-x for x in right)
        ur, uc = sp.MOVES[h]
        assert ur * left[1] - uc * left[0] == 1, h


def test_none_and_what_is_no_facing_look_up():
    w = _distinct()
    for facing in (sp.NONE, 7, 4, 200):
        assert sp.heading_of(facing) == 0 and np.array_equal(sp.view(w, facing), w)
        for k in range(-1, 9):
            assert sp.to_abs(facing, k) == k and sp.to_rel(facing, k) == k
    for facing in range(4):
        for k in (-1, 4, 8, 255, -(2 ** 31), 2 ** 40):
            assert sp.to_abs(facing, k) == k and sp.to_rel(facing, k) == k


def test_the_four_rot90_identities_and_their_inverses():
    w = _distinct(1)
    quarter_turns = {0: 0, 1: 2, 2: 3, 3: 1}
    for h, k in quarter_turns.items():
        e = sp.view(w, h)
        assert np.array_equal(e, np.rot90(w, k)), h
        assert np.array_equal(np.rot90(e, -k), w), h          # the inverse quarter turns give the window back
        assert sorted(e.reshape(-1).tolist()) == list(range(169)) and e[6, 6] == w[6, 6]
    wf = w.astype(np.float32)
    assert np.array_equal(sp.view(wf, 2), sp.view(w, 2).astype(np.float32)) and sp.view(wf, 2).dtype == np.float32


def test_the_cell_of_a_relative_action_is_the_cell_its_absolute_move_goes_towards():
    w = _distinct(2)
    for h in range(4):
        e = sp.view(w, h)
        for k in range(4):
            er, ec = sp.MOVES[k]                      # the ego offset of relative action k: up, down, left, right of the centre
            dr, dc = sp.MOVES[sp.ABS[h][k]]
            for far in range(1, 7):
                assert e[6 + far * er, 6 + far * ec] == w[6 + far * dr, 6 + far * dc], (h, k, far)


def test_view_all_and_abs_all_respect_the_roles_and_the_model_turns_once():
    rs = np.random.RandomState(3)
    w = rs.randint(0, 251, (5, 2, 13, 13)).astype(np.uint8)
    f = np.array([[0, 1], [2, 3], [255, 7], [3, 2], [1, 0]], np.uint8)
    rel = (rs.randint(-1, 6, 5), rs.randint(-1, 6, 5))
    for roles in (1, 2, 3):
        out = sp.view_all(w, f, roles)
        a = sp.abs_all(f, rel, roles)
        for p in range(2):
            for e in range(5):
                inside = (roles >> p) & 1
                assert np.array_equal(out[e, p], sp.view(w[e, p], f[e, p]) if inside else w[e, p])
                assert a[p][e] == (sp.to_abs(f[e, p], rel[p][e]) if inside else rel[p][e])
    assert sp.abs_all(f, (rel[0], None))[1] is None
    m = sp.EnvModel(5, roles=1)
    m.facing = f.copy()
    m.stepped((np.array([3, 9, 1, 0, 2]), np.array([0, 0, 0, 0, 0])), np.array([0, 0, 1, 0, 0]))
    assert m.facing.tolist() == [[3, 1], [2, 3], [255, 7], [0, 2], [2, 0]]             # (the target's bytes stand: roles 1)
    m = sp.EnvModel(5, roles=1, fov=True)
    m.facing = f.copy()
    m.stepped((np.array([3, 9, 1, 0, 2]), np.array([0, 0, 0, 0, 0])), np.array([0, 0, 1, 0, 0]))
    assert m.facing.tolist() == [[3, 0], [2, 0], [255, 255], [0, 0], [2, 0]]           # (the field of view turns both)


# -- csrc/atr_ego_rule.h through a sanitizer-built host program ------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the host program needs g++"
    exe = str(tmp_path_factory.mktemp("ego_host") / "ego_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "active_tracking_rl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "ego_host.cpp"), "-o", exe])
    return exe


def test_host_program_action_tables_equal_the_spec(host_program):
    rows = subprocess.check_output([host_program, "tables"], text=True).split("\n")
    assert rows[-1] == "" and len(rows) - 1 == len(sp.FACINGS) * 10
    seen = set()
    for row in rows[:-1]:
        tag, facing, k, a, r = row.split()
        assert tag == "act"
        assert int(a) == sp.to_abs(int(facing), int(k)) and int(r) == sp.to_rel(int(facing), int(k)), row
        seen.add((int(facing), int(k)))
    assert seen == {(f, k) for f in sp.FACINGS for k in range(-1, 9)}


def test_host_program_cell_map_equals_the_spec(host_program):
    rows = subprocess.check_output([host_program, "cells"], text=True).split("\n")
    assert rows[-1] == "" and len(rows) - 1 == len(sp.FACINGS) * 169
    got = {}
    for row in rows[:-1]:
        tag, facing, cell, src = row.split()
        assert tag == "cell"
        got[(int(facing), int(cell))] = int(src)
    for facing in sp.FACINGS:
        for cell in range(169):
            r, c = sp.source(sp.heading_of(facing), cell // 13, cell % 13)
            assert got[(facing, cell)] == r * 13 + c, (facing, cell)


# -- the ABI -----------------------------------------------------------------------------------------------------------------------

def _ego_header():
    """include/atr_ego.h without comments and preprocessor lines."""
    txt = open(os.path.join(ROOT, "include", "atr_ego.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    return "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", txt).split("\n") if not ln.lstrip().startswith("#"))


def test_header_prototypes_and_exports_agree():
    """The header's two functions are exported by the built library and bound by EGO_PROTOTYPES with the header's parameter
    counts and classes; the constants are the module's and the spec's; the source and both headers are in the build, the kernels
    under their no-scratch check; the dicts that were there before are what they were."""
    from active_tracking_rl_amd import build, ego, fov, fused, occlusion, vec_env
    build.build()
    assert os.path.join("..", "..", "include", "atr_ego.h") in build.HEADERS and "atr_ego_rule.h" in build.HEADERS
    assert "ego_hip.hip" in build.SOURCES and build.NO_SCRATCH_EGO == {"ego_hip.hip": "k_ego"}
    assert build.NO_SCRATCH_FOV == {"fov_hip.hip": "k_fov"} and build.NO_SCRATCH_FOOTPRINTS == {"footprints_hip.hip": "k_footprints"}
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    funcs = _header_functions(_ego_header())
    assert sorted(funcs) == ["atr_ego_actions", "atr_ego_windows"] == sorted(ego.EGO_PROTOTYPES)
    assert sorted(funcs) == _header_symbols("atr_ego.h", "atr_") and _header_structs(_ego_header()) == {}
    counts = {"atr_ego_actions": 9, "atr_ego_windows": 14}
    for name, (res, params) in funcs.items():
        assert hasattr(lib, name), name
        restype, argtypes = ego.EGO_PROTOTYPES[name]
        assert _py_class(restype) == res == ctypes.c_int, name
        assert len(argtypes) == len(params) == counts[name], name
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _py_class(a) == c, (name, i)
    params = funcs["atr_ego_windows"][1]
    assert [i for i, c in enumerate(params) if c is ctypes.c_longlong] == [3, 5, 6]
    assert [i for i, c in enumerate(params) if c == "ptr"] == [0, 1, 7, 8, 9, 11, 13]
    params = funcs["atr_ego_actions"][1]
    assert [i for i, c in enumerate(params) if c is ctypes.c_longlong] == [6]
    assert [i for i, c in enumerate(params) if c == "ptr"] == [0, 1, 2, 3, 4, 8]
    for name in funcs:
        assert name not in fused.ATR_PROTOTYPES and name not in vec_env.ABI_SYMBOLS
    assert ego.window_grid is occlusion.window_grid
    txt = open(os.path.join(ROOT, "include", "atr_ego.h")).read()
    const = lambda name: int(re.search(r"#define\s+ATR_EGO_%s\s+(\d+)" % name, txt).group(1))
    assert [const(n) for n in ("WINDOW", "SIDE", "CENTRE", "FORWARD", "BACK", "LEFT", "RIGHT", "TRACKER", "TARGET")] == \
        [ego.WINDOW, ego.SIDE, ego.CENTRE, ego.FORWARD, ego.BACK, ego.LEFT, ego.RIGHT, ego.ROLES["tracker"], ego.ROLES["target"]] == \
        [sp.WINDOW, sp.SIDE, sp.CENTRE, sp.FORWARD, sp.BACK, sp.LEFT, sp.RIGHT, sp.ROLES["tracker"], sp.ROLES["target"]] == \
        [169, 13, 6, 0, 1, 2, 3, 1, 2]
    assert const("MAX_WINDOWS") == ego.MAX_WINDOWS == (1 << 31) - 1
    assert ego.NONE == fov.NONE == sp.NONE == 255 and ego.ROLES == sp.ROLES and ego.ROLES["both"] == 3
    assert ego.ABS == sp.ABS and ego.REL == sp.REL
    # the table rows as the header prints them
    rows = re.findall(r"heading (\d) \(\w+\)\s+(\d) (\d) (\d) (\d)", txt)
    assert [tuple(int(x) for x in r[1:]) for r in rows] == list(sp.ABS) and [int(r[0]) for r in rows] == [0, 1, 2, 3]
    t2d = open(os.path.join(ROOT, "include", "track2d.h")).read()
    assert re.search(r"T2D_ACT_U8 = 0, T2D_ACT_I32 = 1, T2D_ACT_I64 = 2", t2d)


def test_binding_checks_status_and_refuses_before_any_device():
    """lib() binds the table with an errcheck that raises with the entry point's name and the library's text; every refusal of
    the header comes from the argument checks, before anything touches a device (this test runs without one, on addresses that
    are never read)."""
    from active_tracking_rl_amd import build, ego
    build.build()
    L = ego.lib()
    for name, (restype, argtypes) in ego.EGO_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
        assert f.errcheck(0, None, ()) == 0
        with pytest.raises(RuntimeError, match=r"^%s failed \(-1\): " % name):
            f.errcheck(-1, None, ())
    p = 1 << 20        # any non-null, aligned address: a refused call never reads it
    q = 1 << 24
    ok = dict(src=p, dst=p, is_u8=True, n_env=8, n_win=2, se=338, sp=169, facing=q, a0=q + 64, a1=q + 128, act_dtype=2, done=q + 192,
              roles=3, stream=None)
    span = 7 * 338 + 169 + 169        # bytes from the first cell to the last of the 8 x 2 byte windows
    cases = [(dict(src=0), "null pointer"), (dict(dst=0), "null pointer"), (dict(facing=0), "null pointer"),
             (dict(src=0, dst=0, facing=0), "null pointer"),
             (dict(n_env=0), "n_env > 0"), (dict(n_env=-1), "n_env > 0"), (dict(n_win=0), "n_win > 0"), (dict(n_win=-2), "n_win > 0"),
             (dict(n_win=3), "above the 2 players"), (dict(n_win=1 << 30), "above the 2 players"),
             (dict(n_env=1 << 31, n_win=1), "windows above"), (dict(n_env=1 << 30), "windows above"),
             (dict(n_env=1 << 62), "windows above"),
             (dict(roles=0), r"roles 0 outside 1 \.\. 3"), (dict(roles=4), r"roles 4 outside 1 \.\. 3"), (dict(roles=-1), "roles -1"),
             (dict(act_dtype=3), r"no T2D_ACT_\*"), (dict(act_dtype=-1), r"no T2D_ACT_\*"),
             (dict(act_dtype=7, a0=0), r"no T2D_ACT_\*"), (dict(act_dtype=7, a1=0), r"no T2D_ACT_\*"),
             (dict(se=-338), "negative element stride"), (dict(sp=-1), "negative element stride"),
             (dict(src=p + 2, dst=p + 2, is_u8=False), "not 4-byte aligned"),
             (dict(src=p, dst=p + (1 << 16) + 1, is_u8=False), "not 4-byte aligned"),
             (dict(dst=p + 1), "byte ranges overlap"), (dict(dst=p + span - 1), "byte ranges overlap"),
             (dict(dst=p - span + 1), "byte ranges overlap"), (dict(dst=p + 4 * span - 4, is_u8=False), "byte ranges overlap"),
             (dict(dst=p + 4, n_env=1 << 20, n_win=1, se=1 << 40, sp=0), "byte ranges overlap")]
    for change, text in cases:
        with pytest.raises(RuntimeError, match=r"^atr_ego_windows failed \(-1\): atr_ego_windows: .*%s" % text):
            ego.ego_windows(**dict(ok, **change))
    ok = dict(facing=q, rel0=p, rel1=p + 4096, abs0=p + 8192, abs1=p + 12288, act_dtype=2, n_env=8, roles=3, stream=None)
    cases = [(dict(facing=0), "null pointer"), (dict(rel0=0), "null pointer"), (dict(abs0=0), "null pointer"),
             (dict(rel1=0), "both be NULL or both be given"), (dict(abs1=0), "both be NULL or both be given"),
             (dict(n_env=0), "n_env > 0"), (dict(n_env=-3), "n_env > 0"), (dict(n_env=1 << 30), "players above"),
             (dict(n_env=1 << 62), "players above"),
             (dict(roles=0), r"roles 0 outside 1 \.\. 3"), (dict(roles=4), r"roles 4 outside 1 \.\. 3"),
             (dict(act_dtype=3), r"no T2D_ACT_\*"), (dict(act_dtype=-1), r"no T2D_ACT_\*"),
             (dict(abs0=p + 8), "overlap other than"), (dict(abs0=p + 4096), "overlap other than"),
             (dict(abs1=p + 56), "overlap other than"), (dict(abs1=p + 8192), "overlap other than"),
             (dict(abs0=p + 8192 + 63, abs1=p + 8192), "overlap other than"),
             (dict(abs0=p + 1, act_dtype=0), "overlap other than")]
    for change, text in cases:
        with pytest.raises(RuntimeError, match=r"^atr_ego_actions failed \(-1\): atr_ego_actions: .*%s" % text):
            ego.ego_actions(**dict(ok, **change))


def test_the_tensor_checks_and_roles_of():
    """turn_ and to_absolute refuse host tensors (there is no host path); roles_of maps the three names and nothing else."""
    import torch
    from active_tracking_rl_amd import ego
    with pytest.raises(RuntimeError, match="there is no host path"):
        ego.turn_(torch.zeros(2, 2, 13, 13, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="there is no host path"):
        ego.turn_(np.zeros((2, 2, 13, 13), np.uint8), np.zeros((2, 2), np.uint8))
    with pytest.raises(RuntimeError, match="there is no host path"):
        a = torch.zeros(2, dtype=torch.int64)
        ego.to_absolute((a, a), torch.zeros(2, 2, dtype=torch.uint8), 3, (a, a))
    for bad in (0, 4, True, "3", None):
        with pytest.raises(ValueError, match="roles must be 1"):
            ego.turn_(torch.zeros(2, 2, 13, 13, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.uint8), roles=bad)
    assert (ego.roles_of("tracker"), ego.roles_of("target"), ego.roles_of("both")) == (1, 2, 3)
    for bad in (True, False, None, 1, 3, "Tracker", "all", ("tracker",)):
        with pytest.raises(ValueError, match="egocentric must be one of"):
            ego.roles_of(bad)


def test_relative_lookup_equals_the_spec_on_host_tensors():
    """ego.relative (what VecEnv.relative_actions runs on its device table) on CPU tensors: every facing byte x actions -1 .. 8,
    int64 and int32; it inverts the spec's to_abs."""
    import torch
    from active_tracking_rl_amd import ego
    table = torch.tensor(ego.REL, dtype=torch.int64)
    facings = [f for f in sp.FACINGS for _ in range(10)]
    acts = [a for _ in sp.FACINGS for a in range(-1, 9)]
    want = [sp.to_rel(f, a) for f, a in zip(facings, acts)]
    for dt in (torch.int64, torch.int32):
        got = ego.relative(torch.tensor(acts, dtype=dt), torch.tensor(facings, dtype=torch.uint8), table)
        assert got.dtype == dt and got.tolist() == want
    assert [sp.to_abs(f, r) for f, r in zip(facings, want)] == acts


# -- flags and refusals ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("script", ["main.py", "gym_eval.py"])
def test_both_parsers_list_the_flag(script):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0
    assert "--egocentric [WHO]" in r.stdout
    assert "forward / back / left / right" in " ".join(r.stdout.split())


@pytest.mark.parametrize("script,argv,text", [
    ("main.py", ["--egocentric", "--tracking-stats"], "--tracking-stats / --sight-stats"),
    ("main.py", ["--egocentric", "tracker", "--sight-stats"], "--tracking-stats / --sight-stats"),
    ("main.py", ["--egocentric", "--render"], "cannot be combined with --render"),
    ("main.py", ["--egocentric", "everyone"], "invalid choice"),
    ("main.py", ["--egocentric", "both", "--env", RAM], "the scripted target of --env"),
    ("main.py", ["--egocentric", "target", "--env-base", "Track2D-BlockPartialNav-v0"], "the scripted target of --env-base"),
    ("gym_eval.py", ["--egocentric", "both", "--render"], "cannot be combined with --render"),
    ("gym_eval.py", ["--egocentric", "up"], "invalid choice"),
    ("gym_eval.py", ["--egocentric", "target", "--env", RAM], "the scripted target of"),
])
def test_parsers_refuse(script, argv, text):
    """The refused combinations end the command in the parser, before a device is looked for (this test runs without one)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and text in r.stderr, r.stderr[-400:]


def test_the_flag_parses_bare_and_with_a_name():
    """nargs='?': the bare flag is True (every model-driven player), a name is kept, and without the flag it is None."""
    import importlib.util
    for script in ("main.py", "gym_eval.py"):
        spec = importlib.util.spec_from_file_location("ego_flags_" + script[:-3], os.path.join(ROOT, script))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)          # (the parser is built at import; __main__'s body does not run)
        parse = lambda argv: mod.parser.parse_args(argv).egocentric
        assert parse([]) is None and parse(["--egocentric"]) is True
        assert [parse(["--egocentric", w]) for w in ("tracker", "target", "both")] == ["tracker", "target", "both"]


def test_default_args_and_create_env_refusals():
    """train.default_args carries the flag; create_env refuses --egocentric on a whole-map id, with traces and on the batched
    rng='numpy' envs; VecEnv and Track2DEnv refuse a whole-map id, the Moore actions, traces, a bad name, and "target" / "both"
    on a scripted id themselves — all before a device is touched (this test runs without one)."""
    from active_tracking_rl_amd import environment
    from active_tracking_rl_amd.train import default_args
    assert default_args().egocentric is None and default_args(egocentric="both").egocentric == "both"
    for ego in (True, "tracker"):
        args = argparse.Namespace(egocentric=ego, stack_frames=1, seed=1, gpu_ids=[0])
        for n in (4, 1):
            with pytest.raises(ValueError, match="--egocentric needs the 13 x 13 windows"):
                environment.create_env("Track2D-BlockFullPZR-v0", args, num_envs=n)
            with pytest.raises(NotImplementedError, match="--egocentric with episode traces"):
                environment.create_env(PARTIAL, args, num_envs=n, traces=True)
        for rng in ("numpy", "numpy-device"):
            with pytest.raises(NotImplementedError, match="--egocentric is not wired to the batched rng='numpy' envs"):
                environment.create_env(PARTIAL, args, num_envs=4, rng=rng)
    with pytest.raises(ValueError, match="egocentric=True needs the 13 x 13 windows"):
        environment.VecEnv("Track2D-MazeFullNav-v0", 4, egocentric=True)
    with pytest.raises(ValueError, match="egocentric='both' needs the 13 x 13 windows"):
        environment.Track2DEnv("Track2D-BlockFullPZR-v0", egocentric="both")
    with pytest.raises(NotImplementedError, match="VonNeumann"):
        environment.VecEnv(PARTIAL, 4, egocentric=True, action_type="Moore")
    with pytest.raises(NotImplementedError, match="traces=True"):
        environment.VecEnv(PARTIAL, 4, egocentric="tracker", traces=True, auto_reset=False)
    with pytest.raises(NotImplementedError, match="traces=True"):
        environment.Track2DEnv(PARTIAL, egocentric=True, traces=True)
    for bad in ("everyone", 3, ("tracker",)):
        with pytest.raises(ValueError, match="egocentric must be one of"):
            environment.VecEnv(PARTIAL, 4, egocentric=bad)
    for env_id in (RAM, "Track2D-BlockPartialNav-v0", "Track2D-MazePartialRPF-v0"):
        for who in ("target", "both"):
            with pytest.raises(ValueError, match="only the tracker can be egocentric"):
                environment.VecEnv(env_id, 4, egocentric=who)
            with pytest.raises(ValueError, match="only the tracker can be egocentric"):
                environment.Track2DEnv(env_id, egocentric=who, rng="numpy")


def test_the_bare_option_resolves_by_the_id_and_without_it_nothing_is_launched(monkeypatch):
    """VecEnv(egocentric=True) means both players on a PZR id and the tracker alone on a Ram id (resolved before the handle is
    made: the handle's constructor is stubbed out here and stops the construction). With the option off, _turn hands the tensor
    back and step's translation is not reached; with it on, a reset only fills the facing bytes, a step hands turn_ the
    absolute actions and the core's done — nothing where the field of view has turned the bytes already — and observe() no
    actions."""
    from active_tracking_rl_amd import ego, environment

    class Stop(Exception):
        pass

    def no_handle(*a, **k):
        raise Stop()
    monkeypatch.setattr(environment, "VecTrack2D", no_handle)
    seen = {}
    for env_id, arg in ((PARTIAL, True), (RAM, True), (RAM, "tracker"), (PARTIAL, "target"), (PARTIAL, None), (PARTIAL, False)):
        env = object.__new__(environment.VecEnv)
        with pytest.raises(Stop):
            env.__init__(env_id, 4, egocentric=arg)
        seen[(env_id, arg)] = (env.egocentric, env._ego_roles)
    assert seen == {(PARTIAL, True): ("both", 3), (RAM, True): ("tracker", 1), (RAM, "tracker"): ("tracker", 1),
                    (PARTIAL, "target"): ("target", 2), (PARTIAL, None): (None, 0), (PARTIAL, False): (None, 0)}

    calls = []
    monkeypatch.setattr(ego, "turn_", lambda *a: calls.append(a))
    env = object.__new__(environment.VecEnv)
    env._ego_roles = 0
    obs = object()
    assert env._turn(obs) is obs and env._turn(obs, ("a0", "a1"), "done") is obs and env._turn(obs, fresh=True) is obs
    assert env.relative_actions("moves", 0) == "moves" and calls == []

    class Bytes(object):
        filled = None

        def fill_(self, v):
            self.filled = v

    class Act(object):
        def __init__(self, name):
            self.name = name

        def reshape(self, *shape):
            return self.name

    class Core(object):
        auto_reset = True
    env._ego_roles, env.fov, env._facing, env._scripted_target, env.core = 3, None, Bytes(), False, Core()
    assert env._turn(obs, fresh=True) is obs and env._facing.filled == 255 and calls == []
    assert env._turn(obs, (Act("a0"), Act("a1")), "done") is obs
    assert env._turn(obs) is obs
    env._scripted_target, env._ego_roles = True, 1
    assert env._turn(obs, (Act("a0"), Act("a1")), "done") is obs
    Core.auto_reset = False
    assert env._turn(obs, (Act("a0"), None), "done") is obs
    env.fov = (90, 90)
    assert env._turn(obs, (Act("a0"), Act("a1")), "done") is obs
    f = env._facing
    assert calls == [(obs, f, ("a0", "a1"), "done", 3), (obs, f, None, None, 3), (obs, f, ("a0", None), "done", 1),
                     (obs, f, ("a0", None), None, 1), (obs, f, None, None, 1)]
    assert env.relative_actions("moves", 1) == "moves"          # (the target is not egocentric under roles 1)
