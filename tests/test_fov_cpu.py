"""CPU-side checks of facing and field of view: the rule of include/atr_fov.h as tests/fov_spec.py states it (what never hides, the
counts, the nesting, the quarter turn, the asymmetry between the players, the turn rule); csrc/atr_fov_rule.h through a stand-alone
host program built with the address and undefined-behaviour sanitizers, table for table against the spec; the header against the
built library and fov.FOV_PROTOTYPES; every refusal that comes before a device is touched; the flags of both parsers; the refusals
of create_env and VecEnv."""
import argparse
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fov_spec as sp
from conftest import ROOT
from test_abi_cpu import _header_functions, _header_structs, _header_symbols, _py_class

PARTIAL = "Track2D-BlockPartialPZR-v0"


# -- the spec's own properties ---------------------------------------------------------------------------------------------------

def test_the_centre_is_never_hidden_and_none_and_360_hide_nothing():
    for facing in sp.FACINGS:
        for aperture in sp.APERTURES:
            for near in range(7):
                hid = sp.hidden_cells(facing, aperture, near)
                assert not hid[6, 6], (facing, aperture, near)
                if facing == sp.NONE or aperture == 360:
                    assert not hid.any()
                # the near square is visible all round
                assert not hid[6 - near:7 + near, 6 - near:7 + near].any()
    assert not sp.hidden_cells(0, 90, 6).any()          # near = 6 is the whole window


def test_hidden_counts():
    for facing in (0, 1, 2, 3):
        assert [int(sp.hidden_cells(facing, a, 1).sum()) for a in (90, 180, 270)] == [115, 75, 35], facing
        assert [int(sp.hidden_cells(facing, a, 0).sum()) for a in (90, 180, 270)] == [120, 78, 36], facing


def test_hidden_sets_nest():
    for facing in (0, 1, 2, 3):
        for near in range(7):
            h90, h180, h270 = (sp.hidden_cells(facing, a, near) for a in (90, 180, 270))
            assert (h270 <= h180).all() and (h180 <= h90).all(), (facing, near)
            if near < 6:
                assert h270.sum() < h180.sum() < h90.sum()


def test_what_a_player_facing_up_sees():
    """Facing 0 = (-1, 0): at 90 degrees the cell straight ahead and the forward diagonals are seen, the cells beside and behind
    (beyond near) are not; at 180 the whole row beside is seen; at 270 only the quadrant behind is hidden, its diagonals seen."""
    h = sp.hidden_cells(0, 90, 1)
    assert not h[0, 6] and not h[0, 0] and not h[0, 12] and not h[3, 3] and h[3, 2] and h[6, 0] and h[12, 6] and not h[7, 7]
    h = sp.hidden_cells(0, 180, 1)
    assert not h[6, 0] and not h[6, 12] and h[8, 6] and h[8, 0] and not h[7, 5]
    h = sp.hidden_cells(0, 270, 1)
    assert h[12, 6] and h[12, 1] and not h[12, 0] and not h[12, 12] and not h[9, 3] and h[9, 4]


def test_a_quarter_turn_of_window_and_facing_turns_the_output():
    w = sp.random_windows(6, 2, 3)
    for facing in sp.FACINGS:
        for aperture in sp.APERTURES:
            for near in (0, 1, 3):
                f = np.full((6, 2), facing, np.uint8)
                out = sp.restrict(w, f, (aperture, aperture), near)
                rot = sp.restrict(np.rot90(w, axes=(2, 3)), np.full((6, 2), sp.rot90_facing(facing), np.uint8), (aperture, aperture),
                                  near)
                assert np.array_equal(rot, np.rot90(out, axes=(2, 3))), (facing, aperture, near)
                assert np.array_equal(sp.hidden_cells(sp.rot90_facing(facing), aperture, near),
                                      np.rot90(sp.hidden_cells(facing, aperture, near)))


def test_the_rule_is_not_symmetric_between_the_players():
    """The target four rows behind a tracker that faces up, itself facing up: the target sees the tracker (ahead of it), the
    tracker does not see the target. Under occlusion's rule the two verdicts are always equal."""
    w = np.zeros((1, 2, 13, 13), np.uint8)
    w[0, 0, 6, 6], w[0, 0, 10, 6] = 2, 4         # tracker's window: the target at offset (+4, 0)
    w[0, 1, 6, 6], w[0, 1, 2, 6] = 4, 2          # target's window: the tracker at offset (-4, 0)
    out = sp.restrict(w, np.zeros((1, 2), np.uint8), (90, 90), 1)
    assert out[0, 0, 10, 6] == sp.HIDDEN and out[0, 1, 2, 6] == 2
    assert (out[0, 0] == 4).sum() == 0 and (out[0, 1] == 2).sum() == 1


def test_restrict_copies_everything_else_and_takes_the_callers_value():
    w = sp.random_windows(5, 2, 9)
    f = np.array([[0, 1], [2, 3], [255, 0], [3, 255], [1, 1]], np.uint8)
    out = sp.restrict(w, f, (90, 270), 1, hidden=9)
    for e in range(5):
        for p in range(2):
            hid = sp.hidden_cells(int(f[e, p]), (90, 270)[p], 1)
            assert (out[e, p][hid] == 9).all() and np.array_equal(out[e, p][~hid], w[e, p][~hid])
    assert out.dtype == np.uint8
    wf = w.astype(np.float32)
    assert np.array_equal(sp.restrict(wf, f, (90, 270)), sp.restrict(w, f, (90, 270)).astype(np.float32))


def test_turn_rule():
    for facing in sp.FACINGS:
        for action in (None,) + tuple(range(-1, 9)):
            assert sp.turn(facing, action, 1) == sp.NONE and sp.turn(facing, action, 255) == sp.NONE
            for done in (None, 0):
                want = action if action is not None and 0 <= action <= 3 else facing
                assert sp.turn(facing, action, done) == want, (facing, action, done)
    f = np.array([[0, 1], [2, 3], [255, 255]], np.uint8)
    got = sp.turn_all(f, (np.array([3, 7, 1]), None), np.array([0, 0, 1]))
    assert got.tolist() == [[3, 1], [2, 3], [255, 255]] and got.dtype == np.uint8
    w = sp.random_windows(3, 2, 1)
    out, nf = sp.step(w, f, (np.array([3, 7, 1]), None), np.array([0, 0, 1]))
    assert np.array_equal(nf, got) and np.array_equal(out, sp.restrict(w, got))


# -- csrc/atr_fov_rule.h through a sanitizer-built host program ------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the host program needs g++"
    exe = str(tmp_path_factory.mktemp("fov_host") / "fov_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "active_tracking_rl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fov_host.cpp"), "-o", exe])
    return exe


def test_host_program_visibility_table_equals_the_spec(host_program):
    lines = subprocess.check_output([host_program, "table"], text=True).split("\n")
    seen = 0
    for i in range(0, len(lines) - 1, 14):
        tag, facing, aperture, near = lines[i].split()
        assert tag == "vis"
        got = np.array([[ch == "1" for ch in row] for row in lines[i + 1:i + 14]])
        assert got.shape == (13, 13)
        assert np.array_equal(~got, sp.hidden_cells(int(facing), int(aperture), int(near))), lines[i]
        seen += 1
    assert seen == 5 * 4 * 7 and lines[-1] == ""


def test_host_program_turn_table_equals_the_spec(host_program):
    rows = subprocess.check_output([host_program, "turn"], text=True).split("\n")
    assert rows[-1] == "" and len(rows) - 1 == 5 * 11 * 3
    combos = set()
    for row in rows[:-1]:
        tag, facing, action, done, new = row.split()
        assert tag == "turn"
        a = None if action == "x" else int(action)
        d = None if done == "x" else int(done)
        assert int(new) == sp.turn(int(facing), a, d), row
        combos.add((int(facing), a, d))
    assert combos == {(f, a, d) for f in sp.FACINGS for a in (None,) + tuple(range(-1, 9)) for d in (None, 0, 1)}


# -- the ABI -----------------------------------------------------------------------------------------------------------------------

def _fov_header():
    """include/atr_fov.h without comments and preprocessor lines."""
    txt = open(os.path.join(ROOT, "include", "atr_fov.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    return "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", txt).split("\n") if not ln.lstrip().startswith("#"))


def test_header_prototypes_and_exports_agree():
    """The header's one function is exported by the built library and bound by FOV_PROTOTYPES with the header's parameter count
    and classes; the constants are the module's and the spec's; the source and both headers are in the build, the kernel under
    its no-scratch check; the dicts that were there before are what they were; the policy table and the env's symbol list do not
    know the entry point."""
    from active_tracking_rl_amd import build, fov, fused, occlusion, vec_env
    build.build()
    assert os.path.join("..", "..", "include", "atr_fov.h") in build.HEADERS and "atr_fov_rule.h" in build.HEADERS
    assert "fov_hip.hip" in build.SOURCES and build.NO_SCRATCH_FOV == {"fov_hip.hip": "k_fov"}
    assert build.NO_SCRATCH_OCCLUSION == {"occlusion_hip.hip": "k_occlude"} and build.NO_SCRATCH == {"track2d_hip.hip": "k_gru_step"}
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    funcs = _header_functions(_fov_header())
    assert sorted(funcs) == ["atr_fov_windows"] == sorted(fov.FOV_PROTOTYPES)
    assert sorted(funcs) == _header_symbols("atr_fov.h", "atr_") and _header_structs(_fov_header()) == {}
    for name, (res, params) in funcs.items():
        assert hasattr(lib, name), name
        restype, argtypes = fov.FOV_PROTOTYPES[name]
        assert _py_class(restype) == res == ctypes.c_int, name
        assert len(argtypes) == len(params) == 17, name
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _py_class(a) == c, (name, i)
    params = funcs["atr_fov_windows"][1]
    assert [i for i, c in enumerate(params) if c is ctypes.c_longlong] == [3, 5, 6]
    assert [i for i, c in enumerate(params) if c == "ptr"] == [0, 1, 7, 8, 9, 11, 16]
    assert "atr_fov_windows" not in fused.ATR_PROTOTYPES and "atr_fov_windows" not in vec_env.ABI_SYMBOLS
    assert fov.window_grid is occlusion.window_grid
    txt = open(os.path.join(ROOT, "include", "atr_fov.h")).read()
    const = lambda name: int(re.search(r"#define\s+ATR_FOV_%s\s+(\d+)" % name, txt).group(1))
    assert [const(n) for n in ("WINDOW", "SIDE", "CENTRE", "NONE", "HIDDEN", "NEAR", "MAX_NEAR")] == \
        [fov.WINDOW, fov.SIDE, sp.CENTRE, fov.NONE, fov.HIDDEN, fov.NEAR, fov.MAX_NEAR] == \
        [sp.WINDOW, sp.SIDE, 6, sp.NONE, sp.HIDDEN, sp.NEAR, 6] == [169, 13, 6, 255, 5, 1, 6]
    assert const("HIDDEN") == occlusion.HIDDEN and const("MAX_WINDOWS") == fov.MAX_WINDOWS == (1 << 31) - 1
    assert fov.APERTURES == sp.APERTURES == (90, 180, 270, 360)
    # the action codes the binding passes are track2d.h's
    t2d = open(os.path.join(ROOT, "include", "track2d.h")).read()
    assert re.search(r"T2D_ACT_U8 = 0, T2D_ACT_I32 = 1, T2D_ACT_I64 = 2", t2d)


def test_binding_checks_status_and_refuses_before_any_device():
    """lib() binds the table with an errcheck that raises with the entry point's name and the library's text; every refusal of
    the header comes from the argument checks, before anything touches a device (this test runs without one, on addresses that
    are never read)."""
    from active_tracking_rl_amd import build, fov
    build.build()
    L = fov.lib()
    for name, (restype, argtypes) in fov.FOV_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
        assert f.errcheck(0, None, ()) == 0
        with pytest.raises(RuntimeError, match=r"^%s failed \(-1\): " % name):
            f.errcheck(-1, None, ())
    p = 1 << 20        # any non-null, aligned address: a refused call never reads it
    q = 1 << 24
    ok = dict(src=p, dst=p, is_u8=True, n_env=8, n_win=2, se=338, sp=169, facing=q, a0=q + 64, a1=q + 128, act_dtype=2, done=q + 192,
              aperture0=90, aperture1=180, near=1, hidden=5, stream=None)
    span = 7 * 338 + 169 + 169        # bytes from the first cell to the last of the 8 x 2 byte windows
    cases = [(dict(src=0), "null pointer"), (dict(dst=0), "null pointer"), (dict(facing=0), "null pointer"),
             (dict(src=0, dst=0, facing=0), "null pointer"),
             (dict(n_env=0), "n_env > 0"), (dict(n_env=-1), "n_env > 0"), (dict(n_win=0), "n_win > 0"), (dict(n_win=-2), "n_win > 0"),
             (dict(n_win=3), "above the 2 players"), (dict(n_win=1 << 30), "above the 2 players"),
             (dict(n_env=1 << 31, n_win=1), "windows above"), (dict(n_env=1 << 30), "windows above"),
             (dict(n_env=1 << 62), "windows above"),
             (dict(aperture0=0), "aperture"), (dict(aperture0=45), "aperture"), (dict(aperture1=91), "aperture"),
             (dict(aperture1=-90), "aperture"), (dict(aperture0=450, aperture1=360), "aperture"),
             (dict(near=-1), r"near -1 outside 0 \.\. 6"), (dict(near=7), r"near 7 outside 0 \.\. 6"),
             (dict(hidden=-1), r"outside 0 \.\. 255"), (dict(hidden=256), r"outside 0 \.\. 255"),
             (dict(act_dtype=3), r"no T2D_ACT_\*"), (dict(act_dtype=-1), r"no T2D_ACT_\*"),
             (dict(act_dtype=7, a0=0), r"no T2D_ACT_\*"), (dict(act_dtype=7, a1=0), r"no T2D_ACT_\*"),
             (dict(se=-338), "negative element stride"), (dict(sp=-1), "negative element stride"),
             (dict(src=p + 2, dst=p + 2, is_u8=False), "not 4-byte aligned"),
             (dict(src=p, dst=p + (1 << 16) + 1, is_u8=False), "not 4-byte aligned"),
             (dict(dst=p + 1), "byte ranges overlap"), (dict(dst=p + span - 1), "byte ranges overlap"),
             (dict(dst=p - span + 1), "byte ranges overlap"), (dict(dst=p + 4 * span - 4, is_u8=False), "byte ranges overlap"),
             (dict(dst=p + 4, n_env=1 << 20, n_win=1, se=1 << 40, sp=0), "byte ranges overlap")]
    for change, text in cases:
        with pytest.raises(RuntimeError, match=r"^atr_fov_windows failed \(-1\): atr_fov_windows: .*%s" % text):
            fov.fov_windows(**dict(ok, **change))


def test_the_tensor_checks():
    """restrict_ refuses a host tensor (there is no host path); apertures_of takes one aperture or a pair and nothing else."""
    import torch
    from active_tracking_rl_amd import fov
    with pytest.raises(RuntimeError, match="there is no host path"):
        fov.restrict_(torch.zeros(2, 2, 13, 13, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="there is no host path"):
        fov.restrict_(np.zeros((2, 2, 13, 13), np.uint8), np.zeros((2, 2), np.uint8))
    assert fov.apertures_of(90) == (90, 90) and fov.apertures_of((90, 180)) == (90, 180) and fov.apertures_of([270, 360]) == (270, 360)
    for bad in (0, 45, 91, "90", (90,), (90, 180, 270), (90, 100), True, 90.5, None):
        with pytest.raises(ValueError, match="fov must be an aperture"):
            fov.apertures_of(bad)


# -- flags and refusals ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("script", ["main.py", "gym_eval.py"])
def test_both_parsers_list_the_flags(script):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0
    for flag in ("--fov DEG", "--fov-target DEG", "--fov-near N"):
        assert flag in r.stdout, flag
    assert "not blinded" in " ".join(r.stdout.split())


@pytest.mark.parametrize("script,argv,text", [
    ("main.py", ["--fov", "90", "--tracking-stats"], "--tracking-stats / --sight-stats"),
    ("main.py", ["--fov", "180", "--sight-stats"], "--tracking-stats / --sight-stats"),
    ("main.py", ["--fov", "90", "--render"], "cannot be combined with --render"),
    ("main.py", ["--fov-target", "90"], "--fov-target needs --fov"),
    ("main.py", ["--fov", "360"], "invalid choice"),
    ("main.py", ["--fov", "90", "--fov-near", "7"], "invalid choice"),
    ("gym_eval.py", ["--fov", "90", "--render"], "cannot be combined with --render"),
    ("gym_eval.py", ["--fov-target", "360"], "--fov-target needs --fov"),
    ("gym_eval.py", ["--fov", "45"], "invalid choice"),
])
def test_parsers_refuse(script, argv, text):
    """The refused combinations end the command in the parser, before a device is looked for (this test runs without one)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and text in r.stderr, r.stderr[-400:]


def test_default_args_and_create_env_refusals():
    """train.default_args carries the three flags; create_env refuses --fov on a whole-map id, with traces and on the batched
    rng='numpy' envs, and --fov-target alone; VecEnv and Track2DEnv refuse a whole-map id, the Moore actions, traces and a bad
    aperture or radius themselves — all before a device is touched (this test runs without one)."""
    from active_tracking_rl_amd import environment
    from active_tracking_rl_amd.train import default_args
    d = default_args()
    assert d.fov is None and d.fov_target is None and d.fov_near == 1 and default_args(fov=90).fov == 90
    args = argparse.Namespace(fov=90, fov_target=None, fov_near=1, stack_frames=1, seed=1, gpu_ids=[0])
    for n in (4, 1):
        with pytest.raises(ValueError, match="--fov needs the 13 x 13 windows"):
            environment.create_env("Track2D-BlockFullPZR-v0", args, num_envs=n)
        with pytest.raises(NotImplementedError, match="--fov with episode traces"):
            environment.create_env(PARTIAL, args, num_envs=n, traces=True)
    for rng in ("numpy", "numpy-device"):
        with pytest.raises(NotImplementedError, match="--fov is not wired to the batched rng='numpy' envs"):
            environment.create_env(PARTIAL, args, num_envs=4, rng=rng)
    with pytest.raises(ValueError, match="--fov-target needs --fov"):
        environment.create_env(PARTIAL, argparse.Namespace(fov=None, fov_target=180, stack_frames=1, seed=1, gpu_ids=[0]), num_envs=4)
    with pytest.raises(ValueError, match="fov=90 needs the 13 x 13 windows"):
        environment.VecEnv("Track2D-MazeFullNav-v0", 4, fov=90)
    with pytest.raises(ValueError, match=r"fov=\(90, 180\) needs the 13 x 13 windows"):
        environment.Track2DEnv("Track2D-BlockFullPZR-v0", fov=(90, 180))
    with pytest.raises(NotImplementedError, match="VonNeumann"):
        environment.VecEnv(PARTIAL, 4, fov=90, action_type="Moore")
    with pytest.raises(NotImplementedError, match="traces=True"):
        environment.VecEnv(PARTIAL, 4, fov=90, traces=True, auto_reset=False)
    with pytest.raises(NotImplementedError, match="traces=True"):
        environment.Track2DEnv(PARTIAL, fov=90, traces=True)
    with pytest.raises(ValueError, match="fov must be an aperture"):
        environment.VecEnv(PARTIAL, 4, fov=100)
    for near in (-1, 7):
        with pytest.raises(ValueError, match="fov_near must be 0 .. 6"):
            environment.VecEnv(PARTIAL, 4, fov=90, fov_near=near)


def test_without_the_option_nothing_is_launched(monkeypatch):
    """VecEnv._restrict with fov off hands the tensor back untouched and never reaches the binding; with it on, a reset only
    fills the facing bytes, and a step hands the binding the step's actions, the core's done and the env's apertures — with 360
    and no action for a scripted target."""
    from active_tracking_rl_amd import environment, fov

    calls = []
    monkeypatch.setattr(fov, "restrict_", lambda *a: calls.append(a))
    env = object.__new__(environment.VecEnv)
    env.fov = None
    obs = object()
    assert env._restrict(obs) is obs and env._restrict(obs, ("a0", "a1"), "done") is obs and env._restrict(obs, fresh=True) is obs
    assert calls == []

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
    env.fov, env.fov_near, env._facing, env._scripted_target, env.core = (90, 180), 2, Bytes(), False, Core()
    assert env._restrict(obs, fresh=True) is obs and env._facing.filled == 255 and calls == []
    assert env._restrict(obs, (Act("a0"), Act("a1")), "done") is obs
    assert env._restrict(obs) is obs
    assert env._restrict(obs, (Act("a0"), None), "done") is obs
    env._scripted_target = True
    assert env._restrict(obs, (Act("a0"), Act("a1")), "done") is obs
    Core.auto_reset = False
    assert env._restrict(obs, (Act("a0"), Act("a1")), "done") is obs
    f = env._facing
    assert calls == [(obs, f, ("a0", "a1"), "done", (90, 180), 2), (obs, f, (None, None), None, (90, 180), 2),
                     (obs, f, ("a0", None), "done", (90, 360), 2), (obs, f, ("a0", None), "done", (90, 360), 2),
                     (obs, f, ("a0", None), None, (90, 360), 2)]
