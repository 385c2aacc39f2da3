"""CPU-side checks of sensor noise: the rule of include/atr_noise.h as tests/noise_spec.py states it (what each threshold does and
never does, the clock, the two windows' draws, shard independence, the rates the thresholds stand for); csrc/atr_noise_rule.h
through a stand-alone host program built with the address and undefined-behaviour sanitizers, the Philox known answers and the
verdict tables value for value against the spec; the header against the built library and noise.NOISE_PROTOTYPES; every refusal
that comes before the handle is looked at; the flags of both parsers; the refusals of create_env and VecEnv."""
import argparse
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import noise_spec as sp
from conftest import ROOT
from draw_spec import philox4x32_10
from test_abi_cpu import _header_functions, _header_structs, _header_symbols, _py_class

PARTIAL = "Track2D-BlockPartialPZR-v0"
ONE = sp.ONE
KEY = sp.key_of(1)
VALUES = np.array([0, 0, 0, 0, 1, 1, 1, 5, 6, 7, 8, 255], np.uint8)


def _windows(n, seed=0):
    """uint8 [n, 2, 13, 13] over 0 / 1 / 5 / 6 / 7 / 8 / 255 with the viewer at the centre and the other player on one cell."""
    rs = np.random.RandomState(seed)
    w = VALUES[rs.randint(0, len(VALUES), (n, 2, 169))]
    for e in range(n):
        for p in range(2):
            w[e, p, rs.choice([i for i in range(169) if i != 84])] = sp.other_value(p)
    w[:, 0, 84], w[:, 1, 84] = 2, 4
    return w.reshape(n, 2, 13, 13)


def _clock(n, start=0):
    return np.full((n, 2), start, np.uint32)


# -- the spec's own properties ---------------------------------------------------------------------------------------------------

def test_known_answer_vectors():
    for counter, key, out in sp.KAT:
        assert tuple(int(x) for x in philox4x32_10(counter, key)) == out


def test_loops_and_arrays_state_one_rule():
    """apply() (arrays) equals apply_window() (plain loops) window for window."""
    w = _windows(5, 1)
    w[0, 0, 6, 6] = 0          # (a centre that reads 0 stays)
    for t in ((0, 0, 0), (ONE, ONE, ONE), (0, ONE, ONE), sp.threshold_of(.3), (1 << 22, 1 << 23, 1 << 23)):
        t = (t,) * 3 if isinstance(t, int) else t
        for mode in (sp.PEEK, sp.ADVANCE):
            out, clk = sp.apply(w, _clock(5, 7), KEY, t, 3, mode, env_base=1000)
            assert (clk == 7 + mode).all() and out.dtype == w.dtype
            for e in range(5):
                for p in range(2):
                    want = sp.apply_window(w[e, p], KEY, 1000 + e, 7 + mode, p, t)
                    assert np.array_equal(out[e, p].reshape(-1), want), (t, mode, e, p)
    f = w.astype(np.float32)
    out, _ = sp.apply(f, _clock(5), KEY, (1 << 22, 1 << 23, 1 << 23), 3, sp.ADVANCE)
    assert out.dtype == np.float32 and np.array_equal(out, sp.apply(w, _clock(5), KEY, (1 << 22, 1 << 23, 1 << 23), 3, sp.ADVANCE)[0])


def test_thresholds_zero_change_nothing():
    w = _windows(8)
    for roles in (1, 2, 3):
        out, clk = sp.apply(w, _clock(8, 5), KEY, (0, 0, 0), roles, sp.ADVANCE)
        assert out.tobytes() == w.tobytes()
        assert clk.tolist() == [[5 + (roles & 1), 5 + (roles >> 1)]] * 8          # (ADVANCE still advances the noisy windows' clocks)
        out, clk = sp.apply(w, _clock(8, 5), KEY, (0, 0, 0), roles, sp.PEEK)
        assert out.tobytes() == w.tobytes() and (clk == 5).all()
    out, clk = sp.apply(w, _clock(8, 0xFFFFFFFF), KEY, (0, 0, 0), 3, sp.ADVANCE)
    assert (clk == 0).all()                                                      # (wrapping)


def test_flicker_one_swaps_every_zero_and_one_off_the_centre():
    w = _windows(8)
    w[3, 1, 6, 6] = 1
    w[4, 0, 6, 6] = 0
    out, _ = sp.apply(w, _clock(8), KEY, (ONE, 0, 0), 3, sp.ADVANCE)
    flat, o = w.reshape(8, 2, 169), out.reshape(8, 2, 169)
    off = np.arange(169) != 84
    swap = (flat <= 1) & off
    assert np.array_equal(o[swap], 1 - flat[swap]) and np.array_equal(o[~swap], flat[~swap]) and swap.sum() > 1000
    assert np.array_equal(o[:, :, 84], flat[:, :, 84])


def test_miss_one_removes_every_other_player():
    w = _windows(8)
    w[0, 0, 0, :3] = 4          # (more than one O: every one of them goes)
    w[0, 1, 0, :3] = 4          # (a 4 in the target's window is no O)
    out, _ = sp.apply(w, _clock(8), KEY, (0, ONE, 0), 3, sp.ADVANCE)
    O = np.array([4, 2]).reshape(1, 2, 1, 1)
    was = (w == O)
    was[:, :, 6, 6] = False
    assert (out[was] == 0).all() and np.array_equal(out[~was], w[~was]) and was.sum() == 8 * 2 + 3
    assert (out[0, 1, 0, :3] == 4).all()
    w2 = w.copy()
    w2[1, 1, 6, 6] = 2          # (a centre that reads O stays)
    assert sp.apply(w2, _clock(8), KEY, (0, ONE, 0), 3, sp.ADVANCE)[0][1, 1, 6, 6] == 2


def test_ghost_one_writes_one_other_player_where_the_cell_read_zero():
    n = 64
    w = _windows(n, 3)
    hits = 0
    for clock in range(3):
        out, clk = sp.apply(w, _clock(n, clock), KEY, (0, 0, ONE), 3, sp.ADVANCE)
        for e in range(n):
            for p in range(2):
                g = int(sp.ghost_cell(sp.block(KEY, e, clock + 1, p, 0)[2]))
                assert 0 <= g < 169
                a, b = w[e, p].reshape(-1), out[e, p].reshape(-1)
                changed = np.flatnonzero(a != b)
                if a[g] == 0 and g != 84:
                    assert changed.tolist() == [g] and b[g] == sp.other_value(p)
                    hits += 1
                else:
                    assert changed.size == 0
    assert 60 < hits < 6 * n          # (a third of the cells read 0)
    # a window under occlusion shows a ghost only where the player can see: an all-5 window never changes
    five = np.full_like(w, 5)
    assert np.array_equal(sp.apply(five, _clock(n), KEY, (ONE, ONE, ONE), 3, sp.ADVANCE)[0], five)


def test_the_ghost_beats_a_flicker_on_its_cell():
    n = 64
    w = np.zeros((n, 2, 13, 13), np.uint8)
    out, _ = sp.apply(w, _clock(n), KEY, (ONE, 0, ONE), 3, sp.ADVANCE)
    ghosts = 0
    for e in range(n):
        for p in range(2):
            g = int(sp.ghost_cell(sp.block(KEY, e, 1, p, 0)[2]))
            want = np.ones(169, np.uint8)
            want[84] = 0
            if g != 84:
                want[g] = sp.other_value(p)
                ghosts += 1
            assert np.array_equal(out[e, p].reshape(-1), want), (e, p)
    assert ghosts >= 2 * n - 4


def test_other_values_and_the_centre_are_never_touched():
    w = _windows(16, 4)
    keep = np.isin(w, (5, 6, 7, 8, 255))
    keep[:, :, 6, 6] = True
    keep[:, 0][w[:, 0] == 2] = True          # (a 2 in the tracker's window, a 4 in the target's: not the other player there)
    keep[:, 1][w[:, 1] == 4] = True
    for t in ((ONE, ONE, ONE), (1 << 23, 1 << 23, 1 << 23)):
        for clock in range(4):
            out, _ = sp.apply(w, _clock(16, clock), KEY, t, 3, sp.ADVANCE)
            assert np.array_equal(out[keep], w[keep]) and (out != w).any()


def test_peek_repeats_and_advance_differs():
    w = _windows(8, 5)
    t = (1 << 22, 1 << 23, 1 << 23)
    a, c1 = sp.apply(w, _clock(8), KEY, t, 3, sp.ADVANCE)
    b, c2 = sp.apply(w, c1, KEY, t, 3, sp.PEEK)
    b2, c3 = sp.apply(w, c2, KEY, t, 3, sp.PEEK)
    c, c4 = sp.apply(w, c3, KEY, t, 3, sp.ADVANCE)
    assert np.array_equal(a, b) and np.array_equal(b, b2) and not np.array_equal(a, c)
    assert (c1 == 1).all() and (c2 == 1).all() and (c3 == 1).all() and (c4 == 2).all()
    # a window whose role bit is clear is not touched, and its clock does not move
    for roles, q in ((1, 1), (2, 0)):
        out, clk = sp.apply(w, _clock(8, 9), KEY, (ONE, ONE, ONE), roles, sp.ADVANCE)
        assert np.array_equal(out[:, q], w[:, q]) and (clk[:, q] == 9).all() and (clk[:, 1 - q] == 10).all()
        assert (out[:, 1 - q] != w[:, 1 - q]).any()
    # another key, other draws
    assert not np.array_equal(sp.apply(w, _clock(8), sp.key_of(2), t, 3, sp.ADVANCE)[0], a)


def test_the_two_windows_of_one_env_draw_different_words():
    for e in (0, 5, 1000):
        for blk in (0, 1, 64):
            a, b = sp.block(KEY, e, 1, 0, blk), sp.block(KEY, e, 1, 1, blk)
            assert all(int(x) != int(y) for x, y in zip(a, b))
    fw = sp.flicker_words(KEY, np.arange(4)[:, None].repeat(2, 1), np.ones((4, 2), np.int64), np.arange(2)[None, :].repeat(4, 0))
    assert fw.shape == (4, 2, 169) and len(np.unique(fw)) == fw.size
    # the layout: cell L + 64 j is word j of block 1 + L
    for i in (0, 63, 64, 100, 128, 168):
        assert int(fw[2, 1, i]) == int(sp.block(KEY, 2, 1, 1, 1 + (i & 63))[i >> 6])


def test_shard_independence():
    """Global ids 4 .. 7 are the same from a base-0 batch of 8 and a base-4 batch of 4."""
    w = _windows(8, 6)
    t = (1 << 22, 1 << 23, 1 << 23)
    whole, cw = sp.apply(w, _clock(8, 3), KEY, t, 3, sp.ADVANCE, env_base=0)
    lo, cl = sp.apply(w[:4], _clock(4, 3), KEY, t, 3, sp.ADVANCE, env_base=0)
    hi, ch = sp.apply(w[4:], _clock(4, 3), KEY, t, 3, sp.ADVANCE, env_base=4)
    assert np.array_equal(whole, np.concatenate([lo, hi])) and np.array_equal(cw, np.concatenate([cl, ch]))
    assert not np.array_equal(sp.apply(w[4:], _clock(4, 3), KEY, t, 3, sp.ADVANCE, env_base=0)[0], hi)


def test_the_draws_are_what_the_thresholds_say():
    """Key key_of(1), global env ids 0 .. 63, clocks 1 .. 50, both players: the share of passing flicker words over the 1,081,600
    valid cell draws at p = 0.01, 0.05, 0.25 and of passing miss words over the 6,400 window draws at p = 0.1, 0.5 lies within 4
    binomial standard deviations of p (the inputs are fixed: a condition, not a flaky test); every ghost cell lies in 0 .. 168."""
    env, clock, p = np.meshgrid(np.arange(64), np.arange(1, 51), np.arange(2), indexing="ij")
    fw = sp.flicker_words(KEY, env, clock, p)
    assert fw.shape == (64, 50, 2, 169) and fw.size == 1081600
    for rate in (0.01, 0.05, 0.25):
        share = sp.passes(fw, sp.threshold_of(rate)).mean()
        sigma = np.sqrt(rate * (1 - rate) / fw.size)
        print("flicker %.2f: share %.6f, %+.2f sigma" % (rate, share, (share - rate) / sigma))
        assert abs(share - rate) <= 4 * sigma, (rate, share)
    b0 = sp.block(KEY, env, clock, p, 0)
    assert b0[0].size == 6400
    for rate in (0.1, 0.5):
        share = sp.passes(b0[0], sp.threshold_of(rate)).mean()
        sigma = np.sqrt(rate * (1 - rate) / b0[0].size)
        print("miss %.1f: share %.6f, %+.2f sigma" % (rate, share, (share - rate) / sigma))
        assert abs(share - rate) <= 4 * sigma, (rate, share)
    g = sp.ghost_cell(b0[2])
    assert g.min() >= 0 and g.max() <= 168 and len(np.unique(g)) > 150
    assert not sp.passes(fw, 0).any() and sp.passes(fw, ONE).all()


# -- csrc/atr_noise_rule.h through a sanitizer-built host program ----------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the host program needs g++"
    exe = str(tmp_path_factory.mktemp("noise_host") / "noise_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "active_tracking_rl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "noise_host.cpp"), "-o", exe])
    return exe


def test_host_program_known_answers(host_program):
    rows = subprocess.check_output([host_program, "kat"], text=True).split("\n")
    assert rows[-1] == "" and len(rows) - 1 == 3
    for row, (counter, key, out) in zip(rows, sp.KAT):
        f = row.split()
        assert f[0] == "kat" and tuple(int(x, 16) for x in f[1:]) == out
        assert tuple(int(x) for x in philox4x32_10(counter, key)) == out


def test_host_program_verdict_tables_equal_the_spec(host_program):
    rows = subprocess.check_output([host_program, "verdicts"], text=True).split("\n")
    assert rows[-1] == "" and (len(rows) - 1) % 4 == 0 and len(rows) - 1 == 4 * 9 * 4 * 2
    changed = ghosts = ghost_over_flicker = misses = 0
    for k in range(0, len(rows) - 1, 4):
        case, win, out, draw = (r.split() for r in rows[k:k + 4])
        assert (case[0], win[0], out[0], draw[0]) == ("case", "in", "out", "draw") and len(win) == len(out) == 170
        key, env, clock, p, fl, mi, gh = (int(x) for x in case[1:])
        w, o = np.array(win[1:], np.int64), np.array(out[1:], np.int64)
        want = sp.apply_window(w, key, env, clock, p, (fl, mi, gh))
        assert np.array_equal(o, want), rows[k]
        b0 = [int(x) for x in sp.block(key, env, clock, p, 0)]
        g = (b0[2] * 169) >> 32
        assert [int(x) for x in draw[1:]] == [int((b0[0] >> 8) < mi), int((b0[1] >> 8) < gh), g], rows[k]
        # ... and the array form, with the window as window p of env 0 of a handle at base `env`
        both = np.zeros((1, 2, 13, 13), np.int64)
        both[0, p] = w.reshape(13, 13)
        arr, _ = sp.apply(both, np.full((1, 2), clock, np.uint32), key, (fl, mi, gh), 1 << p, sp.PEEK, env_base=env)
        assert np.array_equal(arr[0, p].reshape(-1), o), rows[k]
        changed += int((o != w).sum())
        if gh and (b0[1] >> 8) < gh and g != 84 and w[g] == 0:
            ghosts += 1
            ghost_over_flicker += fl == ONE
            assert o[g] == sp.other_value(p)
        misses += int(((w == sp.other_value(p)) & (o == 0)).sum())
        assert o[84] == w[84]
    assert changed > 1000 and ghosts >= 5 and ghost_over_flicker >= 1 and misses >= 20


# -- the ABI -----------------------------------------------------------------------------------------------------------------------

def _nz_header():
    """include/atr_noise.h without comments and preprocessor lines."""
    txt = open(os.path.join(ROOT, "include", "atr_noise.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    return "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", txt).split("\n") if not ln.lstrip().startswith("#"))


def test_header_prototypes_and_exports_agree():
    """The header's one function is exported by the built library and bound by NOISE_PROTOTYPES with the header's parameter count
    and classes; the constants are the module's and the spec's; the source and both headers are in the build, the kernel under its
    no-scratch check; the policy table and the env's symbol list do not know the entry point."""
    from active_tracking_rl_amd import build, fused, noise, occlusion, vec_env
    build.build()
    assert os.path.join("..", "..", "include", "atr_noise.h") in build.HEADERS and "atr_noise_rule.h" in build.HEADERS
    assert "noise_hip.hip" in build.SOURCES and build.NO_SCRATCH_NOISE == {"noise_hip.hip": "k_noise"}
    assert build.NO_SCRATCH_MEMORY == {"memory_hip.hip": "k_memory"} and build.NO_SCRATCH_FOOTPRINTS == {"footprints_hip.hip": "k_footprints"}
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    funcs = _header_functions(_nz_header())
    assert sorted(funcs) == ["atr_noise_windows"] == sorted(noise.NOISE_PROTOTYPES)
    assert sorted(funcs) == _header_symbols("atr_noise.h", "atr_") and _header_structs(_nz_header()) == {}
    for name, (res, params) in funcs.items():
        assert hasattr(lib, name), name
        restype, argtypes = noise.NOISE_PROTOTYPES[name]
        assert _py_class(restype) == res == ctypes.c_int, name
        assert len(argtypes) == len(params) == 13, name
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _py_class(a) == c, (name, i)
    params = funcs["atr_noise_windows"][1]
    assert [i for i, c in enumerate(params) if c == "ptr"] == [0, 1, 5, 12]
    assert "atr_noise_windows" not in fused.ATR_PROTOTYPES and "atr_noise_windows" not in vec_env.ABI_SYMBOLS
    assert noise.window_grid is occlusion.window_grid
    txt = open(os.path.join(ROOT, "include", "atr_noise.h")).read()
    const = lambda name: int(re.search(r"#define\s+ATR_NOISE_%s\s+(\d+)" % name, txt).group(1))
    assert [const(n) for n in ("WINDOW", "CENTRE", "ONE", "TAG", "PEEK", "ADVANCE")] == \
        [noise.WINDOW, noise.CENTRE, noise.ONE, noise.TAG, noise.PEEK, noise.ADVANCE] == \
        [sp.WINDOW, sp.CENTRE, sp.ONE, sp.TAG, sp.PEEK, sp.ADVANCE] == [169, 84, 1 << 24, 0x4E5E0000, 0, 1]
    assert noise.ROLES == {"tracker": 1, "target": 2, "both": 3} and noise.KEY_SALT == sp.KEY_SALT == 0x6E6F6973655F7632
    for seed in (0, 1, -1, 2 ** 64 + 5, 12345):
        assert noise.key_of(seed) == sp.key_of(seed) == (seed & (2 ** 64 - 1)) ^ 0x6E6F6973655F7632
    rule = open(os.path.join(ROOT, "active_tracking_rl_amd", "csrc", "atr_noise_rule.h")).read()
    assert "hip_runtime" not in rule
    src = open(os.path.join(ROOT, "active_tracking_rl_amd", "csrc", "noise_hip.hip")).read()
    assert "static_assert" in src and "atr_noise_rule.h" in src and "__shared__" not in src and "atomic" not in src


def test_binding_checks_status_and_refuses_before_the_handle():
    """lib() binds the table with an errcheck that raises with the entry point's name and the library's text; every handle-free
    refusal of the header is reached with h = NULL and one bad argument, in the header's order; all-good arguments with h = NULL
    give the null-handle text (this test runs without a device, on addresses that are never read)."""
    from active_tracking_rl_amd import build, noise
    build.build()
    L = noise.lib()
    for name, (restype, argtypes) in noise.NOISE_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
        assert f.errcheck(0, None, ()) == 0
        with pytest.raises(RuntimeError, match=r"^%s failed \(-1\): " % name):
            f.errcheck(-1, None, ())
    p, q = 1 << 20, 1 << 24        # any non-null, aligned addresses: a refused call never reads them
    ok = dict(h=None, obs=p, is_u8=True, se=338, sp=169, clock=q, key=KEY, flicker=1, miss=2, ghost=3, roles=1, mode=1, stream=None)
    cases = [(dict(obs=0), "null pointer"), (dict(clock=0), "null pointer"), (dict(obs=0, clock=0, flicker=-1), "null pointer"),
             (dict(flicker=-1), r"flicker threshold -1 outside 0 \.\. 16777216"),
             (dict(flicker=ONE + 1, miss=-1), r"flicker threshold 16777217 outside"),
             (dict(miss=-1), r"miss threshold -1 outside 0 \.\. 16777216"), (dict(miss=ONE + 1, ghost=-1), r"miss threshold 16777217"),
             (dict(ghost=-5), r"ghost threshold -5 outside 0 \.\. 16777216"), (dict(ghost=ONE + 1, roles=0), r"ghost threshold 16777217"),
             (dict(roles=0), r"roles 0 outside 1 \.\. 3"), (dict(roles=4), r"roles 4 outside 1 \.\. 3"),
             (dict(roles=-1, mode=2), r"roles -1 outside"),
             (dict(mode=-1), r"mode -1 outside 0 \.\. 1"), (dict(mode=2), r"mode 2 outside 0 \.\. 1"), (dict(mode=2, se=-1), r"mode 2 outside"),
             (dict(se=-338), "negative element stride"), (dict(sp=-1), "negative element stride"),
             (dict(sp=-1, obs=p + 2, is_u8=False), "negative element stride"),
             (dict(obs=p + 2, is_u8=False), "float32 windows not 4-byte aligned"),
             (dict(obs=p + 1, is_u8=False, clock=q + 1), "float32 windows not 4-byte aligned"),
             (dict(clock=q + 2), "is not 4-byte aligned"), (dict(clock=q + 1, obs=p + 3), "is not 4-byte aligned"),
             (dict(), "null handle"), (dict(is_u8=False, mode=0, roles=3, flicker=0, miss=ONE, ghost=ONE, se=0, sp=0, key=0), "null handle"),
             (dict(obs=p + 3, key=2 ** 64 - 1), "null handle")]
    for change, text in cases:
        with pytest.raises(RuntimeError, match=r"^atr_noise_windows failed \(-1\): atr_noise_windows: .*%s" % text):
            noise.noise_windows(**dict(ok, **change))


def test_the_tensor_checks():
    """noise_ refuses a host tensor (there is no host path); threshold_of, thresholds_of and roles_of take what the header allows
    and nothing else."""
    import torch
    from active_tracking_rl_amd import noise
    with pytest.raises(RuntimeError, match="there is no host path"):
        noise.noise_(torch.zeros(2, 2, 13, 13, dtype=torch.uint8), noise.new_clock(2, "cpu"), None, 1, KEY, (1, 1, 1))
    with pytest.raises(RuntimeError, match="there is no host path"):
        noise.noise_(np.zeros((2, 2, 13, 13), np.uint8), np.zeros((2, 2), np.uint32), None, 1, KEY, (1, 1, 1))
    assert [noise.threshold_of(p) for p in (0, 0.0, 1, 1.0, 0.5, 0.05, 2.0 ** -25, 2.0 ** -24)] == \
        [0, 0, ONE, ONE, 1 << 23, round(0.05 * ONE), 0, 1] == [sp.threshold_of(p) for p in (0, 0, 1, 1, 0.5, 0.05, 2.0 ** -25, 2.0 ** -24)]
    for bad in (-0.1, 1.0001, True, False, "0.5", None, float("nan"), (0.5,), 2):
        with pytest.raises(ValueError, match=r"a sensor-noise rate must be a number in \[0, 1\]"):
            noise.threshold_of(bad)
    assert noise.thresholds_of({"flicker": .05, "miss": .1, "ghost": .5}) == (round(.05 * ONE), round(.1 * ONE), 1 << 23)
    assert noise.thresholds_of({"miss": 1}) == (0, ONE, 0) and noise.thresholds_of({"ghost": 0.25, "flicker": 0}) == (0, 0, 1 << 22)
    for bad in ({"flicker": .1, "blur": .1}, {"Miss": .1}, {1: .1}):
        with pytest.raises(ValueError, match="unknown key"):
            noise.thresholds_of(bad)
    for bad in ({}, {"flicker": 0}, {"flicker": 0.0, "miss": 0, "ghost": 0}, {"miss": 1e-9}):
        with pytest.raises(ValueError, match="every rate is 0"):
            noise.thresholds_of(bad)
    for bad in (None, 0.1, "flicker", [("flicker", .1)], True):
        with pytest.raises(ValueError, match="sensor_noise must be a dict"):
            noise.thresholds_of(bad)
    with pytest.raises(ValueError, match="a sensor-noise rate must be a number"):
        noise.thresholds_of({"flicker": "0.1"})
    assert [noise.roles_of(w) for w in ("tracker", "target", "both")] == [1, 2, 3]
    for bad in ("Tracker", "all", 1, None, True):
        with pytest.raises(ValueError, match="noise_for must be one of"):
            noise.roles_of(bad)
    c = noise.new_clock(3, "cpu")
    assert c.dtype == torch.uint32 and tuple(c.shape) == (3, 2) and not c.view(torch.int32).any() and c.is_contiguous()


# -- flags and refusals ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("script", ["main.py", "gym_eval.py"])
def test_both_parsers_list_the_flags(script):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0
    for flag in ("--noise-flicker P", "--noise-miss P", "--noise-ghost P", "--noise-for WHO"):
        assert flag in r.stdout, flag
    assert "--sensor-noise" not in r.stdout


NAV = "Track2D-BlockPartialNav-v0"


@pytest.mark.parametrize("script,argv,text", [
    ("main.py", ["--noise-flicker", "0.1", "--tracking-stats"], "--tracking-stats / --sight-stats"),
    ("main.py", ["--noise-miss", "0.1", "--sight-stats"], "--tracking-stats / --sight-stats"),
    ("main.py", ["--noise-ghost", "0.1", "--render"], "cannot be combined with --render"),
    ("main.py", ["--noise-for", "both"], "--noise-for needs --noise-flicker, --noise-miss or --noise-ghost"),
    ("main.py", ["--noise-for", "tracker"], "--noise-for needs --noise-flicker, --noise-miss or --noise-ghost"),
    ("main.py", ["--noise-flicker", "1.5"], "is not a rate in [0, 1]"),
    ("main.py", ["--noise-miss", "-0.1"], "is not a rate in [0, 1]"),
    ("main.py", ["--noise-ghost", "often"], "is not a number"),
    ("main.py", ["--noise-ghost", "0"], "every rate is 0"),
    ("main.py", ["--noise-miss", "0.1", "--noise-for", "all"], "invalid choice"),
    ("main.py", ["--noise-miss", "0.1", "--noise-for", "both", "--env-base", NAV],
     "the scripted target of --env-base Track2D-BlockPartialNav-v0 reads no window"),
    ("main.py", ["--noise-flicker", "0.1", "--noise-for", "target", "--env", "Track2D-MazePartialRam-v0"],
     "the scripted target of --env Track2D-MazePartialRam-v0 reads no window"),
    ("main.py", ["--noise-flicker", "0.1", "--env", "Track2D-BlockFullPZR-v0"], "--env Track2D-BlockFullPZR-v0 observes the whole map"),
    ("gym_eval.py", ["--noise-ghost", "0.1", "--noise-for", "both", "--env", NAV],
     "the scripted target of Track2D-BlockPartialNav-v0 reads no window"),
    ("gym_eval.py", ["--noise-flicker", "0.1", "--render"], "cannot be combined with --render"),
    ("gym_eval.py", ["--noise-for", "target"], "--noise-for needs --noise-flicker, --noise-miss or --noise-ghost"),
    ("gym_eval.py", ["--noise-miss", "2"], "is not a rate in [0, 1]"),
    ("gym_eval.py", ["--noise-miss", "0.2", "--env", "Track2D-BlockFullPZR-v0"], "observes the whole map"),
])
def test_parsers_refuse(script, argv, text):
    """The refused combinations end the command in the parser, before a device is looked for (this test runs without one)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and text in r.stderr, r.stderr[-400:]


def test_default_args_and_create_env_refusals():
    """train.default_args carries the four settings; create_env refuses the rates on a whole-map id, with traces and on the batched
    rng='numpy' envs, and --noise-for alone; VecEnv and Track2DEnv refuse a whole-map id, traces, a bad dict or role, noise_for
    without sensor_noise and a noisy window for a scripted target themselves — all before a device is touched (this test runs
    without one)."""
    from active_tracking_rl_amd import environment
    from active_tracking_rl_amd.train import default_args
    d = default_args()
    assert d.noise_flicker is None and d.noise_miss is None and d.noise_ghost is None and d.noise_for is None
    assert default_args(noise_miss=0.1).noise_miss == 0.1
    ns = lambda **kw: argparse.Namespace(**dict(dict(noise_flicker=0.05, noise_miss=None, noise_ghost=None, noise_for=None,
                                                     stack_frames=1, seed=1, gpu_ids=[0]), **kw))
    for n in (4, 1):
        with pytest.raises(ValueError, match="need the 13 x 13 windows"):
            environment.create_env("Track2D-BlockFullPZR-v0", ns(), num_envs=n)
        with pytest.raises(NotImplementedError, match="with episode traces"):
            environment.create_env(PARTIAL, ns(), num_envs=n, traces=True)
        with pytest.raises(ValueError, match="--noise-for needs --noise-flicker, --noise-miss or --noise-ghost"):
            environment.create_env(PARTIAL, ns(noise_flicker=None, noise_for="both"), num_envs=n)
        with pytest.raises(ValueError, match="every rate is 0"):
            environment.create_env(PARTIAL, ns(noise_flicker=0.0), num_envs=n)
        with pytest.raises(ValueError, match="scripted"):
            environment.create_env(NAV, ns(noise_for="both"), num_envs=n)
    for rng in ("numpy", "numpy-device"):
        with pytest.raises(NotImplementedError, match="are not wired to the batched rng='numpy' envs"):
            environment.create_env(PARTIAL, ns(noise_flicker=None, noise_ghost=0.5), num_envs=4, rng=rng)
    on = {"miss": 0.1}
    with pytest.raises(ValueError, match="needs the 13 x 13 windows"):
        environment.VecEnv("Track2D-MazeFullNav-v0", 4, sensor_noise=on)
    with pytest.raises(ValueError, match="needs the 13 x 13 windows"):
        environment.Track2DEnv("Track2D-BlockFullPZR-v0", sensor_noise=on)
    with pytest.raises(NotImplementedError, match="traces=True"):
        environment.VecEnv(PARTIAL, 4, sensor_noise=on, traces=True, auto_reset=False)
    with pytest.raises(NotImplementedError, match="traces=True"):
        environment.Track2DEnv(PARTIAL, sensor_noise=on, traces=True)
    for bad, text in (({}, "every rate is 0"), ({"blur": 1}, "unknown key"), (0.1, "must be a dict"), ({"miss": 2}, "number in"),
                      (True, "must be a dict")):
        with pytest.raises(ValueError, match=text):
            environment.VecEnv(PARTIAL, 4, sensor_noise=bad)
    with pytest.raises(ValueError, match="noise_for must be one of"):
        environment.VecEnv(PARTIAL, 4, sensor_noise=on, noise_for="all")
    with pytest.raises(ValueError, match="noise_for='both' needs sensor_noise"):
        environment.VecEnv(PARTIAL, 4, noise_for="both")
    with pytest.raises(ValueError, match="noise_for='tracker' needs sensor_noise"):
        environment.Track2DEnv(PARTIAL, noise_for="tracker")
    for env_id in ("Track2D-BlockPartialRam-v0", NAV, "Track2D-MazePartialRPF-v0"):
        for who in ("target", "both"):
            with pytest.raises(ValueError, match="scripted"):
                environment.VecEnv(env_id, 4, sensor_noise=on, noise_for=who)
            with pytest.raises(ValueError, match="scripted"):
                environment.Track2DEnv(env_id, sensor_noise=on, noise_for=who, rng="numpy" if "RPF" not in env_id else "philox")


def test_none_means_every_model_driven_player(monkeypatch):
    """noise_for=None: both players, the tracker alone where the target is scripted (read off an env whose handle is never made)."""
    from active_tracking_rl_amd import environment, noise

    class Stop(Exception):
        pass

    def no_handle(*a, **k):
        raise Stop()
    monkeypatch.setattr(environment, "VecTrack2D", no_handle)
    seen = {}
    for env_id, who in ((PARTIAL, None), (NAV, None), (NAV, "tracker"), (PARTIAL, "target"), (PARTIAL, "tracker")):
        env = object.__new__(environment.VecEnv)
        with pytest.raises(Stop):
            env.__init__(env_id, 4, seed=7, sensor_noise={"flicker": .05, "ghost": .5}, noise_for=who)
        seen[(env_id, who)] = (env.noise_for, env._noise_roles)
        assert env._noise_thresholds == (round(.05 * ONE), 0, 1 << 23) and env._noise_key == noise.key_of(7)
    assert seen == {(PARTIAL, None): ("both", 3), (NAV, None): ("tracker", 1), (NAV, "tracker"): ("tracker", 1),
                    (PARTIAL, "target"): ("target", 2), (PARTIAL, "tracker"): ("tracker", 1)}
    env = object.__new__(environment.VecEnv)
    with pytest.raises(Stop):
        env.__init__(PARTIAL, 4)
    assert env.sensor_noise is None and env._noise_roles == 0 and env._noise_clock is None


def test_without_the_option_nothing_is_launched(monkeypatch):
    """VecEnv._disturb with the noise off hands the tensor back untouched, never reaches the binding and does not import the
    module; with it on it hands the binding the windows, the env's clock, the core, the mode, the key, the thresholds and the
    roles; fused_step_out declines."""
    code = ("import sys; from active_tracking_rl_amd import environment; "
            "env = object.__new__(environment.VecEnv); env._noise_roles = 0; o = object(); "
            "assert env._disturb(o, 1) is o and env._disturb(o, 0) is o; "
            "assert 'active_tracking_rl_amd.noise' not in sys.modules; print('clean')")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "clean", r.stderr[-400:]

    from active_tracking_rl_amd import environment, noise
    calls = []
    monkeypatch.setattr(noise, "noise_", lambda *a: calls.append(a))
    env = object.__new__(environment.VecEnv)
    env._noise_roles = 0
    obs = object()
    assert env._disturb(obs, 1) is obs and env._disturb(obs, 0) is obs
    assert calls == []

    class Core(object):
        auto_reset = True
        supports_u8 = True
    env._noise_roles, env._noise_clock, env._noise_key, env._noise_thresholds, env.core = 3, "clock", 99, (1, 2, 3), Core()
    assert env._disturb(obs, 1) is obs and env._disturb(obs, 0) is obs
    assert calls == [(obs, "clock", env.core, 1, 99, (1, 2, 3), 3), (obs, "clock", env.core, 0, 99, (1, 2, 3), 3)]
    assert (environment.VecEnv._NOISE_PEEK, environment.VecEnv._NOISE_ADVANCE) == (noise.PEEK, noise.ADVANCE) == (0, 1)
    env.stack_frames, env.rescale, env.occlusion, env.fov, env.obs_u8 = 1, False, False, None, True
    env.footprints, env._memory_roles, env._ego_roles = None, 0, 0
    assert env.fused_step_out(("o", "r", "d")) is None
