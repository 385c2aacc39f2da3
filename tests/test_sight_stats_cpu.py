"""CPU-side checks of the sight statistics: include/atr_sight.h against the built library and sight_stats.SIGHT_PROTOTYPES; the
refusals that come before any device is touched; the host model classify() against the one-sample-at-a-time rule of sight_spec on
synthetic stores, across split calls and on hand-made windows that pin the line's rounding, the enclosed target and the longest
corridor; the table identities; summarize() on tables filled by hand; the occlusion map; the flag of main.py; and the call site in
train.rollout."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sight_spec as sp
from conftest import ROOT
from test_abi_cpu import _header_functions, _header_structs, _header_symbols, _py_class


def _sight_header():
    """include/atr_sight.h without comments and preprocessor lines."""
    txt = open(os.path.join(ROOT, "include", "atr_sight.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    return "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", txt).split("\n") if not ln.lstrip().startswith("#"))


def test_header_prototypes_and_exports_agree():
    """Every function of the header is exported by the built library and bound by SIGHT_PROTOTYPES with the header's parameter
    count and classes; the header's constants are the module's (776 counters in ten segments); the new source is in the build and
    under its no-scratch check; no symbol holds `track_stats`."""
    from active_tracking_rl_amd import build, sight_stats, vec_env
    build.build()
    assert os.path.join("..", "..", "include", "atr_sight.h") in build.HEADERS
    assert "sight_stats_hip.hip" in build.SOURCES and build.NO_SCRATCH_SIGHT == {"sight_stats_hip.hip": "k_sight"}
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    funcs = _header_functions(_sight_header())
    assert sorted(funcs) == ["atr_sight_stats", "atr_sight_stats_drain"] == sorted(sight_stats.SIGHT_PROTOTYPES)
    assert sorted(funcs) == _header_symbols("atr_sight.h", "atr_") and not [s for s in funcs if "track_stats" in s]
    assert _header_structs(_sight_header()) == {}
    for name, (res, params) in funcs.items():
        assert hasattr(lib, name), name
        restype, argtypes = sight_stats.SIGHT_PROTOTYPES[name]
        assert _py_class(restype) == res == ctypes.c_int, name
        assert len(argtypes) == len(params), name
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _py_class(a) == c, (name, i)
    assert [c for c in funcs["atr_sight_stats"][1] if c is ctypes.c_longlong] == [ctypes.c_longlong] * 8        # the strides
    assert len(funcs["atr_sight_stats"][1]) == 18 and len(funcs["atr_sight_stats_drain"][1]) == 3
    txt = open(os.path.join(ROOT, "include", "atr_sight.h")).read()
    const = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, txt).group(1))
    names = ("SEEN", "BLOCKED", "NOPATH", "PATH", "DETOUR", "TRANS", "OUT", "TERMINAL", "INCONSISTENT", "SAMPLES", "TABLE")
    assert [const("ATR_SIGHT_" + n) for n in names] == [getattr(sight_stats, n) for n in names] == [getattr(sp, n) for n in names] \
        == [0, 169, 338, 507, 676, 761, 770, 771, 772, 773, 776]
    assert [const("ATR_SIGHT_" + n) for n in ("WINDOW", "CENTRE", "BIN_OUT", "BIN_TERMINAL", "BIN_INCONSISTENT")] == \
        [sight_stats.WINDOW, sight_stats.CENTRE, sight_stats.BIN_OUT, sight_stats.BIN_TERMINAL, sight_stats.BIN_INCONSISTENT] == \
        [169, 84, 169, 170, 171]
    assert [const("ATR_SIGHT_" + n) for n in ("CLEAR", "BLOCKED_CLASS", "OUT_CLASS")] == \
        [sight_stats.CLEAR, sight_stats.BLOCKED_CLASS, sight_stats.OUT_CLASS] == [0, 1, 2]
    assert const("ATR_SIGHT_MAX_PATH") == sight_stats.MAX_PATH == 168 and const("ATR_SIGHT_MAX_T") == 1 << 20
    assert const("ATR_SIGHT_NO_AUTO_RESET") == sight_stats.NO_AUTO_RESET == 1
    assert sight_stats.DETOUR + sight_stats.N_DETOUR == sight_stats.TRANS and sight_stats.TRANS + 9 == sight_stats.OUT
    # the bins are tracking_stats' own
    from active_tracking_rl_amd import tracking_stats
    assert (sight_stats.BIN_OUT, sight_stats.BIN_TERMINAL, sight_stats.BIN_INCONSISTENT) == \
        (tracking_stats.OUT, tracking_stats.TERMINAL, tracking_stats.INCONSISTENT)


def test_binding_checks_status_and_refuses_before_any_device():
    """lib() binds the table with an errcheck that raises with the entry point's name and the library's text; null or misaligned
    pointers, T <= 0, T above the bound, N <= 0, unknown flags and negative strides are refused by the argument checks, which come
    before anything touches a device (this test runs without one)."""
    from active_tracking_rl_amd import build, sight_stats
    build.build()
    L = sight_stats.lib()
    for name, (restype, argtypes) in sight_stats.SIGHT_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
        assert f.errcheck(0, None, ()) == 0
        with pytest.raises(RuntimeError, match=r"^%s failed \(-1\): " % name):
            f.errcheck(-1, None, ())
    p = 4096        # any non-null, aligned address: a refused call never reads it
    ok = dict(obs=p, obs_is_u8=True, obs_strides=(338 * 5, 338, 169), rew=p, rew_strides=(10, 2, 1), done=p, done_strides=(5, 1),
              carry=p, tab=p, T=20, N=5, flags=0, stream=None)
    cases = [(dict(obs=0), "null pointer"), (dict(rew=0), "null pointer"), (dict(done=0), "null pointer"),
             (dict(carry=0), "null pointer"), (dict(tab=0), "null pointer"),
             (dict(N=0), "N > 0"), (dict(N=-3), "N > 0"), (dict(T=0), "T > 0"), (dict(T=-1), "T > 0"), (dict(T=(1 << 20) + 1), "above"),
             (dict(flags=2), "unknown flags"), (dict(flags=3), "unknown flags"), (dict(tab=p + 4), "not 8-byte aligned"),
             (dict(carry=p + 2), "not 4-byte aligned"), (dict(rew=p + 2), "not 4-byte aligned"),
             (dict(obs=p + 1, obs_is_u8=False), "not 4-byte aligned"), (dict(obs_strides=(1690, -338, 169)), "negative element stride"),
             (dict(obs_strides=(-1690, 338, 169)), "negative element stride"), (dict(obs_strides=(1690, 338, -169)), "negative element stride"),
             (dict(rew_strides=(10, 2, -1)), "negative element stride"), (dict(rew_strides=(-10, 2, 1)), "negative element stride"),
             (dict(done_strides=(5, -1)), "negative element stride"), (dict(done_strides=(-5, 1)), "negative element stride")]
    for change, text in cases:
        with pytest.raises(RuntimeError, match=r"^atr_sight_stats failed \(-1\): atr_sight_stats: .*%s" % text):
            sight_stats.sight_stats(**dict(ok, **change))
    for args, text in (((0, p), "null pointer"), ((p, 0), "null pointer"), ((p + 4, p), "not 8-byte aligned"),
                       ((p, p + 4), "not 8-byte aligned")):
        with pytest.raises(RuntimeError, match=r"^atr_sight_stats_drain failed \(-1\): atr_sight_stats_drain: .*%s" % text):
            sight_stats.sight_stats_drain(*args, None)


def test_no_host_counting_path():
    import torch
    from active_tracking_rl_amd import sight_stats
    with pytest.raises(RuntimeError, match="lives on the GPU"):
        sight_stats.SightStats(object(), torch.device("cpu"))


def test_line_cells_and_masks():
    """line_cells is the header's formula; line_masks holds exactly those cells; m = 1 has none; a diagonal is the diagonal; the
    rule is the tracker's line: drawn from the target's end it differs for 56 of the 168 offsets."""
    from active_tracking_rl_amd import sight_stats
    masks = sight_stats.line_masks()
    assert masks.shape == (169, 13) and masks.dtype == np.uint16 and not masks[84].any()
    asymmetric = 0
    for dr, dc in sp.OFFSETS:
        cells = sight_stats.line_cells(dr, dc)
        assert cells == sp.line(dr, dc) and len(cells) == max(abs(dr), abs(dc)) - 1 and len(set(cells)) == len(cells)
        got = {(r, c) for r in range(13) for c in range(13) if masks[(dr + 6) * 13 + dc + 6, r] >> c & 1}
        assert got == set(cells) and (6, 6) not in got and (6 + dr, 6 + dc) not in got
        back = sorted((r + dr, c + dc) for r, c in sp.line(-dr, -dc))
        asymmetric += back != sorted(cells)
    assert asymmetric == 56
    assert sight_stats.line_cells(4, -4) == [(7, 5), (8, 4), (9, 3)] and sight_stats.line_cells(0, 3) == [(6, 7), (6, 8)]
    assert sight_stats.line_cells(1, 1) == [] and sight_stats.line_cells(-1, 0) == []
    assert sight_stats.line_cells(2, 1) == [(7, 7)] and sight_stats.line_cells(-2, -1) == [(5, 5)]        # the tie rounds away
    assert sight_stats.line_cells(6, 3) == [(7, 7), (8, 7), (9, 8), (10, 8), (11, 9)]


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("steps", [1, 7, 20])
@pytest.mark.parametrize("n", [1, 37])
def test_classify_equals_the_loop_spec(n, steps, flags):
    """The vectorised host model against the rule written one sample at a time, on synthetic stores with every kind of sample;
    the table identities hold, and the SEEN segment is tracking_stats' offset histogram."""
    from active_tracking_rl_amd import sight_stats, tracking_stats
    obs, rew, done, act, kinds = sp.synthetic_store(steps, n, 5)
    tab, carry = sight_stats.classify(obs, rew, done, flags=flags)
    w_tab, w_carry, classes, paths = sp.loop_model(obs, rew, done, flags=flags)
    sp.assert_equal((tab, carry), (w_tab, w_carry), (n, steps, flags))
    assert tab.dtype == np.int64 and tab.shape == (776,) and carry.dtype == np.int32 and carry.shape == (n,)
    sp.check_identities(tab, tracking_stats.classify(obs, rew, done, flags=flags)[0])
    assert tab[sp.SAMPLES] == steps * n and (tab[sp.TERMINAL] == 0 if flags else tab[sp.TERMINAL] == done.sum())
    as_float = sight_stats.classify(obs.astype(np.float32), rew, done, flags=flags)
    sp.assert_equal(as_float, (tab, carry), "float32 store")


def test_the_store_exercises_every_segment():
    """synthetic_store(20, 37, seed=5): 397 in-view, non-co-located samples, 141 CLEAR and 256 BLOCKED; 40 without a path inside
    the window, 357 with one, P up to 33 and detours 0 .. 30."""
    obs, rew, done, act, kinds = sp.synthetic_store(20, 37, 5)
    tab, carry, classes, paths = sp.loop_model(obs, rew, done)
    apart = paths >= 0
    assert apart.sum() == 397 and (classes[apart] == sp.CLEAR).sum() == 141 and (classes[apart] == sp.BLOCKED_CLASS).sum() == 256
    assert (paths[apart] == 0).sum() == 40 == tab[sp.NOPATH:sp.NOPATH + 169].sum() and tab[sp.PATH:sp.PATH + 169].sum() == 357
    assert paths.max() == 33 and np.flatnonzero(tab[sp.PATH:sp.PATH + 169]).max() == 33
    detours = np.flatnonzero(tab[sp.DETOUR:sp.DETOUR + 85])
    assert detours.min() == 0 and detours.max() == 15 and tab[sp.BLOCKED:sp.BLOCKED + 169].sum() == 256
    assert tab[sp.SEEN + 84] > 0 and tab[sp.OUT] > 0 and tab[sp.TERMINAL] > 0 and tab[sp.INCONSISTENT] > 0
    assert (tab[sp.TRANS:sp.TRANS + 9] > 0).all()


def test_split_calls_equal_one_call():
    """T = 7 as 3 + 4 and as 7 x 1 equals one call, counter for counter: the transitions cross the boundary and the carry after a
    done step is -1; a carry outside [-1, 2] is read as -1."""
    from active_tracking_rl_amd import sight_stats
    for flags in (0, 1):
        obs, rew, done, act, _ = sp.synthetic_store(7, 6, 21 + flags, p_bad=0.05)
        done[2, 0], done[3, 1], done[6, 2] = 1, 1, 1          # a done on the last step of the first part, the first of the second
        whole = sight_stats.classify(obs, rew, done, flags=flags)
        assert whole[1][2] == -1
        for cuts in ((3,), (1, 2, 3, 4, 5, 6)):
            tab = carry = None
            for a, b in zip((0,) + cuts, cuts + (7,)):
                tab, carry = sight_stats.classify(obs[a:b + 1], rew[a:b], done[a:b], carry=carry, flags=flags, tab=tab)
                if b == 3:
                    assert carry[0] == -1 and (carry[3:] >= -1).all()
            sp.assert_equal((tab, carry), whole, (flags, cuts))
        # without the carry the boundary's transitions would be lost: the split is not trivially equal
        # (37 envs: some env is sure to be in a classified state on both sides of the cut)
        wide = sp.synthetic_store(7, 37, 23 + flags, p_bad=0.05)[:3]
        trans = lambda o, r, d: sight_stats.classify(o, r, d, flags=flags)[0][sp.TRANS:sp.TRANS + 9].sum()
        assert trans(wide[0][3:], wide[1][3:], wide[2][3:]) + trans(wide[0][:4], wide[1][:3], wide[2][:3]) < trans(*wide)
        bad = np.array([3, -2, 1 << 20, -1, 2, 0], np.int32)
        fixed = np.array([-1, -1, -1, -1, 2, 0], np.int32)
        sp.assert_equal(sight_stats.classify(obs, rew, done, carry=bad, flags=flags),
                        sight_stats.classify(obs, rew, done, carry=fixed, flags=flags), "carry out of range")
        sp.assert_equal(sight_stats.classify(obs, rew, done, carry=bad, flags=flags),
                        sp.loop_model(obs, rew, done, carry=bad, flags=flags)[:2], "carry out of range, loop")


def test_a_wall_on_each_line_cell_blocks_and_walls_elsewhere_do_not():
    """For each of the 168 offsets: a wall on each single line cell in turn gives BLOCKED; walls everywhere EXCEPT the line cells
    and the end cells give CLEAR (and, beyond the 4-neighbours, no path unless the line itself is 4-connected)."""
    from active_tracking_rl_amd import sight_stats
    for dr, dc in sp.OFFSETS:
        b = (dr + 6) * 13 + dc + 6
        n_line = len(sp.line(dr, dc))
        for k in range(n_line):
            tab, _ = sight_stats.classify(*sp.store_of([sp.wall_on_line_cell(dr, dc, k)]))
            assert tab[sp.SEEN + b] == 1 and tab[sp.BLOCKED + b] == 1, (dr, dc, k)
        tab, carry = sight_stats.classify(*sp.store_of([sp.walls_off_the_line(dr, dc)]))
        assert tab[sp.SEEN + b] == 1 and tab[sp.BLOCKED:sp.BLOCKED + 169].sum() == 0 and carry[0] == sp.CLEAR, (dr, dc)
        straight = dr == 0 or dc == 0
        assert tab[sp.NOPATH + b] == (0 if straight else 1), (dr, dc)
        if straight:
            assert tab[sp.PATH + abs(dr) + abs(dc)] == 1 and tab[sp.DETOUR] == 1
    # all of them as one store, against the loop
    samples = [sp.wall_on_line_cell(dr, dc, k) for dr, dc in sp.OFFSETS for k in range(len(sp.line(dr, dc)))]
    samples += [sp.walls_off_the_line(dr, dc) for dr, dc in sp.OFFSETS]
    store = sp.store_of(samples)
    sp.assert_equal(sight_stats.classify(*store), sp.loop_model(*store)[:2], "line store")


def test_enclosed_target_longest_corridor_and_open_windows():
    """A target enclosed by walls gives NOPATH; the serpentine corridor gives its stated length, 64 (at least 48 asked); a
    wall-free window gives P = |dr| + |dc| and detour 0 for all offsets."""
    from active_tracking_rl_amd import sight_stats
    for dr, dc in ((2, 0), (-3, 4), (6, 6), (-6, 0), (1, 1), (0, -5)):
        b = (dr + 6) * 13 + dc + 6
        tab, carry = sight_stats.classify(*sp.store_of([sp.enclosed(dr, dc)]))
        assert tab[sp.NOPATH + b] == 1 and tab[sp.PATH:sp.PATH + 169].sum() == 0 and tab[sp.SEEN + b] == 1, (dr, dc)
    obs, rew, dr, dc, P = sp.longest_window()
    assert P == sp.LONGEST_PATH == 64 >= 48 and sp.bfs(obs[0].reshape(13, 13).tolist(), dr, dc) == P
    tab, carry = sight_stats.classify(*sp.store_of([(obs, rew)]))
    assert tab[sp.PATH + P] == 1 and tab[sp.DETOUR + (P - 12) // 2] == 1 and tab[sp.BLOCKED + 0] == 1 and carry[0] == sp.BLOCKED_CLASS
    sp.check_identities(tab)
    open_ = [sp.pair(np.zeros((13, 13), np.uint8), dr, dc) for dr, dc in sp.OFFSETS]
    tab, carry = sight_stats.classify(*sp.store_of(open_))
    want = np.bincount([abs(dr) + abs(dc) for dr, dc in sp.OFFSETS], minlength=169)
    assert np.array_equal(tab[sp.PATH:sp.PATH + 169], want) and tab[sp.DETOUR] == 168 and tab[sp.DETOUR + 1:sp.TRANS].sum() == 0
    assert tab[sp.BLOCKED:sp.NOPATH + 169].sum() == 0 and (carry == sp.CLEAR).all()
    sp.check_identities(tab)


def test_summarize_on_tables_built_by_hand():
    """Rates are exact rationals of the counts; compared at float64 rounding of the few operations involved (4 ulp)."""
    from active_tracking_rl_amd import sight_stats
    tab = np.zeros(776, np.int64)
    b = lambda dr, dc: (dr + 6) * 13 + dc + 6
    tab[sp.SEEN + b(0, 3)], tab[sp.SEEN + b(-4, 0)], tab[sp.SEEN + b(6, 6)], tab[sp.SEEN + b(0, 0)] = 5, 3, 2, 4
    tab[sp.BLOCKED + b(0, 3)], tab[sp.BLOCKED + b(6, 6)] = 2, 2
    tab[sp.NOPATH + b(6, 6)] = 1
    tab[sp.PATH + 3], tab[sp.PATH + 5], tab[sp.PATH + 4], tab[sp.PATH + 14] = 3, 2, 3, 1
    tab[sp.DETOUR + 0], tab[sp.DETOUR + 1] = 6, 3
    tab[sp.OUT], tab[sp.TERMINAL], tab[sp.INCONSISTENT] = 6, 7, 1
    tab[sp.SAMPLES] = 14 + 6 + 7 + 1
    tab[sp.TRANS:sp.TRANS + 9] = [5, 3, 2, 2, 3, 1, 1, 0, 2]
    sp.check_identities(tab)
    s = sight_stats.summarize(tab)
    close = lambda got, want: abs(got - want) <= 4 * np.spacing(abs(want))
    assert (s["samples"], s["terminal"], s["inconsistent"], s["in_view"], s["apart"], s["blocked"], s["no_path"], s["out"]) == \
        (28, 7, 1, 14, 10, 4, 1, 6) and s["transitions"] == 19
    assert close(s["sight_clear_rate"], 6 / 10) and close(s["occluded_rate"], 4 / 10) and close(s["no_path_rate"], 1 / 10)
    assert close(s["unseen_rate"], (4 + 6) / 20)
    assert close(s["mean_path"], (3 * 3 + 2 * 5 + 3 * 4 + 14) / 9) and close(s["mean_detour"], 6 / 9)
    assert close(s["lost_to_occlusion_rate"], 3 / 10) and close(s["lost_to_range_rate"], 2 / 10)
    assert close(s["reacquire_rate"], (2 + 1) / 9)
    import torch
    assert sight_stats.summarize(torch.from_numpy(tab)) == s
    # empty denominators
    s = sight_stats.summarize(np.zeros(776, np.int64))
    assert (s["samples"], s["terminal"], s["inconsistent"], s["transitions"]) == (0, 0, 0, 0)
    rates = ("sight_clear_rate", "occluded_rate", "no_path_rate", "unseen_rate", "mean_path", "mean_detour", "lost_to_occlusion_rate",
             "lost_to_range_rate", "reacquire_rate")
    for key in rates:
        assert np.isnan(s[key]), key
    only_out = np.zeros(776, np.int64)
    only_out[sp.OUT] = only_out[sp.SAMPLES] = 3
    only_out[sp.TRANS + 8] = 2
    s = sight_stats.summarize(only_out)
    assert s["unseen_rate"] == 1.0 and s["reacquire_rate"] == 0.0 and np.isnan(s["occluded_rate"]) and np.isnan(s["mean_path"])
    assert np.isnan(s["lost_to_range_rate"])
    assert len(sight_stats.TAGS) == len(set(sight_stats.TAGS)) == 11 and all(t.startswith("train/sight_") for t in sight_stats.TAGS)


def test_occlusion_png(tmp_path):
    """occlusion_png writes a [13 * scale, 13 * scale, 3] image of BLOCKED / SEEN: an always-blocked offset brightest, a
    half-blocked one between, a never-blocked and a never-seen one dark."""
    import struct
    import zlib
    from active_tracking_rl_amd import sight_stats
    tab = np.zeros(776, np.int64)
    tab[sp.SEEN + 3 * 13 + 9], tab[sp.BLOCKED + 3 * 13 + 9] = 40, 40
    tab[sp.SEEN + 10 * 13 + 2], tab[sp.BLOCKED + 10 * 13 + 2] = 10, 5
    tab[sp.SEEN + 1 * 13 + 1] = 8
    for scale in (16, 3):
        path = os.path.join(str(tmp_path), "occlusion_%d.png" % scale)
        img = sight_stats.occlusion_png(tab, path, scale=scale)
        assert img.shape == (13 * scale, 13 * scale, 3) and img.dtype == np.uint8
        raw = open(path, "rb").read()
        assert raw[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", raw[16:24]) == (13 * scale, 13 * scale)
        n = struct.unpack(">I", raw[33:37])[0]
        rows = np.frombuffer(zlib.decompress(raw[41:41 + n]), np.uint8).reshape(13 * scale, 1 + 39 * scale)
        assert np.array_equal(rows[:, 1:].reshape(13 * scale, 13 * scale, 3), img)
        cell = lambda r, c: img[r * scale + scale // 2, c * scale + scale // 2].astype(int)
        assert cell(3, 9).tolist() == [255, 255, 64] and cell(10, 2).tolist() == [128, 64, 112]
        assert cell(1, 1).tolist() == cell(0, 0).tolist() == [0, 0, 160]
    assert sight_stats.occlusion_image(np.zeros(776, np.int64), 2).shape == (26, 26, 3)
    with pytest.raises(ValueError):
        sight_stats.occlusion_image(tab, 0)


def test_main_lists_the_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "--sight-stats" in r.stdout and "--tracking-stats" in r.stdout


def test_rollout_calls_the_update_only_when_attached():
    """train.rollout's call site with a stub: nothing attached -> nothing called; attached -> one update per rollout with the
    store's obs [T+1, ...], rew and done; beside an attached tracking-statistics object both are called once; a rollout without a
    store is an error, not a silent skip."""
    import torch
    from active_tracking_rl_amd import train

    class Stats(object):
        def __init__(self):
            self.calls = []

        def update(self, *args):
            self.calls.append(args)

    class Env(object):
        pass

    class Player(object):
        def __init__(self, env):
            self.env, self.model = env, object()
            self.rewards, self.dones, self.actions, self._buf, self._actions_buf = [], [], [], None, None

        def begin_rollout(self, n):
            self._buf = (torch.zeros(n + 1, 3, 2, 13, 13, dtype=torch.uint8), torch.zeros(n, 3, 2), torch.zeros(n, 3, dtype=torch.uint8))
            self._actions_buf = torch.arange(n * 6).reshape(n, 2, 3)

        def action_rollout(self):
            self.rewards.append(torch.zeros(3, 2, 1))
            self.dones.append(torch.zeros(3, dtype=torch.uint8))

        def action_train(self):
            self.rewards.append(torch.zeros(3, 2, 1))
            self.dones.append(torch.zeros(3, dtype=torch.uint8))

        def end_rollout(self):
            pass

        def update_rnn_hiden(self):
            pass

    env = Env()
    p = Player(env)
    train.rollout(p, 4)                                   # nothing attached
    env.sight_stats = Stats()
    train.rollout(p, 4)
    (obs, rew, done), = env.sight_stats.calls
    assert obs is p._buf[0] and rew is p._buf[1] and done is p._buf[2] and obs.shape[0] == 5
    env.tracking_stats = Stats()
    train.rollout(p, 4)
    assert len(env.sight_stats.calls) == 2 and len(env.tracking_stats.calls) == 1 and len(env.tracking_stats.calls[0]) == 4
    assert env.sight_stats.calls[1][0] is p._buf[0] is env.tracking_stats.calls[0][0]
    env.tracking_stats = None
    with pytest.raises(RuntimeError, match="sight statistics read the rollout store"):
        train.rollout(p, 4, fast=False)
    env.sight_stats = None
    train.rollout(p, 4, fast=False)                       # detached again: the slow path runs as before
    assert len(p.rewards) == 20
