"""CPU-side checks of the tracking statistics: include/atr_track_stats.h against the built library and
tracking_stats.TRACK_PROTOTYPES; the refusals that come before any device is touched; the host model classify() against the true
positions of the C oracle's envs, against a per-sample loop, on every inconsistent form and across split calls; summarize() on a
table built by hand; the heat map; the flag of main.py; and the call site in train.rollout."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import tracking_stats_spec as ts
from conftest import ROOT
from test_abi_cpu import _header_functions, _header_structs, _header_symbols, _py_class


def _track_header():
    """include/atr_track_stats.h without comments and preprocessor lines."""
    txt = open(os.path.join(ROOT, "include", "atr_track_stats.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    return "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", txt).split("\n") if not ln.lstrip().startswith("#"))


def test_header_prototypes_and_exports_agree():
    """Every function of the header is exported by the built library and bound by TRACK_PROTOTYPES with the header's parameter
    count and classes; the header's constants are the module's (176 counters, 170 x 8 per player); the new source is in the
    build and under its no-scratch check."""
    from active_tracking_rl_amd import build, tracking_stats, vec_env
    build.build()
    assert os.path.join("..", "..", "include", "atr_track_stats.h") in build.HEADERS
    assert "tracking_stats_hip.hip" in build.SOURCES and build.NO_SCRATCH_STATS == {"tracking_stats_hip.hip": "k_track_stats"}
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    funcs = _header_functions(_track_header())
    assert sorted(funcs) == ["atr_track_stats", "atr_track_stats_drain"] == sorted(tracking_stats.TRACK_PROTOTYPES)
    assert _header_structs(_track_header()) == {}
    for name, (res, params) in funcs.items():
        assert hasattr(lib, name), name
        restype, argtypes = tracking_stats.TRACK_PROTOTYPES[name]
        assert _py_class(restype) == res == ctypes.c_int, name
        assert len(argtypes) == len(params), name
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _py_class(a) == c, (name, i)
    assert [c for c in funcs["atr_track_stats"][1] if c is ctypes.c_longlong] == [ctypes.c_longlong] * 11       # the strides
    for header, prefix in (("atr_policy.h", "atr_"), ("atr_eval.h", "atr_"), ("atr_stats.h", "atr_"), ("track2d.h", "t2d_")):
        assert not [s for s in _header_symbols(header, prefix) if "track_stats" in s], header
    txt = open(os.path.join(ROOT, "include", "atr_track_stats.h")).read()
    const = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, txt).group(1))
    assert const("ATR_TRACK_HIST") == tracking_stats.HIST == 176
    assert (const("ATR_TRACK_ACT_ROWS"), const("ATR_TRACK_MAX_ACTIONS")) == (tracking_stats.ACT_ROWS, tracking_stats.MAX_ACTIONS) == (170, 8)
    assert [const("ATR_TRACK_" + n) for n in ("WINDOW", "CENTRE", "OUT", "TERMINAL", "INCONSISTENT", "SAMPLES")] == \
        [tracking_stats.WINDOW, tracking_stats.CENTRE, tracking_stats.OUT, tracking_stats.TERMINAL, tracking_stats.INCONSISTENT,
         tracking_stats.SAMPLES] == [169, 84, 169, 170, 171, 172]
    assert const("ATR_TRACK_NO_AUTO_RESET") == tracking_stats.NO_AUTO_RESET == 1


def test_binding_checks_status_and_refuses_before_any_device():
    """lib() binds the table with an errcheck that raises with the entry point's name and the library's text; null or misaligned
    pointers, T <= 0, N <= 0, n_actions > 8, unknown flags and negative strides are refused by the argument checks, which come
    before anything touches a device (this test runs without one). act alone may be null."""
    from active_tracking_rl_amd import build, tracking_stats
    build.build()
    L = tracking_stats.lib()
    for name, (restype, argtypes) in tracking_stats.TRACK_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
        assert f.errcheck(0, None, ()) == 0
        with pytest.raises(RuntimeError, match=r"^%s failed \(-1\): " % name):
            f.errcheck(-1, None, ())
    p = 4096        # any non-null, aligned address: a refused call never reads it
    ok = dict(obs=p, obs_is_u8=True, obs_strides=(338 * 5, 338, 169), rew=p, rew_strides=(10, 2, 1), done=p, done_strides=(5, 1),
              act=p, act_strides=(10, 1, 5), carry=p, hist=p, act_hist=p, T=20, N=5, n_actions=4, flags=0, stream=None)
    cases = [(dict(obs=0), "null pointer"), (dict(rew=0), "null pointer"), (dict(done=0), "null pointer"),
             (dict(carry=0), "null pointer"), (dict(hist=0), "null pointer"), (dict(act_hist=0), "null pointer"),
             (dict(N=0), "N > 0"), (dict(N=-3), "N > 0"), (dict(T=0), "T > 0"), (dict(T=-1), "T > 0"), (dict(T=(1 << 20) + 1), "above"),
             (dict(n_actions=9), "n_actions 9 outside"), (dict(n_actions=0), "n_actions 0 outside"), (dict(flags=2), "unknown flags"),
             (dict(hist=p + 4), "not 8-byte aligned"), (dict(act_hist=p + 4), "not 8-byte aligned"),
             (dict(act=p + 4), "not 8-byte aligned"), (dict(carry=p + 2), "not 4-byte aligned"), (dict(rew=p + 2), "not 4-byte aligned"),
             (dict(obs=p + 1, obs_is_u8=False), "not 4-byte aligned"), (dict(obs_strides=(1690, -338, 169)), "negative element stride"),
             (dict(act_strides=(10, 1, -5)), "negative element stride")]
    for change, text in cases:
        with pytest.raises(RuntimeError, match=r"^atr_track_stats failed \(-1\): atr_track_stats: .*%s" % text):
            tracking_stats.track_stats(**dict(ok, **change))
    for args, text in (((0, p, p, p), "null pointer"), ((p, 0, p, p), "null pointer"), ((p, p, 0, p), "null pointer"),
                       ((p, p, p, 0), "null pointer"), ((p + 4, p, p, p), "not 8-byte aligned"), ((p, p, p, p + 4), "not 8-byte aligned")):
        with pytest.raises(RuntimeError, match=r"^atr_track_stats_drain failed \(-1\): atr_track_stats_drain: .*%s" % text):
            tracking_stats.track_stats_drain(*args, None)


def test_no_host_counting_path():
    import torch
    from active_tracking_rl_amd import tracking_stats
    with pytest.raises(RuntimeError, match="lives on the GPU"):
        tracking_stats.TrackingStats(object(), torch.device("cpu"))


PAIRS = (("Block", "PZR"), ("Maze", "Adv"), ("Empty", "Far"), ("Block", "Ram"), ("Maze", "Nav"))


@pytest.fixture(scope="module")
def oracle_walks():
    """Scalar oracle envs (PHILOX mode) under random actions, reset on done: per (map, target, env) the store of one env —
    obs [T+1, 1, 2, 13, 13], rew, done, act — and the true positions after every step. 5 pairs x 3 envs x 420 steps."""
    from oracle import oracle as orc
    walks, T = [], 420
    for k, (mp, tg) in enumerate(PAIRS):
        for i in range(3):
            env = orc.OracleEnv(mp, tg, 0, 60, orc.RNG_PHILOX, 11 + k, i)
            rs = np.random.RandomState(100 * k + i)
            obs, rew, done = np.zeros((T + 1, 1, 2, 13, 13), np.uint8), np.zeros((T, 1, 2), np.float32), np.zeros((T, 1), np.uint8)
            act, pos = np.zeros((T, 1, 2), np.int64), np.zeros((T, 1, 2, 2), np.int64)
            obs[0, 0] = env.reset()
            for t in range(T):
                act[t, 0] = rs.randint(0, 4, size=2)
                o, r, d, _ = env.step(act[t, 0])
                obs[t + 1, 0], rew[t, 0], done[t, 0] = o, r.astype(np.float32), d
                pos[t, 0] = env.state()["pos"]
                if d:
                    env.reset()         # (flags bit 0: the stored observation is the terminal state's own)
            walks.append(((mp, tg, i), obs, rew, done, act, pos))
    return walks


def test_classify_against_true_positions(oracle_walks):
    """Every sample's bin equals the bin of the oracle's true positions, INCONSISTENT is 0 (the oracle alone meets this: a
    condition, not a tolerance), and all three kinds of state — in view, out of view, co-located — and done steps occur."""
    from active_tracking_rl_amd import tracking_stats
    total = np.zeros(ts.HIST, np.int64)
    dones = 0
    for what, obs, rew, done, act, pos in oracle_walks:
        bins = tracking_stats.sample_bins(obs, rew, done, flags=1)
        want = ts.bin_of_positions(pos)
        assert np.array_equal(bins, want), (what, np.argwhere(bins != want)[:5].tolist())
        hist, act_hist, carry = tracking_stats.classify(obs, rew, done, act, flags=1)
        assert hist[ts.INCONSISTENT] == 0 and hist[ts.TERMINAL] == 0 and hist[ts.SAMPLES] == done.shape[0], what
        assert np.array_equal(hist[:170], np.bincount(want.ravel(), minlength=170)), what
        # every action taken from a classified, non-terminal state is paired: all samples but the done ones and the last
        assert act_hist[0].sum() == act_hist[1].sum() == done.shape[0] - int(done[:-1].sum()) - 1, what
        total += hist
        dones += int(done.sum())
    print("oracle walks: %d samples, in view %d, out %d, co-located %d, done %d" % (total[ts.SAMPLES], total[:169].sum(),
                                                                                 total[ts.OUT], total[ts.CENTRE], dones))
    assert total[ts.SAMPLES] == 15 * 420 and total[:169].sum() > 1000 and total[ts.OUT] > 0 and total[ts.CENTRE] > 0 and dones >= 15


def test_classify_equals_the_per_sample_loop():
    """The vectorised host model against the header's walk written one sample at a time, on a synthetic store with every kind
    of sample, both flags values, with and without actions, 4 and 8 actions; samples of the kinds made equal their bins."""
    from active_tracking_rl_amd import tracking_stats
    for seed, n_actions, flags, with_act in ((1, 4, 0, True), (2, 8, 1, True), (3, 4, 1, False)):
        obs, rew, done, act, kinds = ts.synthetic_store(9, 11, seed, n_actions)
        a = act if with_act else None
        hist, act_hist, carry = tracking_stats.classify(obs, rew, done, a, flags=flags, n_actions=n_actions)
        w_hist, w_act, w_carry, bins = ts.loop_model(obs, rew, done, a, flags=flags, n_actions=n_actions)
        ts.assert_tables_equal((hist, act_hist, carry), (w_hist, w_act, w_carry), seed)
        assert hist.dtype == np.int64 and act_hist.shape == (2, 170, 8) and carry.dtype == np.int32
        assert np.array_equal(bins, tracking_stats.sample_bins(obs, rew, done, flags))
        live = (done == 0) | bool(flags)
        assert (bins[live & (kinds >= 3)] == ts.INCONSISTENT).all() and (kinds >= 3).sum() >= 4
        assert (bins[live & (kinds == 1)] == ts.OUT).all() and (bins[live & (kinds == 2)] == ts.CENTRE).all()
        assert (bins[live & (kinds == 0)] < 169).all() and (bins[live & (kinds == 0)] != ts.CENTRE).all()
        assert (bins[~live] == ts.TERMINAL).all()
        assert hist[ts.SAMPLES] == 99 and hist[:172].sum() >= 99 and not hist[173:].any()
        assert (act_hist.sum() > 0) == with_act and not act_hist[:, :, n_actions:].any()


@pytest.mark.parametrize("kind", ts.KINDS[3:])
def test_each_inconsistent_form(kind):
    """Two 4s, a 4 without the mirrored 2, a wrong centre, rew0 == 1 with a visible target: INCONSISTENT, and the carry is -1."""
    from active_tracking_rl_amd import tracking_stats
    w, r = ts.windows(kind, 2, -3, np.random.RandomState(4))
    good, gr = ts.windows("seen", 2, -3, np.random.RandomState(4))
    obs = np.stack([good, good, w]).reshape(3, 1, 2, 13, 13)
    rew = np.array([[[gr, 0]], [[r, 0]]], np.float32)
    hist, act_hist, carry = tracking_stats.classify(obs, rew, np.zeros((2, 1), np.uint8), np.ones((2, 1, 2), np.int64))
    assert hist[ts.INCONSISTENT] == 1 and hist[(2 + 6) * 13 + (-3 + 6)] == 1 and hist[ts.SAMPLES] == 2 and carry[0] == -1
    assert act_hist.sum() == 2 and act_hist[0, 8 * 13 + 3, 1] == 1 and act_hist[1, 8 * 13 + 3, 1] == 1


def test_out_of_range_action_counts_as_inconsistent():
    from active_tracking_rl_amd import tracking_stats
    good, gr = ts.windows("seen", -1, 4, np.random.RandomState(5))
    obs = np.stack([good] * 4).reshape(4, 1, 2, 13, 13)
    rew = np.full((3, 1, 2), gr, np.float32)
    act = np.array([[[0, 0]], [[4, 1]], [[-1, 7]]], np.int64)
    hist, act_hist, carry = tracking_stats.classify(obs, rew, np.zeros((3, 1), np.uint8), act, n_actions=4)
    b = 5 * 13 + 10
    assert hist[b] == 3 and hist[ts.SAMPLES] == 3 and hist[ts.INCONSISTENT] == 3 and carry[0] == b
    assert act_hist.sum() == 1 and act_hist[1, b, 1] == 1          # act[0] had no state to pair with
    hist8, act8, _ = tracking_stats.classify(obs, rew, np.zeros((3, 1), np.uint8), act, n_actions=8)
    assert hist8[ts.INCONSISTENT] == 1 and act8[0, b, 4] == 1 and act8[1, b, 7] == 1


def test_split_calls_equal_one_call():
    """T = 7 as 3 + 4 and as 7 x 1 equals one call, counter for counter: the action pairing crosses the boundary and the carry
    after a done step is -1."""
    from active_tracking_rl_amd import tracking_stats
    for flags in (0, 1):
        obs, rew, done, act, _ = ts.synthetic_store(7, 6, 21 + flags, p_bad=0.05)
        done[2, 0], done[3, 1], done[6, 2] = 1, 1, 1          # a done on the last step of the first part, the first of the second
        whole = tracking_stats.classify(obs, rew, done, act, flags=flags)
        assert whole[2][2] == -1
        for cuts in ((3,), (1, 2, 3, 4, 5, 6)):
            hist = act_hist = carry = None
            for a, b in zip((0,) + cuts, cuts + (7,)):
                hist, act_hist, carry = tracking_stats.classify(obs[a:b + 1], rew[a:b], done[a:b], act[a:b], carry=carry, flags=flags,
                                                                hist=hist, act_hist=act_hist)
                if b == 3:
                    assert carry[0] == -1 and (carry[3:] >= -1).all()
            ts.assert_tables_equal((hist, act_hist, carry), whole, (flags, cuts))
        # without the carry the boundary's actions would be lost: the split is not trivially equal
        lost = tracking_stats.classify(obs[3:], rew[3:], done[3:], act[3:], flags=flags)[1].sum()
        first = tracking_stats.classify(obs[:4], rew[:3], done[:3], act[:3], flags=flags)[1].sum()
        assert lost + first < whole[1].sum()


def test_summarize_on_a_table_built_by_hand():
    """Rates are exact rationals of the counts; compared at float64 rounding of the few operations involved (4 ulp)."""
    from active_tracking_rl_amd import tracking_stats
    hist, act_hist = np.zeros(176, np.int64), np.zeros((2, 170, 8), np.int64)
    b = lambda dr, dc: (dr + 6) * 13 + dc + 6
    hist[b(0, 3)], hist[b(-4, 0)], hist[b(6, 6)], hist[b(0, 0)], hist[ts.OUT] = 5, 3, 2, 4, 6
    hist[ts.TERMINAL], hist[ts.INCONSISTENT] = 7, 1
    hist[ts.SAMPLES] = 5 + 3 + 2 + 4 + 6 + 7 + 1
    act_hist[0, b(0, 3)] = [1, 1, 0, 3, 0, 0, 0, 0]          # target to the right: only action 3 (0, +1) is toward
    act_hist[0, b(-4, 0)] = [2, 1, 0, 0, 0, 0, 0, 0]         # target above: action 0 (-1, 0) is toward
    act_hist[0, b(0, 0)] = [9, 9, 9, 9, 0, 0, 0, 0]          # co-located and OUT rows do not count
    act_hist[0, ts.OUT] = [5, 5, 5, 5, 0, 0, 0, 0]
    act_hist[1, b(0, 3)] = [2, 0, 1, 2, 0, 0, 0, 0]          # target at (0, 3): up, down and right all lengthen |d|; left shortens
    act_hist[1, b(6, 6)] = [1, 0, 0, 1, 0, 0, 0, 0]          # at (6, 6): up shortens, right lengthens
    s = tracking_stats.summarize(hist, act_hist)
    close = lambda got, want: abs(got - want) <= 4 * np.spacing(abs(want))
    assert (s["samples"], s["terminal"], s["inconsistent"]) == (28, 7, 1)
    assert close(s["in_view_rate"], 14 / 20) and close(s["colocated_rate"], 4 / 20)
    assert close(s["in_range_rate"], 12 / 20)                 # (6, 6) is in view and out of range: 72 > 36
    assert close(s["mean_distance"], (5 * 3 + 3 * 4 + 2 * np.sqrt(72.0)) / 14)
    assert s["centroid"][0] == 0.0                            # 3 * -4 + 2 * 6
    assert close(s["centroid"][1], (5 * 3 + 2 * 6) / 14)
    assert close(s["tracker_toward_rate"], (3 + 2) / 8) and close(s["target_away_rate"], (2 + 0 + 2 + 1) / 7)
    import torch
    assert tracking_stats.summarize(torch.from_numpy(hist), torch.from_numpy(act_hist)) == s


def test_toward_and_away_tables():
    """The move tables of track_1v1.py:275-279 and what they do to the squared distance, for both action types."""
    from active_tracking_rl_amd import tracking_stats
    assert tracking_stats.MOVES["VonNeumann"] == ((-1, 0), (1, 0), (0, -1), (0, 1))
    assert tracking_stats.MOVES["Moore"] == ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, 1), (1, 1), (-1, -1), (1, -1))
    b = lambda dr, dc: (dr + 6) * 13 + dc + 6
    for kind, n in (("VonNeumann", 4), ("Moore", 8)):
        toward, away = tracking_stats.move_tables(kind)
        assert toward.shape == away.shape == (169, 8) and not toward[:, n:].any() and not away[:, n:].any()
        for bin_ in range(169):
            dr, dc = bin_ // 13 - 6, bin_ % 13 - 6
            for a, (mr, mc) in enumerate(tracking_stats.MOVES[kind]):
                assert toward[bin_, a] == ((dr - mr) ** 2 + (dc - mc) ** 2 < dr * dr + dc * dc)
                assert away[bin_, a] == ((dr + mr) ** 2 + (dc + mc) ** 2 > dr * dr + dc * dc)
    toward, away = tracking_stats.move_tables("VonNeumann")
    assert toward[b(3, 0)].tolist()[:4] == [False, True, False, False] and away[b(3, 0)].tolist()[:4] == [False, True, True, True]
    toward, away = tracking_stats.move_tables("Moore")
    assert toward[b(2, -2)].tolist() == [False, True, True, False, False, False, False, True]
    assert toward[b(0, 1)].tolist() == [False, False, False, True, False, False, False, False]      # a diagonal from distance 1: sqrt 1 -> 1
    assert away[b(0, 1)].tolist() == [True, True, False, True, True, True, False, False]
    assert not toward[84].any() and away[84, :8].all()


def test_empty_table_gives_nans():
    from active_tracking_rl_amd import tracking_stats
    s = tracking_stats.summarize(np.zeros(176, np.int64), np.zeros((2, 170, 8), np.int64))
    assert (s["samples"], s["terminal"], s["inconsistent"]) == (0, 0, 0)
    for key in ("in_view_rate", "in_range_rate", "colocated_rate", "mean_distance", "tracker_toward_rate", "target_away_rate"):
        assert np.isnan(s[key]), key
    assert all(np.isnan(v) for v in s["centroid"])
    only_out = np.zeros(176, np.int64)
    only_out[ts.OUT] = only_out[ts.SAMPLES] = 3
    s = tracking_stats.summarize(only_out, np.zeros((2, 170, 8), np.int64))
    assert s["in_view_rate"] == 0.0 and np.isnan(s["mean_distance"]) and np.isnan(s["tracker_toward_rate"])


def test_heat_png(tmp_path):
    """heat_png writes a [13 * scale, 13 * scale, 3] image: the most frequent offset brightest, an empty offset dark."""
    import struct
    import zlib
    from active_tracking_rl_amd import tracking_stats
    hist = np.zeros(176, np.int64)
    hist[3 * 13 + 9], hist[10 * 13 + 2] = 40, 10
    for scale in (16, 3):
        path = os.path.join(str(tmp_path), "heat_%d.png" % scale)
        img = tracking_stats.heat_png(hist, path, scale=scale)
        assert img.shape == (13 * scale, 13 * scale, 3) and img.dtype == np.uint8
        raw = open(path, "rb").read()
        assert raw[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", raw[16:24]) == (13 * scale, 13 * scale)
        n = struct.unpack(">I", raw[33:37])[0]
        rows = np.frombuffer(zlib.decompress(raw[41:41 + n]), np.uint8).reshape(13 * scale, 1 + 39 * scale)
        assert np.array_equal(rows[:, 1:].reshape(13 * scale, 13 * scale, 3), img)
        cell = lambda r, c: img[r * scale + scale // 2, c * scale + scale // 2].astype(int)
        assert cell(3, 9)[0] == 255 and 0 < cell(10, 2)[0] < 255 and cell(0, 0)[0] == 0
    assert tracking_stats.heat_image(np.zeros(176, np.int64), 2).shape == (26, 26, 3)


def test_main_lists_the_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "--tracking-stats" in r.stdout and "--episode-stats" in r.stdout


def test_rollout_calls_the_update_only_when_attached():
    """train.rollout's call site with a stub: nothing attached -> nothing called; attached -> one update per rollout with the
    store's obs [T+1, ...], rew, done and the actions as [T, N, 2] — a view of the sampler's [T, 2, N] store where there is one,
    else the stacked list; a rollout without a store is an error, not a silent skip."""
    import torch
    from active_tracking_rl_amd import train

    class Stats(object):
        def __init__(self):
            self.calls = []

        def update(self, obs, rew, done, act=None):
            self.calls.append((obs, rew, done, act))

    class Env(object):
        pass

    class Player(object):
        def __init__(self, env, act_store):
            self.env, self.model, self.act_store = env, object(), act_store
            self.rewards, self.dones, self.actions, self._buf, self._actions_buf = [], [], [], None, None

        def begin_rollout(self, n):
            self._buf = (torch.zeros(n + 1, 3, 2, 13, 13, dtype=torch.uint8), torch.zeros(n, 3, 2), torch.zeros(n, 3, dtype=torch.uint8))
            self._actions_buf = torch.arange(n * 6).reshape(n, 2, 3) if self.act_store else None
            self.k = 0

        def action_rollout(self):
            if self._actions_buf is None:
                self.actions.append(torch.full((3, 2), len(self.actions)))
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
    p = Player(env, act_store=True)
    train.rollout(p, 4)                                   # nothing attached
    env.tracking_stats = Stats()
    train.rollout(p, 4)
    (obs, rew, done, act), = env.tracking_stats.calls
    assert obs is p._buf[0] and rew is p._buf[1] and done is p._buf[2] and obs.shape[0] == 5
    assert act.shape == (4, 3, 2) and act.data_ptr() == p._actions_buf.data_ptr() and act.stride() == (6, 1, 3)
    assert torch.equal(act, p._actions_buf.permute(0, 2, 1))
    q = Player(env, act_store=False)
    train.rollout(q, 4)
    train.rollout(q, 4)                                   # the list keeps growing until the learner clears it: the last 4 count
    obs, rew, done, act = env.tracking_stats.calls[-1]
    assert obs is q._buf[0] and act.shape == (4, 3, 2) and act[:, 0, 0].tolist() == [4, 5, 6, 7]
    assert len(env.tracking_stats.calls) == 3
    with pytest.raises(RuntimeError, match="rollout store"):
        train.rollout(q, 4, fast=False)
    env.tracking_stats = None
    train.rollout(q, 4, fast=False)                       # detached again: the slow path runs as before
    assert len(q.rewards) == 16
