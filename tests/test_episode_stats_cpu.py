"""CPU-side checks of the training-episode statistics: the new header include/atr_stats.h against the built library and against
episode_stats.STATS_PROTOTYPES (the parsing of tests/test_abi_cpu.py, applied to the new header); the binding's errcheck and the
refusals that come before any device is touched; the host models of the two kernels against a per-env loop in the reference's
words; and summarize against numpy on a known list of episodes."""
import ctypes
import os
import re

import numpy as np
import pytest

import episode_stats_spec as es
from conftest import ROOT
from test_abi_cpu import _header_functions, _header_structs, _header_symbols, _py_class


def _stats_header():
    """include/atr_stats.h without comments and preprocessor lines."""
    txt = open(os.path.join(ROOT, "include", "atr_stats.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    return "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", txt).split("\n") if not ln.lstrip().startswith("#"))


def test_library_exports_every_function_of_the_stats_header():
    from active_tracking_rl_amd import build, vec_env
    build.build()
    assert os.path.join("..", "..", "include", "atr_stats.h") in build.HEADERS
    assert "episode_stats_hip.hip" in build.SOURCES
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    funcs = _header_functions(_stats_header())
    assert sorted(funcs) == ["atr_episode_stats", "atr_episode_stats_drain"]
    for name in funcs:
        assert hasattr(lib, name), name
    assert _header_structs(_stats_header()) == {}
    # the other headers' symbol lists are what they were: the new entry points are declared in the new header alone
    for header, prefix in (("atr_policy.h", "atr_"), ("atr_eval.h", "atr_"), ("track2d.h", "t2d_")):
        assert not [s for s in _header_symbols(header, prefix) if "episode_stats" in s], header


def test_stats_prototypes_match_the_header():
    """episode_stats.STATS_PROTOTYPES is include/atr_stats.h's ABI, function by function: the header's parameter count and, per
    parameter and result, the same class (pointer / int / long long)."""
    from active_tracking_rl_amd import episode_stats
    funcs = _header_functions(_stats_header())
    assert sorted(funcs) == sorted(episode_stats.STATS_PROTOTYPES)
    for name, (res, params) in funcs.items():
        restype, argtypes = episode_stats.STATS_PROTOTYPES[name]
        assert _py_class(restype) == res == ctypes.c_int, name
        assert len(argtypes) == len(params), name
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _py_class(a) == c, (name, i)
    assert [c for c in funcs["atr_episode_stats"][1] if c is ctypes.c_longlong] == [ctypes.c_longlong] * 5      # the strides
    txt = open(os.path.join(ROOT, "include", "atr_stats.h")).read()
    assert "train.py:63-88" in txt and "gym_eval.py:110-125" in txt
    m = re.search(r"#define\s+ATR_STATS_FIELDS\s+(\d+)", txt), re.search(r"#define\s+ATR_STATS_DRAIN_LANES\s+(\d+)", txt)
    assert (int(m[0].group(1)), int(m[1].group(1))) == (episode_stats.FIELDS, episode_stats.DRAIN_LANES) == (8, 32)


def test_stats_binding_checks_status_and_refuses_before_any_device():
    """episode_stats.lib() binds the table on the built library with an errcheck that raises with the entry point's name and the
    library's text; null pointers, N <= 0, T <= 0 and a misaligned fin are refused by the argument checks, which come before
    anything touches a device (this test runs without one)."""
    from active_tracking_rl_amd import build, episode_stats
    build.build()
    L = episode_stats.lib()
    for name, (restype, argtypes) in episode_stats.STATS_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
        assert f.errcheck(0, None, ()) == 0
        with pytest.raises(RuntimeError, match=r"^%s failed \(-1\): " % name):
            f.errcheck(-1, None, ())
    p = 4096        # any non-null, aligned address: a refused call never reads it
    ok = dict(rew=p, rew_strides=(38, 2, 1), done=p, done_strides=(19, 1), run_ret=p, run_len=p, fin=p, T=20, N=19, success_len=500,
              stream=None)
    for change, text in ((dict(rew=0), "null pointer"), (dict(done=0), "null pointer"), (dict(run_ret=0), "null pointer"),
                         (dict(run_len=0), "null pointer"), (dict(fin=0), "null pointer"), (dict(N=0), "N > 0"),
                         (dict(N=-3), "N > 0"), (dict(T=0), "T > 0"), (dict(fin=p + 4), "not 8-byte aligned"),
                         (dict(rew_strides=(38, -2, 1)), "negative element stride")):
        with pytest.raises(RuntimeError, match=r"^atr_episode_stats failed \(-1\): atr_episode_stats: .*%s" % text):
            episode_stats.episode_stats(**dict(ok, **change))
    for args, text in (((0, p, 19), "null pointer"), ((p, 0, 19), "null pointer"), ((p, p, 0), "N > 0"),
                       ((p + 4, p, 19), "not 8-byte aligned")):
        with pytest.raises(RuntimeError, match=r"^atr_episode_stats_drain failed \(-1\): atr_episode_stats_drain: .*%s" % text):
            episode_stats.episode_stats_drain(*args, None)


def test_no_host_accounting_path():
    """EpisodeStats on a CPU device raises: the accounts live on the GPU or nowhere."""
    import torch
    from active_tracking_rl_amd import episode_stats
    with pytest.raises(RuntimeError, match="lives on the GPU"):
        episode_stats.EpisodeStats(object(), torch.device("cpu"))


def test_account_equals_the_per_env_loop():
    """episode_stats.account on synthetic rew [57,19,2] / done [57,19] against the per-env loop in the reference's words, bit for
    bit: one env never finishes, one finishes at step 0, one has two dones in consecutive steps, one episode is exactly
    success_len long and one success_len - 1."""
    from active_tracking_rl_amd import episode_stats
    S = 23
    rew, done = es.synthetic(57, 19, S)
    run_ret, run_len, fin = episode_stats.account(rew, done, success_len=S)
    assert run_ret.dtype == np.float32 and run_len.dtype == np.int32 and fin.dtype == np.float64 and fin.shape == (19, 8)
    w_ret, w_len, w_fin, episodes = es.reference_loop(rew, done, S)
    es.assert_accounts_equal((run_ret, run_len, fin), (w_ret, w_len, w_fin))
    assert fin[0, 0] == 0 and run_len[0] == 57 and not fin[0].any()                   # never finishes: all of it still running
    assert episodes[1][0][2] == 1 and fin[1, 0] >= 1                                   # finishes at step 0: an episode of length 1
    assert [L for _, _, L in episodes[2]].count(1) >= 1 and done[10, 2] and done[11, 2]     # second of two consecutive dones
    assert episodes[3][0][2] == S and episodes[4][0][2] == S - 1
    # success is L >= success_len: env 3's first episode counts, env 4's does not
    assert fin[3, 7] == sum(1 for _, _, L in episodes[3] if L >= S) >= 1
    assert fin[4, 7] == sum(1 for _, _, L in episodes[4] if L >= S)
    assert fin[:, 0].sum() == done.sum() and fin[:, 5].sum() + run_len.sum() == 57 * 19      # every step is in exactly one account


def test_consecutive_calls_continue_the_accounts():
    """T steps in one call equal any split into consecutive calls: episodes span calls as they span rollouts."""
    from active_tracking_rl_amd import episode_stats
    S = 23
    rew, done = es.synthetic(57, 19, S)
    whole = episode_stats.account(rew, done, success_len=S)
    for cuts in ((20, 40), (1, 2, 56), (11,), tuple(range(1, 57))):
        acc = (None, None, None)
        for a, b in zip((0,) + cuts, cuts + (57,)):
            acc = episode_stats.account(rew[a:b], done[a:b], *acc, success_len=S)
        es.assert_accounts_equal(acc, whole, cuts[:3])
    # the same holds for the per-env loop given the running accounts
    first = es.reference_loop(rew[:20], done[:20], S)
    second = es.reference_loop(rew[20:], done[20:], S, *first[:3])
    es.assert_accounts_equal(second[:3], whole)


def test_drain_model_order_and_value():
    """drain_model adds in the header's order (32 row lanes, then lane order) and equals the plain sum to rounding; sizes that are
    not a multiple of 32 and a single env included."""
    from active_tracking_rl_amd import episode_stats
    rs = np.random.RandomState(11)
    for n in (1, 19, 32, 33, 100):
        fin = rs.randn(n, 8) * 1e3
        tot = episode_stats.drain_model(fin)
        want = np.zeros(8)
        part = [np.zeros(8) for _ in range(32)]
        for e in range(n):
            part[e % 32] = part[e % 32] + fin[e]
        for r in range(32):
            want = want + part[r]
        assert es.same_bits(tot, want), n
        assert np.allclose(tot, fin.sum(0), rtol=1e-12, atol=1e-9)
    counts = np.arange(19 * 8, dtype=np.float64).reshape(19, 8)
    assert np.array_equal(episode_stats.drain_model(counts), counts.sum(0))          # integers: exact whatever the order


def test_summarize_against_numpy():
    """summarize of the totals of a known list of (R0, R1, L) equals numpy's mean / std of that list to 1e-12 relative (both sides
    float64 arithmetic on the same numbers; the margin covers the sum-of-squares form of the variance); population values as in
    gym_eval.py:117-125; success = L >= success_len."""
    from active_tracking_rl_amd import episode_stats
    S = 23
    rew, done = es.synthetic(57, 19, S)
    _, _, fin, episodes = es.reference_loop(rew, done, S)
    eps = np.array([ep for his in episodes for ep in his], np.float64)
    assert len(eps) >= 30
    s = episode_stats.summarize(episode_stats.drain_model(fin))
    rel = lambda got, want: np.max(np.abs(np.asarray(got) - want) / np.abs(want))
    assert s["episodes"] == len(eps)
    assert rel(s["R_mean"], eps[:, :2].mean(0)) <= 1e-12 and rel(s["R_std"], eps[:, :2].std(0)) <= 1e-12
    assert rel(s["EL_mean"], eps[:, 2].mean()) <= 1e-12 and rel(s["EL_std"], eps[:, 2].std()) <= 1e-12
    assert s["S_rate"] == (eps[:, 2] >= S).mean() and 0 < s["S_rate"] < 1
    assert rel(s["R_step"], eps[:, :2].mean(0) / eps[:, 2].mean()) <= 1e-12
    # no finished episode: NaNs, not an exception
    empty = episode_stats.summarize(np.zeros(8))
    assert empty["episodes"] == 0 and all(np.isnan(v) for v in empty["R_mean"] + empty["R_std"] + empty["R_step"])
    assert np.isnan(empty["EL_mean"]) and np.isnan(empty["EL_std"]) and np.isnan(empty["S_rate"])


def test_pooled_totals_of_disjoint_shards_equal_the_union():
    """Sums of sums pool exactly in meaning: summarize(totals of shard A + totals of shard B) equals summarize(totals of the
    union) to float64 rounding of differently ordered sums, and exactly in the counts."""
    from active_tracking_rl_amd import episode_stats
    S = 23
    rew, done = es.synthetic(57, 19, S)
    _, _, fin = episode_stats.account(rew, done, success_len=S)
    a, b = episode_stats.drain_model(fin[:7]), episode_stats.drain_model(fin[7:])
    u = episode_stats.drain_model(fin)
    sp, su = episode_stats.summarize(a + b), episode_stats.summarize(u)
    assert sp["episodes"] == su["episodes"] and sp["S_rate"] == su["S_rate"] and sp["EL_mean"] == su["EL_mean"]
    for key in ("R_mean", "R_std", "R_step"):
        assert np.allclose(sp[key], su[key], rtol=1e-12, atol=0), key
    assert np.isclose(sp["EL_std"], su["EL_std"], rtol=1e-12, atol=0)
    import torch
    assert episode_stats.summarize(torch.from_numpy(u)) == su                         # a tensor is accepted as it comes from drain()


def test_rollout_calls_the_update_only_when_attached():
    """train.rollout's call site: nothing attached -> nothing called (the env is not even asked twice); attached -> one update
    per rollout with the rollout store's rewards and done flags, or the stacked lists where there is no store, in both
    branches."""
    import torch
    from active_tracking_rl_amd import train

    class Stats(object):
        def __init__(self):
            self.calls = []

        def update(self, rew, done):
            self.calls.append((rew, done))

    class Env(object):
        pass

    class Player(object):
        def __init__(self, env, store):
            self.env, self.model, self.store = env, object(), store
            self.rewards, self.dones, self._buf = [], [], None

        def begin_rollout(self, n):
            self._buf = (None, torch.zeros(n, 3, 2), torch.zeros(n, 3, dtype=torch.uint8)) if self.store else None

        def _step(self):
            self.rewards.append(torch.full((3, 2, 1), float(len(self.rewards))))
            self.dones.append(torch.zeros(3, dtype=torch.uint8))

        action_rollout = action_train = _step

        def end_rollout(self):
            pass

        def update_rnn_hiden(self):
            pass

    env = Env()
    p = Player(env, store=True)
    train.rollout(p, 4)                                   # nothing attached
    env.episode_stats = Stats()
    train.rollout(p, 4)
    (rew, done), = env.episode_stats.calls
    assert rew is p._buf[1] and done is p._buf[2]
    q = Player(env, store=False)
    train.rollout(q, 4)
    train.rollout(q, 4)                                   # the lists keep growing until the learner clears them: the last 4 count
    rew, done = env.episode_stats.calls[-1]
    assert rew.shape == (4, 3, 2, 1) and done.shape == (4, 3) and rew[:, 0, 0, 0].tolist() == [4.0, 5.0, 6.0, 7.0]
    train.rollout(q, 4, fast=False)
    rew, done = env.episode_stats.calls[-1]
    assert len(env.episode_stats.calls) == 4 and rew[:, 0, 0, 0].tolist() == [8.0, 9.0, 10.0, 11.0]
