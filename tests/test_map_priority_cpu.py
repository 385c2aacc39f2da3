"""CPU-side checks of prioritized map replay: the plain-Python statement (tests/map_priority_spec.py) against itself,
map_priority.priorities on CPU tensors against the loop form of the rule, include/track2d_bank_prio.h against the built library
and map_priority.PRIO_PROTOTYPES, main.py's flags, and two gloo ranks that must end a refresh with the same table."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import map_priority_spec as ps
from conftest import ROOT

from active_tracking_rl_amd import map_priority as mp


# -- (1) the spec against itself -------------------------------------------------------------------------------------------
def test_all_equal_bank_is_uniform():
    for K in (1, 2, 5, 64, 1025):
        for v in (1.0, 3.5e-30, 7e37):
            q = ps.quanta(np.full(K, v, np.float32))
            assert q == [ps.TOTAL_MAX // K] * K
            assert ps.table(np.full(K, v, np.float32)).tolist() == [(i + 1) * (ps.TOTAL_MAX // K) for i in range(K)]


def test_zero_weight_is_never_drawn():
    w = np.array([3.0, 0.0, 1.0, 0.5, 2.0], np.float32)
    cum = ps.table(w)
    assert cum[1] == cum[0]
    seen = np.zeros(5, np.int64)
    for e in range(100):
        for ep in range(1, 101):
            seen[ps.draw(cum, 0x1234567890, 1000 + e, ep)] += 1
    assert seen.sum() == 10000 and seen[1] == 0 and (seen[[0, 2, 3, 4]] > 0).all()
    # ... and the shares follow the weights: 3 : 1 : 0.5 : 2 of 6.5, within five binomial standard deviations
    for i, share in ((0, 3 / 6.5), (2, 1 / 6.5), (3, 0.5 / 6.5), (4, 2 / 6.5)):
        assert abs(seen[i] - 10000 * share) < 5 * np.sqrt(10000 * share * (1 - share))


def test_total_stays_below_2_31_at_the_largest_bank():
    K = 65536
    cum = ps.table(np.ones(K, np.float32))
    assert int(cum[-1]) == K * (ps.TOTAL_MAX // K) <= ps.TOTAL_MAX and int(cum[-1]) >= 1
    assert int(ps.table(np.array([1.0], np.float32))[-1]) == ps.TOTAL_MAX


def test_nan_inf_and_negative_weights_count_as_zero():
    w = np.array([np.nan, 2.0, np.inf, -1.0, 1.0, -np.inf, 0.0, -0.0], np.float32)
    S = ps.TOTAL_MAX // 8
    assert ps.quanta(w) == [0, S, 0, 0, S // 2, 0, 0, 0]
    # a weight far below the largest still keeps one quantum; a denormal counts
    assert ps.quanta(np.array([1e38, 1e-38, 1e-45], np.float32)) == [ps.TOTAL_MAX // 3, 1, 1]


def test_all_zero_weights_give_the_uniform_table():
    for w in ([0.0, 0.0, 0.0], [np.nan, -1.0, np.inf], [0.0]):
        assert ps.table(np.array(w, np.float32)).tolist() == list(range(1, len(w) + 1))


def test_draw_is_the_count_of_entries_at_or_below_r_and_k1_draws_nothing():
    assert ps.draw(np.array([7], np.uint32), 5, 1000, 3) == 0
    cum = ps.table(np.array([1.0, 0.0, 0.0, 1.0], np.float32))
    got = {ps.draw(cum, 9, 1000 + e, ep) for e in range(20) for ep in range(1, 9)}
    assert got == {0, 3}


def test_score_spec_counts_spanning_episodes_once():
    rs = np.random.RandomState(0)
    T, n, K = 20, 6, 3
    rew = rs.uniform(-1, 1, (T, n, 2)).astype(np.float32)
    done = (rs.rand(T, n) < 0.15) & (np.arange(T)[:, None] % 4 == 3)       # at most five ends per env: all are attributed
    assert 0 < done.sum(0).max() <= ps.KEEP
    idx = rs.randint(0, K, (T, n))
    whole, lost, _ = ps.score(idx, rew, done, 4, count=K)
    a, la, carry = ps.score(idx[:7], rew[:7], done[:7], 4, count=K)
    b, lb, _ = ps.score(idx[7:], rew[7:], done[7:], 4, carry=carry, count=K)
    assert lost == la + lb == 0 and (whole == a + b).all() and whole[:, 0].sum() == done.sum()


# -- (2) the rule on tensors against the loops -------------------------------------------------------------------------------
def _bound(K):
    """Relative bound on w. Each of P_S's and P_C's denominators is a sum of K non-negative float64 terms: K * 2^-53 relative
    whatever the order (the spec sums exactly). Around them a fixed number of single operations, each within 2^-53 relative:
    the two divisions, the two products by (1 - rho) and rho, the final sum, 1 - rho itself — 6 — and the power rank^(-1/beta)
    by two different libraries, each within one unit in the last place (2 * 2^-53) of the true value: 4 more, in numerator and
    (already counted per term) denominator. All terms of w are non-negative, so relative errors do not grow in the sum. The
    float32 rounding of w is the same operation on both sides unless the float64 values straddle a rounding boundary: the
    comparison is made on float64 values rounded to float32 with one more half unit of float32."""
    return (2 * K + 6 + 4 + 4) * 2.0 ** -53


def _case(K, seed, ties=False, unseen=False):
    rs = np.random.RandomState(seed)
    n = rs.randint(1, 9, K)
    if unseen:
        n[rs.rand(K) < 0.4] = 0
    rq = np.array([int(v) for v in (rs.uniform(-1, 1, K) * n * 500 * 65536)], np.int64)
    if ties and K > 1:
        rq[1::2], n[1::2] = rq[0], n[0]
    return n.astype(np.int64), rq


@pytest.mark.parametrize("K", [1, 2, 5, 64])
@pytest.mark.parametrize("rho", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("kind", ["plain", "ties", "unseen"])
def test_priorities_match_the_loop_rule(K, rho, kind):
    beta, alpha, t_max = 0.1, 0.5, 500
    h_t, s_t = torch.ones(K, dtype=torch.float64), torch.zeros(K, dtype=torch.int64)
    h_s, s_s = [1.0] * K, [0] * K
    w0 = mp.weights(h_t, s_t, 0, beta, rho)
    assert torch.equal(w0, torch.full((K,), np.float32(1.0 / K)))           # an untouched bank is uniform
    for c in (1, 2, 3):                                                         # alpha 0.5 over three refreshes
        n, rq = _case(K, 100 * K + c, ties=kind == "ties", unseen=kind == "unseen")
        h_t, s_t, w_t = mp.priorities(h_t, s_t, torch.from_numpy(n), torch.from_numpy(rq), c, "tracker", t_max, beta, rho, alpha)
        h_s, s_s, w_s = ps.rule(h_s, s_s, n, rq, c, t_max, beta, rho, alpha)
        assert h_t.tolist() == h_s and s_t.tolist() == s_s
        assert w_t.dtype == torch.float32 and w_t.shape == (K,)
        w64 = np.array(w_s, np.float64)
        err = np.abs(w_t.double().numpy() - w64)
        assert (err <= w64 * (_bound(K) + 2.0 ** -24)).all(), (err / w64).max()
        assert abs(float(w_t.double().sum()) - 1.0) <= K * 2.0 ** -23
    if kind == "ties" and K > 2:
        assert len(set(h_s[1::2])) == 1 and len(set(w_t[1::2].tolist())) <= 2   # (equal scores: equal P_S; stamps equal too)


def test_priorities_take_either_column():
    K = 5
    n, rq = _case(K, 7)
    both = torch.stack([torch.from_numpy(rq), -torch.from_numpy(rq)], 1)
    h, s = torch.ones(K, dtype=torch.float64), torch.zeros(K, dtype=torch.int64)
    a = mp.priorities(h, s, torch.from_numpy(n), both, 1, "target", 500)
    b = mp.priorities(h, s, torch.from_numpy(n), -torch.from_numpy(rq), 1, "target", 500)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="tracker"):
        mp.priorities(h, s, torch.from_numpy(n), both, 1, "referee", 500)


# -- (3) the header against the binding ---------------------------------------------------------------------------------------
def test_header_functions_are_exported_and_bound():
    from active_tracking_rl_amd import build, vec_env
    build.build()
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    txt = open(os.path.join(ROOT, "include", "track2d_bank_prio.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    decl = {m.group(1): [p for p in m.group(2).split(",") if p.strip() not in ("", "void")]
            for m in re.finditer(r"\bint\s+(t2d_[a-z_]+)\s*\(([^()]*)\)\s*;", txt)}
    assert sorted(decl) == ["t2d_bank_prio_drain", "t2d_bank_prio_enable", "t2d_bank_prio_score", "t2d_bank_prio_set_weights"]
    assert sorted(decl) == sorted(mp.PRIO_PROTOTYPES)
    for name, params in decl.items():
        assert hasattr(lib, name), name
        restype, argtypes = mp.PRIO_PROTOTYPES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        assert "map_bank" not in name and name not in vec_env.ABI_SYMBOLS
    consts = dict(re.findall(r"#define\s+(T2D_PRIO_[A-Z_]+)\s+(\d+)", txt))
    assert int(consts["T2D_PRIO_RING"]) == mp.RING == ps.RING and int(consts["T2D_PRIO_FIELDS"]) == mp.FIELDS == ps.FIELDS
    assert int(consts["T2D_PRIO_KEEP"]) == mp.KEEP == ps.KEEP


# -- (4) the flags ---------------------------------------------------------------------------------------------------------
def _main(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + list(argv), capture_output=True, text=True, cwd=ROOT,
                          timeout=120)


def test_main_has_the_flags_and_refuses_bad_combinations():
    r = _main("--help")
    assert r.returncode == 0, r.stderr
    for f in ("--map-priority", "--map-priority-every", "--map-priority-beta", "--map-priority-rho", "--map-priority-alpha",
              "--map-priority-load"):
        assert f in r.stdout, f
    r = _main("--map-priority", "tracker")
    assert r.returncode == 2 and "--map-priority needs --map-bank" in r.stderr
    r = _main("--map-priority", "tracker", "--map-bank", "bank.npz", "--save-shard-state")
    assert r.returncode == 2 and "--save-shard-state" in r.stderr
    r = _main("--map-priority", "target", "--map-bank", "bank.npz", "--load-shard-state", "x")
    assert r.returncode == 2 and "--load-shard-state" in r.stderr
    r = _main("--map-priority", "referee", "--map-bank", "bank.npz")
    assert r.returncode == 2


def test_eval_shards_get_no_priorities():
    import argparse
    from active_tracking_rl_amd.environment import eval_args
    a = eval_args(argparse.Namespace(map_bank="train.npz", bank_select="random", eval_map_bank="held.npz", map_priority="tracker"))
    assert a.map_priority is None and a.bank_select == "cycle" and a.map_bank == "held.npz"


# -- (5) two ranks, one table ---------------------------------------------------------------------------------------------
_RANK_SCRIPT = r"""
import sys
import numpy as np
import torch
import torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from active_tracking_rl_amd import map_priority as mp
rank, port, out = int(sys.argv[2]), sys.argv[3], sys.argv[4]
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + port, rank=rank, world_size=2)
K = 5
t = mp.PriorityTable(K, "cpu", "tracker", t_max=500, alpha=0.5)
rs = np.random.RandomState(10 + rank)                    # every rank drains something else
for c in range(3):
    d = np.zeros(K * mp.FIELDS + 1, np.int64)
    stat = d[:K * mp.FIELDS].reshape(K, mp.FIELDS)
    stat[:, 0] = rs.randint(0, 4, K)
    stat[:, 3] = (rs.uniform(-1, 1, K) * stat[:, 0] * 500 * 65536).astype(np.int64)
    stat[:, 4] = -stat[:, 3]
    d[-1] = rank
    t.absorb(torch.from_numpy(d))
np.savez(out, h=t.h.numpy(), stamp=t.stamp.numpy(), w=t.w.numpy(), episodes=t.episodes.numpy(), un=int(t.unattributed), d=d)
dist.destroy_process_group()
"""


def test_two_gloo_ranks_build_the_same_table(tmp_path):
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT)
    outs = [str(tmp_path / ("rank%d.npz" % r)) for r in range(2)]
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(r), port, outs[r]], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(2)]
    for p in procs:
        _, err = p.communicate(timeout=120)
        assert p.returncode == 0, err
    a, b = np.load(outs[0]), np.load(outs[1])
    assert not np.array_equal(a["d"], b["d"])                  # (the ranks did drain different accounts)
    for key in ("h", "stamp", "w", "episodes", "un"):
        assert np.array_equal(a[key], b[key]), key
    assert int(a["un"]) == 3 and (a["stamp"] > 0).any() and len(set(a["w"].tolist())) > 1
