"""-m gpu: prioritized map replay (include/track2d_bank_prio.h; csrc/track2d_hip.hip prio_draw, k_prio_set_weights, k_prio_score,
k_prio_drain; active_tracking_rl_amd/map_priority.py).

  (1) the table: t2d_bank_prio_set_weights is the spec's cum, bit for bit, eagerly and from a replayed graph;
  (2) the draw: every env's map is bank[spec draw] after the reset and after every step, through both pre-generated slots,
      k_gen and k_gen_nav; a zero-weight map is never served;
  (3) a change of the table mid-run: pre-generated slots keep their choice, later episodes follow the new table;
  (4) the accounts: integer for integer the spec's, whole or split into calls, drained in between or not, and the
      unattributed rule;
  (5) every refusal, before any device work;
  (6) training under both graphed schedules."""
import ctypes as C

import numpy as np
import pytest
import torch

import map_bank_spec as bank_spec
import map_priority_spec as ps
from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)
from test_map_bank_gpu import BASE, DEV, NAV, PZR, _actions, _handle, hand_bank

pytestmark = pytest.mark.gpu
SKEW = np.array([3.0, 0.0, 1.0, 0.5, 2.0], np.float32)


def _mp():
    from active_tracking_rl_amd import map_priority
    return map_priority


def _peek(env, ring=False):
    """The handle's table cum [K] (and ring [8, N]) through the library's internal seam."""
    L = _mp().lib()
    f = L.t2d_prio_peek
    f.restype, f.argtypes = C.c_int, [C.c_void_p] * 4
    cum = torch.zeros(env.map_bank_count, dtype=torch.int32, device=DEV)
    chosen = torch.zeros((8, env.num_envs), dtype=torch.int32, device=DEV)
    assert f(env.h, cum.data_ptr(), chosen.data_ptr() if ring else None, None) == 0
    torch.cuda.synchronize()
    cum = cum.cpu().numpy().view(np.uint32)
    return (cum, chosen.cpu().numpy()) if ring else cum


def _set(env, w):
    wd = torch.as_tensor(np.asarray(w, np.float32), device=DEV)
    _mp().lib().t2d_bank_prio_set_weights(env.h, wd.data_ptr(), None)
    torch.cuda.synchronize()
    return wd


def _prio_handle(env_id, n, bank, weights=None, **kw):
    env = _handle(env_id, n, **kw)
    env.attach_map_bank(bank, "cycle")          # (either select: ignored from the enable on)
    env.enable_map_priority()
    if weights is not None:
        _set(env, weights)
    return env


def _attach_raw(env, count, side=82):
    """A bank of `count` empty rooms straight through the C ABI (no per-map Python checks: 65536 maps)."""
    from active_tracking_rl_amd import map_bank
    maps = np.ones((count, side, side), np.uint8)
    maps[:, 1:-1, 1:-1] = 0
    map_bank.lib().t2d_map_bank_attach(env.h, maps.ctypes.data_as(C.c_void_p), None, count, side, 0, None)
    env.enable_map_priority()


def _special_weights(K, seed):
    """Random weights over twelve orders of magnitude with every special value the rule names, where K leaves room."""
    rs = np.random.RandomState(seed)
    w = (10.0 ** rs.uniform(-6, 6, K)).astype(np.float32)
    special = [0.0, np.nan, np.inf, -1.5, 1e-45, 1.1754942e-38 / 4, 3e38, -np.inf, -0.0]     # (1e-45, 2.9e-39: denormals)
    pos = rs.permutation(K)[:len(special)]
    for p, v in zip(pos, special[:K]):
        w[p] = v
    return w


# -- (1) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 5, 64, 65, 1025, 65536])
def test_table_is_the_spec_bit_for_bit(K):
    env = _handle(PZR, 2)
    _attach_raw(env, K)
    assert np.array_equal(_peek(env), np.arange(1, K + 1, dtype=np.uint32))            # enabled: the uniform table q_i = 1
    vectors = [_special_weights(K, 40 + K), np.full(K, 0.25, np.float32), np.full(K, np.nan, np.float32)]
    if K <= 65:
        vectors += [_special_weights(K, s) for s in (1, 2, 3)] + [np.zeros(K, np.float32), np.full(K, 3e38, np.float32)]
    for w in vectors:
        _set(env, w)
        cum = _peek(env)
        assert np.array_equal(cum, ps.table(w)), w[:8]
        assert 1 <= int(cum[-1]) <= ps.TOTAL_MAX
    # the same launch from a graph, replayed twice over a rewritten w_dev
    wd = torch.zeros(K, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _mp().lib().t2d_bank_prio_set_weights(env.h, wd.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for seed in (7, 8):
        w = _special_weights(K, seed)
        wd.copy_(torch.as_tensor(w))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_peek(env), ps.table(w))
    env.reset()                                  # (still a working handle; every map is the same empty room)
    assert env.faults() == 0
    env.close()


# -- (2) ---------------------------------------------------------------------------------------------------------------------
def _check_draws(env, bank, cums, seed, base=BASE):
    """Every env's map is the member the spec draws for its episode under one of the tables `cums`; map_index() names it.
    Returns (episode [N], idx [N], which table index matched per env as a set per env)."""
    st = env.get_state()
    side = bank.shape[1]
    got = env.map_index().cpu().numpy()
    want = [ps.draws(c, seed, base, st["episode"]) for c in cums]
    ok = [got == w for w in want]
    assert np.logical_or.reduce(ok).all()
    maps = env.get_maps()
    assert np.array_equal(maps[:, :side, :side], bank[got])
    return st["episode"], got, ok


@pytest.mark.parametrize("env_id, side", [(PZR, 82), (NAV, 81)])
def test_draw_follows_the_table(env_id, side):
    """70 envs (two waves and a tail), 5 maps, weights 3 : 0 : 1 : 0.5 : 2 set before the first reset, a 3-step time limit:
    reset + 21 steps run every env through at least 7 episodes."""
    n, seed = 70, 11
    bank = hand_bank(5, side)
    env = _prio_handle(env_id, n, bank, SKEW, max_steps=3)
    cum = ps.table(SKEW)
    assert np.array_equal(_peek(env), cum)
    env.reset()
    ep, idx, _ = _check_draws(env, bank, [cum], seed)
    assert (ep == 1).all()
    seen = set(idx.tolist())
    for a0, a1 in _actions(n, 21):
        env.step(a0, a1)
        ep, idx, _ = _check_draws(env, bank, [cum], seed)
        seen.update(idx.tolist())
    assert (ep >= 7).all() and 1 not in seen and seen == {0, 2, 3, 4}
    assert env.faults() == 0
    env.close()


def test_one_map_draws_nothing():
    env = _prio_handle(PZR, 70, hand_bank(1), max_steps=3)
    env.reset()
    for a0, a1 in _actions(70, 7):
        env.step(a0, a1)
        assert not env.map_index().cpu().numpy().any()
    assert np.array_equal(env.get_maps(), hand_bank(1)[np.zeros(70, int)]) and env.faults() == 0
    env.close()


# -- (3) ---------------------------------------------------------------------------------------------------------------------
def test_change_of_table_mid_run():
    """Table A for 7 steps, then B. Every later episode's index is the draw under A or under B; from each env's third episode
    after the change on it is B's (the generator runs at most two episodes ahead)."""
    n, seed = 70, 11
    bank = hand_bank(5)
    wa, wb = SKEW, np.array([0.0, 5.0, 0.0, 0.0, 1.0], np.float32)
    ca, cb = ps.table(wa), ps.table(wb)
    env = _prio_handle(PZR, n, bank, wa, max_steps=3)
    env.reset()
    acts = _actions(n, 7 + 18, seed=4)
    for a0, a1 in acts[:7]:
        env.step(a0, a1)
    ep0, _, _ = _check_draws(env, bank, [ca], seed)
    _set(env, wb)
    assert np.array_equal(_peek(env), cb)
    only_b = 0
    for a0, a1 in acts[7:]:
        env.step(a0, a1)
        ep, idx, ok = _check_draws(env, bank, [ca, cb], seed)
        late = ep >= ep0 + 3
        assert ok[1][late].all()
        only_b += int((late & ~ok[0]).sum())
        assert ok[0][ep == ep0].all()
    assert (ep >= ep0 + 4).all() and only_b > 0        # (the new table was served, to episodes A would have given another map)
    assert env.faults() == 0
    env.close()


# -- (4) ---------------------------------------------------------------------------------------------------------------------
def _roll(env, acts):
    """Step through `acts`: (idx [T, N] the index each env ran during the step, rew [T, N, 2] and done [T, N] device tensors)."""
    idx, rew, done = [], [], []
    for a0, a1 in acts:
        idx.append(env.map_index().cpu().numpy())
        _, r, d = env.step(a0, a1)
        rew.append(r.clone()); done.append(d.clone())
    return np.stack(idx), torch.stack(rew), torch.stack(done)


def _drained(prio, K):
    d = prio.drain().cpu().numpy()
    return d[:K * 5].reshape(K, 5), int(d[-1])


def _as_int(stat):
    return np.array(stat.tolist(), np.int64)


def test_score_is_the_spec_integer_for_integer():
    """70 envs, two windows of 20 steps with a 7-step time limit. Handle A scores 20, drains, scores 20, drains; handle B (same
    seed, same actions) scores 7 + 13 + 20 and drains once."""
    from active_tracking_rl_amd.map_priority import MapPriority
    n, K, T, succ = 70, 5, 20, 7
    bank = hand_bank(K)
    acts = _actions(n, 2 * T, seed=6)
    a = _prio_handle(PZR, n, bank, SKEW, max_steps=7)
    pa = MapPriority(a, DEV, success_len=succ)
    a.reset()
    carry, total, spec_total = None, np.zeros((K, 5), np.int64), np.zeros((K, 5), np.int64)
    record = []
    for win in range(2):
        idx, rew, done = _roll(a, acts[win * T:(win + 1) * T])
        record.append((idx, rew, done))
        pa.update(rew, done)
        stat, lost = _drained(pa, K)
        want, wl, carry = ps.score(idx, rew.cpu().numpy(), done.cpu().numpy(), succ, carry=carry, count=K)
        assert wl == 0 and lost == 0
        assert np.array_equal(stat, _as_int(want)), win
        assert stat[:, 0].sum() == int(done.sum().item()) >= 2 * n and stat[1].sum() == 0
        total += stat; spec_total += _as_int(want)
    assert (np.concatenate([r[2].cpu().numpy() for r in record]).sum(0) >= 4).all()
    stat, lost = _drained(pa, K)
    assert not stat.any() and lost == 0             # a second drain finds nothing
    assert a.faults() == 0
    a.close()
    b = _prio_handle(PZR, n, bank, SKEW, max_steps=7)
    pb = MapPriority(b, DEV, success_len=succ)
    b.reset()
    for lo, hi in ((0, 7), (7, 20), (20, 40)):
        idx, rew, done = _roll(b, acts[lo:hi])
        assert np.array_equal(idx, np.concatenate([r[0] for r in record])[lo:hi])
        pb.update(rew, done)
    stat, lost = _drained(pb, K)
    assert np.array_equal(stat, total) and np.array_equal(stat, spec_total) and lost == 0
    b.close()


def test_more_than_five_ends_in_a_call_are_unattributed():
    """A 2-step time limit and T = 20: ten ends per env in one call; the five oldest of each env add nothing to any map."""
    from active_tracking_rl_amd.map_priority import MapPriority
    n, K, T = 70, 5, 20
    env = _prio_handle(PZR, n, hand_bank(K), SKEW, max_steps=2)
    prio = MapPriority(env, DEV, success_len=2)
    env.reset()
    idx, rew, done = _roll(env, _actions(n, T, seed=8))
    assert (done.sum(0) == 10).all()
    prio.update(rew, done)
    stat, lost = _drained(prio, K)
    want, wl, _ = ps.score(idx, rew.cpu().numpy(), done.cpu().numpy(), 2, count=K)
    assert wl == 5 * n == lost
    assert np.array_equal(stat, _as_int(want)) and stat[:, 0].sum() == 5 * n
    assert env.faults() == 0
    env.close()


# -- (5) ---------------------------------------------------------------------------------------------------------------------
def _refused(code, match, fn, *args):
    from active_tracking_rl_amd.vec_env import T2DError
    with pytest.raises(T2DError, match=r"\(%d\).*%s" % (code, match)):
        fn(*args)


def test_refusals():
    """T2D_ERR_INVALID (-1) and T2D_ERR_STATE (-4), straight at the C ABI, each before any device work."""
    from active_tracking_rl_amd import map_bank
    L = _mp().lib()
    buf = torch.zeros(64, dtype=torch.int64, device=DEV)
    rew, done = torch.zeros((2, 4, 2), device=DEV), torch.zeros((2, 4), dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    score = lambda h, r, d, T=2: L.t2d_bank_prio_score(h, r, 8, 2, 1, d, 4, 1, T, 10, None)
    bare = _handle(PZR, 4)
    _refused(-1, "null", L.t2d_bank_prio_enable, None, None)
    _refused(-4, "no map bank", L.t2d_bank_prio_enable, bare.h, None)
    for fn, args in ((L.t2d_bank_prio_set_weights, (bare.h, p(rew), None)), (L.t2d_bank_prio_drain, (bare.h, p(buf), None)),
                     (score, (bare.h, p(rew), p(done)))):
        _refused(-4, "no priorities", fn, *args)
    bare.attach_map_bank(hand_bank(3), "random")
    for fn, args in ((L.t2d_bank_prio_set_weights, (bare.h, p(rew), None)), (L.t2d_bank_prio_drain, (bare.h, p(buf), None)),
                     (score, (bare.h, p(rew), p(done)))):
        _refused(-4, "no priorities", fn, *args)             # a bank alone is not enough
    bare.reset()
    _refused(-4, "before the first", L.t2d_bank_prio_enable, bare.h, None)
    assert np.array_equal(bare.map_index().cpu().numpy(), bank_spec.indices(bank_spec.RANDOM, 11, BASE, [1] * 4, 3))
    bare.close()
    env = _handle(PZR, 4)
    env.attach_map_bank(hand_bank(3), "cycle")
    env.enable_map_priority()
    _refused(-4, "already", L.t2d_bank_prio_enable, env.h, None)
    _refused(-1, "null", L.t2d_bank_prio_set_weights, env.h, None, None)
    _refused(-1, "null", L.t2d_bank_prio_set_weights, None, p(rew), None)
    _refused(-1, "null", L.t2d_bank_prio_drain, env.h, None, None)
    _refused(-1, "null", score, env.h, None, p(done))
    _refused(-1, "null", score, env.h, p(rew), None)
    _refused(-1, "null", score, None, p(rew), p(done))
    _refused(-4, "t2d_reset first", score, env.h, p(rew), p(done))
    env.reset()
    _refused(-1, "T > 0", score, env.h, p(rew), p(done), 0)
    _refused(-1, "stride", L.t2d_bank_prio_score, env.h, p(rew), -8, 2, 1, p(done), 4, 1, 2, 10, None)
    # snapshots of a prioritised handle
    from active_tracking_rl_amd.vec_env import T2DError
    snap = env.snapshot()
    for call in (snap.save, snap.restore, lambda: snap.load_bytes(b"\0" * 256)):
        with pytest.raises(T2DError, match=r"\(-4\).*priority table"):
            call()
    snap.close()
    # ... and attach's own refusals stand
    other = _handle(PZR, 4)
    maps = np.ascontiguousarray(hand_bank(3))
    _refused(-1, "select", map_bank.lib().t2d_map_bank_attach, other.h, maps.ctypes.data_as(C.c_void_p), None, 3, 82, 2, None)
    other.close()
    env.step(*_actions(4, 1)[0])
    assert score(env.h, p(rew), p(done)) == 0 and env.faults() == 0       # (the refused handle still works)
    torch.cuda.synchronize()
    env.close()


# -- (6) ---------------------------------------------------------------------------------------------------------------------
class _Writer(object):
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, tag, value, step):
        self.scalars[tag] = float(value)


@pytest.mark.parametrize("schedule", ["synchronous", "pipelined"])
def test_training_refreshes_the_table(schedule, tmp_path):
    from active_tracking_rl_amd import map_priority as mp
    from active_tracking_rl_amd.map_bank import MapBank
    from active_tracking_rl_amd.train import GraphedIteration, PipelinedIteration, default_args, make_player
    dev = torch.device(DEV)
    bank = MapBank(hand_bank(5))
    args = default_args(env=PZR, num_envs=64, seed=3, map_bank=bank, map_priority="tracker", map_priority_every=2)
    player, opt = make_player(args, dev)
    prio = player.env.map_priority
    assert isinstance(prio, mp.MapPriority) and prio.role == "tracker" and prio.every == 2
    uniform = prio.w.clone()
    assert torch.equal(uniform, torch.full((5,), 0.2, dtype=torch.float32, device=dev))
    it = GraphedIteration(player, opt, args) if schedule == "synchronous" else PipelinedIteration(player, opt, args)
    for _ in range(6):
        it.run()
    it.finish()
    torch.cuda.synchronize()
    assert prio.ticks == 6 and prio.table.c == 3
    w = _Writer()
    out = prio.record(w, 6 * 20 * 64, 0, str(tmp_path))
    for tag in mp.TAGS + tuple("train/map/%d/hardness" % i for i in range(5)):
        assert tag in w.scalars, tag
    assert int(prio.table.episodes.sum()) > 0                       # episodes are counted ...
    assert out["train/map_priority/unattributed"] == 0              # ... every one on its map
    assert not torch.equal(prio.w, uniform)                         # the table moved
    assert 0 < out["train/map_priority/seen_fraction"] <= 1 and 0.2 < out["train/map_priority/max_weight"] <= 1
    cum = _peek(player.env.core)
    assert np.array_equal(cum, ps.table(prio.w.cpu().numpy()))      # and it is the handle's table
    path = tmp_path / "map_priority.npz"
    assert path.exists()
    with np.load(str(path)) as z:
        assert set(z.files) >= {"h", "stamp", "c", "episodes", "w"} and int(z["c"]) == 3
        assert np.array_equal(z["w"], prio.w.cpu().numpy())
    fresh = mp.PriorityTable(5, dev, "tracker", prio.table.t_max)
    with np.load(str(path)) as z:
        fresh.load_state_dict({k: z[k] for k in z.files})
    assert torch.equal(fresh.w, prio.w) and torch.equal(fresh.h, prio.table.h) and fresh.c == 3
    before = prio.w.clone()
    prio.load_state_dict(str(path))
    torch.cuda.synchronize()
    assert torch.equal(prio.w, before) and np.array_equal(_peek(player.env.core), cum)
    assert player.env.core.faults() == 0 and torch.isfinite(opt.bucket.flat).all()
    player.env.close()


def test_without_the_flag_nothing_is_attached():
    from active_tracking_rl_amd.map_bank import MapBank
    from active_tracking_rl_amd.train import default_args, make_player
    args = default_args(env=PZR, num_envs=64, seed=3, map_bank=MapBank(hand_bank(5)))
    player, _ = make_player(args, torch.device(DEV))
    assert player.env.map_priority is None and not player.env.core.map_priority_enabled
    player.env.close()
