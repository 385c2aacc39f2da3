"""-m gpu: the GRU cores' learner behind the --fused-gru cache — the BPTT launch with the by-action column sums of dG
(csrc/gru_hip.hip: atr_gru_bptt_sums, include/atr_gru_sums.h), the folded tracker-action embedding of 'tat-maze-gru' and the
grouped weight-gradient launch (fused._GruSeqCached, fused.DeferredWeightGrads).

  1 the sums kernel against its own dG; 2 the fold against the explicit embedding below the grouped threshold; 3 grouped launch +
    fold against the learner without a cache, what was launched, the bucket slices; 4 a full group; 5 both captured schedules;
  6 nothing of it without the switch; and the LSTM learner's problem records, unchanged."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENV = "Track2D-BlockPartialPZR-v0"
R = 128


def _dev():
    return torch.device(DEV)


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
def _bptt_case(P, T, N, seed, actions_max=4):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    acts = torch.cat([torch.sigmoid(rnd(P, T, N, 2 * R)), torch.tanh(rnd(P, T, N, R)), rnd(P, T, N, R)], -1)    # (r, z, n, q)
    keep = (torch.rand(T, N, generator=g) > 0.25).float()
    keep[T - 1, 0] = 0.0
    keep[0, N - 1] = 0.0
    store = torch.randint(0, actions_max, (T, 2, N), generator=g, dtype=torch.int64)      # the rollout's [T, players, N] store
    return dict(acts=acts.contiguous().to(DEV), h_all=rnd(P, T + 1, N, R).to(DEV), keep=keep.to(DEV),
                dh=[rnd(T, N, R).to(DEV) for _ in range(P)], whh=[(0.1 * rnd(3 * R, R)).to(DEV) for _ in range(P)],
                store=store.to(DEV))


@pytest.mark.parametrize("P,T,N,emb_player,amax", [(2, 3, 40, 1, 4), (2, 5, 49, 1, 4), (1, 1, 16, 0, 4), (2, 3, 32, 1, 3)],
                         ids=["tile-of-8-rows", "tile-of-1-row", "target-alone", "action-3-absent"])
def test_sums_kernel_against_its_own_dg(P, T, N, emb_player, amax):
    """1. atr_gru_bptt_sums: dG and dh_init bit for bit atr_gru_bptt's; S = act_sums summed over the tiles (float64) against the
    float64 sum of the kernel's own dG[..., 0:3R] grouped by action, |S - S64| <= T N 2^-24 sum|terms| per entry (the bound of an
    f32 sum of that many terms in any order; the tiles' sums are added in float64 here); rows past N counted nowhere (the bound
    says so); an absent action's block exactly zero; every float of the NaN-poisoned buffer written."""
    from active_tracking_rl_amd import fused
    L = fused.lib()
    c = _bptt_case(P, T, N, seed=100 * T + N, actions_max=amax)
    p_, pn = fused._p, fused._pn
    st = fused._stream(c["acts"])
    ps, pa = (T + 1) * N * R, T * N * 4 * R
    new = lambda *s: torch.full(s, float("nan"), device=DEV)
    dg0, dh0 = new(P, T, N, 4 * R), new(P, N, R)
    w = c["whh"]
    L.atr_gru_bptt(p_(c["dh"][0]), pn(c["dh"][1] if P > 1 else None), p_(c["keep"]), p_(c["acts"]), pa, p_(c["h_all"]), ps,
                   p_(w[0]), pn(w[1] if P > 1 else None), p_(dg0), pa, p_(dh0), P, T, N, R, st)
    n_floats = L.atr_gru_bptt_act_sums_floats(N)
    tiles = (N + 15) // 16
    assert n_floats == tiles * 4 * 3 * R
    act = c["store"][:, 0]                                      # [T, N] view, rows 2 N apart: read in place
    assert act.stride(0) == 2 * N and act.stride(1) == 1
    dg1, dh1, sums = new(P, T, N, 4 * R), new(P, N, R), new(n_floats)
    L.atr_gru_bptt_sums(p_(c["dh"][0]), pn(c["dh"][1] if P > 1 else None), p_(c["keep"]), p_(c["acts"]), pa, p_(c["h_all"]), ps,
                        p_(w[0]), pn(w[1] if P > 1 else None), p_(dg1), pa, p_(dh1), emb_player, 4, p_(act), act.stride(0),
                        p_(sums), P, T, N, R, st)
    torch.cuda.synchronize()
    assert torch.isfinite(dg0).all() and torch.isfinite(dh0).all()
    assert torch.equal(dg1, dg0) and torch.equal(dh1, dh0)
    assert torch.isfinite(sums).all()
    S = sums.view(tiles, 4, 3 * R).double().sum(0).cpu()
    terms = dg1[emb_player, :, :, :3 * R].double().cpu()        # [T, N, 3R]
    a = act.cpu()
    worst = 0.0
    for k in range(4):
        m = (a == k).unsqueeze(-1).double()
        S64, mag = (terms * m).sum((0, 1)), (terms.abs() * m).sum((0, 1))
        err, bound = (S[k] - S64).abs(), T * N * 2.0 ** -24 * mag
        print("action %d: %d rows, max|S| %.3e, max err %.2e, min slack %.2e" % (k, int((a == k).sum()), float(S64.abs().max()),
                                                                                 float(err.max()), float((bound - err).min())))
        assert bool((err <= bound).all()), k
        worst = max(worst, float(err.max()))
    if amax == 3:
        assert float(S[3].abs().max()) == 0.0 and float(sums.view(tiles, 4, 3 * R)[:, 3].abs().max()) == 0.0
    with pytest.raises(RuntimeError, match=r"atr_gru_bptt_sums failed \(-1\)"):       # (the four-move table only)
        L.atr_gru_bptt_sums(p_(c["dh"][0]), pn(c["dh"][1] if P > 1 else None), p_(c["keep"]), p_(c["acts"]), pa, p_(c["h_all"]),
                            ps, p_(w[0]), pn(w[1] if P > 1 else None), p_(dg1), pa, p_(dh1), emb_player, 5, p_(act),
                            act.stride(0), p_(sums), P, T, N, R, st)


# ---- the learner's fixtures (as tests/test_gru_fused_gpu.py builds them) ------------------------------------------------------------
def _player(net, n_envs=64, num_steps=3, seed=23, fused_gru=True, **kw):
    from active_tracking_rl_amd.train import default_args, make_player
    args = default_args(env=kw.pop("env", ENV), network=net, aux="reward" if "tat" in net else "none", num_envs=n_envs,
                        num_steps=num_steps, seed=seed, fused_gru=fused_gru, **kw)
    args.gpu_ids = [0]
    player, opt = make_player(args, _dev())
    return args, player, opt


def _rolled(net, warm=5, **kw):
    """An Agent after `warm` rollouts (so that h0 is not zero and some episodes may have ended) plus the one under test."""
    from active_tracking_rl_amd.train import rollout
    args, player, opt = _player(net, **kw)
    with torch.no_grad():
        for p in player.model.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)           # biases start at zero: make b_hn and the rest tell
    for _ in range(warm):
        rollout(player, args.num_steps)
        player.clear_actions()
    rollout(player, args.num_steps)
    torch.cuda.synchronize()
    return args, player, opt


def _loss_grads(player, mode, params, bucket=None, info=None):
    """The loss's gradients over the stored rollout; with `bucket`, inside the grouped weight-gradient launch's context as
    Agent.compute_grads opens it (check, then flush). The bootstrap step's draw is the same in every call: the sampler's ordinal
    is put back."""
    from active_tracking_rl_amd import fused
    sampler = getattr(player.model, "_sampler", None)
    last = getattr(sampler, "_last", None)
    try:
        out = player.loss_recompute(mode)[0]
    finally:
        if sampler is not None and last is not None:
            sampler._last = last
    terms = list(out) if isinstance(out, (tuple, list)) else [out]
    ones = [torch.ones_like(t) for t in terms]
    if bucket is None:
        return torch.autograd.grad(terms, params, grad_outputs=ones, allow_unused=True)
    with fused.deferred_weight_grads(bucket) as q:
        assert q is not None
        grads = torch.autograd.grad(terms, params, grad_outputs=ones, allow_unused=True)
        q.check(grads)
        if info is not None:
            info["registered"] = len(q.problems)
        q.flush()
    return grads


@contextlib.contextmanager
def _tracker_draws(model, a0):
    """model() with the tracker's drawn action replaced by a0 [N] (tat only): the reference is fed the bootstrap step's recorded
    tracker action, on which the tracker-aware target's value depends."""
    if not model.tat:
        yield
        return
    actor = model.player0.actor
    real = actor.forward

    def fed(x, test=False):
        _, entropy, log_prob = real(x, test)
        return a0, entropy, log_prob
    actor.forward = fed
    try:
        yield
    finally:
        del actor.forward


def _grads_with_and_without_the_cache(pl, mode, params, bucket=None, info=None):
    """Every gradient of the Agent's loss over the stored rollout, at the configured gamma and tau: with the cache (the fused
    heads, boot_values on the GRU cache, gru_sequence_cached) and with the cache hidden from the Agent (forward_sequence from h0 and
    model() for the bootstrap value: the path without a cache). Returns (with, without)."""
    m = pl.model
    assert pl.args.gamma > 0 and pl.args.tau > 0
    seen = []
    real = m.boot_values

    def boot(states, cache, done, v_out):
        out = real(states, cache, done, v_out)
        seen.append(cache.boot.actions[0].clone())
        return out
    m.boot_values = boot
    try:
        g_new = _loss_grads(pl, mode, params, bucket=bucket, info=info)
    finally:
        del m.boot_values
    assert len(seen) == 1                    # the bootstrap value came from boot_values, once
    if info is not None and info.get("spy") is not None:
        info["spy"].recording = False        # (what the cached learner launched: the reference's launches are not its)
    if bucket is not None:                   # (the bucket slices are overwritten by nothing below, but keep what was compared)
        g_new = tuple(g.clone() if g is not None else None for g in g_new)
    cache, pl._cache = pl._cache, None
    try:
        with _tracker_draws(m, seen[0]):
            g_ref = _loss_grads(pl, mode, params)
    finally:
        pl._cache = cache
    return g_new, g_ref


def _hold_to_the_uncached_learner(names, g_new, g_ref, mode):
    """tests/test_gru_fused_gpu.py's criterion: err <= 2e-4 max|ref| per parameter; untrained players' gradients None or zero."""
    seen = 0
    for name, a, b in zip(names, g_new, g_ref):
        if mode in (0, 1) and not name.startswith("player%d." % mode) or b is None:
            assert a is None or float(a.abs().max()) == 0.0, name
            continue
        scale = float(b.abs().max())
        ratio = float((a - b).abs().max()) / scale if scale > 0 else float(a.abs().max())
        print("%-40s max|ref| %.3e  err / max|ref| %.2e" % (name, scale, ratio))
        assert a is not None and torch.isfinite(a).all() and ratio <= 2e-4, name
        seen += 1
    assert seen >= 8


class _Spy(object):
    """Counts the library's learner entry points and keeps the problem records handed to atr_gemm_tn_grouped."""
    NAMES = ("atr_gemm_tn", "atr_gemm_tn_grouped", "atr_embed_add", "atr_embed_add_ld", "atr_embed_grad", "atr_embed_fold",
             "atr_gru_bptt", "atr_gru_bptt_sums")

    def __init__(self, monkeypatch):
        from active_tracking_rl_amd import fused
        self.calls, self.groups, self.recording = [], [], True
        L = fused.lib()
        for name in self.NAMES:
            real = getattr(L, name)

            def spy(*a, _name=name, _real=real):
                if self.recording:
                    self.calls.append(_name)
                if self.recording and _name == "atr_gemm_tn_grouped":
                    self.groups.append([dict(x1=a[0][q].x1, x2=a[0][q].x2, c=a[0][q].c, M=a[0][q].M, N=a[0][q].N, ld1=a[0][q].ld1,
                                             ld2=a[0][q].ld2, colsum0=a[0][q].colsum0, colsum1=a[0][q].colsum1,
                                             row_scale=a[0][q].row_scale) for q in range(a[1])])
                return _real(*a)
            monkeypatch.setattr(L, name, spy)

    def count(self, prefix):
        return sum(c == prefix for c in self.calls)


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [-1, 1])
def test_fold_against_the_explicit_embedding_below_the_grouped_threshold(mode, monkeypatch):
    """2. 256 envs x 3 steps, one stored rollout: with fold_embedding the gradients of the target's weight_ih and of
    fc_action_tracker agree with the explicit f + E[a] within 2e-5 max|ref| + 1e-9 (a re-association); every other gradient bit
    for bit; the fold ran (atr_gru_bptt_sums, atr_embed_fold) and the explicit embedding's launches did not."""
    from active_tracking_rl_amd import fused
    args, pl, _ = _rolled("tat-maze-gru", warm=2, n_envs=256)
    names, params = zip(*pl.model.named_parameters())
    monkeypatch.setattr(fused, "fold_embedding", False)
    g_ref = _loss_grads(pl, mode, params)
    monkeypatch.setattr(fused, "fold_embedding", True)
    spy = _Spy(monkeypatch)
    g_new = _loss_grads(pl, mode, params)
    torch.cuda.synchronize()
    assert spy.count("atr_gru_bptt_sums") == 1 and spy.count("atr_embed_fold") == 1
    assert not any(c.startswith("atr_embed_add") or c.startswith("atr_embed_grad") for c in spy.calls)
    assert spy.count("atr_gru_bptt") == 0                  # (one BPTT launch for the group: the sums variant)
    folded = ("player1.lstm.weight_ih", "player1.fc_action_tracker.weight", "player1.fc_action_tracker.bias")
    for name, a, b in zip(names, g_new, g_ref):
        assert (a is None) == (b is None), name
        if b is None:
            continue
        if name in folded:
            err, lim = float((a - b).abs().max()), 2e-5 * float(b.abs().max()) + 1e-9
            print("%-40s max|ref| %.3e  err %.2e  limit %.2e" % (name, float(b.abs().max()), err, lim))
            assert float(b.abs().max()) > 0 and err <= lim, name
        else:
            assert torch.equal(a, b), name
    pl.env.close()


# ---- 3, 4 ----------------------------------------------------------------------------------------------------------------------
def _grouped_case(net, mode, monkeypatch):
    from active_tracking_rl_amd import fused
    assert fused.fold_embedding and fused.use_grouped_dw
    args, pl, opt = _rolled(net, warm=2, n_envs=512, num_steps=8)
    bucket = opt.bucket
    names, params = zip(*pl.model.named_parameters())
    bucket.grad.fill_(float("nan"))
    spy = _Spy(monkeypatch)
    info = dict(spy=spy)
    g_new, g_ref = _grads_with_and_without_the_cache(pl, mode, params, bucket=bucket, info=info)
    torch.cuda.synchronize()
    return pl, bucket, names, params, spy, info, g_new, g_ref


@pytest.mark.parametrize("mode", [-1, 0, 1])
@pytest.mark.parametrize("net", ["tat-maze-gru", "maze-gru"])
def test_grouped_launch_and_fold_against_the_learner_without_a_cache(net, mode, monkeypatch):
    """3. 512 envs x 8 steps (T N = 4096: the smallest grouped shape): every parameter gradient against forward_sequence on the same
    stored rollout (err <= 2e-4 max|ref|; untrained players None or zero); ONE grouped launch holds the fc products and three
    problems per trained player (ld1 = 4R: column blocks of dG), no weight-gradient GEMM, embedding pass or gather beside it; the
    registered gradients are the bucket's slices, written in full over the NaN they held."""
    pl, bucket, names, params, spy, info, g_new, g_ref = _grouped_case(net, mode, monkeypatch)
    _hold_to_the_uncached_learner(names, g_new, g_ref, mode)
    tat = net.startswith("tat")
    trained = [0, 1] if mode == -1 else [mode]
    assert spy.count("atr_gemm_tn_grouped") == 1 and len(spy.groups) == 1
    group = spy.groups[0]
    # three problems per trained player beside BOTH encoders' fc products: an untrained player's fc node still runs, on the zero
    # gradient autograd materialises for it, and registers its product like the trained one's (x1 dense: ld1 == M)
    assert len(group) == info["registered"] == 3 * len(trained) + 2
    slices = {p.data_ptr(): v for p, v in zip(bucket.params, bucket.grad_views())}
    named = dict(zip(names, params))
    fcs = [g for g in group if g["ld1"] == g["M"]]
    assert sorted(g["c"] for g in fcs) == sorted(slices[named["player%d.encoder.fc.weight" % p].data_ptr()].data_ptr()
                                                 for p in (0, 1))
    assert len(group) - len(fcs) == 3 * len(trained)
    assert spy.count("atr_gemm_tn") == 0
    assert not any(c.startswith("atr_embed_add") or c.startswith("atr_embed_grad") for c in spy.calls)
    fold_here = tat and 1 in trained
    assert spy.count("atr_gru_bptt_sums") == (1 if fold_here else 0) and spy.count("atr_embed_fold") == (1 if fold_here else 0)
    assert spy.count("atr_gru_bptt") == (0 if fold_here else 1)
    views = {name: slices[p.data_ptr()] for name, p in zip(names, params) if ".lstm." in name}
    for p in (0, 1):
        wih, whh = views["player%d.lstm.weight_ih" % p], views["player%d.lstm.weight_hh" % p]
        bih, bhh = views["player%d.lstm.bias_ih" % p], views["player%d.lstm.bias_hh" % p]
        mine = [g for g in group if g["c"] in (wih.data_ptr(), whh.data_ptr(), whh[2 * R:].data_ptr())]
        if p not in trained:
            assert mine == [], p
            continue
        assert len(mine) == 3 and all(g["ld1"] == 4 * R for g in mine), p
        a, b, c = sorted(mine, key=lambda g: (g["c"] != wih.data_ptr(), g["c"]))
        assert (a["c"], a["M"], a["colsum0"]) == (wih.data_ptr(), 3 * R, bih.data_ptr())
        assert (b["c"], b["M"], b["N"], b["colsum0"]) == (whh.data_ptr(), 2 * R, R, bhh.data_ptr())
        assert (c["c"], c["M"], c["N"], c["colsum0"]) == (whh[2 * R:].data_ptr(), R, R, bhh[2 * R:].data_ptr())
        assert b["x1"] == a["x1"] and c["x1"] == a["x1"] + 3 * R * 4 and b["x2"] == c["x2"]
        assert b["row_scale"] is None and c["row_scale"] is None           # (the rollout stored every k h row)
    # the gradients autograd got back ARE the slices (check() passed inside), and the slices are written in full
    raw = _loss_grads_slices(pl, mode, params, bucket)
    for name, g, p in zip(names, raw, params):
        if ".lstm." in name and int(name[6]) in trained:
            assert g.data_ptr() == views[name].data_ptr(), name
            assert torch.isfinite(views[name]).all(), name
    pl.env.close()


def _loss_grads_slices(pl, mode, params, bucket):
    """One more pass over the same rollout into a NaN-filled bucket: the raw gradients (no clones), after the flush."""
    bucket.grad.fill_(float("nan"))
    g = _loss_grads(pl, mode, params, bucket=bucket)
    torch.cuda.synchronize()
    return g


def test_a_full_group_leaves_one_product_on_the_spot(monkeypatch):
    """4. DeferredWeightGrads.MAX = 7: the same learner still meets the criterion of 3; seven problems went out grouped, the one
    that found no room was computed on the spot, and nothing raised."""
    from active_tracking_rl_amd import fused
    monkeypatch.setattr(fused.DeferredWeightGrads, "MAX", 7)
    pl, bucket, names, params, spy, info, g_new, g_ref = _grouped_case("tat-maze-gru", -1, monkeypatch)
    _hold_to_the_uncached_learner(names, g_new, g_ref, -1)
    assert spy.count("atr_gemm_tn_grouped") == 1 and len(spy.groups[0]) == 7 == info["registered"]
    pl.env.close()


def test_a_player_joins_with_all_three_products_or_none(monkeypatch):
    """4. DeferredWeightGrads.MAX = 5: the tracker's three products join, the target's find two places and take none (its
    gradients on the spot, the fold included), the fc products fill the group; the criterion of 3 holds."""
    from active_tracking_rl_amd import fused
    monkeypatch.setattr(fused.DeferredWeightGrads, "MAX", 5)
    pl, bucket, names, params, spy, info, g_new, g_ref = _grouped_case("tat-maze-gru", -1, monkeypatch)
    _hold_to_the_uncached_learner(names, g_new, g_ref, -1)
    group = spy.groups[0]
    assert len(group) == 5 and sum(g["ld1"] == 4 * R for g in group) == 3
    assert spy.count("atr_embed_fold") == 1 and spy.count("atr_gru_bptt_sums") == 1
    pl.env.close()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def test_eager_iteration_and_graph_replay_agree_at_the_grouped_shape():
    """5. 512 envs x 8 steps, tat-maze-gru, switch on: one eager iteration and one GraphedIteration replay from identical weights,
    env shard, seed and draw-stream position leave the same weights behind (torch.equal); two more replays: finite weights, a
    cache, cx zero, no env fault."""
    from active_tracking_rl_amd.train import GraphedIteration, rolled_back, rollout, update_tensors
    dev = _dev()
    kw = dict(n_envs=512, num_steps=8)
    args, pa, oa = _player("tat-maze-gru", **kw)
    with rolled_back(update_tensors(oa)):               # what GraphedIteration's constructor does before it captures
        for _ in range(2):
            rollout(pa, args.num_steps)
            pa.optimize(None, oa, pa.model, args.train_mode, dev)
        torch.cuda.synchronize()
    pa.env.flush()
    rollout(pa, args.num_steps)
    assert pa._cache is not None and pa._cache.gru
    pa.optimize(None, oa, pa.model, args.train_mode, dev)
    torch.cuda.synchronize()
    w_eager = oa.bucket.flat.clone()
    pa.env.close()
    args, pb, ob = _player("tat-maze-gru", **kw)
    w0 = ob.bucket.flat.clone()
    it = GraphedIteration(pb, ob, args)
    it.run()
    torch.cuda.synchronize()
    assert torch.isfinite(w_eager).all() and torch.equal(ob.bucket.flat, w_eager)
    it.run()
    it.run()
    it.finish()
    torch.cuda.synchronize()
    assert torch.isfinite(ob.bucket.flat).all() and not torch.equal(ob.bucket.flat, w0)
    assert pb.model.env_step_fused_seen is True and pb._cache is not None and pb._cache.gru
    assert float(it.carry["cxs"].abs().max()) == 0.0 and float(it.carry["hxs"].abs().max()) > 0.0
    assert torch.isfinite(it.carry["hxs"]).all() and pb.env.core.faults() == 0
    pb.env.close()


def test_pipelined_schedule_trains_at_the_grouped_shape():
    """5. PipelinedIteration at 1024 envs x 4 steps (the co-run form of the grouped launch, eight problems), three iterations:
    what tests/test_gru_fused_gpu.py holds the schedule to, and no env fault."""
    from active_tracking_rl_amd.train import PipelinedIteration
    args, player, opt = _player("tat-maze-gru", n_envs=1024, num_steps=4)
    w0 = opt.bucket.flat.clone()
    it = PipelinedIteration(player, opt, args)
    for i in range(3):
        it.run()
        it.sync()
    it.finish()
    torch.cuda.synchronize()
    assert torch.isfinite(opt.bucket.flat).all() and not torch.equal(opt.bucket.flat, w0)
    assert player.model.env_step_fused_seen is True
    assert all(a._cache is not None and a._cache.gru for a in it.players)
    assert float(it.carry["cxs"].abs().max()) == 0.0 and float(it.carry["hxs"].abs().max()) > 0.0
    assert torch.isfinite(it.carry["hxs"]).all() and player.env.core.faults() == 0
    player.env.close()


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def test_without_the_switch_nothing_changes(monkeypatch):
    """6. --fused-gru off, tat-maze-gru at 512 x 8: the learner never reaches atr_gru_bptt_sums nor the fold, and its gradients are
    bit for bit those of a pass made with fold_embedding = False and use_grouped_dw = False."""
    from active_tracking_rl_amd import fused
    from active_tracking_rl_amd.train import rollout
    args, pl, opt = _player("tat-maze-gru", n_envs=512, num_steps=8, fused_gru=False)
    rollout(pl, args.num_steps)
    torch.cuda.synchronize()
    assert pl._cache is None
    names, params = zip(*pl.model.named_parameters())
    assert hasattr(fused.lib(), "atr_gru_bptt_sums")
    spy = _Spy(monkeypatch)

    a0 = torch.zeros(args.num_envs, dtype=torch.int64, device=DEV)       # (the bootstrap step's tracker action: the same twice)

    def grads():
        with _tracker_draws(pl.model, a0):
            out = pl.loss_recompute(-1)[0]
        terms = list(out) if isinstance(out, (tuple, list)) else [out]
        with fused.deferred_weight_grads(opt.bucket) as q:
            g = torch.autograd.grad(terms, params, grad_outputs=[torch.ones_like(t) for t in terms], allow_unused=True)
            if q is not None:
                q.check(g)
                q.flush()
        return [x.clone() if x is not None else None for x in g]
    state = torch.cuda.get_rng_state(0), torch.get_rng_state()
    g_on = grads()
    assert spy.count("atr_gru_bptt_sums") == 0 and spy.count("atr_embed_fold") == 0
    monkeypatch.setattr(fused, "fold_embedding", False)
    monkeypatch.setattr(fused, "use_grouped_dw", False)
    torch.cuda.set_rng_state(state[0], 0)
    torch.set_rng_state(state[1])
    g_off = grads()
    torch.cuda.synchronize()
    for name, a, b in zip(names, g_on, g_off):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), name
    pl.env.close()


# ---- the LSTM learner's records ------------------------------------------------------------------------------------------------
def test_lstm_learner_registers_the_records_it_did(monkeypatch):
    """A tat-maze-lstm learner at 512 x 8: one grouped launch of 6 problems, x1 dense (ld1 == M), dW_ih / dW_hh of either player
    from the same dG, the bias slices on dW_ih's problem — DeferredWeightGrads.add's records for its LSTM callers."""
    from active_tracking_rl_amd.train import rollout
    dev = _dev()
    args, pl, opt = _player("tat-maze-lstm", n_envs=512, num_steps=8)
    rollout(pl, args.num_steps)
    spy = _Spy(monkeypatch)
    pl.optimize(None, opt, pl.model, args.train_mode, dev)
    torch.cuda.synchronize()
    assert spy.count("atr_gemm_tn_grouped") == 1 and spy.count("atr_gemm_tn") == 0
    group = spy.groups[0]
    assert len(group) == 6 and all(g["ld1"] == g["M"] for g in group)
    ptr = {p.data_ptr(): v for p, v in zip(opt.bucket.params, opt.bucket.grad_views())}
    named = dict(pl.model.named_parameters())
    for p in (0, 1):
        pre = "player%d.lstm." % p
        wih, whh = ptr[named[pre + "weight_ih"].data_ptr()], ptr[named[pre + "weight_hh"].data_ptr()]
        bih, bhh = ptr[named[pre + "bias_ih"].data_ptr()], ptr[named[pre + "bias_hh"].data_ptr()]
        a = [g for g in group if g["c"] == wih.data_ptr()]
        b = [g for g in group if g["c"] == whh.data_ptr()]
        assert len(a) == 1 and len(b) == 1 and a[0]["x1"] == b[0]["x1"]
        assert (a[0]["M"], a[0]["colsum0"], a[0]["colsum1"]) == (4 * R, bih.data_ptr(), bhh.data_ptr())
        assert (b[0]["M"], b[0]["N"], b[0]["colsum0"], b[0]["colsum1"]) == (4 * R, R, None, None)
    assert torch.isfinite(opt.bucket.flat).all()
    pl.env.close()
