"""-m gpu: the GRU cores' opt-in fused rollout step, cache and graphed evaluation (--fused-gru; include/atr_gru_step.h,
csrc/track2d_hip.hip k_gru_step, model._new_cache_gru, fused.gru_sequence_cached).

  1 single launches (draw and greedy; the policy half without an env) against the float64 spec, the draw / argmax host models, the
    oracle and the accounts;
  2 the cached rollout's learner against forward_sequence (the path without a cache) on the same stored rollout, its bootstrap
    values against model(), the loss's gradients at the configured gamma;
  3 `need` per player; 4 both graphed schedules; 5 the evaluator; 6 the fallbacks; 7 the drivers."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import draw_spec as ds
import greedy_eval_spec as gs
import gru_fused_spec as spec
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENV = "Track2D-BlockPartialPZR-v0"
NETS = ["tat-maze-gru", "maze-gru"]
R, F, A = spec.R, spec.F, spec.A


def _dev():
    return torch.device(DEV)


def _handle(env_id, n, seed=5, base=77):
    from active_tracking_rl_amd.vec_env import VecTrack2D
    env = VecTrack2D(env_id, num_envs=n, device=DEV, seed=seed, env_id_base=base)
    return env, env.reset().to(torch.uint8)


@pytest.mark.parametrize("env_id", spec.ENV_IDS)
@pytest.mark.parametrize("n", [33, 64])
@pytest.mark.parametrize("tat", [True, False])
def test_gru_step_against_the_spec_the_action_models_and_the_oracle(env_id, n, tat):
    """1. Three chained env steps per form (draw: atr_gru_act_env_step, greedy: atr_gru_eval_act_env_step), each on a handle and
    an oracle of its own; inputs from gru_fused_spec.launch_case (masked rows with zero rows, read at row stride F + R; non-zero
    b_hn), outputs pre-filled with NaN. h_out and (r, z, n, q) against the float64 spec fed the same g and, for the target, the
    kernel's own tracker action; the actions against the draw model / the first maximum of float64 logits from the kernel's own
    h_out on every clear row (at least 0.9 of the rows); obs / rew / done against the oracle stepped with the kernel's actions,
    hm_out = (done == 0) * h_out and the greedy accounts = evaluator.account, all bit for bit."""
    from active_tracking_rl_amd import evaluator, fused
    case = spec.launch_case(n, tat)
    lins = []
    for p in range(2):
        lin = torch.nn.Linear(R, A).to(DEV)
        with torch.no_grad():
            lin.weight.copy_(case["w"][p])
            lin.bias.copy_(case["b"][p])
        lins.append(lin)
    b4 = [b.to(DEV) for b in case["b4"]]
    e4 = case["e4"].to(DEV) if tat else None
    new = lambda *s: torch.full(s, float("nan"), device=DEV)
    for kind in ("draw", "greedy"):
        env, first = _handle(env_id, n)
        oracle = gs.oracle_batch(env_id, n, seed=5, base=77)
        assert np.array_equal(first.cpu().numpy(), oracle.reset())
        sampler = fused.ActionSampler(_dev(), seed=spec.SEED)
        sampler.begin_block()
        torch.cuda.synchronize()
        counter = int(sampler.counter.item())
        rsum = torch.zeros((n, 2), device=DEV)
        length = torch.zeros(n, dtype=torch.int32, device=DEV)
        alive = torch.ones(n, dtype=torch.uint8, device=DEV)
        rews, dones = [], []
        for t in range(spec.T):
            g = case["g"][t].to(DEV).contiguous()
            rows_in, rows_out = new(2, n, F + R), new(2, n, F + R)
            rows_in[:, :, F:] = case["hp"][t].to(DEV)
            h_out, acts_out = new(2, n, R), new(2, n, 4 * R)
            actions = torch.full((2, n), -7, dtype=torch.int64, device=DEV)
            bufs = (torch.zeros((n, 2, 13, 13), dtype=torch.uint8, device=DEV), torch.zeros((n, 2), device=DEV),
                    torch.zeros(n, dtype=torch.uint8, device=DEV))
            ordinal = sampler._ordinal + 1
            fused.gru_act_env_step(env, [g[0], g[1]], b4, [rows_in[0][:, F:], rows_in[1][:, F:]], [h_out[0], h_out[1]],
                                   [acts_out[0], acts_out[1]], sampler, lins, actions, emb=e4, env_out=bufs,
                                   hm_out=[rows_out[0][:, F:], rows_out[1][:, F:]], greedy=kind == "greedy",
                                   eval_out=(rsum, length, alive) if kind == "greedy" else None)
            torch.cuda.synchronize()
            a_k, h_k = actions.cpu().numpy(), h_out.cpu().numpy()
            assert a_k.min() >= 0 and a_k.max() < A
            assert torch.isnan(rows_out[:, :, :F]).all() and torch.isnan(rows_in[:, :, :F]).all()    # only the h columns are touched
            model = spec.step_model(case, t, kind, a_tracker=a_k[0], h=h_k, counter=counter, ordinal=ordinal)
            for p, (h64, acts64, logits, clear, act) in enumerate(model):
                np.testing.assert_allclose(h_k[p], h64, err_msg="h_out %s t%d p%d" % (kind, t, p), **spec.CELL_TOL)
                np.testing.assert_allclose(acts_out[p].cpu().numpy(), acts64, err_msg="acts %s t%d p%d" % (kind, t, p),
                                           **spec.CELL_TOL)
                print("%s t%d p%d: clear rows %d of %d, max|h - spec| %.2e" % (kind, t, p, clear.sum(), n, np.abs(h_k[p] - h64).max()))
                assert clear.mean() >= 0.9
                assert np.array_equal(a_k[p][clear], act[clear]), (kind, t, p)
            wo, wr, wd = oracle.step(np.ascontiguousarray(a_k.T))
            done = bufs[2].cpu().numpy()
            assert np.array_equal(bufs[0].cpu().numpy(), wo) and np.array_equal(bufs[1].cpu().numpy(), wr.astype(np.float32))
            assert np.array_equal(done, wd)
            keep = (done == 0).astype(np.float32)[None, :, None]
            assert np.array_equal(rows_out[:, :, F:].cpu().numpy(), keep * h_k)
            if kind == "greedy":
                rews.append(bufs[1].cpu().numpy())
                dones.append(done)
                w_rsum, w_len, w_alive = evaluator.account(np.stack(rews), np.stack(dones))
                assert np.array_equal(rsum.cpu().numpy(), w_rsum) and np.array_equal(length.cpu().numpy(), w_len)
                assert np.array_equal(alive.cpu().numpy(), w_alive)
        sampler.end_block()
        assert env.faults() == 0
        env.close()


@pytest.mark.parametrize("n", [33, 64])
@pytest.mark.parametrize("tat", [True, False])
def test_gru_step_without_an_env_against_the_spec(n, tat):
    """1. The policy half alone (atr_gru_act_env_step with env == NULL: the learner's bootstrap step, the ENV = false
    instantiations of k_gru_step), one launch per step of the case: no env handle, no env_out, no hm_out. h_out and (r, z, n, q)
    against the float64 spec fed the same g and, for the target, the kernel's own tracker action; the drawn actions against the
    draw model on every clear row (at least 0.9 of the rows); the input rows are left as they were."""
    from active_tracking_rl_amd import fused
    case = spec.launch_case(n, tat)
    lins = []
    for p in range(2):
        lin = torch.nn.Linear(R, A).to(DEV)
        with torch.no_grad():
            lin.weight.copy_(case["w"][p])
            lin.bias.copy_(case["b"][p])
        lins.append(lin)
    b4 = [b.to(DEV) for b in case["b4"]]
    e4 = case["e4"].to(DEV) if tat else None
    new = lambda *s: torch.full(s, float("nan"), device=DEV)
    sampler = fused.ActionSampler(_dev(), seed=spec.SEED)
    sampler.begin_block()
    torch.cuda.synchronize()
    counter = int(sampler.counter.item())
    for t in range(spec.T):
        g = case["g"][t].to(DEV).contiguous()
        rows_in = new(2, n, F + R)
        rows_in[:, :, F:] = case["hp"][t].to(DEV)
        before = rows_in.clone()
        h_out, acts_out = new(2, n, R), new(2, n, 4 * R)
        actions = torch.full((2, n), -7, dtype=torch.int64, device=DEV)
        ordinal = sampler._ordinal + 1
        fused.gru_act_env_step(None, [g[0], g[1]], b4, [rows_in[0][:, F:], rows_in[1][:, F:]], [h_out[0], h_out[1]],
                               [acts_out[0], acts_out[1]], sampler, lins, actions, emb=e4)
        torch.cuda.synchronize()
        a_k, h_k = actions.cpu().numpy(), h_out.cpu().numpy()
        assert a_k.min() >= 0 and a_k.max() < A
        assert torch.equal(torch.nan_to_num(rows_in, nan=-1.0), torch.nan_to_num(before, nan=-1.0))
        model = spec.step_model(case, t, "draw", a_tracker=a_k[0], h=h_k, counter=counter, ordinal=ordinal)
        for p, (h64, acts64, logits, clear, act) in enumerate(model):
            np.testing.assert_allclose(h_k[p], h64, err_msg="h_out t%d p%d" % (t, p), **spec.CELL_TOL)
            np.testing.assert_allclose(acts_out[p].cpu().numpy(), acts64, err_msg="acts t%d p%d" % (t, p), **spec.CELL_TOL)
            print("no env t%d p%d: clear rows %d of %d, max|h - spec| %.2e" % (t, p, clear.sum(), n, np.abs(h_k[p] - h64).max()))
            assert clear.mean() >= 0.9
            assert np.array_equal(a_k[p][clear], act[clear]), (t, p)
    sampler.end_block()


def _player(net, n_envs=64, num_steps=3, seed=23, fused_gru=True, **kw):
    from active_tracking_rl_amd.train import default_args, make_player
    args = default_args(env=kw.pop("env", ENV), network=net, aux="reward" if "tat" in net else "none", num_envs=n_envs,
                        num_steps=num_steps, seed=seed, fused_gru=fused_gru, **kw)
    args.gpu_ids = [0]
    player, opt = make_player(args, _dev())
    return args, player, opt


def _stored(player, T):
    states = player._buf[0][:T].unsqueeze(3).unsqueeze(4)
    return states, player._actions_buf.transpose(1, 2), player._keep


def _rolled(net, warm=5, **kw):
    """A fused-GRU Agent after `warm` rollouts (so that h0 is not zero and some episodes may have ended) plus the one under test."""
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


def _loss_grads(player, mode, params):
    out = player.loss_recompute(mode)[0]
    terms = list(out) if isinstance(out, (tuple, list)) else [out]
    return torch.autograd.grad(terms, params, grad_outputs=[torch.ones_like(t) for t in terms], allow_unused=True)


@contextlib.contextmanager
def _tracker_draws(model, a0):
    """model() with the tracker's drawn action replaced by a0 [N] (tat only: nothing else in the bootstrap forward depends on a
    draw). The cached path draws the bootstrap step's tracker action with the rollout's Philox stream, model() with torch's
    generator; the tracker-aware target's value depends on that action, so the reference is fed the one the kernel recorded."""
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


def _grads_with_and_without_the_cache(pl, mode, params):
    """Every gradient of the Agent's loss over the stored rollout, at the configured gamma and tau: with the cache (the fused
    heads, boot_values on the GRU cache, gru_sequence_cached) and with the cache hidden from the Agent (forward_sequence from h0 and
    model() for the bootstrap value: the path without a cache). Returns (with, without, the cached path's V(s_T) [N, 2, 1], the
    tracker action its bootstrap step recorded [N])."""
    m = pl.model
    assert pl.args.gamma > 0 and pl.args.tau > 0
    seen = []
    real = m.boot_values

    def boot(states, cache, done, v_out):
        out = real(states, cache, done, v_out)
        seen.append((v_out.clone(), cache.boot.actions[0].clone()))
        return out
    m.boot_values = boot
    try:
        g_new = _loss_grads(pl, mode, params)
    finally:
        del m.boot_values
    assert len(seen) == 1                    # the bootstrap value came from boot_values, once
    v_boot, a0 = seen[0]
    cache, pl._cache = pl._cache, None
    try:
        with _tracker_draws(m, a0):
            g_ref = _loss_grads(pl, mode, params)
    finally:
        pl._cache = cache
    return g_new, g_ref, v_boot, a0


@pytest.mark.parametrize("net", NETS)
def test_cached_rollout_against_the_uncached_learner(net):
    """2. The numeric reference is forward_sequence — the path without a cache — on the FUSED Agent's own model and stored
    rollout (states, actions, h0, keep), compared with forward_sequence_cached; then every parameter gradient of the Agent's loss
    over that rollout at the configured gamma, with the cache and with the cache hidden from it. A second Agent of the same
    architecture on an identically seeded shard with the switch off only shows that no cache exists there (a model of its own:
    the switch is read when the model is built). The bootstrap value V(s_T) of boot_values (one more k_gru_step launch from slot
    T without the env, then the critic heads) is compared with model() on the same state, the Agent's published hxs and, for the
    tracker-aware target, the tracker action that launch recorded."""
    from active_tracking_rl_amd.train import rollout
    T = 3
    args_off, off, _ = _player(net, fused_gru=False)
    rollout(off, T)
    assert off._cache is None and off.model.cacheable_core is False and off.model.env_step_fused_seen is False
    off.env.close()
    args, pl, _ = _rolled(net)
    m = pl.model
    assert m.cacheable_core is True and pl._cache is not None and pl._cache.gru and m.env_step_fused_seen
    assert pl._cache.hm_written == T and float(pl._cache.c_all.abs().max()) == 0.0 and float(pl.cxs.abs().max()) == 0.0
    assert float(pl.h0.abs().max()) > 0.0
    states, actions, keep = _stored(pl, T)
    print("%s: %d done flags in the rollout under test" % (net, int((keep == 0).sum())))
    with torch.no_grad():
        ref = m.forward_sequence(states, actions, pl.h0, pl.c0, keep)
        got = m.forward_sequence_cached(pl._cache, states, actions, keep)
    for name, a, b in zip(("values", "entropies", "log_probs"), got[:3], ref[:3]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=2e-5, msg=lambda s, name=name: name + ": " + s)
    if m.tat:
        torch.testing.assert_close(got[3], ref[3], rtol=1e-4, atol=2e-5)
    names, params = zip(*m.named_parameters())
    g_new, g_ref, v_boot, a0 = _grads_with_and_without_the_cache(pl, -1, params)
    with torch.no_grad(), _tracker_draws(m, a0):
        v_ref = m((pl.state, (pl.hxs, pl.cxs)))[0]
    print("%s: max|V(s_T)| %.3e, max|V(s_T) - model()| %.2e" % (net, float(v_ref.abs().max()), float((v_boot - v_ref).abs().max())))
    torch.testing.assert_close(v_boot, v_ref, rtol=1e-4, atol=2e-5, msg=lambda s: "bootstrap values: " + s)
    worst = 0.0
    for name, a, b in zip(names, g_new, g_ref):
        assert (a is None) == (b is None), name
        if b is None:
            continue
        scale = float(b.abs().max())
        ratio = float((a - b).abs().max()) / scale if scale > 0 else float(a.abs().max())
        print("%-40s max|ref| %.3e  err / max|ref| %.2e" % (name, scale, ratio))
        worst = max(worst, ratio)
        assert torch.isfinite(a).all() and ratio <= 2e-4, name
    assert float(pl.cxs.abs().max()) == 0.0
    pl.env.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_need_per_player(mode):
    """3. train-modes 0 / 1: the untrained player's parameters get None or zero gradients, the other's match the path without
    a cache (configured gamma; the reference is fed the bootstrap step's tracker action, as above)."""
    args, pl, _ = _rolled("tat-maze-gru", warm=2)
    names, params = zip(*pl.model.named_parameters())
    g_new, g_ref, _, _ = _grads_with_and_without_the_cache(pl, mode, params)
    trained = "player%d." % mode
    seen = 0
    for name, a, b in zip(names, g_new, g_ref):
        if not name.startswith(trained):
            assert a is None or float(a.abs().max()) == 0.0, name
            continue
        if b is None:
            assert a is None or float(a.abs().max()) == 0.0, name
            continue
        scale = float(b.abs().max())
        assert a is not None and float((a - b).abs().max()) <= 2e-4 * scale, name
        seen += 1
    assert seen >= 8
    pl.env.close()


@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("schedule", ("synchronous", "pipelined"))
def test_graphed_schedules_train_with_the_switch_on(net, schedule):
    """4. 64 envs, 3 iterations: finite weights that change, the env step ran inside k_gru_step, cx stays zero."""
    from active_tracking_rl_amd.train import GraphedIteration, PipelinedIteration
    args, player, opt = _player(net, num_steps=5)
    w0 = opt.bucket.flat.clone()
    it = GraphedIteration(player, opt, args) if schedule == "synchronous" else PipelinedIteration(player, opt, args)
    agents = [player] if schedule == "synchronous" else it.players
    for i in range(3):
        it.run()
        if schedule == "pipelined":
            it.sync()
    it.finish()
    torch.cuda.synchronize()
    assert torch.isfinite(opt.bucket.flat).all() and not torch.equal(opt.bucket.flat, w0)
    assert player.model.env_step_fused_seen is True
    assert all(a._cache is not None and a._cache.gru for a in agents)
    assert float(it.carry["cxs"].abs().max()) == 0.0 and float(it.carry["hxs"].abs().max()) > 0.0
    assert torch.isfinite(it.carry["hxs"]).all() and player.env.core.faults() == 0
    player.env.close()


@pytest.mark.parametrize("net", NETS)
def test_eager_iteration_and_graph_replay_agree_with_the_switch_on(net):
    """4. One eager iteration and one GraphedIteration replay from identical weights, env shard, seed and draw-stream position
    leave the same weights behind (torch.equal): the captured graph holds the launches the eager iteration issues."""
    from active_tracking_rl_amd.train import GraphedIteration, rolled_back, rollout, update_tensors
    dev = _dev()
    args, pa, oa = _player(net, num_steps=5)
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
    args, pb, ob = _player(net, num_steps=5)
    it = GraphedIteration(pb, ob, args)
    it.run()
    it.finish()
    torch.cuda.synchronize()
    assert torch.isfinite(w_eager).all() and torch.equal(ob.bucket.flat, w_eager)
    pb.env.close()


def test_evaluator_round_with_the_switch_on_and_the_eager_round_without(caplog):
    """5. Switch on: evaluator.supported, and one recorded 16-episode graphed round on the Nav id equals the oracle stepped
    with the recorded actions; its accounts equal the host model. Switch off: the eager round with the one warning line."""
    import logging
    from active_tracking_rl_amd import evaluator
    from active_tracking_rl_amd.evaluator import GreedyEvaluator
    from active_tracking_rl_amd.test import evaluate
    env_id, episodes = "Track2D-BlockPartialNav-v0", 16
    args = gs.fixture_args(env_id, episodes, network="tat-maze-gru", fused_gru=True)
    model = gs.fixture_model(args, DEV)
    assert model.fused_gru_step and model.cacheable_core is True
    ev = GreedyEvaluator(model, env_id, args, _dev(), episodes, record=True)
    assert evaluator.supported(ev.env, model) is True
    rsum, length = ev.run()
    rec = ev.record
    steps = rec["actions"].shape[0]
    oracle = gs.oracle_batch(env_id, episodes, seed=args.seed)
    assert np.array_equal(rec["obs"][0], oracle.reset())
    for t in range(steps):
        wo, wr, wd = oracle.step(np.ascontiguousarray(rec["actions"][t].T))
        assert np.array_equal(rec["obs"][t + 1], wo) and np.array_equal(rec["rew"][t], wr.astype(np.float32)), t
        assert np.array_equal(rec["done"][t], wd), t
    w_rsum, w_len, w_alive = evaluator.account(rec["rew"], rec["done"])
    assert np.array_equal(rec["rsum"], w_rsum) and np.array_equal(rec["length"], w_len) and np.array_equal(rec["alive"], w_alive)
    assert np.array_equal(rsum, w_rsum[:episodes]) and np.array_equal(length, w_len[:episodes]) and not rec["alive"].any()
    assert float(np.abs(rec["c"]).max()) == 0.0 and model.training
    args_off = gs.fixture_args(env_id, episodes, network="tat-maze-gru")
    off = gs.fixture_model(args_off, DEV)
    assert off.fused_gru_step is False
    with caplog.at_level(logging.WARNING):
        r2, l2 = evaluate(off, env_id, args_off, _dev(), episodes, graphed=True)
    assert r2.shape == (episodes, 2) and (l2 >= 1).all()
    assert sum("falls back to the eager round" in r.getMessage() for r in caplog.records) == 1


@pytest.mark.parametrize("kw", [dict(env="Track2D-BlockPartialRPF-v0"), dict(stack_frames=2)], ids=["rpf", "stack2"])
def test_fallbacks_take_the_uncached_path(kw):
    """6. Switch on, but the env steps on its own: no cache, today's rollout, and one iteration trains."""
    from active_tracking_rl_amd.train import rollout
    dev = _dev()
    args, pl, opt = _player("tat-maze-gru", **kw)
    w0 = opt.bucket.flat.clone()
    rollout(pl, args.num_steps)
    assert pl.model.fused_gru_step and pl._cache is None and pl.model.env_step_fused_seen is False
    pl.optimize(None, opt, pl.model, args.train_mode, dev)
    torch.cuda.synchronize()
    assert torch.isfinite(opt.bucket.flat).all() and not torch.equal(opt.bucket.flat, w0)
    assert float(pl.cxs.abs().max()) == 0.0
    pl.env.close()


def test_lstm_step_launches_the_same_entry_with_or_without_the_switch(monkeypatch):
    """6. An LSTM model's step ends in atr_act_env_step whether or not the switch is set, and never in the GRU entry."""
    from active_tracking_rl_amd import fused
    from active_tracking_rl_amd.train import rollout
    L = fused.lib()
    for flag in (False, True):
        calls = []
        real_lstm, real_gru = L.atr_act_env_step, L.atr_gru_act_env_step
        monkeypatch.setattr(L, "atr_act_env_step", lambda *a, **k: (calls.append("atr_act_env_step"), real_lstm(*a, **k))[1])
        monkeypatch.setattr(L, "atr_gru_act_env_step", lambda *a, **k: (calls.append("atr_gru_act_env_step"), real_gru(*a, **k))[1])
        args, pl, _ = _player("tat-maze-lstm", fused_gru=flag)
        rollout(pl, args.num_steps)
        torch.cuda.synchronize()
        monkeypatch.undo()
        assert pl.model.fused_gru_step is flag and pl._cache is not None and not getattr(pl._cache, "gru", False)
        assert calls == ["atr_act_env_step"] * args.num_steps
        pl.env.close()


def test_drivers_with_the_switch(tmp_path):
    """7. main.py --network tat-maze-gru --fused-gru --graphed-eval in a fresh child process writes its checkpoint;
    gym_eval.py --fused-gru loads it."""
    d = str(tmp_path) + "/"
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--network", "tat-maze-gru", "--fused-gru", "--graphed-eval",
                        "--num-envs", "64", "--max-step", "3", "--test-eps", "4", "--log-dir", d, "--split"],
                       capture_output=True, text=True, cwd=ROOT, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "falls back" not in r.stderr
    found = [dp for dp, _, files in os.walk(d) if "tracker-best.dat" in files and "target-best.dat" in files]
    assert len(found) == 1, found          # (main.py logs under <log-dir>/<env>/<date>)
    d = found[0] + "/"
    csv_path = os.path.join(d, "eval.csv")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gym_eval.py"), "--network", "tat-maze-gru", "--fused-gru", "--graphed-eval",
                        "--env", "Track2D-BlockPartialNav-v0", "--num-episodes", "4", "--load-tracker",
                        os.path.join(d, "tracker-best.dat"), "--load-target", os.path.join(d, "target-best.dat"), "--log-dir", d,
                        "--csv", csv_path], capture_output=True, text=True, cwd=ROOT, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "falls back" not in r.stderr
    rows = open(csv_path).read().strip().splitlines()
    assert rows[0].startswith("Env,Seed,R_mean") and rows[1].startswith("Track2D-BlockPartialNav-v0,1,")
