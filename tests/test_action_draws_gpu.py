"""-m gpu: every action the rollout kernels draw, predicted row by row on the host (tests/draw_spec.py).

The uniform of a draw is an integer function of its key (seed; row, counter, ordinal), so the host model says which action
each row must get. Rule of every case: a row whose uniform lies outside the margin of draw_spec (float32 softmax against
float64: derived there) must carry exactly the model's action; a row inside it the model's action or the one across the
boundary it is near; at most draw_spec.CAP = 1e-3 of a case's rows may be inside; an action outside [0, A) fails. Each case
prints its rows, excluded rows and mismatches.

What the kernels were found to do, asserted below and written into include/atr_policy.h:
  * atr_sample_actions with bump != 0 draws under the counter value BEFORE its own bump (the bump is a second launch behind
    the draw); a block (ActionSampler.begin_block, or the rollout's first launch) bumps first, so everything inside a
    rollout, its bootstrap step included, draws under the value the counter holds after that rollout.
  * ordinals inside a rollout: the block's ordinals start at 1; step t draws the tracker under 2t + 1 and the target under
    2t + 2 (t = 0 .. T - 1), the learner's bootstrap step continues at 2T + 1 (tracker) / 2T + 2 (target).
  * a PipelinedIteration replica draws under its own seed, (torch.initial_seed() + 7919 (k + 1)) mod 2**64.

Rollout cases as run on an MI355X (rows = T x 2 x N actions + the bootstrap step's 2 x N, per replay; three replays each):

    case                                     counter   rows     excluded      mismatches
    tat-maze-lstm 512, synchronous graph     4, 5, 6    21 504   2,  4,  5    0, 0, 0
    maze-lstm 2048 (Adv), synchronous graph  4, 5, 6    86 016   8, 10,  9    0, 0, 0
    tat-maze-lstm 4096, synchronous graph    6, 7, 8   172 032  27, 29, 34    0, 0, 0
    tat-maze-lstm 4096, pipelined replica 0  1, 2, 3   172 032  19, 20, 20    0, 0, 0

(excluded share at most 2e-4 of a case's rows against the cap of 1e-3). The exact-logit grid, the key-wiring and distinctness
cases and the cell-kernel cases: no mismatch either, at most 4 excluded rows in 16 384. The module takes 11 s on the MI355X.
"""
import numpy as np
import pytest
import torch

import draw_spec as ds

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
M64 = 0xFFFFFFFFFFFFFFFF


def _report(label, res):
    n, excl, wrong, oor = res
    print("%-58s n %7d  excluded %4d  mismatches %d" % (label, n, excl, wrong))
    assert oor == 0, (label, "actions outside [0, A)", oor)
    assert wrong == 0, (label, "mismatches outside the margin", wrong)
    assert excl <= ds.CAP * n, (label, "excluded share above the cap", excl, n)
    return res


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _linear(w, b):
    lin = torch.nn.Linear(w.shape[1], w.shape[0]).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(_dev(w))
        lin.bias.copy_(_dev(b))
    return lin


def _sample(h, w, b, counter, seed, ordinal, bump, n=None):
    """atr_sample_actions through ctypes: every argument of the C entry point."""
    from active_tracking_rl_amd import fused
    n = h.shape[0] if n is None else n
    out = torch.full((max(h.shape[0], 1),), -7, dtype=torch.int64, device=DEV)
    rc = fused.lib().atr_sample_actions(fused._p(h), fused._p(w), fused._p(b), fused._p(out), fused._p(counter), seed & M64,
                                        ordinal, bump, n, h.shape[1], w.shape[0], fused._stream(h))
    assert rc == 0
    return out[:n].cpu().numpy()


def _counter(value=0):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def _read(counter):
    return int(counter.item()) & M64


@pytest.mark.parametrize("family", ds.EXACT_FAMILIES)
def test_sample_actions_on_exact_logits(family):
    """atr_sample_actions through fused.ActionSampler on logits that are exact in float32 in any summation order (small-integer
    rows, head on a 2**-8 grid): A x R grid at n = 4099 (the row loop's one-, two- and three-trip forms, ragged last trips) and
    the block tails n = 1 .. 300 001 at A = 4, R = 128. Only the exponential contributes to the margin."""
    from active_tracking_rl_amd import fused
    for fam, A, R, n in ds.exact_grid_cases():
        if fam != family:
            continue
        h, w, b, logits = ds.exact_case(family, A, R, n)
        seed, ctr, ordinal = ds.exact_key(family, A, R, n)
        sampler = fused.ActionSampler(torch.device(DEV), seed=seed)
        sampler.counter.fill_(ctr)
        a = sampler(_dev(h), _linear(w, b)).cpu().numpy()                  # stand-alone call: ordinal 0, bumps after the draw
        assert _read(sampler.counter) == ctr + 1
        u = ds.uniform(seed, np.arange(n), ctr, ordinal)
        _report("sample %-11s A %d R %3d" % (family, A, R), ds.check(a, logits, u, ds.delta_for(logits)))
        p = np.exp(logits - logits.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        assert (p[np.arange(n), a] > 1e-40).all(), (family, A, R, n, "an action of probability zero came out")
        if family == "plus60":
            assert (a == ds.plus60_action(A)).all(), (A, R, n)
        if family == "neg":                         # softmax is shift-invariant: the same rows 110 higher, the same key
            h2, w2, b2, l2 = ds.exact_case("neg_shifted", A, R, n)
            sampler.counter.fill_(ctr)
            a2 = sampler(_dev(h2), _linear(w2, b2)).cpu().numpy()
            assert np.array_equal(a, a2), (A, R, n, int((a != a2).sum()))


def test_sample_actions_key_wiring():
    """Both seed halves, both counter halves (a bump that carries into the high word), the ordinal, bump 0 / 1 and the
    n == 0 call that only bumps: the counter tensor is read back after every call; a bumping call draws under the value
    BEFORE its bump (and does not match the model under the value after it)."""
    A, R, n = 4, 128, 4099
    h, w, b, logits = ds.exact_case("n1", A, R, n)
    hd, wd, bd = _dev(h), _dev(w), _dev(b)
    delta = ds.delta_for(logits)
    rows = np.arange(n)
    seen = {}
    for seed in (1, 2 ** 32, 2 ** 63 + 12345):
        for c0 in (0, 2 ** 32 - 1, 2 ** 40 + 7):
            for ordinal in (0, 1, 41, 65535):
                for bump in (0, 1):
                    ctr = _counter(c0)
                    a = _sample(hd, wd, bd, ctr, seed, ordinal, bump)
                    assert _read(ctr) == c0 + bump, (seed, c0, ordinal, bump, _read(ctr))
                    label = "key seed %#x ctr %#x ord %d bump %d" % (seed, c0, ordinal, bump)
                    _report(label, ds.check(a, logits, ds.uniform(seed, rows, c0, ordinal), delta))
                    after = ds.check(a, logits, ds.uniform(seed, rows, c0 + 1, ordinal), delta)
                    assert after[2] > n // 4, (label, "also matches the counter value after the bump", after)
                    seen[(seed, c0, ordinal, bump)] = a
                assert np.array_equal(seen[(seed, c0, ordinal, 0)], seen[(seed, c0, ordinal, 1)])
    assert len({v.tobytes() for v in seen.values()}) == len(seen) // 2          # every key its own draws
    for c0 in (0, 2 ** 32 - 1, 2 ** 40 + 7):                                     # n == 0, bump = 1: only the counter moves
        ctr = _counter(c0)
        assert _sample(hd, wd, bd, ctr, 5, 0, 1, n=0).size == 0 and _read(ctr) == c0 + 1
        assert _sample(hd, wd, bd, ctr, 5, 0, 0, n=0).size == 0 and _read(ctr) == c0 + 1
    from active_tracking_rl_amd import fused
    s = fused.ActionSampler(torch.device(DEV), seed=3)
    s.counter.fill_(2 ** 32 - 1)
    s.begin_block()                                                              # bumps first: the block draws under 2**32
    assert _read(s.counter) == 2 ** 32
    lin = _linear(w, b)
    for ordinal in (1, 2):
        a = s(hd, lin).cpu().numpy()
        _report("block ordinal %d" % ordinal, ds.check(a, logits, ds.uniform(3, rows, 2 ** 32, ordinal), delta))
    s.end_block()
    assert _read(s.counter) == 2 ** 32


def test_keys_that_differ_in_one_field_draw_unrelated_actions():
    """On the device only actions are visible: under two keys that differ in one field (row, ordinal, either counter half,
    either seed half) the actions drawn from the same logits agree exactly where the model's do, outside the margins."""
    from test_action_draws_cpu import KEY_VARIANTS
    A, R, n = 4, 128, 300001
    h, w, b, logits = ds.exact_case("n1", A, R, n)
    hd, wd, bd = _dev(h), _dev(w), _dev(b)
    delta = ds.delta_for(logits)
    seed, c0, ordinal = 2 ** 33 + 5, 2 ** 34 + 11, 6
    rows = np.arange(n)
    base_u = ds.uniform(seed, rows, c0, ordinal)
    base = _sample(hd, wd, bd, _counter(c0), seed, ordinal, 0)
    _report("distinct base", ds.check(base, logits, base_u, delta))
    safe = ~ds.margin(logits, base_u, delta)
    for name, d in KEY_VARIANTS.items():
        if name == "base":
            continue
        if name == "row":           # the same logits under the neighbouring row's key: rows 1 .. n - 1 handed in as 0 .. n - 2
            a = _sample(hd[1:], wd, bd, _counter(c0), seed, ordinal, 0)
            u = ds.uniform(seed, rows[:-1], c0, ordinal)
            l, dl, ref, ok = logits[1:], delta[1:], base[1:], safe[1:]
        else:
            a = _sample(hd, wd, bd, _counter(c0 + d.get("counter", 0)), seed + d.get("seed", 0), ordinal + d.get("ordinal", 0), 0)
            u = ds.uniform(seed + d.get("seed", 0), rows, c0 + d.get("counter", 0), ordinal + d.get("ordinal", 0))
            l, dl, ref, ok = logits, delta, base, safe
        _report("distinct %s" % name, ds.check(a, l, u, dl))
        ok = ok & ~ds.margin(l, u, dl)
        model_same = ds.draw(l, u) == ds.draw(l, base_u[1:] if name == "row" else base_u)
        assert np.array_equal((a == ref)[ok], model_same[ok]), name
        share = float((a == ref).mean())
        assert 0.15 < share < 0.7, (name, share)       # independent draws from these rows agree on sum_a p_a^2 of them


def _cell_inputs(R, N, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    done = (torch.rand(N, device=DEV, generator=g) < 0.3).to(torch.uint8)
    return r(2, N, 4 * R), r(2, N, 4 * R) * 0.5, [r(4 * R) * 0.3 for _ in range(2)], r(2, N, R), done


def _predict(acc, h_out, lin, actions, ordinal):
    """Adds (rows, excluded, mismatches, out of range) of one launch's draws to acc: a case's share is taken over all its draws."""
    h = h_out.cpu().numpy()
    w, b = lin.weight.detach().cpu().numpy(), lin.bias.detach().cpu().numpy()
    logits = ds.head_logits(h, w, b)
    u = ds.uniform(ds.CELL_SEED, np.arange(h.shape[0]), ds.CELL_COUNTER, ordinal)
    acc += np.array(ds.check(actions.cpu().numpy(), logits, u, ds.delta_for(logits, h, w, b)))


@pytest.mark.parametrize("kind,R,A,N", ds.CELL_CASES)
def test_cell_kernels_draw_what_their_hidden_rows_say(kind, R, A, N):
    """atr_lstm_cell_forward_act1 / _act2 and atr_act_env_step without an env handle: the hidden rows are read back, the
    logits formed from them in float64, and actions_out predicted (player p under ordinal + p). done_prev mixed; with and
    without the tracker-action embedding. The tracker-aware target's state must be the plain cell's on ig + emb[a_tracker]."""
    from active_tracking_rl_amd import fused
    ig, hg, bias, c_prev, done = _cell_inputs(R, N, 1000 * R + 10 * A + (N & 1))
    lins = [_linear(*ds.head_family(A, R, seed=p)) for p in range(2)]
    emb = torch.randn(A, 4 * R, device=DEV) * 0.5
    sampler = fused.ActionSampler(torch.device(DEV), seed=ds.CELL_SEED)
    sampler.begin_block()
    assert _read(sampler.counter) == ds.CELL_COUNTER
    new = lambda *s: torch.empty(*s, device=DEV)
    tag = "%s R %d A %d N %d" % (kind, R, A, N)
    acc = np.zeros(4, np.int64)
    if kind == "act1":
        a_in = torch.randint(0, A, (N,), device=DEV)
        for k in (1, 2, 3, 4):
            p, use_emb = k % 2, k % 2 == 0
            h_out, c_out, acts, a_out = new(N, R), new(N, R), new(N, 4 * R), torch.full((N,), -7, dtype=torch.int64, device=DEV)
            fused.lstm_cell_act_into(ig[p].contiguous(), hg[p].contiguous(), c_prev[p].contiguous(), done if k > 1 else None,
                                     h_out, c_out, acts, sampler, lins[p], a_out, emb=emb if use_emb else None,
                                     act_in=a_in if use_emb else None, bias=bias[p])
            pre = ig[p] + bias[p] + (emb[a_in] if use_emb else 0)
            h_ref, c_ref = fused.lstm_cell(pre.contiguous(), hg[p].contiguous(), c_prev[p].contiguous(), done=done if k > 1 else None)
            torch.testing.assert_close(h_out, h_ref, rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(c_out, c_ref, rtol=1e-5, atol=1e-6)
            _predict(acc, h_out, lins[p], a_out, k)
    elif kind == "act2":
        for call in range(2):
            h_out, c_out, acts = new(2, N, R), new(2, N, R), new(2, N, 4 * R)
            a_out = torch.full((2, N), -7, dtype=torch.int64, device=DEV)
            fused.lstm_cell_act2_into(ig, hg, bias, c_prev, done if call else None, h_out, c_out, acts, sampler, lins, a_out)
            for p in range(2):
                _predict(acc, h_out[p], lins[p], a_out[p], 2 * call + 1 + p)
    else:
        for call in range(2):
            use_emb = call == 1
            h_out, c_out = new(2, N, R), new(2, N, R)
            a_out = torch.full((2, N), -7, dtype=torch.int64, device=DEV)
            fused.act_env_step(None, [ig[0], ig[1]], [hg[0], hg[1]], bias, [c_prev[0], c_prev[1]], done if call else None,
                               [h_out[0], h_out[1]], [c_out[0], c_out[1]], None, sampler, lins, a_out, emb=emb if use_emb else None)
            for p in range(2):
                _predict(acc, h_out[p], lins[p], a_out[p], 2 * call + 1 + p)
            pre = ig[1] + bias[1] + (emb[a_out[0]] if use_emb else 0)      # the target received emb[the tracker's action]
            h_ref, c_ref = fused.lstm_cell(pre.contiguous(), hg[1], c_prev[1], done=done if call else None)
            torch.testing.assert_close(h_out[1], h_ref, rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(c_out[1], c_ref, rtol=1e-5, atol=1e-6)
    sampler.end_block()
    assert _read(sampler.counter) == ds.CELL_COUNTER
    _report(tag, tuple(int(x) for x in acc))


def test_cells_at_saturation():
    """fused.lstm_cell and the act variants with pre-activations in {+-20, +-45, +-100, +-3e38} and c_prev in {0, +-50}
    (every combination of the four gates): finite, |h| <= 1, and sigmoid / tanh of float64 within the cell tests' tolerance."""
    from active_tracking_rl_amd import fused
    vals = [20.0, -20.0, 45.0, -45.0, 100.0, -100.0, 3e38, -3e38]
    cs = [0.0, 50.0, -50.0]
    grid = np.array([(i, f, g, o, c) for i in vals for f in vals for g in vals for o in vals for c in cs], np.float32)
    N, R, A = len(grid), 128, 4
    ig = _dev(np.repeat(grid[:, :4], R, axis=1))                       # [N, 4R]: gate blocks i, f, g, o
    c_prev = _dev(np.repeat(grid[:, 4:5], R, axis=1))
    zero = torch.zeros(N, 4 * R, device=DEV)
    g64 = torch.from_numpy(grid.astype(np.float64))
    c_ref = torch.sigmoid(g64[:, 1]) * g64[:, 4] + torch.sigmoid(g64[:, 0]) * torch.tanh(g64[:, 2])
    h_ref = torch.sigmoid(g64[:, 3]) * torch.tanh(c_ref)

    def ok(label, h, c):
        h, c = h.double().cpu(), c.double().cpu()
        assert torch.isfinite(h).all() and torch.isfinite(c).all(), label
        assert float(h.abs().max()) <= 1.0, (label, float(h.abs().max()))
        torch.testing.assert_close(h, h_ref[:, None].expand(N, R), rtol=1e-4, atol=2e-5, msg=lambda m: label + ": h " + m)
        torch.testing.assert_close(c, c_ref[:, None].expand(N, R), rtol=1e-4, atol=2e-5, msg=lambda m: label + ": c " + m)

    ok("lstm_cell", *fused.lstm_cell(ig, zero, c_prev))
    lins = [_linear(*ds.head_family(A, R, seed=p)) for p in range(2)]
    sampler = fused.ActionSampler(torch.device(DEV), seed=ds.CELL_SEED)
    sampler.begin_block()
    acc = np.zeros(4, np.int64)
    zb = torch.zeros(4 * R, device=DEV)
    new = lambda *s: torch.empty(*s, device=DEV)
    h_out, c_out, a_out = new(N, R), new(N, R), torch.full((N,), -7, dtype=torch.int64, device=DEV)
    fused.lstm_cell_act_into(ig, zero, c_prev, None, h_out, c_out, None, sampler, lins[0], a_out, bias=zb)
    ok("act1", h_out, c_out)
    _predict(acc, h_out, lins[0], a_out, 1)
    ig2, hg2, c2 = torch.stack([ig, ig]), torch.stack([zero, zero]), torch.stack([c_prev, c_prev])
    h2, c2o, acts2, a2 = new(2, N, R), new(2, N, R), new(2, N, 4 * R), torch.full((2, N), -7, dtype=torch.int64, device=DEV)
    fused.lstm_cell_act2_into(ig2, hg2, [zb, zb], c2, None, h2, c2o, acts2, sampler, lins, a2)
    for p in range(2):
        ok("act2 player %d" % p, h2[p], c2o[p])
        _predict(acc, h2[p], lins[p], a2[p], 2 + p)
    h3, c3, a3 = new(2, N, R), new(2, N, R), torch.full((2, N), -7, dtype=torch.int64, device=DEV)
    fused.act_env_step(None, [ig, ig], [zero, zero], [zb, zb], [c_prev, c_prev], None, [h3[0], h3[1]], [c3[0], c3[1]], None,
                       sampler, lins, a3)
    for p in range(2):
        ok("act_env_step player %d" % p, h3[p], c3[p])
        _predict(acc, h3[p], lins[p], a3[p], 4 + p)
    sampler.end_block()
    _report("saturated cells", tuple(int(x) for x in acc))


# ---- the timed region's own rollouts ------------------------------------------------------------------------------------


def _check_rollout(label, agent, seed_expected=None):
    """Every action of the rollout `agent` just replayed (and of its learner's bootstrap step), predicted from the stored
    hidden rows, the actor heads, and the key (sampler.seed; env, sampler.counter, ordinal)."""
    m, cache = agent.model, agent._cache
    s = m._sampler
    ctr, seed = _read(s.counter), s.seed
    if seed_expected is not None:
        assert seed == seed_expected
    T, N = cache.T, cache.N
    acts = agent._actions_buf.cpu().numpy()                       # [T, 2, N]
    assert acts.shape == (T, 2, N)
    h_all = cache.h_all[:, 1:].cpu().numpy()                      # [2, T, N, R]: the fresh row of every step
    heads = [(p.actor.actor_linear.weight.detach().cpu().numpy(), p.actor.actor_linear.bias.detach().cpu().numpy())
             for p in (m.player0, m.player1)]
    rows = np.arange(N)
    tot = np.zeros(4, np.int64)

    def one(h, a, p, ordinal):
        w, b = heads[p]
        logits = ds.head_logits(h, w, b)
        tot[:] += ds.check(a, logits, ds.uniform(seed, rows, ctr, ordinal), ds.delta_for(logits, h, w, b))

    for t in range(T):
        for p in range(2):
            one(h_all[p, t], acts[t, p], p, 2 * t + 1 + p)
    boot = getattr(cache, "boot", None)
    assert boot is not None and boot.actions is not None, "the bootstrap step ran with the rollout's kernels"
    bh, ba = boot.h.cpu().numpy(), boot.actions.cpu().numpy()
    for p in range(2):
        one(bh[p], ba[p], p, 2 * T + 1 + p)
    _report("%s counter %d" % (label, ctr), tuple(int(x) for x in tot))
    return ctr, acts.copy(), tuple(int(x) for x in tot)


def _replays(label, replay, agent, seed_expected=None):
    """Three replays of a captured rollout + learner without the update: the counter advances by exactly one each, the
    replays differ from each other and each matches the model under its own counter value."""
    seen = []
    for k in range(3):
        before = _read(agent.model._sampler.counter)
        replay()
        torch.cuda.synchronize()
        ctr, acts, _ = _check_rollout("%s replay %d" % (label, k), agent, seed_expected)
        assert ctr == before + 1, (label, k, before, ctr)
        seen.append(acts)
    assert not any(np.array_equal(seen[i], seen[j]) for i in range(3) for j in range(i))


@pytest.mark.parametrize("env_id,n,network,aux", [("Track2D-BlockPartialPZR-v0", 512, "tat-maze-lstm", "reward"),
                                                  ("Track2D-BlockPartialAdv-v0", 2048, "maze-lstm", "none")])
def test_rollout_graph_replays_draw_what_the_model_predicts(env_id, n, network, aux):
    """GraphedIteration at 512 envs (pair kernels) and 2048 envs of Adv / maze-lstm, 20 steps, u8 observations."""
    from test_learner_f64_gpu import _make
    from active_tracking_rl_amd.train import GraphedIteration
    player, opt, args = _make(env_id, n, network, aux, -1)
    try:
        it = GraphedIteration(player, opt, args, mode=-1, keep_warmup_updates=True)
        it.run(-1)
        _replays("%s %d" % (network, n), it.g_rolls[-1].replay, player)
    finally:
        player.env.close()


def test_headline_rollout_and_pipelined_replica_draw_what_the_model_predicts():
    """4096 envs of Track2D-BlockPartialPZR-v0 / tat-maze-lstm (one-GEMM path: k_act_step with an env handle): the synchronous
    graph on the master, then replica 0 of a serial PipelinedIteration, which draws under a seed of its own."""
    from test_learner_f64_gpu import _make
    from active_tracking_rl_amd.train import GraphedIteration, PipelinedIteration
    player, opt, args = _make("Track2D-BlockPartialPZR-v0", 4096, "tat-maze-lstm", "reward", -1)
    try:
        it_p = PipelinedIteration(player, opt, args, mode=-1, serial=True)     # (first: it warms up eagerly on the master)
        it = GraphedIteration(player, opt, args, mode=-1, keep_warmup_updates=True)
        it.run(-1)
        assert player._cache.fh_all is not None
        _replays("tat-maze-lstm 4096", it.g_rolls[-1].replay, player)
        rep = it_p.players[0]
        g_r, g_l, _ = it_p.graphs[(-1, 0)]
        want = (int(torch.initial_seed()) + 7919) & M64
        assert rep.model._sampler.seed == want != player.model._sampler.seed

        def replay():
            g_r.replay()
            g_l.replay()
        _replays("tat-maze-lstm 4096 pipelined replica 0", replay, rep, seed_expected=want)
    finally:
        player.env.close()
