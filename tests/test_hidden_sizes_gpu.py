"""-m gpu: the learner's kernels at hidden sizes other than 128 (--rnn-out), held to float64 by the rule of
tests/test_learner_f64_gpu.py (tests/f64_rule.py: e(hip) <= max(4 e(aten32), 1e-6), e(aten32) <= 1e-4).

  * the heads kernels (csrc/heads_hip.hip: heads_values, heads_values2, heads_loss, heads_loss_pair) at R = 64 / 128 / 256,
    i.e. 16 / 32 / 64 lanes per row (no / one / two cross-row shuffles; 16 / 8 / 4 row slots per workgroup), 4 and 8
    actions, with and without the aux head, at 5 rows and at 2 * 512 * slots + 3 rows (R = 256 also at 2 x 2050) (the 512-workgroup cap reached, every
    slot runs the grid-stride loop at least twice and consumes its prefetched row, the last pass ragged); heads_loss_pair
    reads its actions in place from a [T, 2, N] store and writes value columns 0 and 1;
  * rollout_begin / rollout_end at R = 64 / 256 (they branch on R & 3 only), exactly;
  * the sizes the kernels do not take (model.hidden_size_support): R = 96 has no heads kernel and learns through the
    tensor heads (tests/test_learner_f64_gpu.py runs it end to end), R = 512 has no action draw and is refused when the
    model is built.
The LSTM / GRU recurrences at these sizes are in tests/test_fused_stem_gpu.py and tests/test_gru_gpu.py.

Measured on MI355X, ranges over the 28 heads cases (both players, one-player and two-player launches: the same figures):
  values, values2        e(hip) 5.5e-08 .. 1.8e-07   e(aten32) 1.1e-07 .. 7.7e-07   e(hip) / allowed <= 0.14
  objective              e(hip) 1.2e-10 .. 1.8e-06   e(aten32) 1.2e-10 .. 4.8e-06   e(hip) / allowed <= 0.44
  policy statistic       e(hip) 7.6e-09 .. 2.6e-06   e(aten32) 3.4e-09 .. 2.5e-06   e(hip) / allowed <= 0.39
  value, entropy, |aux|  e(hip) 0       .. 3.5e-07   e(aten32) 0       .. 1.6e-07   e(hip) / allowed <= 0.35
  dL/dh                  e(hip) 6.0e-08 .. 9.2e-08   e(aten32) 5.9e-08 .. 1.3e-07   e(hip) / allowed <= 0.09
  dW actor, critic, aux  e(hip) 3.5e-08 .. 2.0e-07   e(aten32) 3.5e-08 .. 1.2e-06   e(hip) / allowed <= 0.11
  db actor, aux          e(hip) 0       .. 3.0e-07   e(aten32) 0       .. 3.6e-07   e(hip) / allowed <= 0.29
  db critic              e(hip) 3.8e-09 .. 8.5e-07   e(aten32) 3.8e-09 .. 2.4e-06   e(hip) / allowed <= 0.71
  heads_values, 16387 rows at R = 256: e(hip) 8.5e-08, e(aten32) 2.9e-07
(the largest figures of the scalars belong to the 5-row cases, where a sum of five signed terms cancels.)
That these cases bite: with heads_hip.hip's `if (L > 16)` shuffle made unconditional in a scratch build, all eight R = 64 cases
fail (a 16-lane row then adds its neighbour's partial sums) and the R = 128 / 256 cases pass.
"""
import pytest
import torch
import torch.nn.functional as F

from f64_rule import Table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rows_split(rows):
    """rows = T * N with the smallest T > 1 that divides it (a prime row count: T = rows, N = 1)."""
    for t in range(2, 64):
        if rows % t == 0:
            return t, rows // t
    return rows, 1


def _heads_reference(h, prm, actions, ret, gae, rew, scale, scale_aux, w_ent, dtype):
    """One player's heads and loss terms as tests/test_fused_stem_gpu.py::test_heads_loss_matches_autograd_in_float64 writes
    them, in `dtype` with autograd: -> dict(values, objective, stats [4], grads [dh, dWa, dba, dWc, dbc (, dWaux, dbaux)])."""
    hd = h.detach().to(dtype).requires_grad_(True)
    P = [p.detach().to(dtype).requires_grad_(True) for p in prm]
    logits = hd @ P[0].t() + P[1]
    v = (hd @ P[2].t() + P[3]).reshape(-1)
    logp = torch.log_softmax(logits, 1)
    prob = logp.exp()
    ent = -(logp * prob).sum(1)
    lpa = logp.gather(1, actions.view(-1, 1)).reshape(-1)
    R_, G_ = ret.to(dtype).reshape(-1), gae.to(dtype).reshape(-1)
    pol = (-lpa * G_ - w_ent * ent).sum()
    vl = (0.5 * (R_ - v) ** 2).sum()
    obj = scale * (pol + 0.5 * vl)
    aux_sum = torch.zeros((), dtype=dtype, device=h.device)
    if len(P) > 4:
        pred = (hd @ P[4].t() + P[5]).reshape(-1)
        aux_sum = (pred - rew.to(dtype).reshape(-1)).abs().sum()
        obj = obj + scale_aux * aux_sum
    grads = torch.autograd.grad(obj, [hd] + P)
    return dict(values=v.detach(), objective=obj.detach(), stats=torch.stack([pol, vl, ent.sum(), aux_sum]).detach(),
                grads=[g.detach() for g in grads])


GRAD_NAMES = ("dL/dh", "dW_actor", "db_actor", "dW_critic", "db_critic", "dW_aux", "db_aux")
STAT_NAMES = ("policy", "value", "entropy", "aux")
# 5 rows, and 2 * 512 * (256 / (R / 4)) + 3. 4099 is prime (T = 4099, N = 1: the [T, 2, N] action store's player stride is then 1),
# so R = 256 also runs 4100 = 2 x 2050 rows
HEADS_ROWS = {64: (5, 16387), 128: (5, 8195), 256: (5, 4099, 4100)}


@pytest.mark.parametrize("aux", [False, True])
@pytest.mark.parametrize("A", [4, 8])
@pytest.mark.parametrize("R,rows", [(R, n) for R in (64, 128, 256) for n in HEADS_ROWS[R]])
def test_heads_kernels_match_float64(R, rows, A, aux):
    from active_tracking_rl_amd import fused
    torch.manual_seed(R + rows + A)
    T, N = _rows_split(rows)
    actors = [torch.nn.Linear(R, A).to(DEV) for _ in range(2)]
    critics = [torch.nn.Linear(R, 1).to(DEV) for _ in range(2)]
    auxes = [None, torch.nn.Linear(R, 1).to(DEV) if aux else None]           # (the tracker-aware target's reward head)
    hs = [torch.randn(rows, R, device=DEV, requires_grad=True) for _ in range(2)]
    store = torch.randint(0, A, (T, 2, N), device=DEV)                       # the rollout's [T, players, N] action store
    actions = store.transpose(1, 2)                                          # [T, N, players] view
    ret, gae, rew = (torch.randn(T, N, 2, 1, device=DEV) for _ in range(3))
    # (entropy weights 0.01 and 0.05, the latter as in test_heads_loss_matches_autograd_in_float64: with the target's 0.2 the
    # entropy part of the objective, -0.2 * 1.39 per row, all but cancels the value part, +0.25 per row on these inputs, and the
    # relative error of that one scalar would measure the cancellation — ten times the rounding of either sum — not the kernel)
    scale, scale_aux, w_ent = [1.0 / N, 1.0 / N], 1.0 / N, [0.01, 0.05]
    prm = [[actors[p].weight, actors[p].bias, critics[p].weight, critics[p].bias] +
           ([auxes[p].weight, auxes[p].bias] if auxes[p] is not None else []) for p in range(2)]
    ref = [[_heads_reference(hs[p], prm[p], store[:, p].reshape(rows), ret[:, :, p], gae[:, :, p], rew[:, :, 0], scale[p],
                             scale_aux, w_ent[p], dt) for p in range(2)] for dt in (torch.float64, torch.float32)]
    tab = Table("heads R=%d A=%d aux=%d rows=%d" % (R, A, aux, rows))
    # values: both players in one launch, and one launch per player
    val = torch.zeros(T + 1, N, 2, 1, device=DEV)
    val1 = torch.zeros_like(val)
    fused.heads_values2([h.detach() for h in hs], critics, val)
    for p in range(2):
        fused.heads_values(hs[p].detach(), critics[p], val1, p)
        tab.rule("values2[%d]" % p, val[:T, :, p].reshape(rows), ref[0][p]["values"], ref[1][p]["values"])
        tab.rule("values[%d]" % p, val1[:T, :, p].reshape(rows), ref[0][p]["values"], ref[1][p]["values"])
    assert float(val[T].abs().max()) == 0.0 and float(val1[T].abs().max()) == 0.0      # rows past the last one untouched

    def hold(tag, p, term, stats, grads):
        tab.rule("%s[%d] objective" % (tag, p), term, ref[0][p]["objective"], ref[1][p]["objective"])
        for k, name in enumerate(STAT_NAMES):
            tab.rule("%s[%d] %s" % (tag, p, name), stats[k], ref[0][p]["stats"][k], ref[1][p]["stats"][k])
        assert len(grads) == len(ref[0][p]["grads"])
        for name, g, g64, g32 in zip(GRAD_NAMES, grads, ref[0][p]["grads"], ref[1][p]["grads"]):
            tab.rule("%s[%d] %s" % (tag, p, name), g.reshape(g64.shape), g64, g32)
    # one player per launch
    for p in range(2):
        lp, st = fused.heads_loss(hs[p], actors[p], critics[p], auxes[p], store[:, p].reshape(rows), ret, gae, val, p,
                                  rew if auxes[p] is not None else None, 0, scale[p], scale_aux if auxes[p] is not None else 0.0,
                                  w_ent[p], unit_coeff=True)
        hold("loss", p, lp, st, torch.autograd.grad(lp, [hs[p]] + prm[p]))
    # both players in one launch: actions read in place, value offsets 0 and 1
    cfg = [dict(actions=actions[:, :, p], ret=ret, gae=gae, val=val, off=p, r_aux=rew if auxes[p] is not None else None, aux_off=0,
                scale=scale[p], scale_aux=scale_aux if auxes[p] is not None else 0.0, w_ent=w_ent[p], stats_scale=0.5)
           for p in range(2)]
    l0, l1, st = fused.heads_loss_pair(hs, actors, critics, auxes, cfg)
    one = torch.ones((), device=DEV)
    got = torch.autograd.grad([l0, l1], hs + prm[0] + prm[1], grad_outputs=[one, one])
    hold("pair", 0, l0, st[0] / 0.5, [got[0]] + list(got[2:2 + len(prm[0])]))
    hold("pair", 1, l1, st[1] / 0.5, [got[1]] + list(got[2 + len(prm[0]):]))
    tab.finish()


def test_heads_values_stride_loop_matches_float64():
    """16387 rows at R = 256: 16387 * 64 lanes = 4097 workgroups' worth, one more than the 4096-workgroup cap, so the first
    workgroup runs the stride loop a second time."""
    from active_tracking_rl_amd import fused
    torch.manual_seed(11)
    rows, R = 16387, 256
    critic = torch.nn.Linear(R, 1).to(DEV)
    h = torch.randn(rows, R, device=DEV)
    val = torch.zeros(rows + 1, 3, device=DEV)
    fused.heads_values(h, critic, val, 1)
    with torch.no_grad():
        v64 = (h.double() @ critic.weight.double().t() + critic.bias.double()).reshape(-1)
        v32 = F.linear(h, critic.weight, critic.bias).reshape(-1)
    tab = Table("heads_values rows=16387 R=256")
    tab.rule("values", val[:rows, 1], v64, v32)
    tab.finish()
    assert float(val[:, 0].abs().max()) == 0.0 and float(val[:, 2].abs().max()) == 0.0 and float(val[rows].abs().max()) == 0.0


@pytest.mark.parametrize("R", [64, 256])
def test_rollout_bookkeeping_kernels_at_other_hidden_sizes(R):
    """fused.rollout_begin / rollout_end (they branch on R & 3 only) against the tensor expressions of
    tests/test_drivers_gpu.py::test_bootstrap_values_and_rollout_bookkeeping_kernels, at 37 envs: exact."""
    from active_tracking_rl_amd import fused
    torch.manual_seed(R)
    N, A, T = 37, 2, 5
    hxs, cxs = torch.randn(N, A, R, device=DEV), torch.randn(N, A, R, device=DEV)
    h_all, c_all = torch.randn(A, T + 1, N, R, device=DEV), torch.randn(A, T + 1, N, R, device=DEV)
    h_keep, c_keep = h_all[:, 1:].clone(), c_all[:, 1:].clone()
    obs = torch.rand(N, 2, 13, 13, device=DEV)
    obs_dst = torch.zeros_like(obs)
    fused.rollout_begin(hxs, cxs, h_all, c_all, obs, obs_dst)
    assert torch.equal(h_all[:, 0], hxs.transpose(0, 1)) and torch.equal(c_all[:, 0], cxs.transpose(0, 1))
    assert torch.equal(h_all[:, 1:], h_keep) and torch.equal(c_all[:, 1:], c_keep) and torch.equal(obs_dst, obs)
    dones = (torch.rand(T, N, device=DEV) < 0.3).to(torch.uint8)
    assert 0 < int(dones[-1].sum()) < N
    eps0 = torch.randint(0, 50, (N,), dtype=torch.int32, device=DEV)
    eps, keep = eps0.clone(), torch.empty(T, N, device=DEV)
    hx1, cx1 = torch.zeros_like(hxs), torch.zeros_like(cxs)
    obs1, done1 = torch.zeros_like(obs), torch.zeros(N, dtype=torch.uint8, device=DEV)
    fused.rollout_end(h_all, c_all, dones, hx1, cx1, eps, keep, obs_src=obs, obs_dst=obs1, done_dst=done1)
    k = (dones[-1] == 0).float().view(-1, 1, 1)
    assert torch.equal(hx1, h_all[:, T].transpose(0, 1) * k) and torch.equal(cx1, c_all[:, T].transpose(0, 1) * k)
    nd = (dones == 0).to(torch.int32)
    alive = torch.flip(torch.cumprod(torch.flip(nd, [0]), 0), [0])
    assert torch.equal(eps, eps0 * alive[0] + alive.sum(0))
    assert torch.equal(keep, (dones == 0).float())
    assert torch.equal(obs1, obs) and torch.equal(done1, dones[-1])


def test_a_hidden_size_without_an_action_draw_is_refused_when_the_model_is_built():
    """--rnn-out 512 (above the draw kernels' 256) and 130 (no multiple of 4): ValueError from make_player, naming the sizes that
    work, before any launch; on the CPU the same model is built as ever."""
    from active_tracking_rl_amd.environment import VecEnv
    from active_tracking_rl_amd.train import default_args, make_player
    env = VecEnv("Track2D-BlockPartialPZR-v0", 8, device=DEV, seed=1, obs_u8=True)
    try:
        for R in (512, 130):
            args = default_args(num_envs=8, num_steps=3, rnn_out=R)
            with pytest.raises(ValueError, match="multiples of 4 up to 256"):
                make_player(args, torch.device(DEV), 0, 1, env=env)
    finally:
        env.close()


@pytest.mark.parametrize("R", [32, 192])
def test_sizes_without_a_heads_kernel_run_an_iteration(R):
    """R / 4 = 8 and 48 lanes: a rollout cache and an action draw, no heads kernel (hidden_size_support) — the eager iteration
    goes through the tensor heads and the model's own bootstrap forward without a library error, and moves the weights. (What
    that path computes is held to float64 at R = 96 in tests/test_learner_f64_gpu.py.)"""
    from active_tracking_rl_amd.environment import VecEnv
    from active_tracking_rl_amd.model import hidden_size_support
    from active_tracking_rl_amd.train import default_args, make_player, rollout
    assert hidden_size_support(R) == dict(cache=True, fused_heads=False, fused_boot=False, fused_sampler=True)
    args = default_args(num_envs=16, num_steps=3, rnn_out=R, seed=5)
    env = VecEnv(args.env, 16, device=DEV, seed=5, obs_u8=True)
    try:
        player, opt = make_player(args, torch.device(DEV), 0, 1, env=env)
        w0 = opt.bucket.flat.clone()
        for _ in range(2):
            rollout(player, args.num_steps)
            assert player._cache is not None and player._cache.h_all.shape[-1] == R
            stats = player.optimize(None, opt, player.model, -1, player.device)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(s).all()) for s in stats)
        assert bool(torch.isfinite(opt.bucket.flat).all()) and not torch.equal(w0, opt.bucket.flat)
    finally:
        env.close()
