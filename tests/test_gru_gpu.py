"""-m gpu: the GRU recurrent cores (maze-gru, tat-maze-gru) on the HIP path — the cell kernel against nn.GRUCell, the sequence
node against a float64 evaluation of the same recurrence, the one-launch BPTT (csrc/gru_hip.hip: atr_gru_bptt) against the
per-step path, the drivers (eager loop, both graphed schedules, evaluator, checkpoints), and the LSTM nets left as they were."""
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN
from test_gru_cpu import NETS, TOL, load_det_weights

pytestmark = pytest.mark.gpu
ENV = "Track2D-BlockPartialPZR-v0"


def _dev():
    return torch.device("cuda:0")


def test_gru_cell_matches_grucell_on_masked_inputs():
    from active_tracking_rl_amd import fused
    dev = _dev()
    torch.manual_seed(0)
    N, Fd, R = 50, 256, 128
    cell = nn.GRUCell(Fd, R).to(dev)
    with torch.no_grad():
        cell.bias_ih.normal_(0, 0.5); cell.bias_hh.normal_(0, 0.5)
    x, h = torch.randn(N, Fd, device=dev), torch.randn(N, R, device=dev)
    done = (torch.rand(N, device=dev) < 0.4).to(torch.uint8)
    keep = (done == 0).float()
    with torch.no_grad():
        ig = torch.addmm(cell.bias_ih, x, cell.weight_ih.t())
        hg = torch.mm(h, cell.weight_hh.t())
        want_masked, want_plain = cell(x, h * keep.unsqueeze(1)), cell(x, h)
        got = [fused.gru_cell(ig, hg, cell.bias_hh, h, done=done), fused.gru_cell(ig, hg, cell.bias_hh, h, keep=keep),
               fused.gru_cell(ig, hg, cell.bias_hh, h)]
    assert 0 < int(done.sum()) < N
    for g, w in zip(got, (want_masked, want_masked, want_plain)):
        torch.testing.assert_close(g, w, rtol=1e-4, atol=2e-5)
    assert torch.equal(got[0], got[1])


def _f64_recurrence(cells, feats, h0, keep, go, gh):
    """The masked recurrence of P nn.GRUCells in float64 on the CPU: h_seq [T,P,N,R], final masked h, and the gradients of
    sum(h_seq go) + sum(h_final gh) wrt (per cell weight_ih, weight_hh, bias_ih, bias_hh), feats, h0."""
    P = len(cells)
    c64 = [nn.GRUCell(c.input_size, c.hidden_size).double() for c in cells]
    for a, b in zip(c64, cells):
        a.load_state_dict({k: v.detach().cpu().double() for k, v in b.state_dict().items()})
    f = feats.detach().cpu().double().requires_grad_(True)
    h_in = h0.detach().cpu().double().requires_grad_(True)
    k = keep.cpu().double()
    h, outs = list(h_in.unbind(0)), []
    for t in range(f.shape[0]):
        step = [c64[p](f[t, p], h[p]) for p in range(P)]
        outs.append(torch.stack(step, 0))
        h = [s * k[t].unsqueeze(1) for s in step]
    h_seq, h_fin = torch.stack(outs, 0), torch.stack(h, 0)
    params = [p for c in c64 for p in (c.weight_ih, c.weight_hh, c.bias_ih, c.bias_hh)]
    grads = torch.autograd.grad((h_seq * go.cpu().double()).sum() + (h_fin * gh.cpu().double()).sum(), params + [f, h_in])
    return h_seq.detach(), h_fin.detach(), grads


@pytest.mark.parametrize("fused_bptt", (True, False))
def test_gru_sequence_node_matches_float64(fused_bptt):
    from active_tracking_rl_amd import fused
    from active_tracking_rl_amd import model as M
    dev = _dev()
    torch.manual_seed(1)
    T, P, N, Fd, R = 7, 2, 37, 256, 128
    cells = [nn.GRUCell(Fd, R).to(dev) for _ in range(P)]
    with torch.no_grad():
        for c in cells:                     # zero biases would hide a wrong b_hn path
            c.bias_ih.normal_(0, 0.5); c.bias_hh.normal_(0, 0.5)
    feats = torch.randn(T, P, N, Fd, device=dev, requires_grad=True)
    h0 = (torch.randn(P, N, R, device=dev) * 0.5).requires_grad_(True)
    c0 = torch.zeros(P, N, R, device=dev)
    keep = (torch.rand(T, N, device=dev) > 0.3).float()
    go, gh = torch.randn(T, P, N, R, device=dev), torch.randn(P, N, R, device=dev)
    params = [p for c in cells for p in (c.weight_ih, c.weight_hh, c.bias_ih, c.bias_hh)]
    fused.use_fused_gru_bptt = fused_bptt
    try:
        h_seq, h_fin, c_fin = M.gru_sequence(cells, [feats[:, p] for p in range(P)], h0, c0, keep)
        assert isinstance(h_seq, list) and h_seq[0].shape == (T, N, R)          # the HIP recurrence, not the ATen fallback
        h_seq = torch.stack(h_seq, 1)
        grads = torch.autograd.grad((h_seq * go).sum() + (h_fin * gh).sum(), params + [feats, h0])
    finally:
        fused.use_fused_gru_bptt = True
    w_seq, w_fin, w_grads = _f64_recurrence(cells, feats, h0, keep, go, gh)
    torch.testing.assert_close(h_seq.detach().cpu().double(), w_seq, rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(h_fin.detach().cpu().double(), w_fin, rtol=1e-4, atol=2e-5)
    assert float(c_fin.abs().max()) == 0.0
    names = ["%s[%d]" % (n, p) for p in range(P) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] + ["feats", "h0"]
    for name, g, w in zip(names, grads, w_grads):
        err, scale = float((g.detach().cpu().double() - w).abs().max()), float(w.abs().max())
        print("%-14s max|ref| %.4e  max err %.3e  (%.2e of it)" % (name, scale, err, err / scale))
        assert err <= 2e-4 * scale, name
    for p in range(P):                      # b_hn sits inside r * (.): the two bias gradients differ in the n block only
        dbi, dbh = grads[4 * p + 2], grads[4 * p + 3]
        torch.testing.assert_close(dbi[:2 * R], dbh[:2 * R], rtol=1e-5, atol=1e-5 * float(dbi.abs().max()))
        assert float((dbi[2 * R:] - dbh[2 * R:]).abs().max()) > 1e-2 * float(dbi[2 * R:].abs().max())


@pytest.mark.parametrize("N", [1, 37])
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("R", [64, 256])
def test_gru_sequence_node_at_other_hidden_sizes_matches_float64(R, P, N):
    """model.gru_sequence off R = 128 (--rnn-out): the cell kernel forward and, as there is no one-launch BPTT off 128, the
    per-step backward (atr_gru_cell_backward + baddbmm) that such models train through, by the rule of tests/f64_rule.py
    against a float64 per-step nn.GRUCell recurrence: outputs, final state, gradients to the features, h0 and every weight and
    bias. Measured on MI355X over the eight cases:
      h_seq, h_fin          e(hip) 0 .. 2.8e-07         e(aten32) 0 .. 2.7e-07         e(hip) / allowed <= 0.07
      weight_ih, weight_hh  e(hip) 1.5e-07 .. 4.5e-07   e(aten32) 1.4e-07 .. 4.1e-07   e(hip) / allowed <= 0.35
      bias_ih, bias_hh      e(hip) 1.2e-07 .. 3.2e-07   e(aten32) 1.1e-07 .. 3.1e-07   e(hip) / allowed <= 0.30
      feats, h0             e(hip) 8.6e-08 .. 4.1e-07   e(aten32) 1.2e-07 .. 3.7e-07   e(hip) / allowed <= 0.27"""
    from f64_rule import HIDDEN_FLOOR, Table, cell_recurrence
    from active_tracking_rl_amd import model as M
    dev = _dev()
    torch.manual_seed(R + 2 * P + N)
    T, Fd = 7, 256
    cells = [nn.GRUCell(Fd, R).to(dev) for _ in range(P)]
    with torch.no_grad():
        for c in cells:                     # zero biases would hide a wrong b_hn path
            c.bias_ih.normal_(0, 0.5); c.bias_hh.normal_(0, 0.5)
    feats = torch.randn(T, P, N, Fd, device=dev, requires_grad=True)
    h0 = (torch.randn(P, N, R, device=dev) * 0.5).requires_grad_(True)
    keep = (torch.rand(T, N, device=dev) > 0.3).float()
    go, gh = torch.randn(T, P, N, R, device=dev), torch.randn(P, N, R, device=dev)
    names = ["%s[%d]" % (n, p) for p in range(P) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] + ["feats", "h0"]
    wrt = [getattr(cells[p], n) for p in range(P) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] + [feats, h0]
    h_seq, h_fin, c_fin = M.gru_sequence(cells, [feats[:, p] for p in range(P)], h0, torch.zeros(P, N, R, device=dev), keep)
    assert isinstance(h_seq, list) and h_seq[0].shape == (T, N, R)              # the HIP recurrence, not the ATen fallback
    h_seq = torch.stack(h_seq, 1)
    grads = dict(zip(names, torch.autograd.grad((h_seq * go).sum() + (h_fin * gh).sum(), wrt)))
    x64 = cell_recurrence(cells, feats, h0, None, keep, go, gh, torch.float64, "cpu")
    x32 = cell_recurrence(cells, feats, h0, None, keep, go, gh, torch.float32, dev)
    tab = Table("gru R=%d P=%d N=%d T=%d" % (R, P, N, T))
    tab.rule("h_seq", h_seq, x64["h_seq"], x32["h_seq"], floor=HIDDEN_FLOOR)
    tab.rule("h_fin", h_fin, x64["h_fin"], x32["h_fin"], floor=HIDDEN_FLOOR)
    for n in names:
        tab.rule(n, grads[n], x64[n], x32[n])
    tab.finish()
    assert float(c_fin.abs().max()) == 0.0


@pytest.mark.parametrize("N,P,T", [(16, 1, 1), (37, 1, 5), (40, 2, 3), (512, 2, 20)])
def test_one_launch_gru_bptt_matches_the_per_step_path(N, P, T):
    from active_tracking_rl_amd import fused
    dev = _dev()
    torch.manual_seed(5)
    R = 128
    whh = torch.randn(P, R, 3 * R, device=dev) / R ** 0.5
    h_all = torch.randn(P, T + 1, N, R, device=dev) * 0.5
    acts = torch.cat([torch.rand(P, T, N, 2 * R, device=dev) * 0.98 + 0.01, torch.rand(P, T, N, R, device=dev) * 1.96 - 0.98,
                      torch.randn(P, T, N, R, device=dev)], -1).contiguous()       # r, z in (0, 1), n in (-1, 1), q free
    keep = (torch.rand(T, N, device=dev) > 0.2).float()
    keep[0, ::3] = 0
    keep[T - 1, 1::4] = 0
    dhs = [torch.randn(T, N, R, device=dev) for _ in range(P)]
    if (N, P, T) == (40, 2, 3):
        dhs[1] = None
    out = {}
    for flag in (True, False):
        fused.use_fused_gru_bptt = flag
        try:
            out[flag] = fused._gru_bptt(whh, keep, h_all, acts, dhs)
        finally:
            fused.use_fused_gru_bptt = True
    torch.cuda.synchronize()
    for name, a, b in zip(("dG", "dh0", "dW_hh", "db_hh"), out[True], out[False]):
        assert torch.isfinite(a).all() and a.shape == b.shape, name
        scale = max(float(b.abs().max()), 1.0)
        print("%-6s max|per-step| %.4e  max diff %.3e" % (name, float(b.abs().max()), float((a - b).abs().max())))
        torch.testing.assert_close(a, b, rtol=2e-4, atol=2e-5 * scale, msg=lambda m, name=name: name + ": " + m)
    if dhs[-1] is None:                     # no head gradient and nothing downstream: that player's dG is zero
        assert float(out[True][0][1].abs().max()) == 0.0


def _player(net, n_envs=64, num_steps=5, seed=23, **kw):
    from active_tracking_rl_amd.train import default_args, make_player
    args = default_args(env=ENV, network=net, aux="reward" if "tat" in net else "none", num_envs=n_envs, num_steps=num_steps,
                        seed=seed, **kw)
    args.gpu_ids = [0]
    player, opt = make_player(args, _dev())
    return args, player, opt


def _keep_actions(player):
    """Have compute_grads leave the rollout's stored actions in player.kept_actions (it clears the lists)."""
    inner = player.compute_grads

    def compute_grads(optimizer, mode):
        player.kept_actions = list(player.actions)
        return inner(optimizer, mode)
    player.compute_grads = compute_grads


@pytest.mark.parametrize("net", NETS)
def test_eager_iteration_and_graph_replay_agree(net):
    """One eager iteration and one GraphedIteration replay from identical weights, env shard, seed and draw-stream position: the
    same rollout (equal stored actions), gradient buckets within 2e-4 of the largest entry."""
    from active_tracking_rl_amd.train import GraphedIteration, rolled_back, rollout, update_tensors
    dev = _dev()
    args, pa, oa = _player(net)
    _keep_actions(pa)
    with rolled_back(update_tensors(oa)):               # what GraphedIteration's constructor does before it captures
        for _ in range(2):
            rollout(pa, args.num_steps)
            pa.optimize(None, oa, pa.model, args.train_mode, dev)
        torch.cuda.synchronize()
    pa.env.flush()
    torch.cuda.manual_seed(99)                          # (the bootstrap step of the learner draws with torch's generator)
    rollout(pa, args.num_steps)
    assert pa.cache_rollout and pa._cache is None
    pa.compute_grads(oa, args.train_mode)
    torch.cuda.synchronize()
    g_eager, a_eager = oa.bucket.grad.clone(), torch.stack(pa.kept_actions, 0).clone()
    pa.env.close()

    args, pb, ob = _player(net)
    _keep_actions(pb)
    assert torch.equal(ob.bucket.flat, oa.bucket.flat)
    it = GraphedIteration(pb, ob, args)
    ob.bucket.grad.zero_()
    torch.cuda.manual_seed(99)
    it.g_rolls[args.train_mode].replay()
    torch.cuda.synchronize()
    a_graph = torch.stack(pb.kept_actions, 0)
    assert a_eager.shape == (args.num_steps, 64, 2) and torch.equal(a_eager, a_graph)
    scale = float(g_eager.abs().max())
    err = float((ob.bucket.grad - g_eager).abs().max())
    print("%s: max|bucket| %.4e  max diff %.3e" % (net, scale, err))
    assert scale > 0 and torch.isfinite(ob.bucket.grad).all() and err <= 2e-4 * scale
    pb.env.close()


@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("schedule", ("synchronous", "pipelined"))
def test_graphed_schedules_train_gru_nets(net, schedule):
    from active_tracking_rl_amd.train import GraphedIteration, PipelinedIteration
    args, player, opt = _player(net)
    w0 = opt.bucket.flat.clone()
    it = GraphedIteration(player, opt, args) if schedule == "synchronous" else PipelinedIteration(player, opt, args)
    agents = [player] if schedule == "synchronous" else it.players
    assert torch.equal(opt.bucket.flat, w0)
    for i in range(3):
        it.run()
        if schedule == "pipelined":
            it.sync()
        torch.cuda.synchronize()
        # nothing writes cxs but the mask: the carry, and the agent whose rollout has just run (a replica of the pipelined
        # schedule whose graphs have not been replayed yet holds memory nothing has written)
        ran = player if schedule == "synchronous" else it.players[i & 1]
        assert float(ran.cxs.abs().max()) == 0.0 and float(it.carry["cxs"].abs().max()) == 0.0
    it.finish()
    torch.cuda.synchronize()
    assert torch.isfinite(opt.bucket.flat).all() and not torch.equal(opt.bucket.flat, w0)
    assert all(a.cache_rollout and a._cache is None for a in agents)
    assert float(it.carry["cxs"].abs().max()) == 0.0 and float(it.carry["hxs"].abs().max()) > 0.0
    assert torch.isfinite(it.carry["hxs"]).all()
    player.env.close()


@pytest.mark.parametrize("net", NETS)
def test_evaluator_falls_back_to_the_eager_round(net):
    from active_tracking_rl_amd import evaluator
    from active_tracking_rl_amd.test import evaluate
    args, player, _ = _player(net)
    assert evaluator.supported(player.env, player.model) is False
    rsum, length = evaluate(player.model, ENV, args, _dev(), 8)
    assert rsum.shape == (8, 2) and np.isfinite(rsum).all() and (length >= 1).all() and (length <= 500).all()
    rsum_g, length_g = evaluate(player.model, ENV, args, _dev(), 8, graphed=True)      # --graphed-eval: the same eager round
    assert np.array_equal(rsum_g, rsum) and np.array_equal(length_g, length)
    assert player.model.training
    player.env.close()


@pytest.mark.parametrize("net", NETS)
def test_checkpoint_round_trip_and_reference_weights_on_the_gpu(tmp_path, net):
    from active_tracking_rl_amd.model import build_model
    from active_tracking_rl_amd.test import save_checkpoints
    dev = _dev()
    args, player, _ = _player(net, log_dir=str(tmp_path), split=True)
    m = player.model
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)           # biases start at zero: make them tell
    save_checkpoints(m, args, 7, True)
    m2 = build_model(player.env.observation_space, player.env.action_space, args, dev).to(dev)
    m2.player0.load_state_dict(torch.load(os.path.join(str(tmp_path), "tracker-best.dat")))
    m2.player1.load_state_dict(torch.load(os.path.join(str(tmp_path), "target-best.dat")))
    sd = torch.load(os.path.join(str(tmp_path), "tracker-best.dat"))
    assert tuple(sd["lstm.weight_ih"].shape) == (384, 256) and tuple(sd["lstm.bias_hh"].shape) == (384,)
    g = np.load(os.path.join(GOLDEN, "model_gru.npz"))
    states = torch.from_numpy(g[net + "/states"]).to(dev)
    hx, cx = torch.from_numpy(g[net + "/hx"]).to(dev), torch.from_numpy(g[net + "/cx"]).to(dev)
    m.eval(); m2.eval()
    with torch.no_grad():
        o1, o2 = m((states, (hx, cx)), True), m2((states, (hx, cx)), True)
    for a, b in ((o1[0], o2[0]), (o1[2], o2[2]), (o1[3], o2[3]), (o1[4][0], o2[4][0]), (o1[4][1], o2[4][1])):
        assert torch.equal(a, b)
    assert all(torch.equal(a, b) for a, b in zip(o1[1], o2[1]))
    # the reference's outputs on the fixture's deterministic weights, at the fixture's tolerance
    load_det_weights(m2)
    with torch.no_grad():
        v, a, e, lp, (h, c), rp = m2((states, (hx, cx)), True)
    np.testing.assert_allclose(v.cpu().numpy(), g[net + "/values"], **TOL)
    np.testing.assert_allclose(e.cpu().numpy(), g[net + "/entropies"], **TOL)
    np.testing.assert_allclose(lp.cpu().numpy(), g[net + "/log_probs"], **TOL)
    np.testing.assert_allclose(h.cpu().numpy(), g[net + "/hx_out"], **TOL)
    assert np.array_equal(c.cpu().numpy(), g[net + "/cx_out"])
    assert np.array_equal(torch.stack(a, 1).cpu().numpy(), g[net + "/actions"])
    if "tat" in net:
        np.testing.assert_allclose(rp.cpu().numpy().reshape(-1), g[net + "/r_pred"].reshape(-1), **TOL)
    player.env.close()


def _digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd.keys()):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def test_lstm_nets_are_built_and_rolled_out_as_before():
    """build_model('tat-maze-lstm') under a fixed seed = the nn.LSTMCell-based construction written out here (what the model
    file did before it knew a second core), byte for byte; and an LSTM player still takes the cached rollout path."""
    from active_tracking_rl_amd import model as M
    from active_tracking_rl_amd.environment import _spaces
    from active_tracking_rl_amd.train import default_args, rollout
    obs, act = _spaces()
    args = default_args(network="tat-maze-lstm")
    torch.manual_seed(41)
    built = M.build_model(obs, act, args, torch.device("cpu"))

    def lstm_player(space, action_space, frames, tat):
        p = nn.Module()
        p.encoder = M.CNN_maze(space.shape, frames)
        p.lstm = nn.LSTMCell(p.encoder.outdim, 128)
        p.lstm.bias_ih.data.fill_(0)
        p.lstm.bias_hh.data.fill_(0)
        p.actor = M.PolicyNet(128, action_space, "tat-maze-lstm", None)
        p.critic = M.ValueNet(128)
        if tat:
            p.fc_action_tracker = nn.Linear(act[0].n, p.encoder.outdim)
            M.weights_init_mlp(p.fc_action_tracker)
            p.reward_aux = nn.Linear(128, 1)
            p.reward_aux.weight.data = M.norm_col_init(p.reward_aux.weight.data, 0.01)
            p.reward_aux.bias.data.fill_(0)
        p.apply(M.weights_init)
        return p
    torch.manual_seed(41)
    want = nn.Module()
    want.player0 = lstm_player(obs[0], act[0], 1, False)
    want.player1 = lstm_player(obs[1], act[1], 2, True)
    assert sorted(built.state_dict().keys()) == sorted(want.state_dict().keys())
    assert _digest(built.state_dict()) == _digest(want.state_dict())
    assert built.cacheable_core is True
    args, player, _ = _player("tat-maze-lstm")
    rollout(player, args.num_steps)
    assert player._cache is not None and player.model.cacheable_core
    player.env.close()
