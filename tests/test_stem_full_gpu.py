"""-m gpu numerics tests of the whole-map conv stem (csrc/stem_full_hip.hip, fused.stem_full, --full-stem) against the plain
PyTorch reference of the same op: F.conv2d + ReLU in fp32 for the forward, in float64 with autograd for the gradients.
Tolerances are those of tests/test_fused_stem_gpu.py for the 13 x 13 stem: forward rtol = atol = 1e-5 (every output is a sum of
the same 9 and 144 terms), each parameter gradient within 2e-4 of its own maximum (the sums here, at most a few hundred frames
x 1681 cells, are shorter than the 16 391 frames x 16 that test covers)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = ("dw1", "db1", "dw2", "db2")


def _convs(seed, b1=None, b2=None):
    torch.manual_seed(seed)
    conv1 = torch.nn.Conv2d(1, 16, 3, 2, 1).to(DEV)
    conv2 = torch.nn.Conv2d(16, 32, 3, 2, 1).to(DEV)
    with torch.no_grad():
        conv1.weight.mul_(2.0); conv2.weight.mul_(3.0); conv1.bias.normal_(0, 0.2); conv2.bias.normal_(0, 0.2)
        if b1 is not None:
            conv1.bias.fill_(b1)
        if b2 is not None:
            conv2.bias.fill_(b2)
    return conv1, conv2


def _params(conv1, conv2):
    return [conv1.weight, conv1.bias, conv2.weight, conv2.bias]


def _ref(x, params, dtype=torch.float32):
    """relu(conv2(relu(conv1(x)))) of frames x [M, S, S] -> [M, 14112]; leaves of their own in `dtype`."""
    w1, b1, w2, b2 = leaves = [p.detach().to(dtype).requires_grad_(True) for p in params]
    a = F.relu(F.conv2d(x.to(dtype).unsqueeze(1), w1, b1, stride=2, padding=1))
    return F.relu(F.conv2d(a, w2, b2, stride=2, padding=1)).reshape(x.shape[0], -1), leaves


def _check(x, conv1, conv2, seed=0):
    """Forward against fp32 conv2d, the four gradients of sum(y * g) against float64 conv2d; returns (y, grads)."""
    from active_tracking_rl_amd import fused
    params = _params(conv1, conv2)
    M = x.numel() // (x.shape[-1] * x.shape[-2])
    y = fused.stem_full(x, conv1, conv2)
    frames = x.reshape(M, x.shape[-2], x.shape[-1])
    yr, _ = _ref(frames, params)
    assert y.shape == (M, 32 * 21 * 21) and y.dtype == torch.float32
    err = float((y - yr).detach().abs().max()) if M else 0.0
    print("S=%d M=%d forward max err %.3g" % (x.shape[-1], M, err))
    torch.testing.assert_close(y, yr.detach(), rtol=1e-5, atol=1e-5)
    g = torch.randn(y.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(seed + 1))
    got = torch.autograd.grad((y * g).sum(), params)
    y64, leaves = _ref(frames, params, torch.float64)
    want = torch.autograd.grad((y64 * g.double()).sum(), leaves)
    for a, b, name in zip(got, want, NAMES):
        assert a.shape == b.shape
        scale = float(b.abs().max()) + 1e-6
        d = float((a.double() - b).abs().max())
        print("   %s max err %.3g of %.3g (%.3g)" % (name, d, scale, d / scale))
        assert d <= 2e-4 * scale, (name, M, d, scale)
    return y, got


def _frames(seed, M, S):
    return torch.tensor(np.random.RandomState(seed).choice([0, 1, 2, 4], size=(M, S, S)).astype(np.float32), device=DEV)


@pytest.mark.parametrize("S", [81, 82])
@pytest.mark.parametrize("M", [1, 3, 17])
def test_stem_full_matches_conv2d(S, M):
    conv1, conv2 = _convs(100 * S + M)
    _check(_frames(100 * S + M, M, S), conv1, conv2, seed=M)


@pytest.mark.parametrize("S", [81, 82])
def test_stem_full_border_frame(S):
    """A frame that is zero except for its first and last row and column: the taps at the padded edges, where the sides differ."""
    x = torch.zeros(2, S, S, device=DEV)
    x[:, 0, :] = 1.0; x[:, S - 1, :] = 2.0; x[:, :, 0] = 4.0; x[:, :, S - 1] = 3.0
    x[1] *= 0.5
    conv1, conv2 = _convs(S)
    y, _ = _check(x, conv1, conv2)
    assert float(y.detach().abs().max()) > 0


@pytest.mark.parametrize("S", [81, 82])
def test_stem_full_reads_a_strided_view_in_place(S):
    """Agent 1's planes of an [N, 2, S, S] tensor: no copy (frame stride 2 S S), same result as the contiguous copy."""
    from active_tracking_rl_amd import fused
    obs = torch.tensor(np.random.RandomState(S).choice([0, 1, 2, 4], size=(5, 2, S, S)).astype(np.float32), device=DEV)
    view = obs[:, 1]
    rows = fused.full_frames(view)
    assert rows.data_ptr() == view.data_ptr() and rows.stride() == (2 * S * S, S, 1) and rows.shape == (5, S, S)
    six = obs.view(5, 2, 1, 1, S, S)[:, 0]                          # the encoder's [n, stack, C, S, S] view of agent 0
    assert fused.full_frames(six).data_ptr() == obs.data_ptr() and fused.full_frames(six).stride(0) == 2 * S * S
    conv1, conv2 = _convs(7)
    y, grads = _check(view, conv1, conv2)
    y2 = fused.stem_full(view.contiguous(), conv1, conv2)
    assert torch.equal(y, y2)


def test_stem_full_copies_only_views_without_a_constant_stride():
    """Stacked frames of one agent, [N, stack] out of [N, 2, stack, S, S], have a constant frame stride only when N == 1 or
    stack == 1: otherwise the node works on a contiguous copy, and the result is that of the copy."""
    from active_tracking_rl_amd import fused
    S = 81
    obs = torch.tensor(np.random.RandomState(5).choice([0, 1, 2, 4], size=(3, 2, 2, S, S)).astype(np.float32), device=DEV)
    view = obs[:, 1]                                                # [3, 2, S, S]: strides (4 S S, S S): not constant
    rows = fused.full_frames(view)
    assert rows.is_contiguous() and rows.data_ptr() != view.data_ptr() and rows.shape == (6, S, S)
    assert torch.equal(rows, view.reshape(6, S, S))
    one = obs[:1, 1]                                                # one env: its two frames are S S apart
    assert fused.full_frames(one).data_ptr() == one.data_ptr()
    conv1, conv2 = _convs(8)
    _check(view, conv1, conv2)


def test_stem_full_general_float_frames():
    """Negative and fractional cell values: what --inv and --rescale make of the frames."""
    for S in (81, 82):
        x = torch.randn(3, S, S, device=DEV, generator=torch.Generator(DEV).manual_seed(S)) * 1.5 - 0.25
        conv1, conv2 = _convs(S + 1)
        _check(x, conv1, conv2)


def test_stem_full_dead_relu_gives_exactly_zero_gradients():
    from active_tracking_rl_amd import fused
    conv1, conv2 = _convs(9, b2=-1e4)
    x = _frames(9, 4, 82)
    y = fused.stem_full(x, conv1, conv2)
    assert float(y.detach().abs().max()) == 0.0
    grads = torch.autograd.grad((y * torch.randn_like(y)).sum(), _params(conv1, conv2))
    for gname, gr in zip(NAMES, grads):
        assert float(gr.abs().max()) == 0.0, gname


def test_stem_full_more_bands_than_workgroups():
    """A frame count past one pass of the backward's grid (three bands per frame, capped at stem_full_workgroup_cap()
    workgroups) and of the forward's (1.5 x that): the grid-stride passes."""
    from active_tracking_rl_amd import fused
    cap = fused.stem_full_workgroup_cap()
    assert cap >= 1 and fused.lib().atr_stem_full_workspace_floats(1) == 3 * fused.STEM_FULL_RECORD
    M = cap // 2 + 2                                                # 3 M > 1.5 cap
    assert fused.lib().atr_stem_full_workspace_floats(M) == cap * fused.STEM_FULL_RECORD
    conv1, conv2 = _convs(11)
    _check(_frames(11, M, 81), conv1, conv2)


def test_stem_full_zero_frames_and_bad_side():
    from active_tracking_rl_amd import fused
    conv1, conv2 = _convs(12)
    w = [C.c_void_p(p.data_ptr()) for p in _params(conv1, conv2)]
    L = fused.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = _frames(12, 1, 82)
    y = torch.full((1, 32 * 21 * 21), 7.0, device=DEV)
    px, py = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())
    assert L.atr_stem_full_forward(px, 82 * 82, 82, *w, py, 0, stream) == 0
    grads = [torch.full((n,), 7.0, device=DEV) for n in (144, 16, 4608, 32)]
    ws = torch.empty(fused.STEM_FULL_RECORD, device=DEV)
    pg = [C.c_void_p(t.data_ptr()) for t in grads]
    assert L.atr_stem_full_backward(px, 82 * 82, 82, py, py, w[0], w[1], w[2], *pg, C.c_void_p(ws.data_ptr()), 0, stream) == 0
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0 and float(y.max()) == 7.0 and all(float(t.min()) == 7.0 == float(t.max()) for t in grads)
    for S in (80, 83, 13):
        with pytest.raises(RuntimeError, match=r"atr_stem_full_forward failed \(-1\)"):
            L.atr_stem_full_forward(px, 82 * 82, S, *w, py, 1, stream)
    with pytest.raises(RuntimeError, match=r"atr_stem_full_forward failed \(-1\)"):
        L.atr_stem_full_forward(px, 82 * 82 - 1, 82, *w, py, 1, stream)                     # frames would overlap
    with pytest.raises(RuntimeError, match=r"atr_stem_full_backward failed \(-1\)"):
        L.atr_stem_full_backward(px, 82 * 82, 80, py, py, w[0], w[1], w[2], *pg, C.c_void_p(ws.data_ptr()), 1, stream)
    with pytest.raises(ValueError):
        fused.stem_full(torch.zeros(2, 80, 80, device=DEV), conv1, conv2)
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0 and float(y.max()) == 7.0
    # the autograd node on zero frames: an empty output, zero gradients
    y0 = fused.stem_full(torch.zeros(0, 82, 82, device=DEV), conv1, conv2)
    assert y0.shape == (0, 32 * 21 * 21)
    for gr in torch.autograd.grad(y0.sum(), _params(conv1, conv2)):
        assert float(gr.abs().max()) == 0.0


def test_stem_full_backward_is_deterministic():
    from active_tracking_rl_amd import fused
    conv1, conv2 = _convs(13)
    x = _frames(13, fused.stem_full_workgroup_cap() // 3 + 5, 82)       # past one pass: workgroups add several bands
    g = None
    runs = []
    for _ in range(2):
        y = fused.stem_full(x, conv1, conv2)
        g = torch.randn_like(y) if g is None else g
        runs.append((y.detach(), torch.autograd.grad((y * g).sum(), _params(conv1, conv2))))
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("net,side", [("maze-lstm", 82), ("tat-maze-lstm", 81)])
def test_model_with_full_stem_equals_conv2d(net, side):
    """Both encoders of a two-player model, N = 5: the tracker's one frame per env and (tat) the target's two, switch on against
    off — features after fc to rtol 1e-4 / atol 1e-5, encoder parameter gradients to 2e-4 of their maximum."""
    from active_tracking_rl_amd.environment import _spaces
    from active_tracking_rl_amd.model import build_model
    from active_tracking_rl_amd.train import default_args
    obs, act = _spaces((side, side))
    torch.manual_seed(0)
    m = build_model(obs, act, default_args(network=net, aux="reward" if "tat" in net else "none", full_stem=True),
                    torch.device(DEV)).to(DEV)
    assert m.full_stem and m.player0.encoder.use_fused_full and not m.player0.encoder.small
    states = torch.randint(0, 5, (5, 2, 1, 1, side, side), device=DEV).float()
    for k, player in enumerate((m.player0, m.player1)):
        enc = player.encoder
        x = states[:, k]
        if "tat" in net and k == 1:                                  # the target sees both agents' frames: [n, 2, 1, S, S]
            x = states.view(5, 2, 1, side, side)
        with torch.no_grad():
            enc.conv1.bias.normal_(0, 0.2); enc.conv2.bias.normal_(0, 0.2)
        outs = []
        for flag in (True, False):
            enc.use_fused_full = flag
            stem = enc(x, fc=False)
            f = enc(x)
            gr = torch.autograd.grad((f * torch.linspace(-1, 1, 256, device=DEV)).sum(), list(enc.parameters()))
            outs.append((stem.detach(), f.detach(), gr))
        enc.use_fused_full = True
        assert outs[0][0].shape == (5, x.shape[1] * 32 * 21 * 21)
        torch.testing.assert_close(outs[0][0], outs[1][0], rtol=1e-5, atol=1e-5)       # [frame 0 | frame 1] per env
        torch.testing.assert_close(outs[0][1], outs[1][1], rtol=1e-4, atol=1e-5)
        for (name, _), a, b in zip(enc.named_parameters(), outs[0][2], outs[1][2]):
            scale = float(b.abs().max()) + 1e-6
            assert float((a - b).abs().max()) <= 2e-4 * scale, (net, k, name, float((a - b).abs().max()), scale)


def _snapshot(player, boot_action):
    """learner_f64.snapshot for a player without a rollout cache ('Full' ids keep none): what loss_recompute reads, on the CPU."""
    a, m = player.args, player.model
    T = len(player.rewards)
    if player._buf is not None and T == player._buf[1].shape[0]:
        obs, rewards, dones = player._buf[0][:T], player._buf[1], player._buf[2]
    else:
        obs = torch.stack(player.states, 0).reshape(T, player.num_envs, 2, *player.state.shape[-2:])
        rewards, dones = torch.stack(player.rewards, 0).squeeze(3), torch.stack(player.dones, 0)
    acts = player._actions_buf.transpose(1, 2) if player._actions_buf is not None else torch.stack(player.actions, 0)
    obs = torch.cat([obs.reshape(T, *obs.shape[1:3], *obs.shape[-2:]), player.state.reshape(1, *obs.shape[1:3], *obs.shape[-2:])], 0)
    cpu = lambda t: t.detach().cpu().clone()
    return dict(obs=cpu(obs), rewards=cpu(rewards), dones=cpu(dones), actions=cpu(acts), h0=cpu(player.h0.transpose(0, 1)),
                c0=cpu(player.c0.transpose(0, 1)), boot_action=cpu(boot_action) if m.tat else None,
                weights={k: cpu(v) for k, v in m.state_dict().items()}, gamma=float(a.gamma), tau=float(a.tau),
                entropy=float(a.entropy), w_entropy_target=float(player.w_entropy_target), aux=str(a.aux), network=str(a.network),
                rnn_out=int(a.rnn_out))


@pytest.mark.parametrize("env_id,net,aux,side", [("Track2D-BlockFullAdv-v0", "maze-lstm", "none", 82),
                                                 ("Track2D-MazeFullPZR-v0", "tat-maze-lstm", "reward", 81)])
def test_full_stem_learner_matches_the_conv2d_learner_then_trains(env_id, net, aux, side):
    """One stored rollout of a 'Full' id, the recompute learner (player.loss_recompute(-1)) with the switch off and on: the loss
    and its terms agree to rtol 1e-4 / atol 1e-5; every parameter gradient of the switch-on learner is within 2e-4 of the
    gradient's maximum of the conv2d learner evaluated in float64 (tests/learner_f64.py: the yardstick of the gradient cases).
    Then three pipelined iterations with --full-stem: finite weights, and the driver stays on one stream.

    Why float64 and not the switch-off fp32 pass for the gradients: on real map frames with the initial zero biases 38 % of
    conv2's pre-activations are EXACTLY zero (all-free neighbourhoods). The HIP stem and float64 conv2d give 0 there; the
    library's fp32 conv2d leaves residues of 2e-9 .. 3e-8 at 15 950 of them (64 frames of Track2D-BlockFullAdv-v0, measured on
    MI355X), which its ReLU backward lets through: its conv2.bias gradient is then off by 9.55 of 50.6 against float64 (HIP
    stem: 1.6e-5 of 50.6), and in this test by 0.0195 of 0.101 / 0.0125 of 0.12 (Block, tracker / target) and 0.0243 of 0.0544 /
    0.0284 of 0.188 (Maze) where the HIP stem is within 7e-8 — every other gradient of the two fp32 passes agrees to 3e-6 of its
    maximum (the z1 patches of those positions are zero, so nothing else sees them). All three differences are printed, and
    wherever the switch-off fp32 pass itself meets the bound against float64 the two fp32 passes are held to it as well."""
    import learner_f64
    from active_tracking_rl_amd.train import PipelinedIteration, default_args, make_player, rollout
    dev = torch.device("cuda:0")
    args = default_args(env=env_id, network=net, aux=aux, num_envs=16, num_steps=4, full_stem=True)
    player, opt = make_player(args, dev)
    assert player.env.observation_space[0].shape == (1, side, side)
    encoders = [player.model.player0.encoder, player.model.player1.encoder]
    assert all(e.use_fused_full and not e.small for e in encoders)
    rollout(player, args.num_steps)
    boot_actions = []
    hook = player.model.register_forward_hook(lambda mod, inp, out: boot_actions.append(out[1][0].detach().clone()))
    outs = []
    for flag in (False, True):
        for e in encoders:
            e.use_fused_full = flag
        torch.manual_seed(5)                     # the tat bootstrap value depends on a freshly sampled tracker action: pin the draw
        if getattr(player.model, "_sampler", None) is not None:
            player.model._sampler.counter.zero_()
            player.model._sampler._last = None
        loss, pl, vl, ent, pred = player.loss_recompute(-1)
        params = list(player.model.parameters())
        grads = torch.autograd.grad(loss, params, allow_unused=True)
        outs.append((loss.detach(), pl.detach().mean(0), vl.detach().mean(0), ent.detach().mean(0),
                     torch.as_tensor(pred).detach().float().mean(0), grads))
    hook.remove()
    assert len(boot_actions) == 2 and torch.equal(boot_actions[0], boot_actions[1])
    la, pla, vla, ea, pa, ga = outs[1]
    lb, plb, vlb, eb, pb, gb = outs[0]
    torch.testing.assert_close(la, lb, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(pla, plb, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(vla, vlb, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(ea, eb, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(pa.reshape(-1), pb.reshape(-1), rtol=1e-4, atol=1e-5)
    ref = learner_f64.reference(_snapshot(player, boot_actions[1]), -1)
    seen = agree = 0
    for (name, _), a, b in zip(player.model.named_parameters(), ga, gb):
        w = ref["grads"][name].to(dev)
        if a is None:
            assert b is None and float(w.abs().max()) == 0.0, name
            continue
        scale = float(w.abs().max()) + 1e-6
        on, off = float((a.double() - w).abs().max()), float((b.double() - w).abs().max())
        print("%-36s on - f64 %.3g   off - f64 %.3g   on - off %.3g   of %.3g" % (name, on, off, float((a - b).abs().max()), scale))
        assert on <= 2e-4 * scale, (name, on, scale)
        if off <= 2e-4 * scale:
            assert float((a - b).abs().max()) <= 2e-4 * scale, (name, float((a - b).abs().max()), scale)
            agree += 1
        seen += "encoder.conv" in name
    assert seen == 8 and agree >= sum(g is not None for g in ga) - 2          # (all but the two conv2.bias gradients)
    stats = player.optimize(None, opt, player.model, -1, dev)
    assert all(torch.isfinite(s).all() for s in stats)
    it = PipelinedIteration(player, opt, args)
    assert it.serial
    for _ in range(3):
        it.run()
    it.finish()
    torch.cuda.synchronize()
    assert it.serial and torch.isfinite(opt.bucket.flat).all()
    player.env.close()
