"""CPU-side checks of the GRU recurrent cores (maze-gru, tat-maze-gru):
  * the state-dict contract and the golden outputs of the REFERENCE A3C_Dueling.forward(test=True) on deterministic weights
    (tests/golden/model_gru.npz, made by make_golden_gru.py) — the tolerances of tests/test_model.py for the same comparison;
  * model.gru_sequence (ATen fallback, float64) against T masked calls of nn.GRUCell, gradients included;
  * A3C_Dueling.forward_sequence of both GRU nets against T calls of forward()-equivalent stepping;
  * include/atr_gru.h against the built library and fused.GRU_PROTOTYPES (the parsing of tests/test_abi_cpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import GOLDEN, ROOT
from test_abi_cpu import _header_functions, _py_class
from active_tracking_rl_amd import model as M
from active_tracking_rl_amd.environment import _spaces
from active_tracking_rl_amd.model import build_model
from active_tracking_rl_amd.train import default_args

NETS = ("tat-maze-gru", "maze-gru")
TOL = dict(atol=2e-5, rtol=1e-5)


def det_weights(shape, k):
    n = int(np.prod(shape))
    fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else int(shape[0])
    w = np.sin(np.arange(n, dtype=np.float64) * 0.7391 + 0.1 * k) / np.sqrt(max(fan_in, 1))
    return w.astype(np.float32).reshape(shape)


def _model(net, seed=0):
    obs, act = _spaces()
    args = default_args(network=net, aux="reward" if "tat" in net else "none")
    torch.manual_seed(seed)
    return build_model(obs, act, args, torch.device("cpu")), args


def load_det_weights(m):
    sd = m.state_dict()
    for k, name in enumerate(sorted(sd.keys())):
        sd[name].copy_(torch.from_numpy(det_weights(tuple(sd[name].shape), k)))
    return m


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "model_gru.npz"))


@pytest.mark.parametrize("net", NETS)
def test_state_dict_contract_and_reference_outputs(golden, net):
    g = golden
    m, _ = _model(net)
    sd = m.state_dict()
    keys = sorted(sd.keys())
    assert keys == [str(k) for k in g[net + "/keys"]]
    assert [str(tuple(sd[k].shape)) for k in keys] == [str(s) for s in g[net + "/shapes"]]
    assert sum(v.numel() for v in sd.values()) == int(g[net + "/n_params"])
    assert tuple(sd["player0.lstm.weight_ih"].shape) == (384, 256) and tuple(sd["player0.lstm.weight_hh"].shape) == (384, 128)
    assert tuple(sd["player1.lstm.bias_ih"].shape) == (384,) and tuple(sd["player1.lstm.bias_hh"].shape) == (384,)
    # the names are the LSTM net's (the module is still called `lstm`); every bias starts at zero
    assert keys == sorted(_model(net.replace("gru", "lstm"))[0].state_dict().keys())
    for name, p in m.named_parameters():
        if name.endswith("bias") or "bias_" in name:
            assert float(p.detach().abs().max()) == 0.0, name
    load_det_weights(m)
    m.eval()
    states = torch.from_numpy(g[net + "/states"])
    hx, cx = torch.from_numpy(g[net + "/hx"]), torch.from_numpy(g[net + "/cx"])
    with torch.no_grad():
        v, a, e, lp, (h, c), rp = m((states, (hx, cx)), True)                 # batched layout, N = 6
    np.testing.assert_allclose(v.numpy(), g[net + "/values"], **TOL)
    np.testing.assert_allclose(e.numpy(), g[net + "/entropies"], **TOL)
    np.testing.assert_allclose(lp.numpy(), g[net + "/log_probs"], **TOL)
    np.testing.assert_allclose(h.numpy(), g[net + "/hx_out"], **TOL)
    assert np.array_equal(c.numpy(), g[net + "/cx"]) and np.array_equal(g[net + "/cx_out"], g[net + "/cx"])   # cx untouched
    assert np.array_equal(torch.stack(a, 1).numpy(), g[net + "/actions"])
    if "tat" in net:
        np.testing.assert_allclose(rp.numpy().reshape(-1), g[net + "/r_pred"].reshape(-1), **TOL)
    else:
        assert rp == 0
    with torch.no_grad():                                                      # the reference's own one-env layout
        v1, a1, _, _, (h1, c1), _ = m((states[2], (hx[2], cx[2])), True)
    assert v1.shape == (2, 1) and h1.shape == (2, 128) and c1.shape == (2, 128)
    assert [int(x) for x in a1] == g[net + "/actions"][2].tolist()
    np.testing.assert_allclose(v1.numpy(), g[net + "/values"][2], **TOL)


def test_names_with_neither_core_are_refused_and_the_model_says_it_is_not_cacheable():
    obs, act = _spaces()
    with pytest.raises(NotImplementedError):
        build_model(obs, act, default_args(network="tat-maze-rnn"), torch.device("cpu"))
    assert _model("maze-gru")[0].cacheable_core is False and _model("tat-maze-lstm")[0].cacheable_core is True
    m = _model("tat-maze-gru")[0]
    assert isinstance(m.player0.lstm, nn.GRUCell) and isinstance(m.player1.lstm, nn.GRUCell)
    assert m.new_cache(5, torch.zeros(4, 2, 1, 1, 13, 13)) is None


@pytest.mark.parametrize("P", (1, 2))
def test_gru_sequence_float64_matches_masked_grucell_calls(P):
    T, N, Fd, R = 4, 5, 12, 8
    torch.manual_seed(3 + P)
    cells = [nn.GRUCell(Fd, R).double() for _ in range(P)]
    feats = torch.randn(T, P, N, Fd, dtype=torch.float64, requires_grad=True)
    h0 = torch.randn(P, N, R, dtype=torch.float64, requires_grad=True)
    c0 = torch.randn(P, N, R, dtype=torch.float64)
    keep = torch.ones(T, N, dtype=torch.float64)
    keep[0, 1] = 0; keep[0, 3] = 0; keep[2, 0] = 0; keep[2, 3] = 0; keep[T - 1, 2] = 0; keep[T - 1, 4] = 0
    go = torch.randn(T, P, N, R, dtype=torch.float64)
    gh = torch.randn(P, N, R, dtype=torch.float64)
    params = [p for c in cells for p in c.parameters()]

    def reference():
        h, c, outs = list(h0.unbind(0)), c0.clone(), []
        for t in range(T):
            step = [cells[p](feats[t, p], h[p]) for p in range(P)]
            outs.append(torch.stack(step, 0))
            h = [s * keep[t].unsqueeze(1) for s in step]
            c = c * keep[t].view(1, N, 1)
        return torch.stack(outs, 0), torch.stack(h, 0), c

    def grads(fn):
        h_seq, h, c = fn()
        if isinstance(h_seq, (list, tuple)):
            h_seq = torch.stack(list(h_seq), 1)
        loss = (h_seq * go).sum() + (h * gh).sum()
        return (h_seq, h, c), torch.autograd.grad(loss, [feats, h0] + params)

    for list_form in (False, True):
        f_in = [feats[:, p] for p in range(P)] if list_form else feats
        (hs_a, h_a, c_a), g_a = grads(lambda: M.gru_sequence(cells, f_in, h0, c0, keep))
        (hs_b, h_b, c_b), g_b = grads(reference)
        assert hs_a.shape == (T, P, N, R) and h_a.shape == (P, N, R)
        for x, y in [(hs_a, hs_b), (h_a, h_b), (c_a, c_b)] + list(zip(g_a, g_b)):
            assert float((x - y).abs().max()) <= 1e-12
    # env 2 ended at the last step: its final h is zero; c is zero wherever any step ended an episode, else untouched
    assert float(h_a[:, 2].abs().max()) == 0.0 and float(c_a[:, [0, 1, 2, 3, 4]].abs().max()) == 0.0
    keep1 = torch.ones(T, N, dtype=torch.float64)
    assert torch.equal(M.gru_sequence(cells, feats, h0, c0, keep1)[2], c0)


@pytest.mark.parametrize("net", NETS)
def test_forward_sequence_matches_stepping_forward(net):
    """A3C_Dueling.forward_sequence (float32, ATen fallback on the CPU) = T calls of forward() with the stored actions and the
    mask applied after each step, as Agent.action_train steps."""
    T, N, R = 4, 5, 128
    m, _ = _model(net)
    load_det_weights(m)
    rs = np.random.RandomState(11)
    states = torch.from_numpy(rs.choice([0, 1, 2, 4], size=(T, N, 2, 1, 1, 13, 13)).astype(np.float32))
    actions = torch.from_numpy(rs.randint(0, 4, size=(T, N, 2)).astype(np.int64))
    hx = torch.from_numpy(rs.randn(N, 2, R).astype(np.float32) * 0.3)
    cx = torch.zeros(N, 2, R)
    keep = torch.ones(T, N)
    keep[0, 1] = 0; keep[1, 3] = 0; keep[T - 1, 0] = 0
    with torch.no_grad():
        values, entropies, log_probs, preds = m.forward_sequence(states, actions, hx, cx, keep)
        p0, p1 = m.player0, m.player1
        h = hx
        for t in range(T):
            h0 = p0.lstm(p0.encoder(states[t, :, 0]), h[:, 0])
            if m.tat:
                x1 = states[t].reshape(N, -1, 1, 13, 13)
                f1 = p1.encoder(x1) + p1.fc_action_tracker(F.one_hot(actions[t, :, 0], 4).float())
            else:
                f1 = p1.encoder(states[t, :, 1])
            h1 = p1.lstm(f1, h[:, 1])
            for p, (pl, hp) in enumerate(((p0, h0), (p1, h1))):
                np.testing.assert_allclose(values[t, :, p].numpy(), pl.critic(hp).numpy(), **TOL)
                ent, lp = M.policy_stats(pl.actor.actor_linear(hp), actions[t, :, p])
                np.testing.assert_allclose(entropies[t, :, p].numpy(), ent.numpy(), **TOL)
                np.testing.assert_allclose(log_probs[t, :, p].numpy(), lp.numpy(), **TOL)
            if m.tat:
                np.testing.assert_allclose(preds[t].numpy(), p1.reward_aux(h1).numpy(), **TOL)
            h = torch.stack([h0, h1], 1) * keep[t].view(N, 1, 1)
    # one player alone: the same recurrence, final state back (c passed through, masked)
    with torch.no_grad():
        v, e, l, (hT, cT) = m.player0.forward_sequence(states[:, :, 0], actions[:, :, 0], hx[:, 0], torch.ones(N, R), keep)
    np.testing.assert_allclose(v.numpy(), values[:, :, 0].numpy(), **TOL)
    np.testing.assert_allclose(hT.numpy(), h[:, 0].numpy(), **TOL)
    assert np.array_equal(cT.numpy(), keep.prod(0).view(N, 1).expand(N, R).numpy())


def _gru_header():
    """include/atr_gru.h without comments and preprocessor lines."""
    txt = open(os.path.join(ROOT, "include", "atr_gru.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    return "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", txt).split("\n") if not ln.lstrip().startswith("#"))


def test_gru_header_library_and_prototype_table_agree():
    from active_tracking_rl_amd import build, fused, vec_env
    build.build()
    assert os.path.join("..", "..", "include", "atr_gru.h") in build.HEADERS and "gru_hip.hip" in build.SOURCES
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    funcs = _header_functions(_gru_header())
    assert sorted(funcs) == sorted(fused.GRU_PROTOTYPES) == ["atr_gru_bptt", "atr_gru_cell_backward", "atr_gru_cell_forward"]
    for name, (res, params) in funcs.items():
        assert hasattr(lib, name), name
        restype, argtypes = fused.GRU_PROTOTYPES[name]
        assert _py_class(restype) == res == ctypes.c_int, name
        assert len(argtypes) == len(params), name
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _py_class(a) == c, (name, i)
    L = fused.lib()                                      # bound and checked where the policy kernels' entry points are
    for name, (restype, argtypes) in fused.GRU_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
        with pytest.raises(RuntimeError, match=r"^%s failed \(-1\)$" % name):
            f.errcheck(-1, None, ())
    assert not set(fused.GRU_PROTOTYPES) & set(fused.ATR_PROTOTYPES)
