"""The float64 reference of tests/test_lstm_bptt_f64_gpu.py on its own (tests/lstm_bptt_spec.py), no GPU and no project kernel:
without the embedding it is f64_rule.cell_recurrence; its dG explains every other gradient; the stores' slot layout; no reference
tensor of any case is zero; and float32 on the CPU stays under ATEN_MAX (the GPU test asks the same of float32 on the GPU)."""
import pytest
import torch
import torch.nn.functional as F

import f64_rule
import lstm_bptt_spec as spec
from learner_f64 import rel_err

ALL = list(spec.CASES) + list(spec.NODE_CASES)


def _case(name):
    return spec.CASES[name] if name in spec.CASES else spec.NODE_CASES[name]


def test_case_lists_are_the_ones_the_gpu_tests_need():
    shapes = [(c.P, c.T, c.N, c.emb_player) for c in spec.CASES.values()]
    assert shapes == [(1, 1, 1, 0), (1, 1, 16, 0), (2, 2, 17, 1), (2, 3, 15, 1), (2, 7, 37, 1), (2, 2, 130, 0), (2, 1, 2050, 1)]
    cs = list(spec.CASES.values())
    assert {c.no_dh for c in cs} >= {-1, 0, 1} and {c.keep for c in cs} == {"ones", "edges", "dead"}
    assert any(c.actions == 3 and c.n_act == 4 for c in cs) and sum(c.n_act == 8 for c in cs) == 1
    assert sorted((c.N, c.T) for c in spec.NODE_CASES.values()) == [(17, 2), (17, 7), (37, 2), (37, 7)]
    for c in cs + list(spec.NODE_CASES.values()):
        x = spec.inputs(c)
        keep, act = x["keep"], x["store"][:, 0]
        assert int(act.min()) >= 0 and int(act.max()) < min(c.actions, c.n_act)
        if c.keep == "ones":
            assert bool((keep == 1).all())
        else:
            assert keep[c.T - 1, 0] == 0 and keep[0, c.N - 1] == 0 and 0 < float(keep.mean()) < 1
        if c.keep == "dead":
            assert bool((keep[:, c.N // 2] == 0).all())
        if c.actions == 3:
            assert not bool((act == 3).any()) and all(bool((act == k).any()) for k in range(3))


@pytest.mark.parametrize("name", ["2x7x37", "2x2x17", "1x1x16"])
def test_without_the_embedding_it_is_cell_recurrence(name):
    x, case = spec.inputs(_case(name)), _case(name)
    mine = spec.reference(x, torch.float64, "cpu", embed=False)
    gh = torch.zeros(case.P, case.N, spec.R)
    theirs = f64_rule.cell_recurrence(x["cells"], x["feats"], x["h0"], x["c0"], x["keep"], x["go"], gh, torch.float64, "cpu")
    names = ["feats", "h0", "c0", "h_seq"] + ["%s[%d]" % (n, p) for p in range(case.P) for n in spec.PARAMS]
    for n in names:
        assert torch.equal(mine[n], theirs[n]), n
    assert "fa.weight" not in mine


@pytest.mark.parametrize("name", ALL)
def test_dg_explains_every_other_gradient(name):
    """The second evaluation (input projection as a leaf) is the first one: h_seq agrees, and dG gives back nn.LSTMCell's own
    gradients — the features' = dG W_ih, both biases' = dG's column sums, weight_ih's = dG^T (f + E[a]), weight_hh's = dG^T (k h),
    fc_action_tracker's = the by-action sums of dG through W_ih — to float64 round-off."""
    x, ref = spec.problem(name)
    case = x["case"]
    P, T, N = case.P, case.T, case.N
    fwd, dG = ref["fwd"], ref["dG"]
    assert rel_err(fwd["h"].transpose(0, 1), ref["h_seq"]) < 1e-14
    act = x["store"][:, 0]
    tight = lambda a, b, what: rel_err(a, b) < 1e-12 or pytest.fail("%s: %.2e" % (what, rel_err(a, b)))
    for p in range(P):
        if p == case.no_dh:
            assert float(dG[p].abs().max()) == 0.0
            continue
        cell = x["cells"][p]
        w_ih, w_hh = cell.weight_ih.detach().double(), cell.weight_hh.detach().double()
        g2 = dG[p].reshape(T * N, spec.GATES)
        tight(dG[p] @ w_ih, ref["feats"][:, p], "feats")
        tight(g2.sum(0), ref["bias_ih[%d]" % p], "bias_ih")
        tight(g2.sum(0), ref["bias_hh[%d]" % p], "bias_hh")
        xin = x["feats"][:, p].double()
        if p == case.emb_player:
            E = x["fa"].weight.detach().double().t() + x["fa"].bias.detach().double()
            xin = xin + E[act]
            S = spec.by_action(dG[p], act, case.n_act)
            tight((S @ w_ih).t(), ref["fa.weight"], "fa.weight")
            tight((S @ w_ih).sum(0), ref["fa.bias"], "fa.bias")
        tight(g2.t() @ xin.reshape(T * N, -1), ref["weight_ih[%d]" % p], "weight_ih")
        kprev = torch.cat([torch.ones(1, N), x["keep"][:-1]], 0).double().unsqueeze(-1)
        h_prev = torch.cat([x["h0"][p].double().unsqueeze(0), fwd["h"][p, :-1]], 0) * kprev
        tight(g2.t() @ h_prev.reshape(T * N, -1), ref["weight_hh[%d]" % p], "weight_hh")
        tight(dG[p, 0] @ w_hh, ref["h0"][p], "h0")
        # dc0 = dc_0 f_0 and dG_f = dc_0 c0 f_0 (1 - f_0):  dc0 c0 (1 - f_0) = dG_f
        f0 = fwd["gates"][p, 0, :, spec.R:2 * spec.R]
        tight(ref["c0"][p] * x["c0"][p].double() * (1 - f0), dG[p, 0, :, spec.R:2 * spec.R], "c0")


@pytest.mark.parametrize("name", ALL)
def test_store_slots_recompute_the_next_slot(name):
    """Slot t (times keep[t-1] for t > 0) is the state before step t: an nn.LSTMCell step from it, in float64 on the stored float32
    values, reproduces slot t + 1 to float32 rounding; and the same step from the PRE form's stores (pre + bias + emb[a] activated)
    and from the stored gates does too. act is a view of the [T, 2, N] store."""
    x, ref = spec.problem(name)
    case = x["case"]
    P, T, N = case.P, case.T, case.N
    s = spec.stores(x, ref, "cpu")
    assert s["h_all"].shape == s["c_all"].shape == (P, T + 1, N, spec.R) and s["acts"].shape == s["pre"].shape == (P, T, N, spec.GATES)
    assert s["act"].data_ptr() == s["store"].data_ptr() and s["act"].stride(0) == 2 * N and s["emb"].shape == (case.n_act, spec.GATES)
    assert all(t.dtype == torch.float32 for t in (s["h_all"], s["c_all"], s["acts"], s["pre"], s["emb"], s["keep"]) + tuple(s["bias"]))
    assert torch.equal(s["h_all"][:, 0], x["h0"]) and torch.equal(s["c_all"][:, 0], x["c0"])
    E = x["fa"].weight.detach().double().t() + x["fa"].bias.detach().double()
    for p in range(P):
        cell = torch.nn.LSTMCell(spec.FDIM, spec.R).double()
        cell.load_state_dict({k: v.double() for k, v in x["cells"][p].state_dict().items()})
        for t in range(T):
            k = s["keep"][t - 1].double().unsqueeze(1) if t else torch.ones(N, 1, dtype=torch.float64)
            h_prev, c_prev = s["h_all"][p, t].double() * k, s["c_all"][p, t].double() * k
            xin = x["feats"][t, p].double() + (E[s["act"][t]] if p == case.emb_player else 0.0)
            with torch.no_grad():
                h1, c1 = cell(xin, (h_prev, c_prev))
            assert float((h1 - s["h_all"][p, t + 1].double()).abs().max()) < 2e-6, (p, t)
            assert float((c1 - s["c_all"][p, t + 1].double()).abs().max()) < 4e-6, (p, t)
            for form in ("gates", "pre"):
                if form == "gates":
                    i, f, g, o = s["acts"][p, t].double().chunk(4, 1)
                else:
                    a = s["pre"][p, t].double() + s["bias"][p].double()
                    if p == case.emb_player:
                        a = a + s["emb"][s["act"][t]].double()
                    i, f, g, o = a.chunk(4, 1)
                    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
                c2 = f * c_prev + i * g
                h2 = o * torch.tanh(c2)
                assert float((c2 - s["c_all"][p, t + 1].double()).abs().max()) < 4e-6, (form, p, t)
                assert float((h2 - s["h_all"][p, t + 1].double()).abs().max()) < 2e-6, (form, p, t)


@pytest.mark.parametrize("name", ALL)
def test_no_reference_is_zero_and_float32_on_the_cpu_is_close(name):
    """Every float64 reference tensor the GPU tests compare has a norm, per player where they compare per player — but for the
    player whose dL/dh_seq is None (its gradients are exactly zero, and the GPU test asks exactly that of the kernels) and for the
    block of an action no row took (exactly zero too). e(float32 on the CPU) <= ATEN_MAX for each of them."""
    x, ref = spec.problem(name)
    case = x["case"]
    x32 = spec.reference(x, torch.float32, "cpu")
    act = x["store"][:, 0]
    worst = 0.0
    for n, v in sorted(ref.items()):
        if n in ("fwd", "h_seq"):
            continue
        per_player = {"feats": 1, "dG": 0, "h0": 0, "c0": 0}.get(n)
        pieces = [(n, v, x32[n])] if per_player is None else \
            [("%s[%d]" % (n, p), v.select(per_player, p), x32[n].select(per_player, p)) for p in range(case.P)]
        for what, a, b in pieces:
            if case.no_dh >= 0 and what.endswith("[%d]" % case.no_dh):
                assert float(a.abs().max()) == 0.0 and float(b.abs().max()) == 0.0, what
                continue
            assert float(a.norm()) > 0, what
            e = rel_err(b, a)
            worst = max(worst, e)
            assert e <= f64_rule.ATEN_MAX, (what, e)
    if case.n_act == spec.N_ACT:
        S64 = spec.by_action(ref["dG"][case.emb_player], act)
        S32 = spec.by_action(x32["dG"][case.emb_player], act)
        for k in range(spec.N_ACT):
            if not bool((act == k).any()):
                assert float(S64[k].abs().max()) == 0.0
                continue
            assert float(S64[k].norm()) > 0 and rel_err(S32[k], S64[k]) <= f64_rule.ATEN_MAX, k
    print("%s: worst e(float32 on the CPU) %.2e" % (name, worst))
