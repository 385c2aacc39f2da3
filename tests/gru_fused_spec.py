"""Host models of the GRU cores' fused rollout step (include/atr_gru_step.h; numpy float64 + the cases both test files share).

The step's gate tensor g [N, 4R] = [features | k h_prev] W4^T holds (r_pre, z_pre, ig_n, k hg_n) without bias; with b4 = (b_ir +
b_hr, b_iz + b_hz, b_in, b_hn) and, for the tracker-aware target, the embedding row E4[a_tracker] added:

    r = sigmoid(g_r),  z = sigmoid(g_z),  q = g_q,  n = tanh(g_n + r q),  h' = (1 - z) n + z (k h_prev)

`cell` is that expression and nothing else; the block weight itself comes from the code under test (model.gru_step_consts)."""
import numpy as np
import torch

import draw_spec as ds
import greedy_eval_spec as gs

R, F, A, T = 128, 256, 4, 3
SEED = 11                      # the ActionSampler's seed in the single-launch cases
ENV_IDS = ["Track2D-BlockPartialPZR-v0", "Track2D-BlockPartialRam-v0", "Track2D-BlockPartialNav-v0"]
CELL_TOL = dict(rtol=1e-4, atol=2e-5)       # what tests/test_gru_gpu.py holds the GRU cell kernel to


def cell(g, b4, hp, e4_row=None):
    """g [N, 4R] gate product, b4 [4R], hp [N, R] = k h_prev (masked), e4_row [N, 4R] or None -> (h' [N, R], acts [N, 4R] =
    (r, z, n, q)), float64."""
    pre = np.asarray(g, np.float64) + np.asarray(b4, np.float64)[None, :]
    if e4_row is not None:
        pre = pre + np.asarray(e4_row, np.float64)
    hp = np.asarray(hp, np.float64)
    Rr = hp.shape[1]
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    r, z, q = sig(pre[:, :Rr]), sig(pre[:, Rr:2 * Rr]), pre[:, 3 * Rr:]
    n = np.tanh(pre[:, 2 * Rr:3 * Rr] + r * q)
    return (1.0 - z) * n + z * hp, np.concatenate([r, z, n, q], 1)


def launch_case(n, tat, seed=0):
    """The inputs of the single-launch cases, made on the host (the CPU test evaluates the spec alone on them): per step t
    random g [2, n, 4R] and masked previous rows hp [2, n, R] with every fifth row zero (an episode that has just ended), b4
    with a non-zero b_hn block, E4 (tat) and actor heads scaled as tests/test_greedy_eval_gpu.py scales them."""
    gen = torch.Generator().manual_seed(7000 + 10 * n + (3 if tat else 0) + seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    c = dict(w=[rnd(A, R) * 3.0 for _ in range(2)], b=[rnd(A) * 0.1 for _ in range(2)], b4=[rnd(4 * R) * 0.3 for _ in range(2)],
             e4=rnd(A, 4 * R) * 0.5 if tat else None, g=[rnd(2, n, 4 * R) for _ in range(T)], hp=[])
    for t in range(T):
        hp = torch.tanh(rnd(2, n, R))
        hp[:, t::5] = 0.0
        c["hp"].append(hp)
    return c


def step_model(case, t, kind, a_tracker=None, h=None, counter=1, ordinal=1):
    """The spec for step t of a case. Without (a_tracker, h) it runs alone: the tracker's action is the model's own (the draw
    model under (SEED, row, counter, ordinal + p), or the first maximum), and the logits come from the spec's hidden rows. With
    them it is the device check: the target is fed the KERNEL's tracker action, the logits are formed from the kernel's own
    h_out [2, n, R]. Returns per player (h64, acts64, logits64, clear rows, model action)."""
    n = case["g"][t].shape[1]
    out = []
    for p in range(2):
        e4 = None
        if p == 1 and case["e4"] is not None:
            a0 = a_tracker if a_tracker is not None else out[0][4]
            e4 = case["e4"].double().numpy()[np.asarray(a0)]
        h64, acts = cell(case["g"][t][p].numpy(), case["b4"][p].numpy(), case["hp"][t][p].numpy(), e4)
        rows = h64 if h is None else np.asarray(h[p], np.float64)
        logits = ds.head_logits(rows, case["w"][p].numpy(), case["b"][p].numpy())
        if kind == "greedy":
            clear, act = gs.top2_gap(logits) > gs.NEAR_TIE, logits.argmax(1)
        else:
            u = ds.uniform(SEED, np.arange(n), counter, ordinal + p)
            delta = ds.delta_for(logits, rows.astype(np.float32), case["w"][p].numpy(), case["b"][p].numpy())
            clear, act = ~ds.margin(logits, u, delta), ds.draw(logits, u)
        out.append((h64, acts, logits, clear, act))
    return out
