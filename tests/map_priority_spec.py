"""Prioritized map replay (include/track2d_bank_prio.h; active_tracking_rl_amd/map_priority.py) in plain Python: what the tests
hold t2d_bank_prio_set_weights, the generator's weighted draw, t2d_bank_prio_score and map_priority.priorities to.

    table   a weight that is NaN, infinite, zero or negative counts as 0; w_max = the largest remaining one; S = (2^31 - 1) // K;
            q_i = 0 or max(1, floor((float64(w_i) / float64(w_max)) * S)); all q_i = 0 -> all 1; cum = running integer sums
    draw    r = bounded(cum[K - 1] - 1) over the words of the episode's MAP stream (map_bank_spec.map_word), idx = #{i : cum[i] <= r};
            K = 1 draws nothing
    score   per env, steps in order: float32 running returns and length; at a done flag the episode's map m receives
            {1, L, L >= success_len, rint(float64(R0) * 65536), rint(float64(R1) * 65536)} — unless the env ends more than 5
            episodes in the call and this one is older than ep_end - 5, or the recorded index is negative: then `unattributed` + 1
    rule    the loops of the module docstring of map_priority.py
"""
import bisect
import math

import numpy as np

import map_bank_spec as bank_spec

FIELDS, RING, KEEP = 5, 8, 5
TOTAL_MAX = 2 ** 31 - 1


def counts(w):
    """Whether a weight takes part: a finite float32 above zero."""
    w = float(np.float32(w))
    return (not math.isnan(w)) and (not math.isinf(w)) and w > 0.0


def quanta(w):
    """q [K] (Python ints) of float32 weights w [K]."""
    w = [np.float32(v) for v in np.asarray(w, np.float32).reshape(-1)]
    K = len(w)
    S = TOTAL_MAX // K
    live = [v for v in w if counts(v)]
    if not live:
        return [1] * K
    w_max = np.float64(max(live))
    q = []
    for v in w:
        if not counts(v):
            q.append(0)
            continue
        ratio = np.float64(v) / w_max                   # one rounding
        q.append(max(1, int(math.floor(ratio * np.float64(S)))))    # a second one, then floor
    return q


def table(w):
    """cum [K] uint32."""
    out, run = [], 0
    for q in quanta(w):
        run += q
        out.append(run)
    assert 1 <= run <= TOTAL_MAX
    return np.array(out, np.uint32)


def draw(cum, seed, genv, ep):
    """The bank index of episode `ep` of global env `genv` under the table `cum`."""
    cum = [int(v) for v in cum]
    if len(cum) == 1:
        return 0
    genv, ep = int(genv) & 0xFFFFFFFF, int(ep) & 0xFFFFFFFF
    r = bank_spec.bounded(lambda i: bank_spec.map_word(seed, genv, ep, i), cum[-1] - 1)[0]
    return bisect.bisect_right(cum, r)                  # = #{i : cum[i] <= r} of a non-decreasing list


def draws(cum, seed, env_id_base, episodes):
    """int32 [N]: draw() for env e in episode episodes[e]."""
    return np.array([draw(cum, seed, int(env_id_base) + e, ep) for e, ep in enumerate(episodes)], np.int32)


def new_carry(n):
    return np.zeros((n, 2), np.float32), np.zeros(n, np.int64)


def score(idx, rew, done, success_len, carry=None, count=None, keep=KEEP):
    """One t2d_bank_prio_score call from a per-step record: idx [T, N] the bank index of the episode each env ran DURING step t
    (what map_index() said before the step), rew [T, N, 2] float32, done [T, N]. Returns (stat [K, 5] of Python ints as an
    object array, unattributed, carry'). carry = (run_ret f32 [N, 2], run_len [N]) continues episodes across calls."""
    idx, rew, done = np.asarray(idx), np.asarray(rew, np.float32), np.asarray(done) != 0
    T, n = done.shape
    K = int(count if count is not None else idx.max() + 1)
    stat = np.zeros((K, FIELDS), object)
    stat[:] = 0
    lost = 0
    run_ret, run_len = new_carry(n) if carry is None else (carry[0].copy(), carry[1].copy())
    for e in range(n):
        d = int(done[:, e].sum())
        ended = 0
        for t in range(T):
            run_ret[e, 0] = np.float32(run_ret[e, 0] + rew[t, e, 0])
            run_ret[e, 1] = np.float32(run_ret[e, 1] + rew[t, e, 1])
            run_len[e] += 1
            if done[t, e]:
                age = d - ended                         # ep_end - ep: 1 for the env's last finished episode
                m = int(idx[t, e])
                if age <= keep and m >= 0:
                    L = int(run_len[e])
                    stat[m, 0] += 1
                    stat[m, 1] += L
                    stat[m, 2] += 1 if L >= success_len else 0
                    stat[m, 3] += int(np.rint(np.float64(run_ret[e, 0]) * 65536.0))
                    stat[m, 4] += int(np.rint(np.float64(run_ret[e, 1]) * 65536.0))
                else:
                    lost += 1
                run_ret[e] = 0.0
                run_len[e] = 0
                ended += 1
    return stat, lost, (run_ret, run_len)


def rule(h, stamp, n, sum_rq, c, t_max, beta, rho, alpha):
    """(h', stamp', w) with loops, in float64 (Python floats): the rule of map_priority.priorities. sum_rq: the role's column."""
    K = len(h)
    h, stamp = [float(v) for v in h], [int(v) for v in stamp]
    for i in range(K):
        if int(n[i]) > 0:
            mean = float(int(sum_rq[i])) / 65536.0 / (float(int(n[i])) * float(t_max))
            m = min(1.0, max(0.0, 0.5 * (1.0 - mean)))
            h[i] = (1.0 - alpha) * h[i] + alpha * m
            stamp[i] = int(c)
    rank = [1 + sum(1 for j in range(K) if h[j] > h[i]) for i in range(K)]
    ps = [math.pow(float(r), -1.0 / beta) for r in rank]
    ps_sum = math.fsum(ps)
    stale = [int(c) - s for s in stamp]
    stale_sum = sum(stale)
    w = []
    for i in range(K):
        p_s = ps[i] / ps_sum
        p_c = stale[i] / float(stale_sum) if stale_sum > 0 else 1.0 / K
        w.append((1.0 - rho) * p_s + rho * p_c)
    return h, stamp, w
