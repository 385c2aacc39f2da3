"""What the CPU and GPU tests of the tracking statistics share: the classification of include/atr_track_stats.h written one env
and one step at a time, the bin a pair of true positions belongs to, and synthetic rollout stores that hold every kind of sample
— a target in view at every offset, out of view, co-located, and each inconsistent form."""
import numpy as np

WINDOW, CENTRE, OUT, TERMINAL, INCONSISTENT, SAMPLES, HIST = 169, 84, 169, 170, 171, 172, 176
ACT_ROWS, MAX_ACTIONS = 170, 8
KINDS = ("seen", "out", "colocated", "two_fours", "no_mirror", "wrong_centre", "one_with_target")


def bin_of_positions(pos):
    """pos int [..., 2, 2] (agent, (row, column)) -> the bin of the target's offset from the tracker."""
    pos = np.asarray(pos, np.int64)
    dr, dc = pos[..., 1, 0] - pos[..., 0, 0], pos[..., 1, 1] - pos[..., 0, 1]
    inside = (np.abs(dr) <= 6) & (np.abs(dc) <= 6)
    return np.where(inside, (dr + 6) * 13 + dc + 6, OUT).astype(np.int32)


def loop_model(obs, rew, done, act=None, carry=None, flags=0, n_actions=4):
    """The header's per-env walk, one sample at a time. -> (hist, act_hist, carry, bins [T, N])."""
    obs, rew, done = np.asarray(obs), np.asarray(rew, np.float32), np.asarray(done)
    T, N = done.shape
    obs = obs.reshape(T + 1, N, 2, WINDOW)
    rew = rew.reshape(T, N, 2)
    hist, act_hist = np.zeros(HIST, np.int64), np.zeros((2, ACT_ROWS, MAX_ACTIONS), np.int64)
    carry = np.full(N, -1, np.int32) if carry is None else np.array(carry, np.int32)
    bins = np.zeros((T, N), np.int32)
    for e in range(N):
        for t in range(T):
            b = int(carry[e])
            if done[t, e] and not flags & 1:
                bin_, carry[e] = TERMINAL, -1
            else:
                w0, w1 = obs[t + 1, e, 0], obs[t + 1, e, 1]
                four, two = np.flatnonzero(w0 == 4), np.flatnonzero(w1 == 2)
                ok = w0[CENTRE] == 2 and w1[CENTRE] == 4
                one = rew[t, e, 0] == np.float32(1.0)
                if ok and one and len(four) == 0 and len(two) == 0:
                    bin_ = CENTRE
                elif ok and not one and len(four) == 1 and len(two) == 1 and two[0] == 168 - four[0]:
                    bin_ = int(four[0])
                elif ok and not one and len(four) == 0 and len(two) == 0:
                    bin_ = OUT
                else:
                    bin_ = INCONSISTENT
                carry[e] = -1 if bin_ == INCONSISTENT or done[t, e] else bin_
            hist[bin_] += 1
            hist[SAMPLES] += 1
            bins[t, e] = bin_
            if act is not None and b >= 0:
                for p in range(2):
                    a = int(np.asarray(act)[t, e, p])
                    if 0 <= a < n_actions:
                        act_hist[p, b, a] += 1
                    else:
                        hist[INCONSISTENT] += 1
    return hist, act_hist, carry, bins


def windows(kind, dr=0, dc=0, rs=None):
    """(obs u8 [2, 169], rew0 f32) of one sample: walls (0 / 1) at random, the agents' own centres, and what `kind` says."""
    rs = rs or np.random.RandomState(0)
    w = (rs.rand(2, WINDOW) < 0.3).astype(np.uint8)
    w[0, CENTRE], w[1, CENTRE] = 2, 4
    at = lambda r, c: (6 + r) * 13 + 6 + c
    d = float(np.hypot(dr, dc))
    rew = np.float32(max(1.0 - 2.0 * d / 6.0, -1.0))
    if kind in ("seen", "two_fours", "no_mirror", "one_with_target"):
        assert (dr, dc) != (0, 0)
        w[0, at(dr, dc)], w[1, at(-dr, -dc)] = 4, 2
    if kind == "out":
        rew = np.float32(-1.0)
    elif kind == "colocated":
        rew = np.float32(1.0)
    elif kind == "two_fours":
        other = at(-dr, -dc) if at(-dr, -dc) != CENTRE else 0
        w[0, other] = 4
    elif kind == "no_mirror":
        w[1, at(-dr, -dc)] = 0
        w[1, at(dr, dc)] = 2                       # a 2, but not at the mirrored cell (dr, dc != 0, 0: another cell)
    elif kind == "wrong_centre":
        w[0, CENTRE] = 0
    elif kind == "one_with_target":
        rew = np.float32(1.0)
    return w, rew


def synthetic_store(T, N, seed, n_actions=4, p_done=0.15, p_bad=0.12):
    """A rollout store with known content: obs u8 [T+1, N, 2, 13, 13], rew f32 [T, N, 2], done u8 [T, N], act i64 [T, N, 2] and
    the kinds [T, N] (indices into KINDS). Offsets sweep the whole window; a share p_bad of the samples takes an inconsistent
    form and about one action in 25 is outside [0, n_actions)."""
    rs = np.random.RandomState(seed)
    obs = np.zeros((T + 1, N, 2, WINDOW), np.uint8)
    rew = (rs.randn(T, N, 2) * 0.3).astype(np.float32)
    kinds = np.zeros((T, N), np.int32)
    obs[0] = windows("out", rs=rs)[0]
    cells = [c for c in range(WINDOW) if c != CENTRE]
    for t in range(T):
        for e in range(N):
            u = rs.rand()
            k = 3 + rs.randint(4) if u < p_bad else 0 if u < p_bad + 0.6 else 1 if u < p_bad + 0.75 else 2
            c = cells[(seed + 31 * t + 7 * e + rs.randint(3)) % len(cells)]
            obs[t + 1, e], rew[t, e, 0] = windows(KINDS[k], c // 13 - 6, c % 13 - 6, rs)
            kinds[t, e] = k
    done = (rs.rand(T, N) < p_done).astype(np.uint8)
    act = rs.randint(0, n_actions, size=(T, N, 2)).astype(np.int64)
    bad = rs.rand(T, N, 2) < 0.04
    act[bad] = rs.choice([-1, n_actions, 8, 1 << 40], size=int(bad.sum()))
    return obs.reshape(T + 1, N, 2, 13, 13), rew, done, act, kinds


def assert_tables_equal(got, want, what=""):
    for name, g, w in zip(("hist", "act_hist", "carry"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and np.array_equal(g.astype(np.int64), w.astype(np.int64)), \
            (what, name, np.argwhere(g.astype(np.int64) != w.astype(np.int64))[:6].tolist())
