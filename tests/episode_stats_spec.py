"""What the CPU and GPU tests of the training-episode statistics share: the accounting written per env in the reference's words
(train.py:63-88: `reward_sum += player.reward`, written and zeroed on `done`; gym_eval.py:110-125: the finished episodes' list,
`eps_len >= 500` a success), synthetic inputs, and the comparison of two sets of accounts bit for bit."""
import numpy as np

FIELDS = 8


def reference_loop(rew, done, success_len, run_ret=None, run_len=None, fin=None):
    """One env at a time, one step at a time. Returns (run_ret f32 [N,2], run_len i32 [N], fin f64 [N,8], episodes): episodes =
    per env the list of (R0, R1, L) of its finished episodes, R0 / R1 the float32 sums as float64."""
    rew, done = np.asarray(rew, np.float32), np.asarray(done)
    T, N = done.shape
    out_ret, out_len = np.zeros((N, 2), np.float32), np.zeros(N, np.int32)
    fin, episodes = (np.zeros((N, FIELDS), np.float64) if fin is None else np.array(fin, np.float64)), []
    for e in range(N):
        reward_sum = np.zeros(2, np.float32) if run_ret is None else np.array(run_ret[e], np.float32)
        eps_len = 0 if run_len is None else int(run_len[e])
        his = []
        for t in range(T):
            reward_sum = (reward_sum + rew[t, e]).astype(np.float32)
            eps_len += 1
            if done[t, e]:
                R0, R1, L = float(reward_sum[0]), float(reward_sum[1]), float(eps_len)
                his.append((R0, R1, eps_len))
                for k, v in enumerate((1.0, R0, R1, R0 * R0, R1 * R1, L, L * L, 1.0 if eps_len >= success_len else 0.0)):
                    fin[e, k] = fin[e, k] + v
                reward_sum = np.zeros(2, np.float32)
                eps_len = 0
        out_ret[e], out_len[e] = reward_sum, eps_len
        episodes.append(his)
    return out_ret, out_len, fin, episodes


def synthetic(T=57, N=19, success_len=23, seed=5):
    """rew [T,N,2] f32, done [T,N] u8 with the cases the accounting must get right: env 0 never finishes, env 1 finishes at step 0,
    env 2 has two dones in consecutive steps, env 3's first episode is exactly success_len long, env 4's success_len - 1."""
    rs = np.random.RandomState(seed)
    rew = (rs.randn(T, N, 2) * np.float32(0.7)).astype(np.float32)
    done = (rs.rand(T, N) < 0.06).astype(np.uint8)
    done[:, 0] = 0
    done[0, 1] = 1
    done[10:12, 2] = 1
    done[:success_len + 3, 3] = 0
    done[success_len - 1, 3] = 1
    done[:success_len + 3, 4] = 0
    done[success_len - 2, 4] = 1
    return rew, done


def random_inputs(T, N, seed, p_done=0.08):
    rs = np.random.RandomState(seed)
    return (rs.randn(T, N, 2) * np.float32(0.5)).astype(np.float32), (rs.rand(T, N) < p_done).astype(np.uint8)


def same_bits(a, b):
    """Equal shape, dtype and bytes (NaN-safe, and -0.0 is not 0.0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_accounts_equal(got, want, what=""):
    for name, g, w in zip(("run_ret", "run_len", "fin"), got, want):
        assert same_bits(np.asarray(g), np.asarray(w)), (what, name, np.argwhere(np.asarray(g) != np.asarray(w))[:6].tolist())
