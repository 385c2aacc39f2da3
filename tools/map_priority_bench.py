#!/usr/bin/env python
"""The measurements of profiles/map_priority.txt (include/track2d_bank_prio.h): what prioritized map replay costs where it runs.

    python tools/map_priority_bench.py gen ENV_ID NUM_ENVS BANK_MAPS {random,prio}    reset + generator pass, replayed in a graph
    python tools/map_priority_bench.py score NUM_ENVS NUM_STEPS                       one t2d_bank_prio_score next to atr_episode_stats
    python tools/map_priority_bench.py weights BANK_MAPS                              one t2d_bank_prio_set_weights launch

Every figure is a captured graph of the launches named, replayed: 20 warm-up replays, then 7 regions of 50 replays between two
device events on the launch stream; the median region over its replays is the time per replay (tools/map_bank_bench.py's
method). gen: the bank holds the first-episode maps of BANK_MAPS generated envs of the id; 'prio' draws from a skewed table
(weights 1 .. BANK_MAPS). Both variants reset through an all-ones mask: a reset of every env WITHOUT a mask also clears the
score carry of a prioritised handle, one more small launch that no training iteration issues (the auto-reset is in-launch),
and the masked reset keeps it out of the comparison (so these lines are not profiles/map_bank.txt's unmasked ones).
score / weights: a graph of ONE launch measures launch-to-launch time on an otherwise idle stream, which for kernels this short
is mostly the launch itself; the first two score lines are the same store read by the two kernels, so their difference is the
kernels'."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

DEV = "cuda:0"
PZR = "Track2D-BlockPartialPZR-v0"


def replay_time(fn):
    """Median microseconds per replay of the launches fn() issues, and the regions' range."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        fn()
    for _ in range(20):
        g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(7):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(50):
            g.replay()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3 / 50)
    return float(np.median(times)), min(times), max(times)


def bank_env(env_id, n, k, prio, **kw):
    from active_tracking_rl_amd.map_bank import MapBank
    from active_tracking_rl_amd.vec_env import VecTrack2D
    env = VecTrack2D(env_id, num_envs=n, device=DEV, seed=1, **kw)
    env.attach_map_bank(MapBank.from_env(env_id, k, seed=99, device=DEV), "random")
    if prio:
        env.enable_map_priority()
    return env


def gen(env_id, n, k, mode):
    from active_tracking_rl_amd import map_priority as mp
    env = bank_env(env_id, n, k, mode == "prio")
    if mode == "prio":
        w = torch.arange(1, k + 1, dtype=torch.float32, device=DEV)
        mp.lib().t2d_bank_prio_set_weights(env.h, w.data_ptr(), None)
    obs = env.reset()
    everyone = torch.ones(n, dtype=torch.uint8, device=DEV)
    ep0 = env.get_state()["episode"].copy()
    med, lo, hi = replay_time(lambda: env.reset(mask=everyone, out=obs))
    st = env.get_state()
    assert ((st["episode"] - ep0) == 1 + 20 + 7 * 50).all() and env.faults() == 0       # every replay started N new episodes
    if mode == "prio":                                                                  # ... on maps drawn by weight
        idx = env.map_index().cpu().numpy()
        assert idx.min() >= 0 and idx.max() < k and idx.mean() > 0.55 * k
    print("%s, %d envs, bank of %d maps, %s: %.1f us per reset + generator pass (regions %.1f .. %.1f)"
          % (env_id, n, k, "prioritised draw" if mode == "prio" else "--bank-select random", med, lo, hi), flush=True)
    env.close()


def score(n, T):
    from active_tracking_rl_amd import episode_stats as es
    from active_tracking_rl_amd.map_priority import MapPriority
    env = bank_env(PZR, n, 64, True, max_episode_steps=10)
    prio = MapPriority(env, DEV)
    env.reset()
    rs = np.random.RandomState(0)
    rew = torch.as_tensor(rs.uniform(-1, 1, (T, n, 2)).astype(np.float32), device=DEV)
    done = torch.zeros((T, n), dtype=torch.uint8, device=DEV)        # (no done flag: the handle has not stepped, its episodes stand)
    med, lo, hi = replay_time(lambda: prio.update(rew, done))
    print("t2d_bank_prio_score, %d envs x %d steps, no episode ends: %.1f us per launch (regions %.1f .. %.1f)" % (n, T, med, lo, hi),
          flush=True)

    class Shard(object):
        num_envs, core, episode_stats = n, env, None

        def core_max_steps(self):
            return 500
    stats = es.EpisodeStats(Shard(), torch.device(DEV))
    med, lo, hi = replay_time(lambda: stats.update(rew, done))
    print("atr_episode_stats, %d envs x %d steps, the same store: %.1f us per launch (regions %.1f .. %.1f)" % (n, T, med, lo, hi),
          flush=True)
    # with episode ends (two per env, as a 20-step rollout has at most): the ring lookups and five atomic adds per end. The
    # handle's episode counters are moved on by stepping it first, so that the ends fall on episodes the ring still holds.
    acts = torch.zeros(n, dtype=torch.int64, device=DEV)
    for _ in range(30):
        env.step(acts, acts)
    done[T // 2 - 1] = 1
    done[T - 1] = 1
    ep = env.get_state()["episode"]
    assert (ep >= 3).all()
    med, lo, hi = replay_time(lambda: prio.update(rew, done))
    d = prio.drain().cpu().numpy()
    assert d[:-1].reshape(64, 5)[:, 0].sum() + d[-1] == 2 * n * (1 + 20 + 7 * 50) and d[-1] == 0
    print("t2d_bank_prio_score, %d envs x %d steps, two episode ends per env: %.1f us per launch (regions %.1f .. %.1f)"
          % (n, T, med, lo, hi), flush=True)
    env.close()


def weights(k):
    from active_tracking_rl_amd import map_bank, map_priority as mp
    from active_tracking_rl_amd.vec_env import VecTrack2D
    import ctypes as C
    env = VecTrack2D(PZR, num_envs=64, device=DEV, seed=1)
    maps = np.ones((k, 82, 82), np.uint8)
    maps[:, 1:-1, 1:-1] = 0
    map_bank.lib().t2d_map_bank_attach(env.h, maps.ctypes.data_as(C.c_void_p), None, k, 82, 0, None)
    env.enable_map_priority()
    w = torch.as_tensor(np.random.RandomState(0).uniform(0.01, 1, k).astype(np.float32), device=DEV)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    med, lo, hi = replay_time(lambda: mp.lib().t2d_bank_prio_set_weights(env.h, w.data_ptr(), stream()))
    print("t2d_bank_prio_set_weights, %d maps: %.1f us per launch (regions %.1f .. %.1f)" % (k, med, lo, hi), flush=True)
    env.close()


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "gen" and len(sys.argv) == 6 and sys.argv[5] in ("random", "prio"):
        gen(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
    elif what == "score" and len(sys.argv) == 4:
        score(int(sys.argv[2]), int(sys.argv[3]))
    elif what == "weights" and len(sys.argv) == 3:
        weights(int(sys.argv[2]))
    else:
        print(__doc__)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
