#!/usr/bin/env python
"""The measurement of profiles/sight_stats.txt (include/atr_sight.h): what one atr_sight_stats launch costs next to one
atr_track_stats launch on the same store.

    python tools/sight_stats_profile.py [num_envs] [num_steps]          (default: 4096 envs x 20 steps, the headline shape)

A real rollout store of Track2D-BlockPartialPZR-v0 (uint8 windows): the shard is brought into mid-episode states by 300 random
steps, then num_steps steps under random actions of both players are written into env.rollout_buffers. Three graphs of LAUNCHES
launches each are replayed — the sight statistics alone, the tracking statistics alone (with the actions), and both one after the
other as train.rollout issues them: 5 warm-up replays, then 7 regions of 20 replays each between two device events; the median
region over its launches is the time per launch. Every replay reads the same store, so every launch does the same work (the carry
it starts from differs, the cost does not). The device table of one launch is checked against the host model before anything is
timed, and the flood levels per sample of that store — the PATH histogram's mean and maximum — are printed beside the times."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

DEV = "cuda:0"
LAUNCHES = 10


def _median_region(graph, launches, warm=5, regions=7, replays=20):
    for _ in range(warm):
        graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(regions):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(replays):
            graph.replay()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3 / (replays * launches))
    return float(np.median(times)), float(min(times)), float(max(times))


def _graph(fn):
    fn()                    # (code objects loaded before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(LAUNCHES):
            fn()
    return g


def main(n=4096, steps=20, env_id="Track2D-BlockPartialPZR-v0"):
    from active_tracking_rl_amd import sight_stats, tracking_stats
    from active_tracking_rl_amd.environment import VecEnv
    env = VecEnv(env_id, n, device=DEV, seed=1, obs_u8=True)
    env.reset()
    env.core.step_random(300, action_seed=5)
    env.flush()
    buf = env.rollout_buffers(steps)
    buf[0][0].copy_(env.core.observe().to(torch.uint8).reshape(buf[0][0].shape))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    acts = torch.randint(0, 4, (steps, 2, n), device=DEV, generator=gen)
    for t in range(steps):
        env.step([acts[t, 0], acts[t, 1]], out=(buf[0][t + 1], buf[1][t], buf[2][t]))
    env.flush()
    torch.cuda.synchronize()
    sight = sight_stats.SightStats(env, torch.device(DEV))
    track = tracking_stats.TrackingStats(env, torch.device(DEV))
    act = acts.permute(0, 2, 1)
    sight.update(*buf)
    torch.cuda.synchronize()
    tab = sight.tab.cpu().numpy()
    want = sight_stats.classify(*(b.cpu().numpy() for b in buf), flags=sight.flags)[0]
    if not np.array_equal(tab, want):
        raise RuntimeError("the device table differs from the host model: nothing is timed")
    s = sight_stats.summarize(tab)
    paths = tab[sight_stats.PATH:sight_stats.PATH + 169]
    print("%s, %d envs x %d steps (uint8 store, random actions): %d samples, in view and apart %d, clear %.3f, occluded %.3f, "
          "no path %.3f, out %d, terminal %d; flood levels per sample with a path: mean %.2f, max %d (mean detour %.2f)"
          % (env_id, n, steps, s["samples"], s["apart"], s["sight_clear_rate"], s["occluded_rate"], s["no_path_rate"], s["out"],
             s["terminal"], s["mean_path"], int(np.flatnonzero(paths).max()) if paths.any() else 0, s["mean_detour"]), flush=True)
    g_sight = _graph(lambda: sight.update(*buf))
    g_track = _graph(lambda: track.update(buf[0], buf[1], buf[2], act))
    g_both = _graph(lambda: (track.update(buf[0], buf[1], buf[2], act), sight.update(*buf)))
    for round_ in range(2):        # (the same three graphs again: the spread between two rounds of one run)
        for name, g in (("atr_sight_stats", g_sight), ("atr_track_stats", g_track), ("both, one after the other", g_both)):
            print("round %d, graph of %d launches: %s %.2f us per launch (regions %.2f .. %.2f)"
                  % ((round_, LAUNCHES, name) + _median_region(g, LAUNCHES)), flush=True)
    env.close()


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
