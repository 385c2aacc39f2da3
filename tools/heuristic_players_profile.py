#!/usr/bin/env python
"""The two measurements of profiles/heuristic_players.txt (include/track2d_heuristic.h).

    python tools/heuristic_players_profile.py launch      # (a) one t2d_heuristic_actions launch next to one t2d_step
    python tools/heuristic_players_profile.py baseline    # (b) what the pursuit tracker scores

(a) 4096 envs of Track2D-BlockPartialPZR-v0 and of Track2D-MazePartialNav-v0, brought into mid-episode states by 300 random
    steps. A graph of one generator cycle of t2d_step launches (fixed actions; its generator passes included) and a graph of the
    same number of t2d_heuristic_actions launches (both roles, with distances) are replayed: 5 warm-up replays, then 7 regions of
    20 replays each between two device events; the median region over its launches is the time per launch. The heuristic launch
    reads the state the step graphs left behind and changes nothing, so every one of its replays does the same work; the
    distribution of the path distances of that state is printed beside it.
(b) 100 episodes per row through test.evaluate with heuristic_tracker='pursuit' (evaluation env ids, seed 1): the four ids of
    BASELINE.json against the id's own target — scripted for Ram / Nav; for PZR / Adv the target is a policy, here the
    UNTRAINED tat-maze-lstm of seed 1 — and Track2D-BlockPartialPZR-v0 against the evading target, with no model at all."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

DEV = "cuda:0"


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


def launch(n=4096):
    from active_tracking_rl_amd.vec_env import VecTrack2D
    for env_id in ("Track2D-BlockPartialPZR-v0", "Track2D-MazePartialNav-v0"):
        env = VecTrack2D(env_id, num_envs=n, device=DEV, seed=1)
        env.reset()
        env.step_random(300, action_seed=5)
        env.flush()
        k = max(1, env.generator_cycle)
        g = torch.Generator().manual_seed(2)
        acts = torch.randint(0, 4, (k, 2, n), generator=g, dtype=torch.int64).to(DEV)
        out = (env._new_obs(), torch.empty((n, 2), device=DEV), torch.empty((n,), dtype=torch.uint8, device=DEV))
        act = torch.zeros((n, 2), dtype=torch.int64, device=DEV)
        dist = torch.zeros((n,), dtype=torch.int32, device=DEV)
        env.step(acts[0, 0], acts[0, 1], out=out)
        env.heuristic_actions(out=act, dist=dist)
        env.flush()
        torch.cuda.synchronize()
        g_step = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_step):
            for i in range(k):
                env.step(acts[i, 0], acts[i, 1], out=out)
        step_us = _median_region(g_step, k)
        g_heur = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_heur):
            for i in range(k):
                env.heuristic_actions(out=act, dist=dist)
        heur_us = _median_region(g_heur, k)
        d = dist.cpu().numpy()
        reach = d[d >= 0]
        print("%s, %d envs, graphs of %d launches: t2d_step %.2f us per launch (regions %.2f .. %.2f), t2d_heuristic_actions "
              "(both roles + dist) %.2f us per launch (regions %.2f .. %.2f); path distance of the state: mean %.1f, median %d, "
              "max %d, no path in %d envs"
              % ((env_id, n, k) + step_us + heur_us + (reach.mean() if reach.size else -1.0, int(np.median(reach)) if reach.size
                                                       else -1, int(reach.max()) if reach.size else -1, int((d < 0).sum()))),
              flush=True)
        del g_step, g_heur
        env.close()


def baseline(episodes=100):
    from active_tracking_rl_amd import registry
    from active_tracking_rl_amd.environment import _spaces
    from active_tracking_rl_amd.model import build_model
    from active_tracking_rl_amd.test import evaluate
    from active_tracking_rl_amd.train import default_args
    dev = torch.device(DEV)
    rows = [(i, None) for i in ("Track2D-BlockPartialRam-v0", "Track2D-BlockPartialPZR-v0", "Track2D-MazePartialNav-v0",
                                "Track2D-BlockPartialAdv-v0")] + [("Track2D-BlockPartialPZR-v0", "evade")]
    print("pursuit tracker, %d episodes per row: env id | target | ave eps reward (tracker, target) | ave eps length | success rate"
          % episodes)
    for env_id, target in rows:
        args = default_args(env=env_id, env_base=env_id, test_eps=episodes, num_envs=episodes, seed=1)
        mode = registry.spec(env_id)["target_mode"]
        model, who = None, "the id's scripted %s target" % mode
        if target == "evade":
            who = "evade"
        elif mode not in ("Ram", "Nav", "RPF"):
            torch.manual_seed(args.seed)
            model = build_model(*_spaces((13, 13)), args, dev).to(dev)
            who = "untrained tat-maze-lstm policy (seed 1)"
        rsum, length = evaluate(model, env_id, args, dev, episodes, heuristic_tracker="pursuit", heuristic_target=target)
        print("%s | %s | %.2f, %.2f | %.1f | %.2f" % (env_id, who, rsum[:, 0].mean(), rsum[:, 1].mean(), length.mean(),
                                                     float((length >= 500).mean())), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "both"
    if what in ("launch", "both"):
        launch()
    if what in ("baseline", "both"):
        baseline()
