#!/usr/bin/env python
"""The measurement of profiles/rooms.txt (include/track2d.h T2D_MAP_ROOMS; csrc/t2d_device.h gen_rooms): what one generator pass
costs on Rooms maps next to the same pass on Block maps of the same build.

    python tools/rooms_bench.py pass [NUM_ENVS]       reset + generator pass of Track2D-RoomsPartialPZR-v0, -v1 and
                                                      Track2D-BlockPartialPZR-v0 (NUM_ENVS = 4096), two rounds, with the maps'
                                                      free-cell fraction
    python tools/rooms_bench.py heuristic [EPISODES]  the heuristic yardstick: pursuit tracker against the evading target on
                                                      Track2D-BlockPartialPZR-v0 and Track2D-RoomsPartialPZR-v1 (100 episodes)

`pass` is the measurement of tools/map_bank_bench.py: a full t2d_reset of a primed handle is two launches — the reset kernel,
which moves every env into its pre-generated next episode, and the generator pass that refills the N slots just consumed, N whole
episodes (map, free-cell index, spawns, goals, slot store). That pair is captured once and replayed: 20 warm-up replays, then 7
regions of 50 replays between two device events on the launch stream; the median region over its replays is the time per
reset + pass. The reset kernel is the same code for every id, so differences between lines are the pass's."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

DEV = "cuda:0"
IDS = ("Track2D-BlockPartialPZR-v0", "Track2D-RoomsPartialPZR-v0", "Track2D-RoomsPartialPZR-v1")


def one_pass(env_id, n):
    from active_tracking_rl_amd.vec_env import VecTrack2D
    env = VecTrack2D(env_id, num_envs=n, device=DEV, seed=1)
    obs = env.reset()
    env.reset(out=obs)                  # (the captured launches' code objects are loaded)
    torch.cuda.synchronize()
    ep0 = env.get_state()["episode"].copy()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        env.reset(out=obs)
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
    st = env.get_state()
    assert ((st["episode"] - ep0) == 20 + 7 * 50).all() and env.faults() == 0       # every replay started N new episodes
    free = 1.0 - env.get_maps(0, min(n, 256))[:, 1:81, 1:81].mean()
    print("%s, %d envs: %.1f us per reset + generator pass (regions %.1f .. %.1f); free fraction of the interior %.3f"
          % (env_id, n, float(np.median(times)), min(times), max(times), free), flush=True)
    del g
    env.close()


def heuristic(episodes):
    from active_tracking_rl_amd.test import evaluate
    from active_tracking_rl_amd.train import default_args
    dev = torch.device(DEV)
    print("pursuit tracker against the evading target, %d episodes per row: env id | ave eps reward (tracker, target) | "
          "ave eps length | success rate" % episodes)
    for env_id in ("Track2D-BlockPartialPZR-v0", "Track2D-RoomsPartialPZR-v1"):
        args = default_args(env=env_id, env_base=env_id, test_eps=episodes, num_envs=episodes, seed=1)
        rsum, length = evaluate(None, env_id, args, dev, episodes, heuristic_tracker="pursuit", heuristic_target="evade")
        print("%s | %.2f, %.2f | %.1f | %.2f" % (env_id, rsum[:, 0].mean(), rsum[:, 1].mean(), length.mean(),
                                                 float((length >= 500).mean())), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "pass"
    if what == "pass":
        n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
        for _ in range(2):
            for env_id in IDS:
                one_pass(env_id, n)
    elif what == "heuristic":
        heuristic(int(sys.argv[2]) if len(sys.argv) > 2 else 100)
    else:
        sys.exit(__doc__)
