#!/usr/bin/env python
"""The measurement of profiles/map_bank.txt (include/track2d_bank.h): what one generator pass costs with a map bank next to the
same pass with the map generators.

    python tools/map_bank_bench.py ENV_ID NUM_ENVS BANK_MAPS [label]        (BANK_MAPS = 0: no bank, generated maps)

A full t2d_reset of a primed handle is two launches: the reset kernel, which moves every env into its pre-generated next episode,
and the generator pass that refills the N slots just consumed — N whole episodes (map, free-cell index, spawns, goals, target
plans, slot store), every wave of the pass at work. That pair is captured once and replayed: 20 warm-up replays, then 7 regions of
50 replays between two device events on the launch stream; the median region over its replays is the time per reset + pass. The
reset kernel is the same code in every variant, so differences between lines are the pass's. The bank holds the first-episode
maps of BANK_MAPS generated envs of the same id (MapBank.from_env), selected at random: maps of the kind the generators make.
T2D_LIB_PATH in the environment selects another build of the library (the parent commit's, for the no-bank line)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

DEV = "cuda:0"


def main():
    env_id, n, k = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    label = sys.argv[4] if len(sys.argv) > 4 else ("bank of %d maps" % k if k else "generated maps")
    from active_tracking_rl_amd.vec_env import VecTrack2D
    env = VecTrack2D(env_id, num_envs=n, device=DEV, seed=1)
    if k:
        from active_tracking_rl_amd.map_bank import MapBank
        env.attach_map_bank(MapBank.from_env(env_id, k, seed=99, device=DEV), "random")
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
    print("%s, %d envs, %s: %.1f us per reset + generator pass (regions %.1f .. %.1f)"
          % (env_id, n, label, float(np.median(times)), min(times), max(times)), flush=True)
    env.close()


if __name__ == "__main__":
    main()
