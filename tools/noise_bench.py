#!/usr/bin/env python
"""The measurement of profiles/noise.txt (include/atr_noise.h): what the sensor-noise launch costs next to the footprint launch,
the field-of-view launch and the env step, and what the noise costs a training iteration.

    python tools/noise_bench.py [num_envs] [num_steps] [all | launch | iteration]
                                                                    (default: 4096 envs x 20 steps, the headline shape, both parts)

Part 1, the launch. A Track2D-BlockPartialPZR-v0 shard is brought into mid-episode states by 64 real steps under random actions.
The input of a timed launch is what the env hands the pass: the windows of the current state, uint8 and float32, ADVANCE mode,
both windows, in place. The clock advances with every launch, so every replay draws afresh and stores what its draws change: at
the rates (0.05, 0.1, 0.1) about one cell in twenty of those that read 0 or 1, and at (ONE, ONE, ONE) every such cell, every
launch (the windows flicker back and forth; the other player, once missed, comes back only as a ghost). How many cells the first
launch changed is printed. Graphs of 10 launches each are replayed (the method of tools/occlusion_bench.py, whose helpers this
file uses: 5 warm-up replays, 7 regions of 20 replays between two device events, the median region over its launches), next to
atr_footprint_windows (K = 4), atr_fov_windows (90 degrees) and t2d_step_u8 of the same build. The numpy rule is the tests'
business.

Part 2, the iteration. train.GraphedIteration (the synchronous schedule) at the given shape, three shards one after the other:
--occlusion with the three rates (0.05, 0.1, 0.1); --occlusion alone (the same unfused path: the difference to the first line is the
noise launch alone); and the default fused path without either, for context."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tools")):
    if path not in sys.path:
        sys.path.insert(0, path)

import torch

import occlusion_bench as ob

DEV, ENV_ID, LAUNCHES = ob.DEV, ob.ENV_ID, ob.LAUNCHES
RATES = dict(flicker=0.05, miss=0.1, ghost=0.1)


def launch_times(n):
    from active_tracking_rl_amd import footprints, fov, noise
    from active_tracking_rl_amd.environment import VecEnv
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    env = VecEnv(ENV_ID, n, device=DEV, seed=1)
    env.reset()
    for _ in range(64):
        acts = torch.randint(0, 4, (2, n), device=DEV, generator=gen)
        env.step([acts[0], acts[1]])
    env.flush()
    raw_f = env.core.observe().clone()
    key = noise.key_of(1)
    done = torch.zeros(n, dtype=torch.uint8, device=DEV)
    graphs = []           # (name, graph, tensors): the tensors a graph addresses are kept for as long as the graph is
    for what, t in (("rates 0.05 / 0.1 / 0.1", noise.thresholds_of(RATES)), ("every threshold ONE", (noise.ONE,) * 3)):
        for name, raw in (("uint8", raw_f.to(torch.uint8)), ("float32", raw_f)):
            work, clock = raw.clone(), noise.new_clock(n, DEV)
            noise.noise_(work, clock, env.core, noise.ADVANCE, key, t, 3)
            torch.cuda.synchronize()
            changed = int((work != raw).sum())
            print("%s, %d envs x 2 windows (%s, %s, 64 steps in): the first launch changed %d of %d cells (%.2f %%)"
                  % (ENV_ID, n, name, what, changed, raw.numel(), 100.0 * changed / raw.numel()), flush=True)
            graphs.append(("atr_noise_windows %s, %s, ADVANCE, both windows, in place" % (name, what),
                           ob._graph(lambda work=work, clock=clock, t=t: noise.noise_(work, clock, env.core, noise.ADVANCE, key, t, 3)),
                           (work, clock)))
    acts = torch.randint(0, 4, (2, n), device=DEV, generator=gen)
    a0, a1 = acts[0], acts[1]
    for name, raw in (("uint8", raw_f.to(torch.uint8)), ("float32", raw_f)):
        trail = footprints.new_trail(n, 4, DEV)
        marked = raw.clone()
        footprints.mark_(marked, trail, env.core, footprints.BEGIN, None, 3)
        graphs.append(("atr_footprint_windows %s, STEP, both windows, K = 4" % name,
                       ob._graph(lambda marked=marked, trail=trail: footprints.mark_(marked, trail, env.core, footprints.STEP, done, 3)),
                       (marked, trail)))
        facing = torch.randint(0, 4, (n, 2), device=DEV, generator=gen).to(torch.uint8)
        cone = raw.clone()
        graphs.append(("atr_fov_windows %s, in place, aperture 90" % name,
                       ob._graph(lambda cone=cone, facing=facing: fov.restrict_(cone, facing, (a0, a1), done, (90, 90))), (cone, facing)))
    if not env.core.supports_u8:
        raise RuntimeError("the shard has no byte step")
    bufs = env.core.step_u8(a0, a1)
    cycle = env.generator_cycle
    after = env.flush if LAUNCHES % cycle != 0 else None
    graphs.append(("t2d_step_u8" + (" + t2d_flush per %d" % LAUNCHES if after else ""),
                   ob._graph(lambda: env.core.step_u8(a0, a1, out=bufs), before=env.flush, after=after), (a0, a1, done) + tuple(bufs)))
    for round_ in range(2):        # (the same graphs again: the spread between two rounds of one run)
        for name, g, _ in graphs:
            print("round %d, graph of %d launches: %s %.2f us per launch (regions %.2f .. %.2f)"
                  % ((round_, LAUNCHES, name) + ob._median_region(g.replay, LAUNCHES)), flush=True)
    if env.core.faults() != 0:
        raise RuntimeError("the env kernels flagged a fault")
    del graphs
    env.close()


def iteration_times(n, steps):
    from active_tracking_rl_amd.train import GraphedIteration, default_args, make_player
    dev = torch.device(DEV)
    for name, kw in (("--occlusion --noise-flicker 0.05 --noise-miss 0.1 --noise-ghost 0.1",
                      dict(occlusion=True, noise_flicker=RATES["flicker"], noise_miss=RATES["miss"], noise_ghost=RATES["ghost"])),
                     ("--occlusion alone (the same unfused path)", dict(occlusion=True)),
                     ("neither, fused env step (the default path)", dict())):
        args = default_args(env=ENV_ID, num_envs=n, num_steps=steps, seed=1, **kw)
        args.gpu_ids = [0]
        player, opt = make_player(args, dev)
        it = GraphedIteration(player, opt, args)
        for _ in range(3):
            it.run()
        med, lo, hi = ob._median_region(it.run, 1, warm=2, regions=7, replays=10)
        fused = bool(player.model.env_step_fused_seen)
        if fused != (not kw) or player.env.core.faults() != 0 or not bool(torch.isfinite(opt.bucket.flat).all()):
            raise RuntimeError("%s: unexpected path (fused env step seen: %s) or a fault" % (name, fused))
        print("synchronous iteration, %d envs x %d steps, %s: %.1f us per iteration (regions %.1f .. %.1f), %.2f M env steps/s"
              % (n, steps, name, med, lo, hi, n * steps / med), flush=True)
        torch.cuda.synchronize()
        del it                  # (the graphs go before the stores they address)
        player.env.close()
        del player, opt
        torch.cuda.empty_cache()


def main(n=4096, steps=20, part="all"):
    if part in ("all", "launch"):
        launch_times(n)
    if part in ("all", "iteration"):
        iteration_times(n, steps)


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]), *sys.argv[3:4])
