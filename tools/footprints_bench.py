#!/usr/bin/env python
"""The measurement of profiles/footprints.txt (include/atr_footprints.h): what the footprint launch costs next to the field-of-view
launch, the occlusion launch and the env step, and what --footprints costs a training iteration.

    python tools/footprints_bench.py [num_envs] [num_steps] [all | launch | iteration]
                                                                    (default: 4096 envs x 20 steps, the headline shape, both parts)

Part 1, the launch. A Track2D-BlockPartialPZR-v0 shard is brought into mid-episode states by 300 random steps; its raw observation
(uint8 and float32, [N, 2, 13, 13]) is the input. The trails are filled by 64 more real steps of the env with the pass in STEP mode,
so that they hold what a rollout's would; every timed launch is handed what the env hands it: STEP mode, the step's done flags, both
windows painted. (The positions do not change between the replays of a graph, so after the first one a timed launch records
nothing new and paints cells that already read 6: the loads and the compare are all there, the stores are not. The one launch
before the capture is counted: how many cells it painted is printed.) Graphs of 10 launches each are replayed (the method of
tools/occlusion_bench.py, whose helpers this file uses: 5 warm-up replays, 7 regions of 20 replays between two device events, the
median region over its launches): atr_footprint_windows at K = 4 and K = 63, both dtypes; atr_fov_windows at 90 degrees and
atr_occlude_windows in place on the same windows; and t2d_step_u8 of the same handle. The numpy rule is the tests' business.

Part 2, the iteration. train.GraphedIteration (the synchronous schedule) at the given shape, three shards one after the other:
--footprints 4; no footprints with the env step kept out of the policy step's last launch (the path --footprints takes: the
difference to the first line is the launch alone); and the default fused path, for context."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tools")):
    if path not in sys.path:
        sys.path.insert(0, path)

import torch

import occlusion_bench as ob

DEV, ENV_ID, LAUNCHES = ob.DEV, ob.ENV_ID, ob.LAUNCHES


def launch_times(n):
    from active_tracking_rl_amd import footprints, fov, occlusion
    from active_tracking_rl_amd.environment import VecEnv
    env = VecEnv(ENV_ID, n, device=DEV, seed=1, obs_u8=True)
    env.reset()
    env.core.step_random(300, action_seed=5)
    env.flush()
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    graphs = []           # (name, graph, tensors): the tensors a graph addresses are kept for as long as the graph is
    trails = {k: footprints.new_trail(n, k, DEV) for k in (4, 63)}
    for k, trail in trails.items():
        footprints.mark_(env.core.observe(), trail, env.core, footprints.BEGIN, None, 3)
    for _ in range(64):   # both trails record the same 64 real steps, so both are current when the timing starts
        acts = torch.randint(0, 4, (2, n), device=DEV, generator=gen)
        obs, _, d = env.core.step_u8(acts[0], acts[1])
        for k, trail in trails.items():
            footprints.mark_(obs.clone(), trail, env.core, footprints.STEP, d, 3)
    env.flush()
    raw_f = env.core.observe()
    raw_b = raw_f.to(torch.uint8)
    acts = torch.randint(0, 4, (2, n), device=DEV, generator=gen)
    a0, a1 = acts[0], acts[1]
    done = torch.zeros(n, dtype=torch.uint8, device=DEV)
    for name, raw in (("uint8", raw_b), ("float32", raw_f)):
        for k in (4, 63):
            work, trail = raw.clone(), trails[k].clone()
            footprints.mark_(work, trail, env.core, footprints.STEP, done, 3)
            torch.cuda.synchronize()
            painted = int((work != raw).sum())
            prints = int((trail[:, :, 1:].view(torch.int16) != -1).sum())
            print("%s, %d envs x 2 windows (%s, mid-episode states), K = %d: %d prints held, %d of %d cells painted (%.2f %%)"
                  % (ENV_ID, n, name, k, prints, painted, raw.numel(), 100.0 * painted / raw.numel()), flush=True)
            graphs.append(("atr_footprint_windows %s, STEP, both windows, K = %d" % (name, k),
                           ob._graph(lambda work=work, trail=trail: footprints.mark_(work, trail, env.core, footprints.STEP, done, 3)),
                           (work, trail)))
        facing = torch.randint(0, 4, (n, 2), device=DEV, generator=gen).to(torch.uint8)
        cone = raw.clone()
        graphs.append(("atr_fov_windows %s, in place, aperture 90" % name,
                       ob._graph(lambda cone=cone, facing=facing: fov.restrict_(cone, facing, (a0, a1), done, (90, 90))), (cone, facing)))
        occ = raw.clone()
        graphs.append(("atr_occlude_windows %s, in place" % name, ob._graph(lambda occ=occ: occlusion.occlude_(occ)), (occ,)))
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
    for name, k, unfuse in (("--footprints 4", 4, False), ("no footprints, env step in a launch of its own", None, True),
                            ("no footprints, fused env step (the default path)", None, False)):
        args = default_args(env=ENV_ID, num_envs=n, num_steps=steps, seed=1, footprints=k)
        args.gpu_ids = [0]
        player, opt = make_player(args, dev)
        if unfuse:
            player.env.fused_step_out = lambda out: None        # what an env that declines the fused step answers
        it = GraphedIteration(player, opt, args)
        for _ in range(3):
            it.run()
        med, lo, hi = ob._median_region(it.run, 1, warm=2, regions=7, replays=10)
        fused = bool(player.model.env_step_fused_seen)
        if fused != (k is None and not unfuse) or player.env.core.faults() != 0 or not bool(torch.isfinite(opt.bucket.flat).all()):
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
