#!/usr/bin/env python
"""The measurement of profiles/memory.txt (include/atr_memory.h): what the map-memory launch costs next to the footprint launch, the
field-of-view launch, the occlusion launch and the env step, and what --map-memory costs a training iteration.

    python tools/memory_bench.py [num_envs] [num_steps] [all | launch | iteration]
                                                                    (default: 4096 envs x 20 steps, the headline shape, both parts)

Part 1, the launch. Two Track2D-BlockPartialPZR-v0 shards, one with --occlusion and one with a 90-degree cone, both with map memory
for both players, are brought into mid-episode states by 64 real steps under random actions, so that the seen tiles hold what a
rollout's would. The input of a timed launch is what the env hands the pass: the occluded (restricted) windows of the current
state, uint8 and float32, STEP mode, a done-flag array, both players. In place, the first launch paints and every replay after it
finds the windows painted already (the loads, the ballots, the tile and the staging are all there, the window stores are not), so
a second form is timed as well: a copy of the unpainted windows into the work buffer followed by the launch, next to the copy
alone — their difference is a launch that paints every time. How many cells the first launch painted is printed. Graphs of 10
launches each are replayed (the method of tools/occlusion_bench.py, whose helpers this file uses: 5 warm-up replays, 7 regions of
20 replays between two device events, the median region over its launches), next to atr_footprint_windows (K = 4),
atr_fov_windows (90 degrees), atr_occlude_windows and t2d_step_u8 of the same build. The numpy rule is the tests' business.

Part 2, the iteration. train.GraphedIteration (the synchronous schedule) at the given shape, three shards one after the other:
--occlusion --map-memory; --occlusion alone (the same unfused path: the difference to the first line is the launch alone); and
the default fused path without either, for context."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tools")):
    if path not in sys.path:
        sys.path.insert(0, path)

import torch

import occlusion_bench as ob

DEV, ENV_ID, LAUNCHES = ob.DEV, ob.ENV_ID, ob.LAUNCHES


def _shard(n, gen, **kw):
    """(env, its occluded / restricted windows without memory as float32 [N, 2, 13, 13], the seen tiles) after 64 real steps."""
    from active_tracking_rl_amd.environment import VecEnv
    env = VecEnv(ENV_ID, n, device=DEV, seed=1, map_memory="both", **kw)
    env.reset()
    for _ in range(64):
        acts = torch.randint(0, 4, (2, n), device=DEV, generator=gen)
        env.step([acts[0], acts[1]])
    env.flush()
    raw = env._mark(env._restrict(env._occlude(env.core.observe())), env._FP_PEEK).clone()     # (every pass but memory's)
    return env, raw, env._seen


def launch_times(n):
    from active_tracking_rl_amd import footprints, fov, memory, occlusion
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    graphs = []           # (name, graph, tensors): the tensors a graph addresses are kept for as long as the graph is
    envs = []
    done = torch.zeros(n, dtype=torch.uint8, device=DEV)
    for what, kw in (("occlusion-only windows", dict(occlusion=True)), ("90-degree cone windows", dict(fov=90))):
        env, raw_f, seen = _shard(n, gen, **kw)
        envs.append(env)
        for name, raw in (("uint8", raw_f.to(torch.uint8)), ("float32", raw_f)):
            work, tiles = raw.clone(), seen.clone()
            memory.remember_(work, tiles, env.core, memory.STEP, done, 3)
            torch.cuda.synchronize()
            hidden, painted = int((raw == 5).sum()), int((work != raw).sum())
            bits = int(memory.unpack(tiles, env.core.map_side).sum())
            print("%s, %d envs x 2 windows (%s, %s, 64 steps in): %d cells seen, %d of %d cells hidden, %d of them painted (%.2f %% "
                  "of all cells)" % (ENV_ID, n, name, what, bits, hidden, raw.numel(), painted, 100.0 * painted / raw.numel()), flush=True)
            graphs.append(("atr_memory_windows %s, %s, STEP, both players, in place" % (name, what),
                           ob._graph(lambda work=work, tiles=tiles, env=env: memory.remember_(work, tiles, env.core, memory.STEP, done, 3)),
                           (work, tiles)))
            again, tiles2 = raw.clone(), seen.clone()
            graphs.append(("copy of the windows + atr_memory_windows %s, %s (paints every time)" % (name, what),
                           ob._graph(lambda again=again, raw=raw, tiles2=tiles2, env=env:
                                     memory.remember_(again.copy_(raw), tiles2, env.core, memory.STEP, done, 3)), (again, raw, tiles2)))
            alone = raw.clone()
            graphs.append(("copy of the windows alone %s" % name, ob._graph(lambda alone=alone, raw=raw: alone.copy_(raw)), (alone, raw)))
    env = envs[0]
    acts = torch.randint(0, 4, (2, n), device=DEV, generator=gen)
    a0, a1 = acts[0], acts[1]
    raw_f = env.core.observe()
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
        occ = raw.clone()
        graphs.append(("atr_occlude_windows %s, in place" % name, ob._graph(lambda occ=occ: occlusion.occlude_(occ)), (occ,)))
    plain = envs[0]
    if not plain.core.supports_u8:
        raise RuntimeError("the shard has no byte step")
    bufs = plain.core.step_u8(a0, a1)
    cycle = plain.generator_cycle
    after = plain.flush if LAUNCHES % cycle != 0 else None
    graphs.append(("t2d_step_u8" + (" + t2d_flush per %d" % LAUNCHES if after else ""),
                   ob._graph(lambda: plain.core.step_u8(a0, a1, out=bufs), before=plain.flush, after=after), (a0, a1, done) + tuple(bufs)))
    for round_ in range(2):        # (the same graphs again: the spread between two rounds of one run)
        for name, g, _ in graphs:
            print("round %d, graph of %d launches: %s %.2f us per launch (regions %.2f .. %.2f)"
                  % ((round_, LAUNCHES, name) + ob._median_region(g.replay, LAUNCHES)), flush=True)
    if any(e.core.faults() != 0 for e in envs):
        raise RuntimeError("the env kernels flagged a fault")
    del graphs
    for e in envs:
        e.close()


def iteration_times(n, steps):
    from active_tracking_rl_amd.train import GraphedIteration, default_args, make_player
    dev = torch.device(DEV)
    for name, kw in (("--occlusion --map-memory", dict(occlusion=True, map_memory=True)),
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
