#!/usr/bin/env python
"""The measurement of profiles/ego.txt (include/atr_ego.h): what the two egocentric launches cost next to the field-of-view launch
and the env step, and what --egocentric costs a training iteration.

    python tools/ego_bench.py [num_envs] [num_steps] [all | launch | iteration]
                                                                    (default: 4096 envs x 20 steps, the headline shape, both parts)

Part 1, the launches. A Track2D-BlockPartialPZR-v0 shard is brought into mid-episode states by 300 random steps; its raw
observation (uint8 and float32, [N, 2, 13, 13]) is the input. Graphs of 10 launches each are replayed (the method of
tools/occlusion_bench.py, whose helpers this file uses: 5 warm-up replays, 7 regions of 20 replays between two device events, the
median region over its launches): atr_ego_windows in place, both dtypes, with every heading turned (headings drawn from 1 .. 3:
every window is read and written) and with every heading NONE (the waves end after the turn), no actions and no done flags so that
the headings stand from launch to launch; atr_ego_actions on int64 actions; atr_fov_windows in place at 90 degrees on the same
windows; and t2d_step_u8 of the same handle. One launch is checked against the out-of-place form before anything is timed; the
numpy rule is the tests' business.

Part 2, the iteration. train.GraphedIteration (the synchronous schedule) at the given shape, three shards one after the other:
--egocentric; no egocentric view with the env step kept out of the policy step's last launch (the path --egocentric takes: the
difference to the first line is the two launches alone); and the default fused path, for context."""
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
    from active_tracking_rl_amd import ego, fov
    from active_tracking_rl_amd.environment import VecEnv
    env = VecEnv(ENV_ID, n, device=DEV, seed=1, obs_u8=True)
    env.reset()
    env.core.step_random(300, action_seed=5)
    env.flush()
    raw_f = env.core.observe()
    raw_b = raw_f.to(torch.uint8)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    acts = torch.randint(0, 4, (2, n), device=DEV, generator=gen)
    a0, a1 = acts[0], acts[1]
    bufs = env.core.step_u8(a0, a1)
    done = bufs[2].clone()
    turned = torch.randint(1, 4, (n, 2), device=DEV, generator=gen).to(torch.uint8)
    none = torch.full((n, 2), ego.NONE, dtype=torch.uint8, device=DEV)
    graphs = []           # (name, graph, tensors): the tensors a graph addresses are kept for as long as the graph is
    for name, raw in (("uint8", raw_b), ("float32", raw_f)):
        work, out, f2 = raw.clone(), torch.empty_like(raw), turned.clone()
        ego.turn_(work, turned)
        ego.ego_windows(raw.data_ptr(), out.data_ptr(), raw.dtype == torch.uint8, n, 2, 338, 169, f2.data_ptr(), None, None, 0, None, 3,
                        ob._stream())
        torch.cuda.synchronize()
        if not torch.equal(out, work) or not torch.equal(turned, f2):
            raise RuntimeError("in place and out of place disagree (%s): nothing is timed" % name)
        moved = int((work != raw).sum())
        print("%s, %d envs x 2 windows (%s, mid-episode states), headings 1 .. 3: %d of %d cells changed (%.1f %%)"
              % (ENV_ID, n, name, moved, raw.numel(), 100.0 * moved / raw.numel()), flush=True)
        graphs.append(("atr_ego_windows %s, in place, every heading turned" % name,
                       ob._graph(lambda work=work: ego.turn_(work, turned)), (work, turned)))
        still = raw.clone()
        graphs.append(("atr_ego_windows %s, in place, every heading NONE" % name,
                       ob._graph(lambda still=still: ego.turn_(still, none)), (still, none)))
        cone, facing = raw.clone(), turned.clone()
        graphs.append(("atr_fov_windows %s, in place, aperture 90" % name,
                       ob._graph(lambda cone=cone, facing=facing: fov.restrict_(cone, facing, (a0, a1), done, (90, 90))), (cone, facing)))
    absolute = torch.empty_like(acts)
    graphs.append(("atr_ego_actions int64, both players",
                   ob._graph(lambda: ego.to_absolute((a0, a1), turned, 3, (absolute[0], absolute[1]))), (absolute,)))
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
    for name, egocentric, unfuse in (("--egocentric", True, False),
                                     ("no egocentric view, env step in a launch of its own", None, True),
                                     ("no egocentric view, fused env step (the default path)", None, False)):
        args = default_args(env=ENV_ID, num_envs=n, num_steps=steps, seed=1, egocentric=egocentric)
        args.gpu_ids = [0]
        player, opt = make_player(args, dev)
        if unfuse:
            player.env.fused_step_out = lambda out: None        # what an env that declines the fused step answers
        it = GraphedIteration(player, opt, args)
        for _ in range(3):
            it.run()
        med, lo, hi = ob._median_region(it.run, 1, warm=2, regions=7, replays=10)
        fused = bool(player.model.env_step_fused_seen)
        if fused != (egocentric is None and not unfuse) or player.env.core.faults() != 0 or not bool(torch.isfinite(opt.bucket.flat).all()):
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
