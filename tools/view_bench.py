#!/usr/bin/env python
"""The measurement of profiles/view.txt (include/atr_view.h): what one atr_view_rgb and one atr_view_cells launch cost next to
t2d_render_rgb and t2d_render_cells of the same build.

    python tools/view_bench.py [num_envs] [scale]                                   (default: 256 envs, scale 4)

A Track2D-BlockPartialPZR-v0 shard with views (no in-launch auto-reset) is brought into mid-episode states by 64 real steps under
random actions and occluded, so that the windows hold 5s; a twin shard of the same seed with episode traces takes the same steps
for the renderer. For count 4 and count 64 (the first ids of the shard) graphs of 10 launches each are replayed (the method of
tools/occlusion_bench.py, whose helpers this file uses: 5 warm-up replays, 7 regions of 20 replays between two device events, the
median region over its launches): atr_view_rgb on uint8 and float32 windows, both viewers, the tracker's window turned and not;
t2d_render_rgb with the trace; atr_view_cells and t2d_render_cells likewise. The bytes a launch stores and the rate that makes
are printed with every line. The numpy rule is the tests' business."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tools")):
    if path not in sys.path:
        sys.path.insert(0, path)

import torch

import occlusion_bench as ob

DEV, ENV_ID, LAUNCHES = ob.DEV, ob.ENV_ID, ob.LAUNCHES
COUNTS = (4, 64)


def main(n=256, scale=4):
    from active_tracking_rl_amd import occlusion, view
    from active_tracking_rl_amd.environment import VecEnv
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    env = VecEnv(ENV_ID, n, device=DEV, seed=1, views=True, auto_reset=False)
    twin = VecEnv(ENV_ID, n, device=DEV, seed=1, traces=True)
    env.reset()
    twin.reset()
    for _ in range(64):
        acts = torch.randint(0, 4, (2, n), device=DEV, generator=gen)
        env.step([acts[0], acts[1]])
        twin.step([acts[0], acts[1]])
    raw_f = env.core.observe().clone()
    occlusion.occlude_(raw_f)
    raw_b = raw_f.to(torch.uint8)
    facing = torch.randint(0, 4, (n, 2), device=DEV, generator=gen).to(torch.uint8)
    torch.cuda.synchronize()
    print("%s, %d envs, 64 steps in, occluded: %.1f %% of the window cells read 5; scale %d"
          % (ENV_ID, n, 100.0 * float((raw_b == 5).float().mean()), scale), flush=True)
    graphs = []           # (name, graph, bytes stored per launch, tensors): the tensors a graph addresses are kept with it
    for count in COUNTS:
        ids = torch.arange(count, dtype=torch.int32, device=DEV)
        vp, rp = view.min_pitch(scale), (3 * 162 * scale + 15) // 16 * 16
        vbytes, rbytes = count * 82 * scale * vp, count * 82 * scale * rp
        for name, raw in (("uint8", raw_b), ("float32", raw_f)):
            for viewer, turned in ((0, 0), (1, 0), (0, 1)):
                canvas = torch.empty((count, 82 * scale, vp), dtype=torch.uint8, device=DEV)
                graphs.append(("atr_view_rgb count %d, %s, viewer %d, turned %d" % (count, name, viewer, turned),
                               ob._graph(lambda raw=raw, ids=ids, viewer=viewer, turned=turned, canvas=canvas:
                                         view.view_rgb(raw, env.core, ids, scale=scale, viewer=viewer, facing=facing, turned=turned,
                                                       out=canvas)), vbytes, (canvas, ids)))
        canvas = torch.empty((count, 82 * scale, rp), dtype=torch.uint8, device=DEV)
        graphs.append(("t2d_render_rgb count %d, with the trace" % count,
                       ob._graph(lambda ids=ids, canvas=canvas: twin.core.render_rgb(ids, scale=scale, out=canvas)), rbytes,
                       (canvas, ids)))
        for name, raw in (("uint8", raw_b), ("float32", raw_f)):
            out = (torch.empty((count, 82, 82), dtype=torch.uint8, device=DEV),
                   torch.empty((count, 2, 13, 13), dtype=torch.uint8, device=DEV))
            graphs.append(("atr_view_cells count %d, %s, viewer 0, turned 1, cells and windows" % (count, name),
                           ob._graph(lambda raw=raw, ids=ids, out=out: view.view_cells(raw, env.core, ids, facing=facing, turned=1,
                                                                                       out=out)), count * (6724 + 338), (out, ids)))
        out = (torch.empty((count, 82, 82), dtype=torch.uint8, device=DEV),
               torch.empty((count, 13, 13), dtype=torch.uint8, device=DEV))
        graphs.append(("t2d_render_cells count %d, with the trace, cells and window" % count,
                       ob._graph(lambda ids=ids, out=out: twin.core.render_cells(ids, out=out)), count * (6724 + 169), (out, ids)))
    for round_ in range(2):        # (the same graphs again: the spread between two rounds of one run)
        for name, g, nbytes, _ in graphs:
            med, lo, hi = ob._median_region(g.replay, LAUNCHES)
            print("round %d, graph of %d launches: %s %.2f us per launch (regions %.2f .. %.2f), %d bytes stored, %.1f GB/s"
                  % (round_, LAUNCHES, name, med, lo, hi, nbytes, nbytes / med * 1e-3), flush=True)
    if env.core.faults() != 0 or twin.core.faults() != 0:
        raise RuntimeError("the env kernels flagged a fault")
    del graphs
    env.close()
    twin.close()


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
