"""One evaluation round, eager (test.evaluate: Agent.action_test per step) against graphed (evaluator.GreedyEvaluator: the
rollout's kernels in their greedy form, a --num-steps chunk captured per round and replayed), in one process.

  python tools/eval_bench.py [--episodes 100 1024] [--env Track2D-BlockPartialNav-v0] [--rounds 5] [--out FILE]

Per episode count: one warm-up round of each path (code objects, library plans, the evaluator's throw-away warm-up chunk), then
`--rounds` rounds of each, alternating, each timed with a host clock around the whole call (env shard creation, reset, capture,
replays and the final read-back included; the call ends in a device synchronise) and with a pair of HIP events on the current
stream around the same call. Reported: the median of each, the graphed round's capture time separately (median), its replays
and host reads, and the eager / graphed ratio of the wall medians. The policy is build_model's seeded initial weights, the same
object for both paths; both paths run the same episodes (same env ids and seed), so they take the same number of env steps
unless a logit near-tie sends them apart — the steps of each are printed."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from active_tracking_rl_amd import build  # noqa: E402


def timed(fn, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return out, (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="Track2D-BlockPartialNav-v0")
    ap.add_argument("--episodes", type=int, nargs="*", default=[100, 1024])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--num-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    from active_tracking_rl_amd.environment import _spaces
    from active_tracking_rl_amd.evaluator import GreedyEvaluator
    from active_tracking_rl_amd.model import build_model
    from active_tracking_rl_amd.test import evaluate
    from active_tracking_rl_amd.train import default_args
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    lines = ["eval_bench: %s, %s, torch %s, median of %d rounds after one warm-up round per path, times in ms"
             % (a.env, torch.cuda.get_device_name(0), torch.__version__, a.rounds)]
    for episodes in a.episodes:
        args = default_args(env=a.env, env_base=a.env, test_eps=episodes, num_steps=a.num_steps)
        torch.manual_seed(args.seed)
        model = build_model(*_spaces((13, 13)), args, dev).to(dev)
        stats = {}

        def eager():
            return evaluate(model, a.env, args, dev, episodes)

        def graphed():
            ev = GreedyEvaluator(model, a.env, args, dev, episodes)
            out = ev.run()
            stats.update(ev.stats)
            return out

        res = {"eager": [], "graphed": []}
        cap, extra = [], {}
        for r in range(a.rounds + 1):
            for name, fn in (("eager", eager), ("graphed", graphed)):
                (rsum, length), wall, evt = timed(fn, dev)
                if r == 0:
                    if name == "graphed":
                        extra["first_round_ms"], extra["warmup_ms"] = wall, stats["warmup_s"] * 1e3
                    continue
                res[name].append((wall, evt))
                extra[name + "_steps"] = int(length.max())
                extra[name + "_mean_len"] = float(length.mean())
                if name == "graphed":
                    cap.append(stats["capture_s"] * 1e3)
        med = lambda xs: statistics.median(xs)
        we, wg = med([w for w, _ in res["eager"]]), med([w for w, _ in res["graphed"]])
        ee, eg = med([e for _, e in res["eager"]]), med([e for _, e in res["graphed"]])
        lines += [
            "episodes %d  (longest episode: eager %d steps, graphed %d; mean length %.1f / %.1f)"
            % (episodes, extra["eager_steps"], extra["graphed_steps"], extra["eager_mean_len"], extra["graphed_mean_len"]),
            "  eager    round  wall %8.2f  events %8.2f   (min %.2f max %.2f)   %.3f ms per env step of the longest episode"
            % (we, ee, min(w for w, _ in res["eager"]), max(w for w, _ in res["eager"]), we / max(extra["eager_steps"], 1)),
            "  graphed  round  wall %8.2f  events %8.2f   (min %.2f max %.2f)   of which capture %.2f; %d replays of %d steps, %d host reads"
            % (wg, eg, min(w for w, _ in res["graphed"]), max(w for w, _ in res["graphed"]), med(cap), stats["replays"],
               a.num_steps, stats["host_reads"]),
            "  graphed  first round of the process (with the one-off warm-up chunk, %.2f) %.2f" % (extra["warmup_ms"],
                                                                                                 extra["first_round_ms"]),
            "  eager / graphed (wall medians, capture included): %.2fx" % (we / wg),
        ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
