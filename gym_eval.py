#!/usr/bin/env python
"""gym_eval.py — drop-in for the reference's gym_eval.py (same flags, gym_eval.py:15-37): loads a full / tracker /
target checkpoint (reference names and keys), evaluates `--num-episodes` episodes with the argmax policy and reports
R_mean / R_std / EL_mean / EL_std / S_rate (success = episode length >= 500), optionally appending a CSV row
(gym_eval.py:122-141). The episodes run as one batch on the GPU."""
from __future__ import division
import os
os.environ["OMP_NUM_THREADS"] = "1"
import argparse
import logging

import numpy as np
import torch

from active_tracking_rl_amd import build
from active_tracking_rl_amd.environment import _spaces
from active_tracking_rl_amd.model import build_model
from active_tracking_rl_amd.test import evaluate, per_map_summary
from active_tracking_rl_amd import registry
from active_tracking_rl_amd.utils import check_path, setup_logger

def _noise_rate(text):
    """A sensor-noise rate: a float in [0, 1]."""
    try:
        p = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not a number" % (text,))
    if not 0.0 <= p <= 1.0:
        raise argparse.ArgumentTypeError("%r is not a rate in [0, 1]" % (text,))
    return p


parser = argparse.ArgumentParser(description='A3C_EVAL')
parser.add_argument('--env', default='Track2D-BlockPartialNav-v0', metavar='ENV', help='environment to evaluate on')
parser.add_argument('--num-episodes', type=int, default=100, metavar='NE', help='how many episodes in evaluation')
parser.add_argument('--load-model-dir', default=None, metavar='LMD', help='full checkpoint')
parser.add_argument('--load-tracker', default=None, metavar='LCD', help='tracker checkpoint')
parser.add_argument('--load-target', default=None, metavar='LCD', help='target checkpoint')
parser.add_argument('--log-dir', default='logs/', metavar='LG', help='folder to save logs')
parser.add_argument('--csv', default=None, metavar='SV', help='write to csv')
parser.add_argument('--render', dest='render', action='store_true',
                    help='draw the first --render-eps episodes on the device and write them as PNG frames under --render-dir '
                         '(runs the eager round on a shard that keeps episode traces)')
parser.add_argument('--render-dir', default=None, metavar='DIR',
                    help='--render: folder for ep{e:03d}/step{t:04d}.png and traces.npz (default: <log-dir>/render)')
parser.add_argument('--render-eps', type=int, default=4, metavar='K', help='--render: episodes to draw (default: 4)')
parser.add_argument('--render-scale', type=int, default=4, metavar='S', help='--render: pixels per map cell, 1..8 (default: 4)')
parser.add_argument('--view', nargs='?', const='tracker', default=None, choices=('tracker', 'target'), metavar='WHO',
                    help='draw what each player was shown: the first --view-eps episodes as PNG frames under --view-dir, each the '
                         'map as WHO (tracker or target; the bare flag means tracker) was shown it — what it was told where it saw '
                         'something, the dimmed truth where it saw nothing — next to both players\' 13 x 13 windows as they were '
                         'handed to the policy. Combines with every observation flag (--occlusion, --fov, --footprints, '
                         '--map-memory, --noise-*, --egocentric); runs the eager round. Not with --render')
parser.add_argument('--view-dir', default=None, metavar='DIR',
                    help='--view: folder for ep{e:03d}/step{t:04d}.png (default: <log-dir>/view)')
parser.add_argument('--view-eps', type=int, default=4, metavar='K', help='--view: episodes to draw (default: 4)')
parser.add_argument('--view-scale', type=int, default=4, metavar='S', help='--view: pixels per canvas cell, 1..8 (default: 4)')
parser.add_argument('--heuristic-tracker', default=None, choices=('pursuit',),
                    help='pursuit: the tracker walks a shortest path to the target (computed on the device) instead of following '
                         'a checkpoint')
parser.add_argument('--heuristic-target', default=None, choices=('evade',),
                    help='evade: the target steps to the neighbouring cell farthest from the tracker by path length instead of '
                         'following a checkpoint (or the id\'s own scripted target)')
parser.add_argument('--network', default='tat-maze-lstm', metavar='M', help='Model type to use')
parser.add_argument('--stack-frames', type=int, default=1, metavar='SF', help='Choose whether to stack observations')
parser.add_argument('--seed', type=int, default=1, metavar='S', help='random seed (default: 1)')
parser.add_argument('--gpu-id', type=int, default=0, help='GPU to use')
parser.add_argument('--obs', default='img', metavar='UE', help='unreal env')
parser.add_argument('--single', dest='single', action='store_true', help='single agent')
parser.add_argument('--rescale', dest='rescale', action='store_true', help='rescale image to [-1, 1]')
parser.add_argument('--rnn-out', type=int, default=128, metavar='LO', help='lstm output size: on the GPU a multiple of 4 up to 256')
parser.add_argument('--aux', default='reward', help='auxiliary task: reward/none')
parser.add_argument('--graphed-eval', dest='graphed_eval', action='store_true',
                    help='run the episodes on the rollout kernels as replayed hipGraphs where the env allows it')
parser.add_argument('--num-steps', type=int, default=20, metavar='NS', help='env steps per replayed graph (--graphed-eval)')
parser.add_argument('--fused-gru', dest='fused_gru', action='store_true',
                    help='maze-gru / tat-maze-gru: the fused one-GEMM step, which --graphed-eval needs for a GRU model '
                         '(also ATR_FUSED_GRU=1)')
parser.add_argument('--full-stem', dest='full_stem', action='store_true',
                    help="whole-map ('Full') ids: the encoders' two convolutions through the HIP stem for 81 / 82 wide frames "
                         'instead of F.conv2d (also ATR_FULL_STEM=1)')
parser.add_argument('--map-bank', default=None, metavar='FILE',
                    help='evaluate on the maps of a bank file (.npz / .txt: python -m active_tracking_rl_amd.map_bank), episode e '
                         'on map (eval env id of e + 1) mod K; --csv then also writes <csv>.maps.csv, one row per map')
parser.add_argument('--occlusion', dest='occlusion', action='store_true',
                    help='walls hide what is behind them: in both players\' 13 x 13 windows every cell whose line of sight from '
                         'the centre is blocked by a wall reads 5 ("unseen"); --graphed-eval falls back to the eager evaluator')
parser.add_argument('--fov', type=int, default=None, choices=(90, 180, 270), metavar='DEG',
                    help='a player sees only a cone of DEG degrees (90, 180 or 270) ahead: it faces the way of its last move, and '
                         'every cell of its 13 x 13 window outside the cone and farther than --fov-near from the centre reads 5 '
                         '("unseen"); a new episode starts looking all round. --graphed-eval falls back to the eager evaluator. '
                         'The heuristic players (--heuristic-tracker, --heuristic-target) read true state and are not blinded. '
                         'Not with --render')
parser.add_argument('--fov-target', type=int, default=None, choices=(90, 180, 270, 360), metavar='DEG',
                    help='--fov: the target\'s aperture (default: as --fov; 360: the target is not restricted)')
parser.add_argument('--fov-near', type=int, default=1, choices=tuple(range(7)), metavar='N',
                    help='--fov: cells within N of the centre (Chebyshev) stay visible all round (default: 1)')
parser.add_argument('--footprints', type=int, default=None, choices=tuple(range(1, 64)), metavar='K',
                    help='players leave a trail the other can see: each player leaves footprints on the last K (1 .. 63) cells it '
                         'stepped off, and the other player\'s 13 x 13 window shows them as 6 wherever it could see a free cell '
                         'there (a print behind a wall or outside the cone stays hidden); a new episode starts with no prints. '
                         '--graphed-eval falls back to the eager evaluator. Not with --render')
parser.add_argument('--footprints-for', default=None, choices=('tracker', 'target', 'both'), metavar='WHO',
                    help='--footprints: whose window shows the other\'s prints: tracker, target or both (default: tracker; a '
                         'scripted Ram / Nav / RPF target reads no window: tracker only)')
parser.add_argument('--egocentric', nargs='?', const=True, default=None, choices=('tracker', 'target', 'both'), metavar='WHO',
                    help='egocentric view: a player\'s 13 x 13 window is turned so that the player always looks up (it faces the way '
                         'of its last move; a new episode starts north-up), and its four actions mean forward / back / left / right. '
                         'WHO: tracker, target or both; the bare flag means every model-driven player (the tracker alone where the '
                         'target is scripted). --graphed-eval falls back to the eager evaluator; the heuristic players\' compass '
                         'moves are translated. Not with --render')
parser.add_argument('--map-memory', nargs='?', const=True, default=None, choices=('tracker', 'target', 'both'), metavar='WHO',
                    help='map memory: a cell of a player\'s 13 x 13 window that reads 5 ("unseen") shows 7 where the map has a wall '
                         'and 8 where it has none, if the player has seen that cell in this episode; a new episode starts with an '
                         'empty memory. Needs --occlusion or --fov. WHO: tracker, target or both; the bare flag means every '
                         'model-driven player (the tracker alone where the target is scripted). --graphed-eval falls back to the eager '
                         'evaluator. Not with --render')
parser.add_argument('--noise-flicker', type=_noise_rate, default=None, metavar='P',
                    help='sensor noise: every free cell (0) and wall (1) of a noisy 13 x 13 window off its centre reads as the other '
                         'of the two with probability P, drawn afresh at every env step. Any of --noise-flicker / --noise-miss / '
                         '--noise-ghost turns the pass on. One more launch per env step ('
                         'after --occlusion\'s, --fov\'s, --footprints\' and --map-memory\'s and ahead of --egocentric\'s turn); --graphed-eval '
                         'falls back to the eager evaluator. Not with --render')
parser.add_argument('--noise-miss', type=_noise_rate, default=None, metavar='P',
                    help='sensor noise: with probability P per window and env step the other player is missing from a noisy window '
                         '(its cell reads 0)')
parser.add_argument('--noise-ghost', type=_noise_rate, default=None, metavar='P',
                    help='sensor noise: with probability P per window and env step one cell of a noisy window, drawn uniformly, '
                         'shows the other player if it read 0 (a false detection; never on a cell the player cannot see)')
parser.add_argument('--noise-for', default=None, choices=('tracker', 'target', 'both'), metavar='WHO',
                    help='sensor noise: whose window is noisy: tracker, target or both (default: every model-driven player, the '
                         'tracker alone where the target is scripted)')

if __name__ == '__main__':
    args = parser.parse_args()
    if args.view is not None and args.render:
        parser.error("--view cannot be combined with --render: one drawing mode per run")
    if args.view is not None and '2D' in args.env and registry.spec(args.env)["obs_type"] == "Full":
        parser.error("--view needs the 13 x 13 windows of a 'Partial' id, %s observes the whole map" % (args.env,))
    if args.fov is None and args.fov_target is not None:
        parser.error("--fov-target needs --fov")
    if args.fov is not None and args.render:
        parser.error("--fov cannot be combined with --render: the drawn tracker's window would show what the tracker does not see")
    if args.footprints is None and args.footprints_for is not None:
        parser.error("--footprints-for needs --footprints")
    if args.footprints is not None and args.render:
        parser.error("--footprints cannot be combined with --render: the drawn tracker's window comes from the renderer's own "
                     "cells and would not show the prints")
    if args.footprints_for is None:
        args.footprints_for = "tracker"
    if (args.footprints is not None and args.footprints_for != "tracker" and '2D' in args.env
            and registry.spec(args.env)["target_mode"] in ("Ram", "Nav", "RPF")):
        parser.error("--footprints-for %s: the scripted target of %s reads no window, only the tracker's is painted there: use "
                     "--footprints-for tracker, or an id whose target is a player" % (args.footprints_for, args.env))
    if args.egocentric is not None and args.render:
        parser.error("--egocentric cannot be combined with --render: the renderer draws the tracker's window north-up")
    if (args.egocentric in ("target", "both") and '2D' in args.env
            and registry.spec(args.env)["target_mode"] in ("Ram", "Nav", "RPF")):
        parser.error("--egocentric %s: the scripted target of %s reads no window and takes no action of a player: use "
                     "--egocentric tracker, or an id whose target is a player" % (args.egocentric, args.env))
    if args.map_memory is not None and not args.occlusion and args.fov is None:
        parser.error("--map-memory needs --occlusion or --fov: without either no cell of a window ever reads 5, so there is nothing "
                     "to fill in")
    if args.map_memory is not None and args.render:
        parser.error("--map-memory cannot be combined with --render: the drawn tracker's window comes from the renderer's own "
                     "cells and would not show what is remembered")
    if args.map_memory is not None and '2D' in args.env and registry.spec(args.env)["obs_type"] == "Full":
        parser.error("--map-memory needs the 13 x 13 windows of a 'Partial' id, %s observes the whole map" % (args.env,))
    if (args.map_memory in ("target", "both") and '2D' in args.env
            and registry.spec(args.env)["target_mode"] in ("Ram", "Nav", "RPF")):
        parser.error("--map-memory %s: the scripted target of %s reads no window, only the tracker can remember there: use "
                     "--map-memory tracker, or an id whose target is a player" % (args.map_memory, args.env))
    noise_on = any(r is not None for r in (args.noise_flicker, args.noise_miss, args.noise_ghost))
    if args.noise_for is not None and not noise_on:
        parser.error("--noise-for needs --noise-flicker, --noise-miss or --noise-ghost")
    if noise_on and not any((args.noise_flicker, args.noise_miss, args.noise_ghost)):
        parser.error("--noise-flicker / --noise-miss / --noise-ghost: every rate is 0, so the pass would change nothing")
    if noise_on and args.render:
        parser.error("--noise-flicker / --noise-miss / --noise-ghost cannot be combined with --render: the drawn tracker's window "
                     "comes from the renderer's own cells and would not show the noise")
    if noise_on and '2D' in args.env and registry.spec(args.env)["obs_type"] == "Full":
        parser.error("--noise-flicker / --noise-miss / --noise-ghost need the 13 x 13 windows of a 'Partial' id, %s observes the "
                     "whole map" % (args.env,))
    if (noise_on and args.noise_for in ("target", "both") and '2D' in args.env
            and registry.spec(args.env)["target_mode"] in ("Ram", "Nav", "RPF")):
        parser.error("--noise-for %s: the scripted target of %s reads no window, only the tracker's can be noisy there: use "
                     "--noise-for tracker, or an id whose target is a player" % (args.noise_for, args.env))
    build.build()
    check_path(args.log_dir)
    name = '{}_mon_log'.format(args.env)
    setup_logger(name, os.path.join(args.log_dir, name))
    log = logging.getLogger(name)
    device = torch.device('cuda', max(args.gpu_id, 0))
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed(args.seed)
    for k, v in vars(args).items():
        log.info('{0}: {1}'.format(k, v))
    # the model is sized by the env's observation space, as in the reference (gym_eval.py:62-69): 13x13 crops for the
    # 'Partial' ids, the whole S x S map (S = 81 Maze, 82 Block/Empty) for the 'Full' ids
    sp = registry.spec(args.env)
    full_side = 81 if sp["map_type"] == "Maze" else 82
    obs_space, act_space = _spaces((full_side, full_side) if sp["obs_type"] == "Full" else (13, 13))
    model = build_model(obs_space, act_space, args, device).to(device)
    load = lambda path: torch.load(path, map_location=lambda storage, loc: storage)
    if args.load_model_dir is not None:
        model.load_state_dict(load(args.load_model_dir), strict=False)     # gym_eval.py:74-78
    if args.load_tracker is not None:
        model.player0.load_state_dict(load(args.load_tracker))            # :81-85
    if args.load_target is not None:
        model.player1.load_state_dict(load(args.load_target))             # :88-92
    args.gpu_ids = [device.index]
    render_dir = (args.render_dir or os.path.join(args.log_dir, 'render')) if args.render else None
    view_dir = (args.view_dir or os.path.join(args.log_dir, 'view')) if args.view is not None else None
    args.eval_map_bank, args.map_bank = args.map_bank, None        # (the evaluation shard's flag: environment.eval_args)
    info = {}
    rsum, length = evaluate(model, args.env, args, device, args.num_episodes, graphed=args.graphed_eval, render_dir=render_dir,
                            heuristic_tracker=args.heuristic_tracker, heuristic_target=args.heuristic_target, info=info,
                            view_dir=view_dir)
    reward_mean, reward_std = rsum.mean(0), rsum.std(0)
    len_mean, len_std = length.mean(), length.std()
    success_rate = float((length >= 500).mean())
    log.info("El, {0}, R, {1}, R_mean: {2}, R_std: {3}, EL_mean: {4:.2f}, EL_std {5:.2f}, R_step: {6}, S_rate: {7}".format(
        int(length[-1]), rsum[-1], reward_mean, reward_std, len_mean, len_std, reward_mean / len_mean, success_rate))
    if args.csv is not None:
        import csv
        header = ['Env', 'Seed', 'R_mean', 'R_std', 'EL_mean', 'EL_std', 'S_rate']
        row = {'Env': args.env, 'Seed': args.seed, 'R_mean': float(reward_mean[0]), 'R_std': float(reward_std[0]),
               'EL_mean': float(len_mean), 'EL_std': float(len_std), 'S_rate': success_rate}
        new = not os.path.exists(args.csv)
        with open(args.csv, 'a') as f:
            w = csv.DictWriter(f, header)
            if new:
                w.writeheader()
            w.writerows([row])
        if info.get("map_index") is not None:          # --map-bank: the same figures per map, beside the summary
            root = args.csv[:-4] if args.csv.endswith('.csv') else args.csv
            with open(root + '.maps.csv', 'w') as f:
                w = csv.writer(f)
                w.writerow(['Map', 'Episodes', 'EL_mean', 'S_rate', 'R0_mean', 'R1_mean'])
                for r in per_map_summary(info["map_index"], rsum, length):
                    w.writerow([r["map"], r["episodes"], r["eps_len"], r["success_rate"], float(r["reward"][0]), float(r["reward"][1])])
