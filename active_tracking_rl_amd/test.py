"""test — the evaluator of test.py:16-136, vectorised: `test_eps` evaluation episodes run as ONE batch of envs on the
GPU (argmax policy, Agent.action_test) instead of one env in a side process.

Kept from the reference: evaluation on `--env-base` (default Track2D-BlockPartialNav-v0, main.py:27), the summary line
("ave eps reward / ave eps length / reward step", test.py:101-109), the checkpoint names and contents
(`all-best-{n_iter}.dat` / `all-new.dat`, and with --split `tracker-{best,new}.dat`, `target-{best,new}.dat`:
state_dicts with the reference's keys, test.py:111-127), the train_modes schedule (test.py:84-92, including the
--train-mode 2 tracker / target alternation, which needs the --adv-step flag the reference forgot to define), the
`test/reward{i}`, `test/fps`, `test/eps_len` scalars (test.py:93-97; one record per evaluation episode, as there) and the
stop sentinel -100 once n_iter > max_step (test.py:129-134). Success = episode length >= 500 (gym_eval.py:114-115).
"""
import logging
import os
import time

import numpy as np
import torch

from . import registry
from .environment import create_env, eval_args
from .model import build_model
from .player_util import Agent
from .utils import ScalarWriter, check_path, setup_logger, write_png


class FrameWriter(object):
    """--render: the frames of the first `eps` episodes of an evaluation round, drawn on the device in ONE t2d_render_rgb
    launch per step and written as <dir>/ep{e:03d}/step{t:04d}.png (t = 0: the reset state); an episode stops producing files
    after its terminal frame. close() adds <dir>/traces.npz: `pos` / `len` of the trace store for all evaluated episodes."""

    def __init__(self, ev, directory, eps, scale, episodes):
        self.core, self.dir, self.scale, self.episodes = ev.core, directory, int(scale), int(episodes)
        self.k = max(0, min(int(eps), int(episodes)))
        self.ids = torch.arange(self.k, dtype=torch.int32, device=ev.device)
        self.open = np.ones(self.k, bool)
        for e in range(self.k):
            check_path(os.path.join(directory, "ep%03d" % e))
        check_path(directory)

    def frame(self, t, done=None):
        if self.k == 0 or not self.open.any():
            return
        frames = self.draw().cpu().numpy()
        fin = np.zeros(self.k, bool) if done is None else (done[:self.k].cpu().numpy() != 0)
        for e in np.nonzero(self.open)[0]:
            write_png(os.path.join(self.dir, "ep%03d" % e, "step%04d.png" % t), frames[e])
        self.open &= ~fin

    def draw(self):
        return self.core.render_rgb(self.ids, scale=self.scale)

    def close(self):
        tr = self.core.traces(0, self.episodes)
        np.savez_compressed(os.path.join(self.dir, "traces.npz"), pos=tr["pos"], len=tr["len"])


class ViewWriter(FrameWriter):
    """--view: FrameWriter's file tree with the frames of atr_view_rgb (VecEnv.view_rgb, ONE launch per step): the map as
    `viewer` was shown it and both players' windows as they were handed to the policy. There is no trace store, so close()
    writes nothing."""

    def __init__(self, ev, directory, eps, scale, episodes, viewer=0):
        FrameWriter.__init__(self, ev, directory, eps, scale, episodes)
        self.ev, self.viewer = ev, viewer

    def draw(self):
        return self.ev.view_rgb(self.ids, scale=self.scale, viewer=self.viewer)

    def close(self):
        pass


_warned_heuristic_graphed = False


def heuristic_players(model, env_id, heuristic_tracker=None, heuristic_target=None):
    """The Agent.heuristic pair of an evaluation round, checked without an env: 'pursuit' may replace the tracker, 'evade' the
    target (include/track2d_heuristic.h). model=None is accepted exactly when no model action reaches the env — the tracker is
    heuristic and the target is heuristic or scripted by the id (Ram / Nav / RPF); else ValueError names the player without a
    policy."""
    if heuristic_tracker not in (None, "pursuit"):
        raise ValueError("heuristic_tracker=%r: the heuristic tracker is 'pursuit'" % (heuristic_tracker,))
    if heuristic_target not in (None, "evade"):
        raise ValueError("heuristic_target=%r: the heuristic target is 'evade'" % (heuristic_target,))
    mode = registry.spec(env_id)["target_mode"]
    if model is None:
        if heuristic_tracker is None:
            raise ValueError("evaluate: no model and no heuristic_tracker: the tracker has no policy")
        if heuristic_target is None and mode not in ("Ram", "Nav", "RPF"):
            raise ValueError("evaluate: no model and no heuristic_target on %s, whose %s target is model-driven: the target has "
                             "no policy" % (env_id, mode))
    return (heuristic_tracker, heuristic_target)


@torch.no_grad()
def evaluate(model, env_id, args, device, episodes, seed=None, graphed=False, render_dir=None, heuristic_tracker=None,
             heuristic_target=None, info=None, view_dir=None):
    """Run `episodes` envs of `env_id` in parallel until each has finished ONE episode. Returns per-episode reward
    sums [episodes, 2] and lengths [episodes] (numpy). graphed: the round on the rollout's kernels as replayed hipGraphs
    (evaluator.GreedyEvaluator) where they apply, else — with one warning line — the eager round below.
    render_dir: draw the first args.render_eps episodes into it (FrameWriter). The round then runs here, on a shard without the
    in-launch auto-reset that keeps episode traces; the round ignores an env after its first done either way, so the returned
    numbers are those of a round without rendering. (A finished env of such a shard is simply stepped on from where it stands —
    the step kernels treat it like any other env — while its trace stays closed: no masked reset is needed.)
    heuristic_tracker='pursuit' / heuristic_target='evade': that player's actions come from the heuristic player
    (heuristic_players: the round is the eager one; model may be None when no model action reaches the env).
    view_dir: draw the first args.view_eps episodes into it as the players were shown them (ViewWriter; args.view names the
    viewer). Like a rendered round it runs here, on a shard without the in-launch auto-reset, so that a terminal frame shows the
    terminal state; there is no traces.npz. Not together with render_dir.
    info: a dict that receives what the round knows beyond its return value — with --eval-map-bank, info['map_index']: int32
    [episodes], the bank index of each evaluation episode's map (map_index() right after the reset)."""
    global _warned_heuristic_graphed
    heuristic = heuristic_players(model, env_id, heuristic_tracker, heuristic_target)
    if graphed and heuristic != (None, None):
        if not _warned_heuristic_graphed:
            logging.getLogger(__name__).warning("heuristic players use the eager evaluation round: the graphed step takes both "
                                                "actions from the model")
            _warned_heuristic_graphed = True
        graphed = False
    if render_dir is not None and view_dir is not None:
        raise ValueError("evaluate: render_dir and view_dir are one drawing mode each, give one")
    if graphed and render_dir is not None:
        logging.getLogger(__name__).warning("--render uses the eager evaluation round: the graphed step restarts episodes in-launch")
        graphed = False
    if graphed and view_dir is not None:
        logging.getLogger(__name__).warning("--view uses the eager evaluation round: the graphed step restarts episodes in-launch")
        graphed = False
    if graphed:
        from . import evaluator
        try:
            gev = evaluator.GreedyEvaluator(model, env_id, args, device, episodes)
            out = gev.run()
            if info is not None and gev.map_index is not None:
                info["map_index"] = gev.map_index
            return out
        except evaluator.Unsupported as ex:
            logging.getLogger(__name__).warning("graphed evaluation falls back to the eager round: %s", ex)
    ev = create_env(env_id, eval_args(args), num_envs=max(2, episodes), device=str(device),
                    env_id_base=getattr(args, "eval_env_id_base", 1 << 20), traces=render_dir is not None,
                    views=view_dir is not None, auto_reset=False if view_dir is not None else None)
    n = ev.num_envs
    was_training = model is not None and model.training
    if model is not None:
        model.eval()
    player = Agent(model, ev, args, None, device)
    player.heuristic = heuristic
    player.reset()
    if info is not None and getattr(ev, "map_bank", None) is not None:
        info["map_index"] = ev.map_index()[:episodes].cpu().numpy()
    rsum = torch.zeros(n, player.num_agents, device=device)
    length = torch.zeros(n, dtype=torch.int32, device=device)
    alive = torch.ones(n, dtype=torch.bool, device=device)
    frames = None
    if render_dir is not None:
        frames = FrameWriter(ev, render_dir, getattr(args, "render_eps", 4), getattr(args, "render_scale", 4), episodes)
        frames.frame(0)
    elif view_dir is not None:
        frames = ViewWriter(ev, view_dir, getattr(args, "view_eps", 4), getattr(args, "view_scale", 4), episodes,
                            getattr(args, "view", None) or "tracker")
        frames.frame(0)
    for t in range(ev.core_max_steps()):
        player.action_test()
        if frames is not None:
            frames.frame(t + 1, player.done)
        rsum += player.reward * alive.unsqueeze(1)
        length += alive.to(length.dtype)
        alive &= (player.done == 0)
        if not bool(alive.any()):
            break
    if frames is not None:
        frames.close()
    ev.close()
    if was_training:
        model.train()
    return rsum[:episodes].cpu().numpy(), length[:episodes].cpu().numpy()


def schedule_train_modes(args, train_modes, n_iter, state):
    """test.py:84-92, verbatim semantics: tracker only while n_iter < --init-step; with --train-mode 2 the mode of every rank
    flips (1 - mode) whenever more than `iter_th` iterations have passed since the last flip — iter_th starts at --init-step
    and becomes --init-step after a flip to the tracker, --adv-step after a flip away from it — and is otherwise reset to
    --train-mode. `state` carries last_iter / iter_th between calls (locals of the reference's one long loop). The reference
    applies this at the end of every evaluation episode; here it runs once per evaluation round (all episodes of a round
    finish together)."""
    state.setdefault("last_iter", 0)
    state.setdefault("iter_th", args.init_step)
    for rank in range(len(train_modes)):
        if n_iter < args.init_step:
            train_modes[rank] = 0
        elif args.train_mode == 2 and n_iter - state["last_iter"] > state["iter_th"]:
            train_modes[rank] = 1 - train_modes[rank]
            state["last_iter"] = n_iter
            adv_step = getattr(args, "adv_step", None)
            if adv_step is None:
                raise AttributeError("--train-mode 2 needs --adv-step (test.py:90 of the reference reads args.adv_step, which "
                                     "its main.py never defines)")
            state["iter_th"] = args.init_step if train_modes[rank] == 0 else adv_step
        else:
            train_modes[rank] = args.train_mode
    return train_modes


def save_checkpoints(model, args, n_iter, best):
    """test.py:111-127."""
    check_path(args.log_dir)
    if best:
        model_dir = os.path.join(args.log_dir, 'all-best-{0}.dat'.format(n_iter))
        tracker_model_dir = os.path.join(args.log_dir, 'tracker-best.dat')
        target_model_dir = os.path.join(args.log_dir, 'target-best.dat')
    else:
        model_dir = os.path.join(args.log_dir, 'all-new.dat')
        tracker_model_dir = os.path.join(args.log_dir, 'tracker-new.dat')
        target_model_dir = os.path.join(args.log_dir, 'target-new.dat')
    cpu = lambda sd: {k: v.detach().cpu().clone() for k, v in sd.items()}
    torch.save(cpu(model.state_dict()), model_dir)
    if args.split:
        torch.save(cpu(model.player0.state_dict()), tracker_model_dir)
        if not args.single:
            torch.save(cpu(model.player1.state_dict()), target_model_dir)
    return model_dir


PER_MAP_LOG_MAX = 64        # --eval-map-bank: banks of at most this many maps get per-map scalars


def per_map_summary(map_index, rsum, length):
    """The evaluation episodes of a round grouped by bank index: a list of dict(map, episodes, eps_len, success_rate, reward)
    in index order — mean length, share of episodes that lasted the 500 steps, mean returns per player."""
    map_index, rsum, length = np.asarray(map_index), np.asarray(rsum), np.asarray(length)
    rows = []
    for m in np.unique(map_index):
        sel = map_index == m
        rows.append(dict(map=int(m), episodes=int(sel.sum()), eps_len=float(length[sel].mean()),
                         success_rate=float((length[sel] >= registry.MAX_EPISODE_STEPS).mean()), reward=rsum[sel].mean(0)))
    return rows


def log_per_map(writer, map_index, rsum, length, n_iter, count=None):
    """test/map/<idx>/eps_len and test/map/<idx>/reward0: the round's means per bank map (banks of at most PER_MAP_LOG_MAX maps)."""
    if map_index is None or (count if count is not None else int(np.max(map_index)) + 1) > PER_MAP_LOG_MAX:
        return
    for row in per_map_summary(map_index, rsum, length):
        writer.add_scalar('test/map/{0}/eps_len'.format(row["map"]), row["eps_len"], n_iter)
        writer.add_scalar('test/map/{0}/reward0'.format(row["map"]), row["reward"][0], n_iter)


def heuristic_rounds(args, model, device, writer, log, n_iter, state):
    """--eval-heuristic: two more rounds of --test-eps episodes on args.env after an evaluation round — the model's tracker
    against the evading target (test/vs_evade/reward0, test/vs_evade/eps_len) and the model's target against the pursuit tracker
    (test/vs_pursuit/reward1, test/vs_pursuit/eps_len), one record per episode and one log line each. Only where args.env's
    target is model-driven (Adv / PZR / Far); else one warning and nothing."""
    mode = registry.spec(args.env)["target_mode"]
    if mode in ("Ram", "Nav", "RPF"):
        if not state.get("warned_eval_heuristic"):
            log.warning("--eval-heuristic does nothing on {0}: its {1} target is scripted by the env".format(args.env, mode))
            state["warned_eval_heuristic"] = True
        return
    for tag, col, kw in (("vs_evade", 0, dict(heuristic_target="evade")), ("vs_pursuit", 1, dict(heuristic_tracker="pursuit"))):
        rsum, length = evaluate(model, args.env, args, device, args.test_eps, **kw)
        for ep in range(len(length)):
            writer.add_scalar('test/{0}/reward{1}'.format(tag, col), rsum[ep, col], n_iter)
            writer.add_scalar('test/{0}/eps_len'.format(tag), length[ep], n_iter)
        writer.flush()
        log.info("{0}: ave eps reward{1} {2}, ave eps length {3}".format(
            tag, col, rsum[:, col].sum() / args.test_eps, length.sum() / args.test_eps))


def test(args, shared_model, train_modes, n_iters, rounds=None, state=None):
    """Evaluator loop with the reference signature. `shared_model` is the (rank-0) replica being trained; call it
    between training iterations or from a side thread. `rounds` bounds the number of evaluation rounds (None = until
    the stop rule fires, as in the reference). `state`: a dict the caller keeps between bounded calls, so that the
    elapsed time, the best score and the one-off flag dump continue across them as in the reference's single loop."""
    gpu_id = args.gpu_ids[-1]
    device = torch.device('cuda:%d' % gpu_id)
    check_path(args.log_dir)
    name = '{}_log'.format(args.env)
    setup_logger(name, os.path.join(args.log_dir, 'logger'))
    log = logging.getLogger(name)
    state = {} if state is None else state
    if not state.get("started"):
        for k, v in vars(args).items():
            log.info('{0}: {1}'.format(k, v))
        state.update(started=True, start_time=time.time(), max_score=-100)
    if state.get("writer") is None:
        state["writer"] = ScalarWriter(os.path.join(args.log_dir, 'Test'))          # test.py:19
    writer = state["writer"]
    env_id = args.env if args.env_base is None else args.env_base
    start_time, max_score = state["start_time"], state["max_score"]
    done_rounds = 0
    while rounds is None or done_rounds < rounds:
        t0 = time.time()
        n_iter = int(sum(n_iters))
        render_dir = os.path.join(args.log_dir, 'render', 'iter{0}'.format(n_iter)) if getattr(args, "render", False) else None
        view_dir = None
        if getattr(args, "view", None):
            view_dir = os.path.join(getattr(args, "view_dir", None) or os.path.join(args.log_dir, 'view'), 'iter{0}'.format(n_iter))
        info = {}
        rsum, length = evaluate(shared_model, env_id, args, device, args.test_eps,
                                graphed=bool(getattr(args, "graphed_eval", False)), render_dir=render_dir, info=info,
                                view_dir=view_dir)
        schedule_train_modes(args, train_modes, n_iter, state)                       # test.py:84-92
        # test.py:93-97: one record per evaluation episode at step n_iter. test/fps in the reference is the env steps per
        # second of the evaluator's one env; here the episodes of a round run as one batch, so it is the round's env steps
        # (all episodes) over its wall time
        fps = float(length.sum()) / max(time.time() - t0, 1e-9)
        for ep in range(len(length)):
            for i in range(rsum.shape[1]):
                writer.add_scalar('test/reward' + str(i), rsum[ep, i], n_iter)
            writer.add_scalar('test/fps', fps, n_iter)
            writer.add_scalar('test/eps_len', length[ep], n_iter)
        log_per_map(writer, info.get("map_index"), rsum, length, n_iter)
        writer.flush()
        ave_reward_sum = rsum[:, :2].sum(0) / args.test_eps
        len_mean = length.sum() / args.test_eps
        reward_step = rsum[:, :2].sum(0) / max(length.sum(), 1)
        log.info("Time {0}, ave eps reward {1}, ave eps length {2}, reward step {3}".format(
            time.strftime("%Hh %Mm %Ss", time.gmtime(time.time() - start_time)), ave_reward_sum, len_mean, reward_step))
        best = ave_reward_sum[0] >= max_score
        if best:
            max_score = state["max_score"] = ave_reward_sum[0]
        save_checkpoints(shared_model, args, n_iter, best)
        if getattr(args, "eval_heuristic", False):
            heuristic_rounds(args, shared_model, device, writer, log, n_iter, state)
        done_rounds += 1
        if n_iter > args.max_step:                             # test.py:129-134
            for rank in range(len(train_modes)):
                train_modes[rank] = -100
            break
    return max_score
