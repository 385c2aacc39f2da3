#!/usr/bin/env python
"""Generate tests/golden/traces.npz by RUNNING THE REFERENCE ENV: info['traces'], info['traces_relative'] and what render()
draws (track_1v1.py:90-93,120-123,160-164,170-216), per step of four short episodes.

Run once where the reference checkout is (T2D_REFERENCE, default: a `reference` folder next to this repository); a machine
that only has this repository never needs it:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_traces.py

Like make_golden.py it imports the reference env through tests/golden/_refstubs and neutralises the argument-less
np.random.seed() calls of generators.py. render() itself is never called (it needs a display and, under numpy >= 1.23, its
`obs[list(zip(*traces[:-1]))] = 6` paints whole rows): the script applies the paint the line intends,
`obs[tuple(zip(*traces[:-1]))] = 6`, to _get_full_obs(), and nothing when traces[:-1] is empty. The palette is
cmap(norm(v)) of the env's own colour map for the values that occur. Outputs are DATA only.

Per episode e<i>/: maze (packed bits), side, init [2, 2], actions [T, 2] as consumed by _next_state, done [T], pos [T, 2, 2],
traces [T + 1, 2] (info['traces'] of step t is its first t + 2 rows: checked here), rel0 [2, 2] (reset's traces_relative),
rel [T, 2, 2, 2], cells0 / full0 / partial0 (after reset) and cells / full / partial [T, ...] (82 x 82 images are padded with
255 outside the env's side).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("T2D_REFERENCE") or os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference")
sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, os.path.join(HERE, "_refstubs"))
sys.path.insert(0, os.path.join(REF, "envs", "gym-track2d"))

import numpy as np  # noqa: E402

import gym_track2d  # noqa: E402,F401  (fills the registry stub)
from gym.envs.registration import REGISTRY  # noqa: E402
from gym_track2d.envs.track_1v1 import Track1v1Env  # noqa: E402

_real_seed = np.random.seed


def patched_seed(*a, **k):
    if a or k:
        return _real_seed(*a, **k)
    return None  # argument-less re-seed neutralised


np.random.seed = patched_seed

MOVES = {0: (-1, 0), 1: (1, 0), 2: (0, -1), 3: (0, 1)}
MAX_STEPS = 40


def make_env(env_id):
    kw = REGISTRY[env_id]["kwargs"]
    return Track1v1Env(**kw)


def pad82(a):
    out = np.full((82, 82), 255, np.uint8)
    a = np.asarray(a)
    out[: a.shape[0], : a.shape[1]] = a.astype(np.uint8)
    return out


def snapshot(env):
    """(painted cells, unpainted full observation, the tracker's window) as render() would draw them now."""
    full = np.array(env._get_full_obs())
    cells = full.copy()
    head = [tuple(int(v) for v in p) for p in env.traces[:-1]]
    if head:
        cells[tuple(zip(*head))] = 6
    partial = np.array(env._get_partial_obs(0, env.pob_size))
    assert partial.shape == (13, 13)
    return pad82(cells), pad82(full), partial.astype(np.uint8)


def toward(src, dst, fallback):
    """Greedy VonNeumann action from src toward dst (rows first); `fallback` when already there."""
    if dst[0] < src[0]:
        return 0
    if dst[0] > src[0]:
        return 1
    if dst[1] < src[1]:
        return 2
    if dst[1] > src[1]:
        return 3
    return fallback


class Recorder(object):
    def __init__(self, env_id, seed):
        self.env_id = env_id
        self.env = env = make_env(env_id)
        self.emitted = []
        if env.Target:
            tgt = env.Target[0]
            orig = tgt.step

            def rec_step(*a, **k):
                out = orig(*a, **k)
                act = out[0] if isinstance(out, tuple) else out
                self.emitted.append(int(np.asarray(act).reshape(-1)[0]))
                return out

            tgt.step = rec_step
        np.random.seed(seed)
        env.reset()
        self.maze = np.array(env.maze)
        self.init = np.array(env.init_states, np.int32).copy()
        self.rel0 = np.array(env.traces_relative, np.int32).copy()
        assert [list(map(int, p)) for p in env.traces] == [list(map(int, self.init[0]))]
        self.cells0, self.full0, self.partial0 = snapshot(env)
        self.rec = dict(actions=[], done=[], pos=[], rel=[], cells=[], full=[], partial=[])
        self.flags = dict(tracker6=0, target6=0, colocated=0, bump=0, target_bump=0)
        self.final_traces = None

    def state(self):
        return [list(map(int, s)) for s in self.env.state]

    def step(self, a0, a1):
        env = self.env
        before = self.state()
        n_em = len(self.emitted)
        _, _, done, info = env.step([a0, a1])
        applied1 = self.emitted[n_em] if len(self.emitted) > n_em else a1
        after = self.state()
        t = len(self.rec["actions"]) + 1
        traces = [list(map(int, p)) for p in info["traces"]]
        assert len(traces) == t + 1 and traces[0] == list(map(int, self.init[0])) and traces[-1] == after[1]
        if self.final_traces is not None:
            assert traces[:-1] == self.final_traces            # the list only grows
        self.final_traces = traces
        rel = np.array(info["traces_relative"], np.int32)
        assert rel.shape == (2, 2, 2)
        cells, full, partial = snapshot(env)
        r = self.rec
        r["actions"].append([a0, applied1]); r["done"].append(bool(done)); r["pos"].append(np.array(after, np.int32))
        r["rel"].append(rel); r["cells"].append(cells); r["full"].append(full); r["partial"].append(partial)
        head = traces[:-1]
        f = self.flags
        f["tracker6"] += int(after[0] in head and cells[after[0][0], after[0][1]] == 6)
        f["target6"] += int(after[1] in head and cells[after[1][0], after[1][1]] == 6)
        f["colocated"] += int(after[0] == after[1])
        f["bump"] += int(after[0] == before[0]) + int(after[1] == before[1])
        f["target_bump"] += int(after[1] == before[1])
        return bool(done)

    def flatten(self, prefix, out):
        r = self.rec
        m = (self.maze != 0).astype(np.uint8)
        out[prefix + "env_id"] = np.array(self.env_id)
        out[prefix + "maze"] = np.packbits(m.reshape(-1)); out[prefix + "side"] = np.int32(m.shape[0])
        out[prefix + "init"] = self.init; out[prefix + "rel0"] = self.rel0
        out[prefix + "cells0"] = self.cells0; out[prefix + "full0"] = self.full0; out[prefix + "partial0"] = self.partial0
        out[prefix + "actions"] = np.array(r["actions"], np.uint8); out[prefix + "done"] = np.array(r["done"], np.uint8)
        out[prefix + "pos"] = np.array(r["pos"], np.int32); out[prefix + "traces"] = np.array(self.final_traces, np.int32)
        out[prefix + "rel"] = np.array(r["rel"], np.int32); out[prefix + "cells"] = np.array(r["cells"], np.uint8)
        out[prefix + "full"] = np.array(r["full"], np.uint8); out[prefix + "partial"] = np.array(r["partial"], np.uint8)


def episode_scripted_empty():
    """Track2D-EmptyPartialPZR-v0: the target walks 3 right and 2 back left (it revisits its cells); the tracker follows onto the
    target's old cells, then heads for the cell the target is about to enter and ends co-located with it. Both agents move at every
    step away from walls, so the parity of their distance never changes: the seed is searched for an even spawn distance."""
    for seed in range(100, 400):
        rec = Recorder("Track2D-EmptyPartialPZR-v0", seed)
        (r0, c0), (r1, c1) = rec.state()
        if (abs(r0 - r1) + abs(c0 - c1)) % 2 or min(r0, c0, r1, c1) < 12 or max(r0, c0, r1, c1) > 68:
            continue
        script = [3, 3, 3, 2, 2] + [0, 1] * 17
        for t, a1 in enumerate(script[:MAX_STEPS]):
            trk, tgt = rec.state()
            nxt = [tgt[0] + MOVES[a1][0], tgt[1] + MOVES[a1][1]]
            a0 = toward(trk, tgt, 2) if t < 5 else toward(trk, nxt, 2)     # follow, then intercept
            rec.step(a0, a1)
            trk, tgt = rec.state()
            if t >= 5 and trk == tgt:
                break
        f = rec.flags
        trk, tgt = rec.state()
        if trk == tgt and f["tracker6"] and f["target6"]:
            return rec, seed
    raise RuntimeError("no seed gives the scripted Empty episode")


def episode_random_block():
    """Track2D-BlockPartialPZR-v0, seeded random actions: wall bumps give repeated trace entries."""
    for seed in range(200, 600):
        rec = Recorder("Track2D-BlockPartialPZR-v0", seed)
        rs = np.random.RandomState(20_000 + seed)
        for t in range(MAX_STEPS):
            if rec.step(int(rs.randint(0, 4)), int(rs.randint(0, 4))):
                break
        if rec.flags["target_bump"] >= 2 and len(rec.rec["actions"]) == MAX_STEPS:
            return rec, seed
    raise RuntimeError("no seed gives a Block episode with target bumps")


def episode_maze_nav():
    """Track2D-MazePartialNav-v0 (side 81): the target is the env's scripted Navigator; the tracker chases."""
    seed = 300
    rec = Recorder("Track2D-MazePartialNav-v0", seed)
    assert rec.maze.shape == (81, 81)
    rs = np.random.RandomState(30_000 + seed)
    for t in range(MAX_STEPS):
        trk, tgt = rec.state()
        a0 = toward(trk, tgt, 0) if rs.rand() > 0.2 else int(rs.randint(0, 4))
        if rec.step(a0, 0):
            break
    return rec, seed


def episode_far_block():
    """A Block episode that ends by the far counter (track_1v1.py:106-111): the agents walk apart."""
    for seed in range(400, 800):
        rec = Recorder("Track2D-BlockPartialPZR-v0", seed)
        done = False
        for t in range(MAX_STEPS):
            done = rec.step(2, 3)
            if done:
                break
        if done and int(rec.env.C_far) > 10:
            return rec, seed
    raise RuntimeError("no seed gives a far-counter ending")


def main():
    out = {}
    total = dict(tracker6=0, target6=0, colocated=0, bump=0, target_bump=0)
    names = []
    for i, make in enumerate((episode_scripted_empty, episode_random_block, episode_maze_nav, episode_far_block)):
        rec, seed = make()
        rec.flatten("e%d/" % i, out)
        out["e%d/seed" % i] = np.int32(seed)
        names.append("e%d" % i)
        for k in total:
            total[k] += rec.flags[k]
        print("e%d" % i, rec.env_id, "seed", seed, "steps", len(rec.rec["actions"]), "done", rec.rec["done"][-1], rec.flags)
    # the fixture must prove it exercises these
    assert total["tracker6"] >= 1 and total["target6"] >= 1 and total["colocated"] >= 1 and total["bump"] >= 1, total
    assert out["e3/done"][-1] == 1 and out["e2/side"] == 81
    env = make_env("Track2D-EmptyPartialPZR-v0")
    values = np.array([0, 1, 2, 4, 6], np.uint8)
    out["palette_values"] = values
    out["palette"] = np.array([env.cmap(env.norm(int(v)), bytes=True)[:3] for v in values], np.uint8)
    out["coverage"] = np.array([total[k] for k in ("tracker6", "target6", "colocated", "bump")], np.int32)
    out["names"] = np.array(names)
    path = os.path.join(HERE, "traces.npz")
    np.savez_compressed(path, **out)
    print("palette", out["palette"].tolist(), "coverage", total, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
