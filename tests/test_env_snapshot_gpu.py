"""-m gpu: env shard snapshots (include/track2d_state.h, csrc/state_hip.hip k_state_copy) on the device. The reference
throughout is the UNINTERRUPTED run of the existing step path on a handle that is never saved or restored, compared bit for bit
(torch.equal on observations, rewards and done flags): no tolerance enters. 70 envs (no multiple of 64, of the 4 waves of a
workgroup or of the 2 envs a k_step2 wave steps; 69 once) with max_episode_steps=12, so every env turns its episode over at
least every 12 steps and both next-episode slots are consumed and refilled inside a test."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

N, T_MAX, PRE, LEN = 70, 12, 37, 45
PZR = "Track2D-BlockPartialPZR-v0"
CONFIGS = [(PZR, 70), ("Track2D-BlockPartialRam-v0", 70), ("Track2D-MazePartialNav-v0", 70), ("Track2D-BlockPartialRPF-v0", 70),
           ("Track2D-BlockPartialAdv-v0", 70), (PZR, 69)]
IDS = ["PZR", "Ram", "MazeNav", "RPF", "Adv", "PZR-69"]


def _dev():
    return torch.device("cuda:0")


def _make(env_id=PZR, n=N, **kw):
    from active_tracking_rl_amd.vec_env import VecTrack2D
    kw.setdefault("max_episode_steps", T_MAX)
    return VecTrack2D(env_id, num_envs=n, device="cuda:0", **kw)


_ACTIONS = {}


def _actions(n, steps=PRE + 3 * LEN):
    """[steps, 2, n] int64 on the device, from a seeded CPU generator (the same for every handle of n envs)."""
    if n not in _ACTIONS:
        g = torch.Generator().manual_seed(1234 + n)
        _ACTIONS[n] = torch.randint(0, 4, (PRE + 3 * LEN, 2, N), generator=g)[:, :, :n].contiguous().to(_dev())
    return _ACTIONS[n][:steps]


def _run(env, acts):
    """Step through acts [T, 2, n]; the records (obs [T,n,2,13,13], rew [T,n,2], done [T,n]) as clones."""
    obs, rew, done = [], [], []
    for a in acts:
        o, r, d = env.step(a[0], a[1])
        obs.append(o.clone()); rew.append(r.clone()); done.append(d.clone())
    return torch.stack(obs), torch.stack(rew), torch.stack(done)


def _same(a, b, envs=None):
    for x, y in zip(a, b):
        if envs is not None:
            x, y = x[:, envs], y[:, envs]
        if not torch.equal(x, y):
            return False
    return True


def _cut(rec, lo, hi):
    return tuple(x[lo:hi] for x in rec)


_CONTROL = {}


def _control(env_id, n):
    """The uninterrupted run: reset + PRE + 3 * LEN steps on a handle that no snapshot call ever touches. Computed once per
    configuration and left unchanged."""
    key = (env_id, n)
    if key not in _CONTROL:
        c = _make(env_id, n)
        c.reset()
        _CONTROL[key] = _run(c, _actions(n))
        c.close()
    return _CONTROL[key]


def _readbacks(env):
    st, tg = env.get_state(), env.get_target()
    return dict(maps=env.get_maps(), **{"s_" + k: v for k, v in st.items()}, **{"t_" + k: v for k, v in tg.items()})


@pytest.mark.parametrize("env_id, n", CONFIGS, ids=IDS)
def test_save_does_not_perturb_and_restore_continues(env_id, n):
    """1. A: reset, 37 steps, save, 45 steps. The control's steps 38..82 equal A's (saving perturbs nothing); after a restore
    the same 45 actions give the same 45 records. In those 45 steps every env finishes at least 3 episodes (asserted), so both
    next-episode slots of every env are used and refilled after the snapshot was taken."""
    ctrl, acts = _control(env_id, n), _actions(n)
    assert int(ctrl[2][PRE:PRE + LEN].sum(0).min()) >= 3
    a = _make(env_id, n)
    a.reset()
    head = _run(a, acts[:PRE])
    assert _same(head, _cut(ctrl, 0, PRE))
    snap = a.snapshot().save()
    first = _run(a, acts[PRE:PRE + LEN])
    assert _same(first, _cut(ctrl, PRE, PRE + LEN))
    snap.restore()
    again = _run(a, acts[PRE:PRE + LEN])
    assert _same(again, first)
    assert a.faults() == 0
    snap.close()
    a.close()


@pytest.mark.parametrize("env_id, n", CONFIGS, ids=IDS)
def test_through_the_host_blob_into_a_fresh_handle(env_id, n):
    """2. to_bytes() of A's snapshot, loaded into a handle B of the same configuration that was only reset: B's readbacks
    right after the restore equal A's right after its save, and B's next 45 records are the control's."""
    from active_tracking_rl_amd.vec_env import snapshot_header
    ctrl, acts = _control(env_id, n), _actions(n)
    a = _make(env_id, n)
    a.reset()
    _run(a, acts[:PRE])
    snap = a.snapshot().save()
    want = _readbacks(a)
    blob = snap.to_bytes()
    hdr = snapshot_header(blob)
    assert hdr["num_envs"] == n and hdr["max_episode_steps"] == T_MAX and hdr["seed"] == 1 and hdr["env_id_base"] == 0
    assert hdr["header_bytes"] + hdr["payload_bytes"] == len(blob) == snap.nbytes
    assert hdr["sections"] == {"Track2D-MazePartialNav-v0": 3, "Track2D-BlockPartialRPF-v0": 1}.get(env_id, 0)
    snap.close()
    a.close()
    b = _make(env_id, n)
    b.reset()
    sb = b.snapshot().load_bytes(blob).restore()
    got = _readbacks(b)
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert _same(_run(b, acts[PRE:PRE + LEN]), _cut(ctrl, PRE, PRE + LEN))
    assert b.faults() == 0
    sb.close()
    b.close()


def _mask(n):
    m = torch.zeros(n, dtype=torch.uint8)
    m[0::2] = 1                  # env 0 and every other one ...
    m[n - 1] = 1                 # ... the last env ...
    m[21] = 1                    # ... and both envs (20, 21) of one k_step2 wave
    return m.to(_dev())


@pytest.mark.parametrize("env_id, n", [CONFIGS[0], CONFIGS[2], CONFIGS[3]], ids=[IDS[0], IDS[2], IDS[3]])
def test_masked_restore_and_masked_save(env_id, n):
    """3. After A's 45 steps past the save, a restore of about half the envs: stepped 45 more, the masked envs repeat records
    1..45 (under those steps' actions), the others carry on as the control's steps 46..90 do. Then a masked SAVE of the others:
    the masked envs' rows of the snapshot are unchanged (their words in the blob, and their behaviour after a full restore)
    while the saved envs continue from where they stood (the control's next 45 steps)."""
    ctrl, acts = _control(env_id, n), _actions(n)
    m = _mask(n)
    mb = m.bool()
    assert 0.4 * n < int(mb.sum()) < 0.6 * n and bool(mb[0]) and bool(mb[n - 1]) and bool(mb[20]) and bool(mb[21])
    a = _make(env_id, n)
    a.reset()
    _run(a, acts[:PRE])
    snap = a.snapshot().save()
    _run(a, acts[PRE:PRE + LEN])
    snap.restore(m)
    mixed = torch.where(mb.view(1, 1, n), acts[PRE:PRE + LEN], acts[PRE + LEN:PRE + 2 * LEN])
    second = _run(a, mixed)
    assert _same(second, _cut(ctrl, PRE, PRE + LEN), mb)
    assert _same(second, _cut(ctrl, PRE + LEN, PRE + 2 * LEN), ~mb)
    before = np.frombuffer(snap.to_bytes(), np.uint8)
    snap.save(1 - m)
    after = np.frombuffer(snap.to_bytes(), np.uint8)
    words = lambda blob, k: blob[96 + n * 1024 + 4 * n * k:][:4 * n].view(np.uint32)      # word array k after the maps: pos, goals, cnt, episode
    keep, moved = mb.cpu().numpy(), False
    for k in range(4):
        assert np.array_equal(words(before, k)[keep], words(after, k)[keep]), k
        moved = moved or not np.array_equal(words(before, k)[~keep], words(after, k)[~keep])
    assert moved
    snap.restore()
    mixed = torch.where(mb.view(1, 1, n), acts[PRE:PRE + LEN], acts[PRE + 2 * LEN:PRE + 3 * LEN])
    third = _run(a, mixed)
    assert _same(third, _cut(ctrl, PRE, PRE + LEN), mb)
    assert _same(third, _cut(ctrl, PRE + 2 * LEN, PRE + 3 * LEN), ~mb)
    assert a.faults() == 0
    snap.close()
    a.close()


def _steps_like_a_control(env, make_control, n, k=3):
    """After a refusal: k more steps of `env` equal those of a control handle of the same configuration in the same position."""
    acts = _actions(n)[:k]
    c = make_control()
    c.reset()
    ok = _same(_run(env, acts), _run(c, acts))
    c.close()
    return ok


@pytest.mark.parametrize("field, kw", [("seed", dict(seed=2)), ("env_id_base", dict(env_id_base=N)), ("num_envs", dict(n=64)),
                                       ("max_episode_steps", dict(max_episode_steps=13))],
                         ids=["seed", "env_id_base", "N", "max_episode_steps"])
def test_refuses_a_blob_of_another_configuration(field, kw):
    """4. A blob of the PZR handle (seed 1, base 0, 70 envs, 12 steps) is refused by a handle that differs in one field, with a
    message naming it, before anything reaches the device: the handle then steps like one that was never asked."""
    from active_tracking_rl_amd.vec_env import T2DError
    a = _make()
    a.reset()
    sa = a.snapshot().save()
    blob = sa.to_bytes()
    sa.close()
    a.close()
    n = kw.get("n", N)
    b = _make(**kw)
    b.reset()
    sb = b.snapshot()
    with pytest.raises(T2DError, match=r"t2d_snapshot_import failed \(-1\): .*\b%s\b" % field):
        sb.load_bytes(blob)
    with pytest.raises(T2DError, match="holds nothing yet"):
        sb.restore()
    assert _steps_like_a_control(b, lambda: _make(**kw), n)
    sb.close()
    b.close()


def test_refuses_trace_stores_foreign_handles_changed_cfg_and_damaged_blobs():
    """4. (the rest) A handle with trace_attach() called; a snapshot used with a handle other than its own; a blob whose handle
    differs in one env's cfg word (one env of level 1); a blob with a damaged magic, version or size."""
    from active_tracking_rl_amd.vec_env import T2DError, state_lib
    t = _make(auto_reset=False)
    t.trace_attach()
    t.reset()
    with pytest.raises(T2DError, match=r"t2d_snapshot_create failed \(-1\): .*trace store"):
        t.snapshot()
    assert _steps_like_a_control(t, lambda: _make(auto_reset=False), N)
    t.close()
    a, b = _make(), _make()
    a.reset(); b.reset()
    sa, sb = a.snapshot().save(), b.snapshot().save()
    with pytest.raises(T2DError, match="created for another handle"):
        state_lib().t2d_snapshot_restore(b.h, sa.s, None, b._stream())
    with pytest.raises(T2DError, match="created for another handle"):
        state_lib().t2d_snapshot_save(b.h, sa.s, None, b._stream())
    levels = np.zeros(N, np.uint8)
    levels[5] = 1
    c = _make(level_per_env=levels)
    c.reset()
    sc = c.snapshot().save()
    with pytest.raises(T2DError, match=r"\bcfg\b"):
        sa.load_bytes(sc.to_bytes())
    good = sb.to_bytes()
    for damaged, text in ((b"X" + good[1:], "magic"), (good[:8] + b"\x02" + good[9:], "version"), (good[:-4], "size"),
                          (good[:40], "shorter than")):
        with pytest.raises(T2DError, match=text):
            sa.load_bytes(damaged)
    with pytest.raises(T2DError, match="first save into a snapshot must cover every env"):
        a.snapshot().save(_mask(N))
    sa.restore()                         # the refused imports left the snapshot's own contents alone
    assert _steps_like_a_control(a, _make, N) and _steps_like_a_control(b, _make, N)
    for x in (sa, sb, sc, a, b, c):
        x.close()


def test_restore_between_replays_of_a_captured_chunk():
    """5. A 20-step chunk (one generator stamp cycle) of step calls with fixed action tensors, captured with torch.cuda.graph
    as GreedyEvaluator captures its chunk: replayed twice, the snapshot taken before the first replay restored, replayed twice
    again — chunks 1 = 3 and 2 = 4 (the handle's arrays keep their addresses, a captured chunk starts at stamp 0)."""
    T = 20
    a = _make()
    assert a.generator_cycle == T
    acts = _actions(N)[:T]
    a.reset()
    _run(a, acts)                        # one eager cycle first: every kernel of the chunk has run before the capture
    out = (torch.empty((T, N, 2, 13, 13), device=_dev()), torch.empty((T, N, 2), device=_dev()),
           torch.empty((T, N), dtype=torch.uint8, device=_dev()))
    snap = a.snapshot().save()           # (flushes: no generator launch in flight and stamp 0 when the capture starts)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for t in range(T):
            a.step(acts[t, 0], acts[t, 1], out=(out[0][t], out[1][t], out[2][t]))
        a.generator_join()
    chunks = []
    for i in range(4):
        if i == 2:
            snap.restore()
        g.replay()
        chunks.append(tuple(x.clone() for x in out))
    torch.cuda.synchronize()
    assert _same(chunks[0], chunks[2]) and _same(chunks[1], chunks[3])
    assert not _same(chunks[0], chunks[1]) and int(chunks[0][2].sum()) >= N
    assert a.faults() == 0
    snap.close()
    a.close()


def test_vec_env_state_carries_frames_and_inv_flags():
    """6. VecEnv(stack_frames=2, rescale=True, inv=True): clone_state, 30 steps, restore_state, the same 30 actions under the
    same torch seed (the per-episode coin flips) give identical stacked observations; observe() after the restore is the
    observation that preceded the clone."""
    from active_tracking_rl_amd.environment import VecEnv
    n = 16
    env = VecEnv(PZR, n, device="cuda:0", stack_frames=2, rescale=True, inv=True, max_episode_steps=T_MAX)
    acts = _actions(n)[:40]
    torch.manual_seed(5)
    obs = env.reset()
    for a in acts[:10]:
        obs, _, _, _ = env.step([a[0], a[1]])
    before = obs.clone()
    assert torch.equal(env.observe(), before)
    st = env.clone_state()

    def play():
        torch.manual_seed(7)
        rec = [env.step([a[0], a[1]])[:3] for a in acts[10:]]
        return tuple(torch.stack([r[k].clone() for r in rec]) for k in range(3))
    first = play()
    assert int(first[2].sum()) >= 2 * n and not torch.equal(env.observe(), before)
    env.restore_state(st)
    assert torch.equal(env.observe(), before) and env.observe().shape == (n, 2, 2, 1, 13, 13)
    assert _same(play(), first)
    env.close()


def test_track2d_env_clone_and_restore():
    """6. Track2DEnv: clone_state / restore_state round trip over 25 gym-protocol steps (finished episodes reset); an env with
    traces=True refuses both with NotImplementedError."""
    from active_tracking_rl_amd.environment import Track2DEnv
    env = Track2DEnv(PZR, device="cuda:0", seed=3)
    rs = np.random.RandomState(11)
    moves = rs.randint(0, 4, (30, 2))
    env.reset()
    for a in moves[:5]:
        env.step(a)
    st = env.clone_state()

    def play():
        rec = []
        for a in moves[5:]:
            o, r, d, info = env.step(a)
            rec.append((o.copy(), r.copy(), d, info["distance"]))
            if d:
                rec.append((env.reset().copy(),))
        return rec
    first = play()
    env.restore_state(st)
    again = play()
    assert len(first) == len(again) >= 25
    for x, y in zip(first, again):
        assert len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y))
    env.close()
    traced = Track2DEnv(PZR, device="cuda:0", seed=3, traces=True)
    traced.reset()
    with pytest.raises(NotImplementedError, match="traces=True"):
        traced.clone_state()
    with pytest.raises(NotImplementedError, match="traces=True"):
        traced.restore_state(st)
    traced.close()


@pytest.mark.parametrize("net", ["tat-maze-lstm", "maze-gru"])
def test_agent_shard_state_continues_in_a_second_player(net):
    """7. 64 envs, num_steps=5, through train.make_player and train.rollout. Player P: two rollouts, shard_state(), a third
    rollout. A second player Q built the same way (same seed: same weights) loads the shard state and does one rollout: its
    store, actions, hxs and cxs equal P's third rollout bit for bit. (maze-gru runs on the path without a rollout cache.)"""
    from active_tracking_rl_amd.train import default_args, make_player, rollout

    def player():
        args = default_args(env=PZR, network=net, aux="reward" if "tat" in net else "none", num_envs=64, num_steps=5, seed=23)
        args.gpu_ids = [0]
        return make_player(args, _dev())[0]

    def result(p):
        acts = p._actions_buf.clone() if p._actions_buf is not None else torch.stack(p.actions).transpose(1, 2).clone()
        return [x.clone() for x in p._buf] + [acts, p.hxs.clone(), p.cxs.clone(), p.eps_len.clone(), p.done.clone(), p.state.clone()]
    P = player()
    assert bool(getattr(P.model, "gru_core", False) and not P.model.cacheable_core) == (net == "maze-gru")
    for _ in range(2):
        rollout(P, 5)
        P.clear_actions()                # (what compute_grads does at the end of an iteration: the per-step lists start over)
    torch.cuda.synchronize()
    d = P.shard_state()
    assert d["env"].dtype == torch.uint8 and all(not v.is_cuda for v in d.values() if torch.is_tensor(v))
    assert d["meta"] == dict(env=PZR, N=64, env_id_base=0, network=net, rnn_out=128) and "sampler_counter" in d
    rollout(P, 5)
    want = result(P)
    Q = player()
    Q.load_shard_state(d)
    rollout(Q, 5)
    got = result(Q)
    for i, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(x, y), i
    assert float(want[4].abs().max()) > 0
    with pytest.raises(ValueError, match="rnn_out"):
        Q.load_shard_state(dict(d, meta=dict(d["meta"], rnn_out=64)))
    P.env.close()
    Q.env.close()


def test_main_saves_and_loads_a_shard(tmp_path):
    """8. main.py --save-shard-state writes shard-0.pt; a second child with --load-shard-state on that file runs to its end and
    prints the restored line; a third with --num-envs 32 exits non-zero and names N. Each child under its own time limit."""
    common = [sys.executable, os.path.join(ROOT, "main.py"), "--num-steps", "5", "--max-step", "4", "--test-every", "100",
              "--log-every", "0", "--no-graph", "--test-eps", "2"]

    def child(name, *flags):
        return subprocess.run(common + ["--log-dir", os.path.join(str(tmp_path), name)] + list(flags), capture_output=True, text=True,
                              cwd=ROOT, timeout=300)
    r = child("save", "--num-envs", "64", "--save-shard-state")
    assert r.returncode == 0, r.stderr[-3000:]
    found = [os.path.join(dp, "shard-0.pt") for dp, _, files in os.walk(str(tmp_path)) if "shard-0.pt" in files]
    assert len(found) == 1, found
    d = torch.load(found[0], map_location="cpu")
    assert d["meta"]["N"] == 64 and d["hxs"].shape == (64, 2, 128)
    r = child("load", "--num-envs", "64", "--load-shard-state", found[0])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "burn-in skipped: the shard was restored from --load-shard-state" in r.stderr
    r = child("load32", "--num-envs", "32", "--load-shard-state", os.path.dirname(found[0]))
    assert r.returncode != 0 and "ValueError" in r.stderr and "shard's N is 64" in r.stderr, r.stderr[-3000:]
