"""-m gpu: the training-episode statistics on the device — the two kernels against their host models bit for bit, their
refusals, the accounts kept inside the replayed rollout graphs of both schedules (episodes crossing from one replica's rollout
into the other's included) and on a rollout path that does not end in k_act_step, the same trained weights with and without
the statistics attached, and main.py --episode-stats end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import episode_stats_spec as es
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T = 20
LIMIT = 37        # a short TimeLimit (the trick of test_timed_region_parity_gpu.py): many episodes end, by time limit and before it


def _launch(rew, done, run_ret, run_len, fin, success_len):
    from active_tracking_rl_amd import episode_stats
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    episode_stats.episode_stats(rew.data_ptr(), rew.stride(), done.data_ptr(), done.stride(), run_ret.data_ptr(), run_len.data_ptr(),
                                fin.data_ptr(), done.shape[0], done.shape[1], success_len, stream)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("steps", [1, 20])
@pytest.mark.parametrize("n", [1, 33, 64, 4096])
def test_kernels_equal_the_host_models_bit_for_bit(n, steps, strided):
    """Three successive calls on random rew / done continue the same accounts: run_ret, run_len and fin equal account()'s, totals
    equals drain_model()'s, fin is all zero after the drain and the running accounts are untouched by it. strided: the inputs
    are slices of a larger store (rew [T+3, n+5, 3] -> [T, n, 2], done [T+3, n+5] -> [T, n])."""
    from active_tracking_rl_amd import episode_stats
    S = 9
    run_ret = torch.zeros((n, 2), dtype=torch.float32, device=DEV)
    run_len = torch.zeros(n, dtype=torch.int32, device=DEV)
    fin = torch.zeros((n, 8), dtype=torch.float64, device=DEV)
    totals = torch.full((8,), -1.0, dtype=torch.float64, device=DEV)
    want = (None, None, None)
    for call in range(3):
        rew, done = es.random_inputs(steps, n, seed=1000 * call + 7 * n + steps, p_done=0.12)
        if strided:
            big_r = torch.full((steps + 3, n + 5, 3), float("nan"), dtype=torch.float32, device=DEV)
            big_d = torch.ones((steps + 3, n + 5), dtype=torch.uint8, device=DEV)
            d_rew, d_done = big_r[2:2 + steps, 3:3 + n, 1:], big_d[1:1 + steps, 2:2 + n]
            d_rew.copy_(torch.from_numpy(rew))
            d_done.copy_(torch.from_numpy(done))
            # views into the store: its strides and an offset (at n = 1, steps = 1 torch calls such a view contiguous)
            assert d_rew.stride() == big_r.stride() and d_done.stride() == big_d.stride()
            assert d_rew.data_ptr() != big_r.data_ptr() and d_done.data_ptr() != big_d.data_ptr()
        else:
            d_rew, d_done = torch.from_numpy(rew).to(DEV), torch.from_numpy(done).to(DEV)
        _launch(d_rew, d_done, run_ret, run_len, fin, S)
        want = episode_stats.account(rew, done, *want, success_len=S)
        torch.cuda.synchronize()
        es.assert_accounts_equal((run_ret.cpu().numpy(), run_len.cpu().numpy(), fin.cpu().numpy()), want, ("call", call))
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    episode_stats.episode_stats_drain(fin.data_ptr(), totals.data_ptr(), n, stream)
    torch.cuda.synchronize()
    assert es.same_bits(totals.cpu().numpy(), episode_stats.drain_model(want[2]))
    assert not fin.cpu().numpy().any()
    assert es.same_bits(run_ret.cpu().numpy(), want[0]) and es.same_bits(run_len.cpu().numpy(), want[1])
    if n * steps >= 64:
        assert totals[0].item() >= 1                     # (the comparison was not one of empty accounts)


def _short_env(env_id, n, seed=1, **kw):
    from active_tracking_rl_amd.environment import VecEnv
    return VecEnv(env_id, n, device=DEV, seed=seed, max_episode_steps=LIMIT, **kw)


def _player(env_id, n, seed=1, env_kw=None, **over):
    from active_tracking_rl_amd.train import default_args, make_player
    args = default_args(env=env_id, num_envs=n, num_steps=T, seed=seed, **over)
    args.gpu_ids = [0]
    env = _short_env(env_id, n, seed, **(env_kw if env_kw is not None else dict(obs_u8=True)))
    player, opt = make_player(args, torch.device(DEV), 0, 1, env=env)
    return args, env, player, opt


def test_refusals_on_the_device():
    """Null pointers and N = 0 with real device tensors for the rest; an object attached to a shard that has already stepped;
    a second object on the same shard."""
    from active_tracking_rl_amd import episode_stats
    from active_tracking_rl_amd.train import rollout
    n = 64
    rew = torch.zeros((T, n, 2), device=DEV)
    done = torch.zeros((T, n), dtype=torch.uint8, device=DEV)
    run_ret, run_len = torch.zeros((n, 2), device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    fin, totals = torch.zeros((n, 8), dtype=torch.float64, device=DEV), torch.zeros(8, dtype=torch.float64, device=DEV)
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    ok = [rew.data_ptr(), rew.stride(), done.data_ptr(), done.stride(), run_ret.data_ptr(), run_len.data_ptr(), fin.data_ptr(), T, n,
          500, stream]
    for i in (0, 2, 4, 5, 6):
        bad = list(ok)
        bad[i] = 0
        with pytest.raises(RuntimeError, match=r"^atr_episode_stats failed \(-1\): .*null pointer"):
            episode_stats.episode_stats(*bad)
    bad = list(ok)
    bad[8] = 0
    with pytest.raises(RuntimeError, match=r"^atr_episode_stats failed \(-1\): .*N > 0"):
        episode_stats.episode_stats(*bad)
    with pytest.raises(RuntimeError, match=r"^atr_episode_stats_drain failed \(-1\): .*null pointer"):
        episode_stats.episode_stats_drain(0, totals.data_ptr(), n, stream)
    with pytest.raises(RuntimeError, match=r"^atr_episode_stats_drain failed \(-1\): .*N > 0"):
        episode_stats.episode_stats_drain(fin.data_ptr(), totals.data_ptr(), 0, stream)
    torch.cuda.synchronize()
    assert not fin.cpu().numpy().any() and not run_len.cpu().numpy().any()
    args, env, player, opt = _player("Track2D-BlockPartialPZR-v0", n)
    try:
        rollout(player, 3)
        player.clear_actions()
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="freshly reset shard"):
            episode_stats.EpisodeStats(env, torch.device(DEV))
        assert getattr(env, "episode_stats", None) is None
        player.reset()                                   # a reset shard is fresh again
        st = episode_stats.EpisodeStats(env, torch.device(DEV))
        assert env.episode_stats is st and st.success_len == env.core_max_steps()
        with pytest.raises(RuntimeError, match="already has episode statistics"):
            episode_stats.EpisodeStats(env, torch.device(DEV))
        st.run_len.fill_(5)
        player.reset()                                   # Agent.reset() zeroes the running accounts of an attached object
        torch.cuda.synchronize()
        assert not st.run_len.cpu().numpy().any()
    finally:
        env.close()


def _check_against_the_store(st, chunks, n, what):
    """The device accounts against account() applied to the concatenation of every rollout's stored rewards / done flags."""
    from active_tracking_rl_amd import episode_stats
    torch.cuda.synchronize()
    rew = np.concatenate([c[0] for c in chunks], 0).reshape(-1, n, 2)
    done = np.concatenate([c[1] for c in chunks], 0)
    want = episode_stats.account(rew, done, success_len=st.success_len)
    episodes = want[2][:, 0].sum()
    print("%s: %d steps, %d finished episodes over %d envs, %d successes" % (what, done.shape[0], episodes, n, want[2][:, 7].sum()))
    assert episodes >= n, (what, "the host model shows less than one finished episode per env", episodes)
    es.assert_accounts_equal((st.run_ret.cpu().numpy(), st.run_len.cpu().numpy(), st.fin.cpu().numpy()), want, what)
    totals = st.drain()
    torch.cuda.synchronize()
    assert es.same_bits(totals.cpu().numpy(), episode_stats.drain_model(want[2])) and not st.fin.cpu().numpy().any()
    s = episode_stats.summarize(totals)
    assert s["episodes"] == episodes and 0.0 < s["S_rate"] < 1.0, s
    assert all(np.isfinite(v) for v in s["R_mean"] + s["R_std"] + s["R_step"] + [s["EL_mean"], s["EL_std"]])
    assert 1.0 <= s["EL_mean"] <= LIMIT
    return s


def _keep(chunks, agent):
    chunks.append((agent._buf[1].cpu().numpy().copy(), agent._buf[2].cpu().numpy().copy()))


@pytest.mark.parametrize("n", [64, 512])
@pytest.mark.parametrize("schedule", ["synchronous", "pipelined"])
def test_accounts_inside_the_replayed_graphs(schedule, n):
    """GraphedIteration / PipelinedIteration over a 37-step TimeLimit shard of Track2D-BlockPartialPZR-v0 with the statistics
    attached: two eager iterations (what the drivers' warm-up does), then 12 replayed ones; every rollout's stored rew / done
    is cloned after it ran. The device accounts equal account() of the concatenation bit for bit — in the pipelined case the
    two replicas alternate, so episodes cross from one replica's rollout into the other's."""
    from active_tracking_rl_amd import episode_stats
    from active_tracking_rl_amd.train import GraphedIteration, PipelinedIteration, rollout
    args, env, player, opt = _player("Track2D-BlockPartialPZR-v0", n, seed=3, network="tat-maze-lstm", aux="reward", train_mode=-1)
    try:
        st = episode_stats.EpisodeStats(env, torch.device(DEV), success_len=LIMIT)
        chunks = []
        for _ in range(2):
            rollout(player, T)
            torch.cuda.synchronize()
            _keep(chunks, player)
            player.optimize(None, opt, player.model, -1, torch.device(DEV))
        if schedule == "synchronous":
            it = GraphedIteration(player, opt, args, warmup=0)
            for _ in range(12):
                it.run()
                torch.cuda.synchronize()
                _keep(chunks, player)
        else:
            it = PipelinedIteration(player, opt, args, warmup=0)
            assert not it.serial
            for _ in range(6):
                it.run()
                it.run()
                it.finish()
                torch.cuda.synchronize()
                _keep(chunks, it.players[0])
                _keep(chunks, it.players[1])
        assert len(chunks) == 14 and env.core.faults() == 0
        _check_against_the_store(st, chunks, n, "%s %d envs" % (schedule, n))
    finally:
        env.close()


@pytest.mark.parametrize("env_id,env_kw,over", [("Track2D-BlockPartialRPF-v0", {}, {}),
                                                ("Track2D-BlockPartialPZR-v0", {"stack_frames": 2}, {"stack_frames": 2})])
def test_accounts_on_a_step_that_does_not_end_in_the_fused_env_step(env_id, env_kw, over):
    """The eager loop on an RPF id (the env steps in a launch of its own, into the rollout store) and with two stacked frames
    (no rollout store: the statistics read the stacked lists). Same check as for the graphs."""
    from active_tracking_rl_amd import episode_stats
    from active_tracking_rl_amd.train import rollout
    n = 64
    args, env, player, opt = _player(env_id, n, seed=5, env_kw=env_kw, **over)
    try:
        st = episode_stats.EpisodeStats(env, torch.device(DEV), success_len=LIMIT)
        chunks = []
        for _ in range(8):
            rollout(player, T)
            torch.cuda.synchronize()
            assert not getattr(player.model, "env_stepped", False)
            if player._buf is not None:
                _keep(chunks, player)
            else:
                chunks.append((torch.stack(player.rewards[-T:]).cpu().numpy().reshape(T, n, 2),
                               torch.stack(player.dones[-T:]).cpu().numpy()))
            player.optimize(None, opt, player.model, -1, torch.device(DEV))
        assert (player._buf is None) == bool(env_kw.get("stack_frames"))
        _check_against_the_store(st, chunks, n, env_id + str(env_kw))
    finally:
        env.close()


def _trained_weights(schedule, attach, n=512, iters=6):
    from active_tracking_rl_amd import episode_stats
    from active_tracking_rl_amd.train import GraphedIteration, PipelinedIteration
    args, env, player, opt = _player("Track2D-BlockPartialPZR-v0", n, seed=2, network="tat-maze-lstm", aux="reward", train_mode=-1)
    try:
        st = episode_stats.EpisodeStats(env, torch.device(DEV), success_len=LIMIT) if attach else None
        it = (GraphedIteration if schedule == "synchronous" else PipelinedIteration)(player, opt, args)
        for _ in range(iters):
            it.run()
        it.finish()
        torch.cuda.synchronize()
        steps = int(st.fin[:, 5].sum().item() + st.run_len.sum().item()) if attach else None
        return opt.bucket.flat.detach().clone(), steps
    finally:
        env.close()


@pytest.mark.parametrize("schedule", ["synchronous", "pipelined"])
def test_statistics_do_not_touch_training(schedule):
    """Same seed, with the statistics attached and without: the flat parameter bucket is torch.equal after 6 iterations. With
    them attached every env step of the run (the schedule's two warm-up iterations included) is in exactly one account."""
    with_stats, steps = _trained_weights(schedule, True)
    without, _ = _trained_weights(schedule, False)
    assert torch.isfinite(without).all() and torch.equal(with_stats, without)
    assert steps == (2 + 6) * T * 512


def _run_main(tmp_path, name, *flags):
    log_dir = os.path.join(str(tmp_path), name)
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--env", "Track2D-BlockPartialPZR-v0", "--num-envs", "1024", "--seed", "4",
           "--schedule", "synchronous", "--log-every", "2", "--test-every", "100000", "--test-eps", "2", "--log-dir", log_dir] + list(flags)
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=420)
    assert r.returncode == 0, r.stderr[-3000:]
    records = []
    for dirpath, _, files in os.walk(log_dir):
        if "scalars.jsonl" in files and os.path.basename(dirpath) == "Agent:0":
            records += [json.loads(ln) for ln in open(os.path.join(dirpath, "scalars.jsonl"))]
    assert records, "no train scalars were written"
    return records, r.stderr


def test_main_writes_training_episode_scalars(tmp_path):
    """main.py --episode-stats (a subprocess under its own timeout): every --log-every record holds train/episodes, and
    train/reward_0, train/reward_1, train/eps_len, train/success_rate with finite values once episodes have finished. The first
    record after --burn-in 40 counts the episodes of its own two iterations only: the burn-in's were drained and dropped, so
    it is smaller than everything a run without burn-in has counted by its iteration 42 (same seed, same 42 iterations of env
    steps behind it) — without the post-burn-in drain it would hold about as many. Without the flag none of the tags appear."""
    from active_tracking_rl_amd.episode_stats import TAGS
    burn, err = _run_main(tmp_path, "burn", "--episode-stats", "--burn-in", "40", "--max-step", "5")
    by_tag = lambda recs, tag: [(r["step"], r["value"]) for r in recs if r["tag"] == tag]
    for tag in ("train/reward_0", "train/reward_1", "train/eps_len", "train/success_rate", "train/episodes"):
        vals = by_tag(burn, tag)
        assert vals and all(np.isfinite(v) for _, v in vals), tag
    assert len(by_tag(burn, "train/episodes")) == 3 and "train episodes at" in err           # records at iterations 2, 4, 6
    first_burn = by_tag(burn, "train/episodes")[0][1]
    assert first_burn >= 1 and by_tag(burn, "train/eps_len")[0][1] >= 1.0
    plain, _ = _run_main(tmp_path, "plain", "--episode-stats", "--burn-in", "0", "--max-step", "43")
    eps = by_tag(plain, "train/episodes")
    counted_by_42 = sum(v for step, v in eps if step <= 42 * 20 * 1024)
    print("first record after --burn-in 40: %d episodes; --burn-in 0: first record %d, through iteration 42: %d"
          % (first_burn, eps[0][1], counted_by_42))
    assert first_burn < counted_by_42
    off, err = _run_main(tmp_path, "off", "--burn-in", "0", "--max-step", "3")
    assert not [r for r in off if r["tag"] in TAGS] and "train episodes at" not in err
    assert by_tag(off, "train/fps")
