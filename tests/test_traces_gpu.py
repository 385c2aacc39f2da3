"""-m gpu: the device's episode traces and renderer (include/track2d_trace.h, csrc/render_hip.hip) against the reference's own
record (tests/golden/traces.npz) and the host model (tests/render_spec.py). The fixture's four episodes are injected, one per
env plus a duplicate, stepped with the recorded actions and recorded ONCE (module fixture `replay`); the tests read that
record. Tolerance: none — everything here is bytes and small integers."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_spec as rs
from conftest import ROOT

pytestmark = pytest.mark.gpu

MODE = {"PZR": 1, "Adv": 0}
RENDER_IDS = [4, 3, 2, 1, 0, 2]            # reversed, with a repeat
RGB_STEPS = (0, 5, 13, 40)
PITCH_EXTRA = {1: 0, 3: 48, 4: 0}          # scale 3 on a canvas wider than the minimum


def _make(eps, **kw):
    from active_tracking_rl_amd.vec_env import VecTrack2D
    modes = np.array([MODE["Adv"] if "Nav" in ep["env_id"] else MODE["PZR"] for ep in eps], np.uint8)
    env = VecTrack2D(num_envs=len(eps), map_type="Block", target_mode="Adv", level=1, auto_reset=False, max_episode_steps=500,
                     target_mode_per_env=modes, **kw)
    for i, ep in enumerate(eps):           # (per env: the sides differ)
        env.inject(ep["maze"], ep["init"].reshape(1, 4), first=i)
    return env


def _actions(eps, T):
    acts = np.zeros((T, len(eps), 2), np.int64)
    for i, ep in enumerate(eps):
        acts[: len(ep["actions"]), i] = ep["actions"][:T]
    return torch.from_numpy(acts).cuda()


def _canvas_ok(env, scale, extra):
    """render_rgb of RENDER_IDS on a pre-filled canvas: (frames [6, H, W, 3], whether every pad byte is 0)."""
    row = 486 * scale
    pitch = (row + 15) // 16 * 16 + extra
    canvas = torch.full((len(RENDER_IDS), 82 * scale, pitch), 0xAA, dtype=torch.uint8, device="cuda")
    img = env.render_rgb(RENDER_IDS, scale=scale, pitch=pitch, out=canvas)
    return img.cpu().numpy(), bool((canvas[:, :, row:] == 0).all().item()), pitch > row


@pytest.fixture(scope="module")
def fixture():
    return rs.load_fixture()


@pytest.fixture(scope="module")
def replay(fixture):
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    eps, palette, _ = fixture
    eps = list(eps) + [eps[1]]
    T = max(len(ep["actions"]) for ep in eps)
    env = _make(eps)
    env.trace_attach()
    assert env.trace_capacity == 500
    env.trace_begin()
    acts = _actions(eps, T)
    rec = dict(eps=eps, T=T, tr=[], cells=[], cells_plain=[], partial=[], rgb={}, done=[])

    def snap(t):
        rec["tr"].append(env.traces())
        c, p = env.render_cells(RENDER_IDS, trace=True)
        rec["cells"].append(c.cpu().numpy()); rec["partial"].append(p.cpu().numpy())
        rec["cells_plain"].append(env.render_cells(RENDER_IDS, trace=False)[0].cpu().numpy())
        if t in RGB_STEPS:
            for scale, extra in PITCH_EXTRA.items():
                rec["rgb"][(t, scale)] = _canvas_ok(env, scale, extra)

    snap(0)
    for t in range(T):
        _, _, done = env.step(acts[t, :, 0].contiguous(), acts[t, :, 1].contiguous())
        env.trace_append(done)
        rec["done"].append(done.cpu().numpy())
        snap(t + 1)
    rec["faults"] = env.faults()
    env.close()
    return rec


def test_trace_get_reproduces_the_reference_traces(replay):
    """traces and traces_relative at every step of every episode, assembled from the store as the header says."""
    assert replay["faults"] == 0
    checked = 0
    for i, ep in enumerate(replay["eps"]):
        assert np.array_equal(replay["tr"][0]["pos"][i, 0], ep["init"]) and replay["tr"][0]["len"][i] == 1
        rel0 = [ep["init"][k] - ep["init"][0] for k in range(2)]
        assert np.array_equal(np.array(rel0), ep["rel0"])
        for t in range(1, len(ep["actions"]) + 1):
            tr = replay["tr"][t]
            n, pos = int(tr["len"][i]), tr["pos"][i].astype(np.int64)
            assert n == t + 1 and tr["dropped"][i] == 0, (ep["name"], t)
            traces = [pos[0, 0].tolist()] + [pos[k, 1].tolist() for k in range(1, n)]
            assert traces == ep["traces"][: t + 1].tolist(), (ep["name"], t)
            cur = pos[n - 1]
            assert np.array_equal(cur, ep["pos"][t - 1])
            rel = np.array([[cur[a] - cur[b] for a in range(2)] for b in range(2)])
            assert np.array_equal(rel, ep["rel"][t - 1]), (ep["name"], t)
            assert bool(replay["done"][t - 1][i]) == bool(ep["done"][t - 1])
            checked += 1
    assert checked >= 120


def test_entries_stop_after_done_while_others_go_on(replay):
    eps, T = replay["eps"], replay["T"]
    end = len(eps[3]["actions"])                       # the far-counter episode: done at its last step
    assert eps[3]["done"][-1] == 1 and end < T
    final = replay["tr"][end]
    for t in range(end, T + 1):
        tr = replay["tr"][t]
        assert tr["len"][3] == end + 1 and tr["dropped"][3] == 0
        assert np.array_equal(tr["pos"][3, : end + 1], final["pos"][3, : end + 1])
        assert tr["len"][1] == t + 1 and tr["len"][4] == t + 1          # the 40-step episode and its duplicate go on
    assert np.array_equal(replay["tr"][T]["pos"][1], replay["tr"][T]["pos"][4])


def test_render_cells_equal_the_reference_images(replay):
    """The painted full observation (with and without T2D_RENDER_TRACE) and the tracker's window at every step, ids reversed
    and repeated; 255 outside the side-81 map."""
    eps = replay["eps"]
    checked = 0
    for t in range(replay["T"] + 1):
        for k, i in enumerate(RENDER_IDS):
            ep = eps[i]
            if t > len(ep["actions"]):
                continue
            want, plain, part = (ep["cells0"], ep["full0"], ep["partial0"]) if t == 0 else \
                (ep["cells"][t - 1], ep["full"][t - 1], ep["partial"][t - 1])
            assert np.array_equal(replay["cells"][t][k], want), (ep["name"], t, k)
            assert np.array_equal(replay["cells_plain"][t][k], plain), (ep["name"], t, k)
            assert np.array_equal(replay["partial"][t][k], part), (ep["name"], t, k)
            assert not (replay["cells_plain"][t][k] == 6).any()
            checked += 1
        assert np.array_equal(replay["cells"][t][2], replay["cells"][t][5])          # the repeated id
    c81 = replay["cells"][3][2]
    assert eps[2]["side"] == 81 and (c81[81, :] == 255).all() and (c81[:, 81] == 255).all() and (c81[:81, :81] != 255).all()
    assert (np.stack([replay["cells"][t][3] for t in range(2, 30)]) == 6).any()
    assert checked >= 150


@pytest.mark.parametrize("scale", [1, 3, 4])
def test_render_rgb_equals_the_host_model(replay, fixture, scale):
    """Byte for byte the palette image of the fixture's cells and window on the fixed canvas; pad bytes written as 0."""
    eps, palette = replay["eps"], fixture[1]
    checked = 0
    for t in RGB_STEPS:
        img, pad_zero, padded = replay["rgb"][(t, scale)]
        assert img.shape == (len(RENDER_IDS), 82 * scale, 162 * scale, 3) and pad_zero
        assert padded == (PITCH_EXTRA[scale] > 0 or (486 * scale) % 16 != 0)
        for k, i in enumerate(RENDER_IDS):
            ep = eps[i]
            if t > len(ep["actions"]):
                continue
            cells, part = (ep["cells0"], ep["partial0"]) if t == 0 else (ep["cells"][t - 1], ep["partial"][t - 1])
            assert np.array_equal(img[k], rs.rgb(cells, part, palette, scale)), (ep["name"], t, scale)
            checked += 1
    assert checked >= 12


def test_capacity_overflow_and_masked_begin(fixture):
    """Capacity 4 on a 12-step episode: len stops at 5 and 8 appends are dropped; the store of the next env (never begun) is
    not touched; a masked begin restarts only the masked env."""
    ep = fixture[0][1]
    env = _make([ep, ep])
    env.trace_attach(4)
    mask = torch.tensor([1, 0], dtype=torch.uint8, device="cuda")
    env.trace_begin(mask)
    before = env.traces()
    assert before["len"].tolist() == [1, 0] and not before["pos"][1].any()
    acts = _actions([ep, ep], 12)
    for t in range(12):
        _, _, done = env.step(acts[t, :, 0].contiguous(), acts[t, :, 1].contiguous())
        env.trace_append(done)
        assert not done.any().item()
    tr = env.traces()
    assert tr["len"].tolist() == [5, 0] and tr["dropped"].tolist() == [8, 0]
    assert np.array_equal(tr["pos"][0, 0], ep["init"]) and np.array_equal(tr["pos"][0, 1:5], ep["pos"][:4])
    assert not tr["pos"][1].any()                      # slot 0 .. 4 of the neighbour: as allocated
    cells, _ = env.render_cells([0])                   # paints traces[:-1] of what was kept: the spawn and three target cells
    want = rs.full_obs(ep["maze"], ep["pos"][11].tolist())
    for r, c in [ep["init"][0].tolist()] + [ep["pos"][k][1].tolist() for k in range(3)]:
        want[r, c] = 6
    assert np.array_equal(cells[0].cpu().numpy(), want)
    env.trace_begin(1 - mask)                          # now only env 1: slot 0 = where it stands, env 0 as it was
    tr2 = env.traces()
    assert tr2["len"].tolist() == [5, 1] and tr2["dropped"].tolist() == [8, 0]
    assert np.array_equal(tr2["pos"][0], tr["pos"][0]) and np.array_equal(tr2["pos"][1, 0], ep["pos"][11])
    _, _, done = env.step(acts[0, :, 0].contiguous(), acts[0, :, 1].contiguous())
    env.trace_append(done)
    tr3 = env.traces()
    assert tr3["len"].tolist() == [5, 2] and tr3["dropped"].tolist() == [9, 0]
    assert env.faults() == 0
    env.close()


def test_bad_arguments_are_refused_with_text(fixture):
    from active_tracking_rl_amd import vec_env
    T2DError = vec_env.T2DError
    auto = vec_env.VecTrack2D("Track2D-BlockPartialPZR-v0", num_envs=2)            # auto_reset = 1
    with pytest.raises(T2DError, match="auto_reset"):
        auto.trace_attach()
    auto.close()
    ep = fixture[0][0]
    env = _make([ep, ep])
    with pytest.raises(T2DError, match="trace store"):
        env.render_cells([0])
    with pytest.raises(T2DError, match="trace store"):
        env.trace_begin()
    with pytest.raises(T2DError, match="capacity"):
        env.trace_attach(0)
    env.trace_attach(8)
    env.trace_begin()
    for ids in ([2], [-1], [0, 5]):
        with pytest.raises(T2DError, match="env id"):
            env.render_cells(ids)
        with pytest.raises(T2DError, match="env id"):
            env.render_rgb(ids, scale=1)
    with pytest.raises(T2DError, match="count"):
        env.render_cells([])
    with pytest.raises(T2DError, match="scale"):
        env.render_rgb([0], scale=0)
    with pytest.raises(T2DError, match="scale"):
        env.render_rgb([0], scale=9)
    for pitch in (480, 486, 488, 500):                 # too small; not a multiple of 16
        canvas = torch.zeros((1, 82, 512), dtype=torch.uint8, device="cuda")[:, :, :pitch].contiguous()
        with pytest.raises(T2DError, match="pitch"):
            env.render_rgb([0], scale=1, pitch=pitch, out=canvas)
    assert env.faults() == 0
    # ids that are already on the device cannot be checked without a synchronisation: the kernel clamps them and says so
    good, _ = env.render_cells([1, 0])
    bad, _ = env.render_cells(torch.tensor([7, -3], dtype=torch.int32, device="cuda"))
    assert torch.equal(good, bad)
    assert env.faults() == vec_env.FAULT_RENDER_ID
    env.close()


def test_append_and_render_in_one_captured_graph(fixture):
    """Three steps, each followed by append, and a render_rgb captured as ONE linear graph (no side streams) and replayed twice
    give the traces and the last frame of the same six steps run eagerly."""
    ep = fixture[0][1]
    acts = _actions([ep, ep], 6).permute(0, 2, 1).contiguous()         # [step, agent, env]
    ids = torch.tensor([1, 0], dtype=torch.int32, device="cuda")

    def fresh():
        env = _make([ep, ep])
        env.trace_attach(16)
        env.trace_begin()
        out = (torch.empty((2, 2, 13, 13), dtype=torch.float32, device="cuda"), torch.empty((2, 2), dtype=torch.float32, device="cuda"),
               torch.empty(2, dtype=torch.uint8, device="cuda"))
        canvas = torch.zeros((2, 82 * 2, 976), dtype=torch.uint8, device="cuda")
        return env, out, canvas

    def three(env, out, canvas, a):
        for k in range(3):
            _, _, done = env.step(a[k, 0], a[k, 1], out=out)
            env.trace_append(done)
        return env.render_rgb(ids, scale=2, pitch=976, out=canvas)

    a_eager = acts.clone()
    env, out, canvas = fresh()
    three(env, out, canvas, a_eager[:3].contiguous())
    frame_eager = three(env, out, canvas, a_eager[3:].contiguous()).clone()
    tr_eager = env.traces()
    env.close()

    env, out, canvas = fresh()
    static = acts[:3].clone().contiguous()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        frame = three(env, out, canvas, static)
    assert env.traces()["len"].tolist() == [1, 1]      # capturing ran nothing
    graph.replay()
    static.copy_(acts[3:])
    graph.replay()
    torch.cuda.synchronize()
    tr = env.traces()
    assert tr["len"].tolist() == [7, 7] == tr_eager["len"].tolist()
    assert np.array_equal(tr["pos"][:, :7], tr_eager["pos"][:, :7]) and np.array_equal(tr["pos"][0, 1:7], ep["pos"][:6])
    assert torch.equal(frame, frame_eager) and env.faults() == 0
    env.close()


def test_track2denv_info_and_rgb_array(fixture):
    from active_tracking_rl_amd.environment import Track2DEnv
    eps, palette, _ = fixture
    ep = eps[0]
    plain = Track2DEnv(ep["env_id"])
    plain.reset()
    _, _, _, info = plain.step([0, 0])
    assert sorted(info) == ["distance"]                # nothing new unless asked for
    with pytest.raises(NotImplementedError):
        plain.render(mode="rgb_array")
    plain.close()
    env = Track2DEnv(ep["env_id"], traces=True)
    env.reset()
    core = env.vec.core
    core.inject(ep["maze"], ep["init"].reshape(1, 4))
    core.trace_begin()
    for t, a in enumerate(ep["actions"]):
        _, _, done, info = env.step([int(a[0]), int(a[1])])
        assert sorted(info) == ["distance", "traces", "traces_relative"]
        assert info["traces"] == ep["traces"][: t + 2].tolist() and isinstance(info["traces"][0], list)
        rel = info["traces_relative"]
        assert len(rel) == 2 and all(len(x) == 2 and isinstance(x[0], np.ndarray) for x in rel)
        assert np.array_equal(np.array(rel), ep["rel"][t])
        assert done == bool(ep["done"][t])
    img = env.render(mode="rgb_array")
    assert img.dtype == np.uint8 and img.shape == (328, 648, 3)
    assert np.array_equal(img, rs.rgb(ep["cells"][-1], ep["partial"][-1], palette, 4))
    assert np.array_equal(env.render("rgb_array", scale=1), rs.rgb(ep["cells"][-1], ep["partial"][-1], palette, 1))
    with pytest.raises(NotImplementedError, match="display"):
        env.render()
    with pytest.raises(NotImplementedError, match="display"):
        env.render(mode="human")
    env.close()


def test_gym_eval_render_writes_frames_and_keeps_the_numbers(tmp_path):
    """gym_eval.py --render --render-eps 2 on 8 episodes of a fresh model: PNG frames whose first one is render_rgb of the reset
    state, traces.npz for all 8 episodes, and the same result line as a run without the flag."""
    from active_tracking_rl_amd.environment import VecEnv
    env_id = "Track2D-BlockPartialPZR-v0"

    def run(tag, extra):
        cmd = [sys.executable, os.path.join(ROOT, "gym_eval.py"), "--env", env_id, "--num-episodes", "8", "--seed", "3",
               "--log-dir", str(tmp_path / tag)] + extra
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        lines = [ln.split(" : ", 1)[1] for ln in r.stdout.splitlines() if " : El, " in ln]
        assert len(lines) == 1, r.stdout[-3000:]
        return lines[0]

    out = tmp_path / "frames"
    with_render = run("a", ["--render", "--render-eps", "2", "--render-scale", "2", "--render-dir", str(out)])
    without = run("b", [])
    assert with_render == without and "S_rate" in without and "EL_mean" in without
    assert sorted(os.listdir(str(out))) == ["ep000", "ep001", "traces.npz"]
    tr = np.load(str(out / "traces.npz"))
    assert tr["pos"].shape == (8, 501, 2, 2) and tr["len"].shape == (8,)
    lengths = [int(x) for x in re.search(r"El, (\d+),", without).groups()]
    assert int(tr["len"][7]) == lengths[0] + 1                              # 'El' is the last episode's length
    env = VecEnv(env_id, 8, seed=3, env_id_base=1 << 20, traces=True)
    env.reset()
    want = env.core.render_rgb([0, 1], scale=2).cpu().numpy()
    spawn = env.core.traces()["pos"][:, 0]
    env.close()
    assert np.array_equal(tr["pos"][:, 0], spawn)
    for e in range(2):
        files = sorted(os.listdir(str(out / ("ep%03d" % e))))
        assert files == ["step%04d.png" % t for t in range(int(tr["len"][e]))]          # stops after the terminal frame
        first = rs.decode_png(open(str(out / ("ep%03d" % e) / files[0]), "rb").read())
        assert np.array_equal(first, want[e])
