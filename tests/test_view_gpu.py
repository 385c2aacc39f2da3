"""-m gpu: the player views on the device. The rule is integer arithmetic on the windows, the map tile and the positions, so
everything is compared for EQUALITY with tests/view_spec.py: both kernels on a stepped handle at env_id_base 1000 (maps, positions
and sides read back through get_state / get_maps) in every layout the ABI addresses, with guard bytes round every output;
VecEnv(views=True) under the whole stack of passes against its own windows, its own state and a twin without views; the
gym-protocol env; one step plus one atr_view_rgb captured in a graph; and gym_eval.py --view."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_spec
import view_spec as sp
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PZR = "Track2D-BlockPartialPZR-v0"
RAM = "Track2D-BlockPartialRam-v0"
NAV = "Track2D-BlockPartialNav-v0"
BASE = 1000
POISON = 0xA5
GUARD = 64
RATES = {"flicker": .05, "miss": .1, "ghost": .5}
STACK = dict(occlusion=True, fov=90, footprints=4, map_memory=True, sensor_noise=RATES, egocentric=True)


def _corner_maze():
    """A side-81 map (walls round it, a few inside) for env 0: its players stand within 6 cells of two map edges each."""
    m = np.zeros((81, 81), np.uint8)
    m[0], m[-1], m[:, 0], m[:, -1] = 1, 1, 1, 1
    m[3, 2:6], m[5:9, 4], m[76, 70:79], m[70:75, 77] = 1, 1, 1, 1
    return m


def _core(n):
    """A Block / Adv handle of n envs at env_id_base 1000 after 6 random steps, env 0 replaced by the corner map (side 81) with
    the tracker at (2, 1) and the target at (78, 79)."""
    from active_tracking_rl_amd.vec_env import VecTrack2D
    core = VecTrack2D(num_envs=n, map_type="Block", target_mode="Adv", level=1, auto_reset=False, max_episode_steps=500,
                      device=DEV, env_id_base=BASE, seed=3)
    core.reset()
    gen = torch.Generator(device=DEV)
    gen.manual_seed(n)
    for _ in range(6):
        a = torch.randint(0, 4, (2, n), device=DEV, generator=gen)
        core.step(a[0], a[1])
    core.inject(_corner_maze(), np.array([[2, 1, 78, 79]], np.int32), first=0)
    return core


def _state(core):
    st = core.get_state()
    return core.get_maps(), st["side"].astype(np.int64), st["pos"].astype(np.int64)


def _planted(windows, seed, floats):
    """The handle's own windows with 5, 6, 7, 8 and the unknowns 3, 9, 255 planted in a fifth of the cells (0.5 and NaN too in a
    float window)."""
    rs = np.random.RandomState(seed)
    w = np.array(windows, np.float32 if floats else np.uint8)
    plant = rs.random_sample(w.shape) < 0.2
    w[plant] = rs.choice([5, 5, 6, 7, 8, 3, 9, 255], int(plant.sum()))
    if floats:
        odd = rs.random_sample(w.shape) < 0.03
        w[odd] = rs.choice([0.5, np.nan, -1.0, 4.0000005], int(odd.sum()))
    return w


def _guarded(numel, align=GUARD):
    buf = torch.full((GUARD + numel + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0 and align % 16 == 0
    return buf, buf[GUARD:GUARD + numel]


def _intact(buf, numel):
    return bool((buf[:GUARD] == POISON).all()) and bool((buf[GUARD + numel:] == POISON).all())


def _id_lists(n, rs):
    return [[n - 1], [n - 1, 0], [0] + [int(x) for x in rs.randint(0, n, 3)] + [0]]


def _layouts(w, floats):
    """(name, device view [n, 2, 13, 13]) of the windows w in every layout: dense; a slice of a wider poisoned store (se = 845);
    a store with the players far apart (se = 676, sp = 338); byte windows at an odd address."""
    dt = torch.float32 if floats else torch.uint8
    n = w.shape[0]
    src = torch.from_numpy(w).to(DEV)
    dense = src.clone()
    wide = torch.full((n, 5, 13, 13), 3, dtype=dt, device=DEV)
    wide[:, 1:3] = src
    apart = torch.full((n, 2, 2, 13, 13), 9, dtype=dt, device=DEV)
    apart[:, :, 1] = src
    out = [("dense", dense), ("wide", wide[:, 1:3]), ("apart", apart[:, :, 1])]
    if not floats:
        odd = torch.full((1 + n * 338 + 3,), 3, dtype=dt, device=DEV)
        v = odd[1:1 + n * 338].view(n, 2, 13, 13)
        v.copy_(src)
        assert v.data_ptr() % 2 == 1
        out.append(("odd", v))
    for name, v in out:
        assert (v.stride(0), v.stride(1)) == {"dense": (338, 169), "wide": (845, 169), "apart": (676, 338), "odd": (338, 169)}[name]
    return out


@pytest.mark.parametrize("floats", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("n", [1, 3, 130])
def test_view_cells_equal_the_spec(n, floats):
    """atr_view_cells on a stepped handle (env 0: side 81, both players within 6 cells of two map edges) with planted windows:
    both viewers, turned 0 .. 3 with facings over 0 .. 3, NONE and a byte that is no facing, counts 1, 2 and 5 with ids repeated
    and out of order, every layout; cells alone, windows alone and both; the guard bytes round every output are intact."""
    from active_tracking_rl_amd import view
    core = _core(n)
    try:
        maps, side, pos = _state(core)
        assert side[0] == 81 and pos[0].tolist() == [[2, 1], [78, 79]] and (n == 1 or (side[1:] == 82).all())
        rs = np.random.RandomState(40 + n)
        w = _planted(core.observe().cpu().numpy(), n, floats)
        facing = rs.choice([0, 1, 2, 3, sp.NONE, 7], (n, 2)).astype(np.uint8)
        facing[0] = (3, 1)
        dfacing = torch.from_numpy(facing).to(DEV)
        launches = 0
        for name, dw in _layouts(w, floats):
            for ids in _id_lists(n, rs):
                count = len(ids)
                for viewer in (0, 1):
                    for turned in range(4):
                        if name != "dense" and (turned + viewer + count) % 3:      # (the other layouts: a third of the combinations)
                            continue
                        want_c, want_w = sp.view_cells(maps[ids], side[ids], pos[ids], w[ids], facing[ids], turned, viewer)
                        cbuf, cells = _guarded(count * 6724)
                        wbuf, wins = _guarded(count * 338)
                        fac = dfacing if turned or (viewer + count) % 2 else None
                        got = view.view_cells(dw, core, ids, viewer=viewer, facing=fac, turned=turned, out=(cells, wins))
                        what = (name, ids, viewer, turned)
                        assert np.array_equal(got[0].cpu().numpy().reshape(count, 82, 82), want_c), what
                        assert np.array_equal(got[1].cpu().numpy().reshape(count, 2, 13, 13), want_w), what
                        assert _intact(cbuf, count * 6724) and _intact(wbuf, count * 338), what
                        launches += 1
                        if turned == 2:
                            cbuf, cells = _guarded(count * 6724)
                            wbuf, wins = _guarded(count * 338)
                            view.view_cells(dw, core, ids, viewer=viewer, facing=dfacing, turned=turned, out=(cells, None))
                            view.view_cells(dw, core, ids, viewer=viewer, facing=dfacing, turned=turned, out=(None, wins))
                            assert np.array_equal(cells.cpu().numpy().reshape(count, 82, 82), want_c), what
                            assert np.array_equal(wins.cpu().numpy().reshape(count, 2, 13, 13), want_w), what
                            assert _intact(cbuf, count * 6724) and _intact(wbuf, count * 338), what
        # the codes that must occur: every band, the unknown, outside the map (env 0's side is 81)
        allc, _ = sp.view_cells(maps[[0]], side[[0]], pos[[0]], w[[0]], facing[[0]], 3, 0)
        assert {15, 255}.issubset(set(np.unique(allc))) and (allc < 16).any() and ((allc >= 16) & (allc < 32)).any()
        # allocation by the binding itself: shapes and dtypes
        c, ww = view.view_cells(dw, core, [0], viewer="target", facing=dfacing, turned=3)
        assert c.dtype == ww.dtype == torch.uint8 and tuple(c.shape) == (1, 82, 82) and tuple(ww.shape) == (1, 2, 13, 13)
        assert core.faults() == 0 and launches >= 24
    finally:
        core.close()


RGB_CASES = [(1, 0), (3, 0), (3, 64), (8, 0), (8, 16)]          # (scale, bytes of pitch beyond the minimum)


@pytest.mark.parametrize("floats", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("n", [1, 3, 130])
def test_view_rgb_equals_the_spec_and_its_own_cells(n, floats):
    """atr_view_rgb at scale 1, 3 and 8, minimal and padded pitch, on a poisoned canvas with guard bytes before the first and
    after the last frame: every frame equals the spec's (pad bytes 0 included) and equals the colouring of atr_view_cells' own
    output; the guards are intact."""
    from active_tracking_rl_amd import view
    core = _core(n)
    try:
        maps, side, pos = _state(core)
        rs = np.random.RandomState(60 + n)
        w = _planted(core.observe().cpu().numpy(), 7 + n, floats)
        facing = rs.choice([0, 1, 2, 3, sp.NONE], (n, 2)).astype(np.uint8)
        dfacing = torch.from_numpy(facing).to(DEV)
        layouts = _layouts(w, floats)
        for k, (scale, extra) in enumerate(RGB_CASES):
            name, dw = layouts[k % len(layouts)]
            ids = _id_lists(n, rs)[(k + 1) % 3] if scale < 8 else [n - 1, 0]
            count, viewer, turned = len(ids), k % 2, (k + 1) % 4
            pitch = view.min_pitch(scale) + extra
            assert pitch % 16 == 0 and pitch >= 726 * scale
            numel = count * 82 * scale * pitch
            buf, canvas = _guarded(numel)
            img = view.view_rgb(dw, core, ids, scale=scale, viewer=viewer, facing=dfacing, turned=turned, pitch=pitch,
                                out=canvas.view(count, 82 * scale, pitch))
            assert tuple(img.shape) == (count, 82 * scale, 242 * scale, 3) and img.data_ptr() == canvas.data_ptr()
            want_c, want_w = sp.view_cells(maps[ids], side[ids], pos[ids], w[ids], facing[ids], turned, viewer)
            want = sp.view_rgb(want_c, want_w, scale, pitch)
            got = canvas.cpu().numpy().reshape(count, 82 * scale, pitch)
            what = (name, scale, extra, ids, viewer, turned)
            assert np.array_equal(got, want), what
            assert not got[:, :, 726 * scale:].any() and _intact(buf, numel), what
            c, ww = view.view_cells(dw, core, ids, viewer=viewer, facing=dfacing, turned=turned)
            assert np.array_equal(got, sp.view_rgb(c.cpu().numpy(), ww.cpu().numpy(), scale, pitch)), what
        # the binding's own canvas: minimal pitch, the padding cut off
        img = view.view_rgb(layouts[0][1], core, [0], scale=2, viewer=1)
        assert tuple(img.shape) == (1, 164, 484, 3) and img.dtype == torch.uint8
        want_c, want_w = sp.view_cells(maps[[0]], side[[0]], pos[[0]], w[[0]], None, 0, 1)
        assert np.array_equal(img.cpu().numpy().reshape(1, 164, 1452), sp.view_rgb(want_c, want_w, 2, 1456)[:, :, :1452])
        assert core.faults() == 0
    finally:
        core.close()


def test_a_bad_id_is_clamped_and_sets_the_fault_bit():
    """Ids on the host are checked by the binding; ids on the device are clamped by the kernel (below 0 to env 0, above to the
    last env), which sets bit 5 of the fault word."""
    from active_tracking_rl_amd import vec_env, view
    n = 3
    core = _core(n)
    try:
        dw = core.observe().to(torch.uint8)
        for f in (view.view_cells, view.view_rgb):
            with pytest.raises(vec_env.T2DError, match=r"env id 3 outside \[0, 3\)"):
                f(dw, core, [0, 3])
            with pytest.raises(vec_env.T2DError, match=r"env id -1 outside \[0, 3\)"):
                f(dw, core, [-1])
        assert core.faults() == 0
        good = view.view_cells(dw, core, torch.tensor([0, 2, 1], dtype=torch.int32, device=DEV))
        assert core.faults() == 0
        bad = view.view_cells(dw, core, torch.tensor([-7, n + 4, 1], dtype=torch.int32, device=DEV))
        assert torch.equal(good[0], bad[0]) and torch.equal(good[1], bad[1])
        assert core.faults() == vec_env.FAULT_RENDER_ID == 32
        good = view.view_rgb(dw, core, torch.tensor([2, 0], dtype=torch.int32, device=DEV), scale=1)
        bad = view.view_rgb(dw, core, torch.tensor([1 << 30, -(1 << 30)], dtype=torch.int32, device=DEV), scale=1)
        assert torch.equal(good, bad) and core.faults() == 32
    finally:
        core.close()


def test_binding_refusals_on_the_device():
    """From the handle's state: a handle that was never reset and a whole-map handle are refused with text; the tensor checks of
    the binding name what is wrong."""
    from active_tracking_rl_amd import view
    from active_tracking_rl_amd.vec_env import VecTrack2D
    dw = torch.zeros((2, 2, 13, 13), dtype=torch.uint8, device=DEV)
    fresh = VecTrack2D(num_envs=2, map_type="Block", target_mode="Adv", level=1, auto_reset=False, device=DEV)
    full = VecTrack2D("Track2D-BlockFullPZR-v0", num_envs=2, auto_reset=False, device=DEV)
    try:
        with pytest.raises(RuntimeError, match="atr_view_cells: call t2d_reset"):
            view.view_cells(dw, fresh, [0])
        with pytest.raises(RuntimeError, match="atr_view_rgb: call t2d_reset"):
            view.view_rgb(dw, fresh, [0])
        full.reset()
        with pytest.raises(RuntimeError, match="atr_view_cells: the handle observes the whole map"):
            view.view_cells(dw, full, [0])
        with pytest.raises(RuntimeError, match="atr_view_rgb: the handle observes the whole map"):
            view.view_rgb(dw, full, [0])
        fresh.reset()
        with pytest.raises(ValueError, match="obs holds 3 envs, the handle 2"):
            view.view_cells(torch.zeros((3, 2, 13, 13), dtype=torch.uint8, device=DEV), fresh, [0])
        with pytest.raises(ValueError, match="obs must be uint8 / float32"):
            view.view_cells(dw.to(torch.int32), fresh, [0])
        with pytest.raises(ValueError, match="turned=1 needs the facing bytes"):
            view.view_rgb(dw, fresh, [0], turned=1)
        with pytest.raises(ValueError, match="facing must be a contiguous uint8"):
            view.view_cells(dw, fresh, [0], turned=1, facing=torch.zeros((2, 2), dtype=torch.int32, device=DEV))
        with pytest.raises(ValueError, match="scale must be 1 .. 8"):
            view.view_rgb(dw, fresh, [0], scale=9)
        with pytest.raises(RuntimeError, match="pitch 720 must be a multiple of 16 and at least 726"):
            view.view_rgb(dw, fresh, [0], scale=1, pitch=720)
        assert fresh.faults() == 0
    finally:
        fresh.close()
        full.close()


# -- the env ---------------------------------------------------------------------------------------------------------------------

ENV_CASES = {
    "stack": (PZR, dict(STACK), {}),
    "stack-bytes": (PZR, dict(STACK, obs_u8=True), {}),
    "stack-gym-protocol": (PZR, dict(STACK, obs_u8=True), dict(auto_reset=False)),
    "scripted": (NAV, dict(STACK), {}),
    "scripted-bytes": (RAM, dict(STACK, obs_u8=True), {}),
    "plain-rescale-stack2": (PZR, dict(rescale=True, stack_frames=2), {}),
}


@pytest.mark.parametrize("case", list(ENV_CASES))
def test_env_views_show_its_own_windows_and_state(case):
    """VecEnv(views=True) with the whole stack (occlusion, fov 90, footprints 4, map memory, the three noise rates, egocentric)
    against a twin of the same seed and flags without views, 6 envs, TimeLimit 13: after reset(), after each of 15 steps and
    after an observe(), view_cells(ids)[1] equals the windows the call returned for the listed envs, the map panel equals the
    spec on the env's own state, its windows and its _facing, for both viewers, and view_rgb is the spec's colouring; the twin
    returns identical observations, rewards and dones. (With rescale and a frame stack the kept windows are the raw ones.)"""
    from active_tracking_rl_amd.environment import VecEnv
    env_id, kw, extra = ENV_CASES[case]
    n, seed, ids = 6, 9, [4, 0, 4, 5]
    env = VecEnv(env_id, n, device=DEV, seed=seed, views=True, max_episode_steps=13, **kw, **extra)
    twin = VecEnv(env_id, n, device=DEV, seed=seed, max_episode_steps=13, **kw, **extra)
    try:
        scripted = env_id != PZR
        ego = (1 if scripted else 3) if kw.get("egocentric") else 0
        assert env.views and not twin.views and twin._view_obs is None and env._ego_roles == ego
        assert env.obs_u8 == twin.obs_u8 == bool(kw.get("obs_u8"))
        raw = not kw.get("rescale")
        bands = set()

        def check(o, what):
            torch.cuda.synchronize()
            maps, st = env.core.get_maps(), env.core.get_state()
            side, pos = st["side"].astype(np.int64), st["pos"].astype(np.int64)
            kept = env._view_obs.cpu().numpy()
            assert kept.shape == (n, 2, 13, 13) and kept.dtype == (np.uint8 if env.obs_u8 else np.float32)
            if raw:
                assert np.array_equal(o.cpu().numpy().reshape(n, 2, 13, 13), kept), what
            facing = env._facing.cpu().numpy() if ego else None
            for viewer in (0, 1):
                cells, wins = env.view_cells(ids, viewer=viewer)
                assert np.array_equal(wins.cpu().numpy(), kept[ids].astype(np.uint8)), what        # (no unknown value occurs)
                want_c, want_w = sp.view_cells(maps[ids], side[ids], pos[ids], kept[ids], None if facing is None else facing[ids],
                                               ego, viewer)
                assert np.array_equal(cells.cpu().numpy(), want_c) and np.array_equal(wins.cpu().numpy(), want_w), (what, viewer)
                bands.update(int(x) >> 4 for x in np.unique(want_c))
            img = env.view_rgb(ids[:2], scale=2, viewer="target")
            assert np.array_equal(img.cpu().numpy().reshape(2, 164, 1452), sp.view_rgb(want_c[:2], want_w[:2], 2, 1452)), what

        o, p = env.reset(), twin.reset()
        assert torch.equal(o, p)
        check(o, "reset")
        gen = torch.Generator(device=DEV)
        gen.manual_seed(4)
        acts = torch.randint(0, 4, (15, 2, n), device=DEV, generator=gen)
        ends = 0
        for t in range(15):
            a = [acts[t, 0]] if scripted else [acts[t, 0], acts[t, 1]]
            o, r, d, _ = env.step(a)
            p, r2, d2, _ = twin.step(a)
            assert torch.equal(o, p) and torch.equal(r, r2) and torch.equal(d, d2), t
            check(o, "step %d" % t)
            ends += int(d.sum())
        o, p = env.observe(), twin.observe()
        assert torch.equal(o, p)
        check(o, "observe")
        assert bands == ({0, 1, 2} if "occlusion" in kw else {0, 2})        # (Block maps fill the tile: no cell is outside)
        assert ends >= n
        assert env.core.faults() == 0 and twin.core.faults() == 0
    finally:
        env.close()
        twin.close()


def test_views_need_the_option_and_a_reset():
    from active_tracking_rl_amd.environment import VecEnv
    plain = VecEnv(PZR, 2, device=DEV, seed=1)
    env = VecEnv(PZR, 2, device=DEV, seed=1, views=True)
    try:
        plain.reset()
        assert plain._view_obs is None
        with pytest.raises(NotImplementedError, match="views=True"):
            plain.view_cells([0])
        with pytest.raises(RuntimeError, match="call reset"):
            env.view_rgb([0])
        assert env._view_obs is None
    finally:
        plain.close()
        env.close()


@pytest.mark.parametrize("env_id", [PZR, NAV], ids=["pzr", "nav"])
def test_gym_protocol_env_render_view(env_id):
    """Track2DEnv(views=True).render_view: uint8 [82 * scale, 242 * scale, 3], the spec's colouring of the windows the env just
    returned projected on its own state, for both viewers; render() is untouched and an env without views refuses."""
    from active_tracking_rl_amd.environment import Track2DEnv
    env = Track2DEnv(env_id, device=DEV, seed=3, views=True, occlusion=True, fov=180, egocentric=True)
    plain = Track2DEnv(env_id, device=DEV, seed=3, occlusion=True, fov=180, egocentric=True)
    try:
        ego = 3 if env_id == PZR else 1
        rs = np.random.RandomState(5)
        o = env.reset()
        assert np.array_equal(o, plain.reset())
        for t in range(6):
            a = rs.randint(0, 4, 2)
            o, r, d, info = env.step(a)
            o2, r2, d2, info2 = plain.step(a)
            assert np.array_equal(o, o2) and np.array_equal(r, r2) and d == d2 and info == info2
            core = env.vec.core
            maps, st = core.get_maps(), core.get_state()
            for viewer, scale in ((0, 4), ("target", 1)):
                img = env.render_view(scale=scale, viewer=viewer)
                assert img.dtype == np.uint8 and img.shape == (82 * scale, 242 * scale, 3)
                c, w = sp.view_cells(maps, st["side"], st["pos"], o.reshape(1, 2, 13, 13), env.vec._facing.cpu().numpy(), ego,
                                     0 if viewer == 0 else 1)
                assert np.array_equal(w[0], o.reshape(2, 13, 13).astype(np.uint8))
                assert np.array_equal(img.reshape(82 * scale, -1), sp.view_rgb(c, w, scale, 726 * scale)[0]), (t, viewer)
        assert env.render_view().shape == (328, 968, 3) and np.array_equal(env.render_view(), env.render_view(4, "tracker"))
        with pytest.raises(NotImplementedError, match="traces=True"):
            env.render(mode="rgb_array")
        with pytest.raises(NotImplementedError, match="views=True"):
            plain.render_view()
    finally:
        env.close()
        plain.close()


def test_a_step_and_a_view_in_one_captured_graph():
    """One env step into static buffers followed by one atr_view_rgb of those buffers, captured as ONE graph: each replay draws
    the state that replay's step produced (the spec on the state and windows read back), and equals the same calls run eagerly."""
    from active_tracking_rl_amd import view
    from active_tracking_rl_amd.vec_env import VecTrack2D
    n, scale, pitch = 2, 2, 1456 + 32
    gen = torch.Generator(device=DEV)
    gen.manual_seed(12)
    acts = torch.randint(0, 4, (3, 2, n), device=DEV, generator=gen)
    ids = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)

    def fresh():
        core = VecTrack2D(num_envs=n, map_type="Block", target_mode="Adv", level=1, auto_reset=False, max_episode_steps=500,
                          device=DEV, env_id_base=BASE, seed=5)
        core.reset()
        out = (torch.empty((n, 2, 13, 13), dtype=torch.float32, device=DEV), torch.empty((n, 2), dtype=torch.float32, device=DEV),
               torch.empty(n, dtype=torch.uint8, device=DEV))
        canvas = torch.full((3, 82 * scale, pitch), POISON, dtype=torch.uint8, device=DEV)
        return core, out, canvas

    def one(core, out, canvas, a):
        core.step(a[0], a[1], out=out)
        return view.view_rgb(out[0], core, ids, scale=scale, viewer=1, pitch=pitch, out=canvas)

    core, out, canvas = fresh()
    eager = []
    for t in range(3):
        eager.append(one(core, out, canvas, acts[t].contiguous()).clone())
    core.close()

    core, out, canvas = fresh()
    try:
        static = acts[0].clone().contiguous()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            frame = one(core, out, canvas, static)
        assert core.get_state()["t"].tolist() == [0, 0]        # capturing ran nothing
        sel = ids.cpu().numpy()
        frames = []
        for t in range(3):
            static.copy_(acts[t])
            graph.replay()
            torch.cuda.synchronize()
            assert core.get_state()["t"].tolist() == [t + 1, t + 1]
            maps, side, pos = _state(core)
            c, w = sp.view_cells(maps[sel], side[sel], pos[sel], out[0].cpu().numpy()[sel], None, 0, 1)
            assert np.array_equal(canvas.cpu().numpy(), sp.view_rgb(c, w, scale, pitch)), t
            assert torch.equal(frame, eager[t]), t
            frames.append(frame.clone())
        assert not torch.equal(frames[0], frames[2]) and core.faults() == 0
    finally:
        core.close()


def test_gym_eval_view_writes_the_frames(tmp_path):
    """gym_eval.py --view --heuristic-tracker pursuit on a scripted-target id (no checkpoint) with observation passes on: the
    file tree ep{e:03d}/step{t:04d}.png for the first --view-eps episodes and nothing else, every frame of the canvas' size, and
    frame 0 of episodes 0 and 1 decodes to view_rgb of an env made the way the evaluation round makes its own."""
    from active_tracking_rl_amd.environment import VecEnv
    out = tmp_path / "frames"
    cmd = [sys.executable, os.path.join(ROOT, "gym_eval.py"), "--env", NAV, "--num-episodes", "4", "--seed", "3", "--log-dir",
           str(tmp_path / "log"), "--heuristic-tracker", "pursuit", "--occlusion", "--fov", "90", "--egocentric", "--graphed-eval",
           "--view", "target", "--view-eps", "2", "--view-scale", "2", "--view-dir", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert len([ln for ln in r.stdout.splitlines() if " : El, " in ln]) == 1, r.stdout[-3000:]
    assert sorted(os.listdir(str(out))) == ["ep000", "ep001"]
    env = VecEnv(NAV, 4, device=DEV, seed=3, env_id_base=1 << 20, views=True, auto_reset=False, occlusion=True, fov=(90, 90),
                 egocentric=True)
    try:
        env.reset()
        want = env.view_rgb([0, 1], scale=2, viewer="target").cpu().numpy()
    finally:
        env.close()
    for e in range(2):
        files = sorted(os.listdir(str(out / ("ep%03d" % e))))
        assert 2 <= len(files) <= 501 and files == ["step%04d.png" % t for t in range(len(files))]
        first = render_spec.decode_png(open(str(out / ("ep%03d" % e) / files[0]), "rb").read())
        last = render_spec.decode_png(open(str(out / ("ep%03d" % e) / files[-1]), "rb").read())
        assert first.shape == last.shape == (164, 484, 3) and np.array_equal(first, want[e])
