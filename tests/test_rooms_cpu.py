"""Rooms maps without a GPU: the properties of the rule (rooms_spec.py), the rule header (csrc/t2d_rooms_rule.h) through a
stand-alone host program built with the address and undefined-behaviour sanitizers, the env ids and the ABI constant.
Every comparison is for equality."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import draw_spec
import rooms_spec as rs
from conftest import ROOT

SEED = 1234567
CASES = [(0, g, e) for g in range(20) for e in range(2)] + \
        [(lv, g, e) for lv in (1, 4, 15) for g in (0, 3, 4095, 70000, 2**31 + 5) for e in range(2)]


def test_cases_are_what_the_issue_asks_for():
    assert sum(1 for c in CASES if c[0] == 0) == 40
    assert all(sum(1 for c in CASES if c[0] == lv) == 10 for lv in (1, 4, 15))


@pytest.mark.parametrize("level", [0, 1, 4, 15])
def test_spec_properties(level):
    odd = np.arange(1, rs.SIDE - 1, 2)                       # interior rows / columns 1, 3, .. 79 (81 is the border)
    for lv, genv, ep in CASES:
        if lv != level:
            continue
        info = {}
        g = rs.rooms_map(SEED, genv, ep, lv, info=info)
        assert g.shape == (82, 82) and g.dtype == np.uint8
        assert (g[0] == 1).all() and (g[-1] == 1).all() and (g[:, 0] == 1).all() and (g[:, -1] == 1).all()
        assert set(np.unique(g).tolist()) <= {0, 1}
        assert rs.connected(g)
        assert (g[np.ix_(odd, odd)] == 0).all()              # no wall cell at (odd, odd)
        m = info["m"]
        assert (m == 3 + 2 * lv) if lv else (m in (5, 7, 9, 11))
        for r0, c0, r1, c1 in info["rooms"]:
            assert r1 - r0 + 1 >= m and c1 - c0 + 1 >= m
            assert (g[r0:r1 + 1, c0:c1 + 1] == 0).all()       # a final room is free floor
        assert info["regions"] <= rs.MAX_REGIONS and info["regions"] == 2 * len(info["rooms"]) - 1
        # the order regions are processed in does not matter
        assert np.array_equal(g, rs.rooms_map(SEED, genv, ep, lv, order="bfs"))


def test_maps_differ_between_envs_episodes_and_seeds():
    base = rs.rooms_map(SEED, 5, 0, 0)
    assert not np.array_equal(base, rs.rooms_map(SEED, 6, 0, 0))
    assert not np.array_equal(base, rs.rooms_map(SEED, 5, 1, 0))
    assert not np.array_equal(base, rs.rooms_map(SEED + 1, 5, 0, 0))
    assert not np.array_equal(base, rs.rooms_map(SEED + (1 << 32), 5, 0, 0))      # the high key word counts


def test_spec_philox_is_the_projects():
    for ctr, key in (((0, 0, 0, 0), (0, 0)), ((1 | 1 << 7 | 80 << 14 | 80 << 21, 3, 4095, 3), (SEED, 0)),
                     ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF)),
                     ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))):
        ref = [int(w) for w in draw_spec.philox4x32_10(list(ctr), list(key))]
        assert list(rs.philox4x32_10(ctr, key)) == ref


HOST_TUPLES = [(SEED, 0, 0, 0), (SEED, 4095, 1, 0), (SEED, 70000, 7, 0), ((9 << 32) | 77, 12, 3, 0),
               (SEED, 3, 0, 1), (SEED, 2**31 + 5, 2, 4), (1, 8, 1, 15), (2**64 - 1, 2**32 - 1, 2**32 - 1, 2)]


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the host program needs g++"
    exe = str(tmp_path_factory.mktemp("rooms_host") / "rooms_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "active_tracking_rl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "rooms_host.cpp"), "-o", exe])
    return exe


def test_host_program_philox(host_program):
    for ctr, key in (((0, 0, 0, 0), (0, 0)), ((0xFFFFFFFF, 2, 4095, 3), (SEED, 9)),
                     ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))):
        out = subprocess.check_output([host_program, "philox"] + [str(k) for k in key] + [str(c) for c in ctr], text=True)
        assert [int(w) for w in out.split()] == [int(w) for w in draw_spec.philox4x32_10(list(ctr), list(key))]


def test_host_program_maps_equal_the_spec(host_program):
    assert len(HOST_TUPLES) == 8
    args = [str(v) for t in HOST_TUPLES for v in t]
    r = subprocess.run([host_program, "map"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = r.stdout.split("\n")
    assert len(lines) == 8 * 83 + 1 and lines[-1] == ""
    for i, (seed, genv, ep, lv) in enumerate(HOST_TUPLES):
        head = lines[i * 83].split()
        info = {}
        g = rs.rooms_map(seed, genv, ep, lv, info=info)
        assert head == ["map", str(seed), str(genv), str(ep), str(lv), str(info["m"]), str(info["regions"]), str(info["deepest"])]
        got = np.array([[int(ch) for ch in row] for row in lines[i * 83 + 1:i * 83 + 83]], np.uint8)
        assert got.shape == (82, 82) and np.array_equal(got, g)


def test_registry_resolves_rooms_ids():
    from active_tracking_rl_amd import registry
    assert len(registry.REGISTRY) == 72 and not any("Rooms" in k for k in registry.REGISTRY)
    assert registry.MAP_CODE["Rooms"] == 3
    for obs in ("Full", "Partial"):
        for mode in ("Adv", "PZR", "Far", "Nav", "Ram"):
            for lv in range(16):
                sp = registry.spec("Track2D-Rooms%s%s-v%d" % (obs, mode, lv))
                assert sp == dict(map_type="Rooms", obs_type=obs, level=lv, target_mode=mode, max_episode_steps=500)
    for bad in ("Track2D-RoomsPartialRPF-v0", "Track2D-RoomsFullRPF-v1", "Track2D-RoomsPartialPZR-v16", "Track2D-RoomsPartialPZR-v01",
                "Track2D-RoomsPartialPZR-v-1", "Track2D-RoomsPartialPZR", "Track2D-RoomPartialPZR-v0", "Track2D-Nope-v0",
                "Track2D-BlockPartialPZR-v2"):
        with pytest.raises(KeyError):
            registry.spec(bad)
    assert registry.spec("Track2D-BlockPartialPZR-v0")["map_type"] == "Block"


def test_abi_constant():
    from active_tracking_rl_amd import registry
    txt = open(os.path.join(ROOT, "include", "track2d.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    assert int(re.search(r"\bT2D_MAP_ROOMS\s*=\s*(\d+)", txt).group(1)) == 3 == registry.MAP_CODE["Rooms"]
    assert int(re.search(r"#define\s+T2D_ABI_VERSION\s+(\d+)", txt).group(1)) == 1           # the layout did not change
    dev = open(os.path.join(ROOT, "active_tracking_rl_amd", "csrc", "t2d_device.h")).read()
    assert int(re.search(r"\bMAP_ROOMS\s*=\s*(\d+)", dev).group(1)) == 3
    assert int(re.search(r"\bSTREAM_ROOMS\s*=\s*(\d+)", dev).group(1)) == rs.STREAM_ROOMS == 3


def test_np_create_refuses_rooms():
    """t2d_np_create is host code: the refusal is checked without a GPU, with the library's text."""
    from active_tracking_rl_amd import build, np_mode
    build.build()
    with pytest.raises(np_mode.NpError, match=r"t2d_np_create: Rooms maps \(map_type 3\) are not a reference generator"):
        np_mode.NpEpisodeSource("Rooms", "PZR", 0, 1)
    np_mode.NpEpisodeSource("Block", "PZR", 0, 1).close()


def test_numpy_stream_mode_refuses_rooms_before_a_device_is_touched():
    from active_tracking_rl_amd import environment
    with pytest.raises(NotImplementedError, match="Rooms maps are generated by this project's device generator only"):
        environment.Track2DEnv("Track2D-RoomsPartialPZR-v0", rng="numpy")
    with pytest.raises(NotImplementedError, match="Rooms maps"):
        environment.NumpyVecEnv("Track2D-RoomsPartialNav-v1", [1, 2])
