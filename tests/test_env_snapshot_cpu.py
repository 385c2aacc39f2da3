"""CPU-side checks of the env shard snapshots: include/track2d_state.h against the built library and against
vec_env.STATE_PROTOTYPES (the parsing of tests/test_abi_cpu.py, applied to the new header); the pure-Python blob header
reader; the shard file's `meta` comparison; the build's no-scratch entry; and the two flags of main.py."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import pytest

from conftest import ROOT
from test_abi_cpu import _c_class, _py_class


def _state_functions():
    """{name: (class of the result, [class per parameter])} of every t2d_* function include/track2d_state.h declares."""
    txt = open(os.path.join(ROOT, "include", "track2d_state.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", txt).split("\n") if not ln.lstrip().startswith("#"))
    out = {}
    for m in re.finditer(r"([^;{}()]*?)\b(t2d_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", txt):
        params = [p.strip() for p in m.group(3).split(",")]
        assert m.group(2) not in out
        out[m.group(2)] = (_c_class(m.group(1)), [_c_class(re.sub(r"\w+$", "", p)) for p in params])
    return out


EXPECTED = ["t2d_snapshot_bytes", "t2d_snapshot_create", "t2d_snapshot_destroy", "t2d_snapshot_export", "t2d_snapshot_import",
            "t2d_snapshot_restore", "t2d_snapshot_save"]


def test_state_prototypes_match_the_header():
    """vec_env.STATE_PROTOTYPES is include/track2d_state.h's ABI: every declared function, the header's parameter count and,
    per parameter and result, the same class (pointer / int / long long)."""
    from active_tracking_rl_amd import vec_env
    funcs = _state_functions()
    assert sorted(funcs) == EXPECTED == sorted(vec_env.STATE_PROTOTYPES)
    for name, (res, params) in funcs.items():
        restype, argtypes = vec_env.STATE_PROTOTYPES[name]
        assert _py_class(restype) == res, name
        assert len(argtypes) == len(params), name
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _py_class(a) == c, (name, i)
    assert funcs["t2d_snapshot_bytes"][0] == ctypes.c_longlong
    assert funcs["t2d_snapshot_export"][1][2] == ctypes.c_longlong and funcs["t2d_snapshot_save"][1] == ["ptr"] * 4


def test_library_exports_every_function_of_the_state_header():
    from active_tracking_rl_amd import build, vec_env
    build.build()
    assert os.path.join("..", "..", "include", "track2d_state.h") in build.HEADERS and "t2d_state_view.h" in build.HEADERS
    assert "state_hip.hip" in build.SOURCES and build.NO_SCRATCH_STATE == {"state_hip.hip": "k_state_copy"}
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    for name in _state_functions():
        assert hasattr(lib, name), name


def test_state_binding_checks_status():
    """vec_env.state_lib() binds the table with an errcheck that raises T2DError with the library's text; a refused call
    touches no device (the null checks come first)."""
    from active_tracking_rl_amd import build, vec_env
    build.build()
    L = vec_env.state_lib()
    f = L.t2d_snapshot_save
    assert f.restype is ctypes.c_int and list(f.argtypes) == vec_env.STATE_PROTOTYPES["t2d_snapshot_save"][1]
    assert f.errcheck(0, None, ()) == 0
    with pytest.raises(vec_env.T2DError, match=r"^t2d_snapshot_save failed \(-1\): "):
        f.errcheck(-1, None, ())
    with pytest.raises(vec_env.T2DError, match="null snapshot"):
        f(None, None, None, None)
    with pytest.raises(vec_env.T2DError, match="null argument"):
        L.t2d_snapshot_import(None, None, 0, None)
    assert L.t2d_snapshot_bytes(None) < 0 and L.t2d_snapshot_destroy(None) == 0


def _header(magic=b"T2DSNAP\0", version=1, header_bytes=96, n=70, base=3, seed=(5 << 32) | 9, max_steps=12, auto_reset=1,
            obs_type=0, action_type=0, cfg_hash=0x0123456789abcdef, sections=3, random_step=17, payload=64):
    """The blob header as include/track2d_state.h's comment lays it out, field by field at its documented offset."""
    b = bytearray(96)
    b[0:8] = magic
    for off, fmt, val in ((8, "<I", version), (12, "<I", header_bytes), (16, "<I", n), (20, "<I", base), (24, "<Q", seed),
                          (32, "<i", max_steps), (36, "<i", auto_reset), (40, "<I", obs_type), (44, "<I", action_type),
                          (48, "<Q", cfg_hash), (56, "<I", sections), (60, "<I", random_step), (64, "<Q", payload)):
        struct.pack_into(fmt, b, off, val)
    return bytes(b)


def test_snapshot_header_parses_a_hand_built_blob():
    from active_tracking_rl_amd.vec_env import snapshot_header
    h = snapshot_header(_header() + bytes(64))
    assert h == dict(version=1, header_bytes=96, num_envs=70, env_id_base=3, seed=(5 << 32) | 9, max_episode_steps=12,
                     auto_reset=1, obs_type=0, action_type=0, cfg_hash=0x0123456789abcdef, sections=3, random_step=17,
                     payload_bytes=64)
    assert snapshot_header(bytearray(_header(payload=0)))["payload_bytes"] == 0       # a header alone, as a bytearray


@pytest.mark.parametrize("blob, text", [
    (_header(magic=b"T2DSNAP1") + bytes(64), "magic"),
    (_header(version=2) + bytes(64), "version"),
    ((_header() + bytes(64))[:95], "shorter than"),
    (b"", "shorter than"),
    (_header(payload=65) + bytes(64), "the blob has 160"),
], ids=["magic", "version", "truncated", "empty", "size"])
def test_snapshot_header_refuses(blob, text):
    from active_tracking_rl_amd.vec_env import snapshot_header
    with pytest.raises(ValueError, match=text):
        snapshot_header(blob)


def test_shard_meta_comparison_names_the_first_differing_field():
    from active_tracking_rl_amd.player_util import SHARD_META_FIELDS, shard_meta_mismatch
    assert SHARD_META_FIELDS == ("env", "N", "env_id_base", "network", "rnn_out")
    mine = dict(env="Track2D-BlockPartialPZR-v0", N=64, env_id_base=0, network="tat-maze-lstm", rnn_out=128)
    assert shard_meta_mismatch(dict(mine), mine) is None
    for key, other in (("env", "Track2D-BlockPartialRam-v0"), ("N", 32), ("env_id_base", 64), ("network", "maze-gru"),
                       ("rnn_out", 64)):
        assert shard_meta_mismatch(dict(mine, **{key: other}), mine) == key
        missing = dict(mine)
        del missing[key]
        assert shard_meta_mismatch(missing, mine) == key
    assert shard_meta_mismatch(dict(mine, N=32, rnn_out=64), mine) == "N"             # the first one in the table's order


def test_main_lists_the_shard_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--save-shard-state" in r.stdout and "--load-shard-state PATH" in r.stdout
