"""CPU-side checks of the drop-in boundary: the C-ABI library loads without a GPU and exports every symbol that
include/track2d.h declares; the ctypes prototypes and structures of the policy kernels equal include/atr_policy.h; the env-id table equals the reference registry (golden registry.npz); the product
path refuses to run without the GPU instead of falling back."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT


def _header_symbols(header="track2d.h", prefix="t2d_"):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return sorted(set(re.findall(r"\b(%s[a-z_0-9]+)\s*\(" % prefix, txt)))


def test_library_exports_every_declared_symbol():
    from active_tracking_rl_amd import build, vec_env
    build.build()
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    syms = _header_symbols()
    assert len(syms) >= 15
    for s in syms:
        assert hasattr(lib, s), s
    assert sorted(vec_env.ABI_SYMBOLS) == syms
    lib.t2d_abi_version.restype = ctypes.c_int
    assert lib.t2d_abi_version() == vec_env.ABI_VERSION
    lib.t2d_config_size.restype = ctypes.c_int
    assert lib.t2d_config_size() == ctypes.sizeof(vec_env._Config) == 64      # action_type sits in former padding
    # the other two headers of the boundary: policy-side kernels and the reference-exact episode source
    from active_tracking_rl_amd import np_mode
    np_syms = _header_symbols("track2d_np.h", "t2d_np_")
    assert sorted(np_mode.NP_SYMBOLS) == np_syms and len(np_syms) >= 9
    atr_syms = _header_symbols("atr_policy.h", "atr_")
    assert len(atr_syms) >= 16 and "atr_stem_forward_u8" in atr_syms
    for s in np_syms + atr_syms:
        assert hasattr(lib, s), s


_C_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "long long": ctypes.c_longlong,
              "unsigned long long": ctypes.c_ulonglong, "float": ctypes.c_float, "double": ctypes.c_double}


def _policy_header():
    """include/atr_policy.h without comments and preprocessor lines."""
    txt = open(os.path.join(ROOT, "include", "atr_policy.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    return "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", txt).split("\n") if not ln.lstrip().startswith("#"))


def _c_class(decl):
    """The class of a C parameter / result / field type (the declared name already removed): "ptr" for any pointer, else the
    ctypes scalar it must be bound as. An unknown type is a KeyError: the header uses nothing else."""
    if "*" in decl:
        return "ptr"
    return _C_SCALARS[" ".join(w for w in decl.split() if w != "const")]


def _py_class(t):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return "ptr"
    assert t in _C_SCALARS.values(), t
    return t


def _header_functions(txt):
    """{name: (class of the result, [class per parameter])} of every atr_* function the header declares."""
    out = {}
    for m in re.finditer(r"([^;{}()]*?)\b(atr_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", txt):
        params = [p.strip() for p in m.group(3).split(",")]
        if params == ["void"]:
            params = []
        assert m.group(2) not in out
        # (every parameter is named: what precedes the last identifier is its type)
        out[m.group(2)] = (_c_class(m.group(1)), [_c_class(re.sub(r"\w+$", "", p)) for p in params])
    return out


def _header_structs(txt):
    """{struct name: [(field, class, array length or None)]} of every typedef struct, multi-declarators expanded."""
    out = {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", txt, flags=re.S):
        assert m.group(1) == m.group(3)
        fields = []
        for decl in (d.strip() for d in m.group(2).split(";")):
            if not decl:
                continue
            first, *more = decl.split(",")
            f = re.match(r"^([\w\s]+?)\s*(\**)\s*(\w+)\s*(?:\[(\d+)\])?$", first.strip())
            assert f, decl
            base = f.group(1)
            decls = [f.groups()[1:]] + [re.match(r"^(\**)\s*(\w+)\s*(?:\[(\d+)\])?$", d.strip()).groups() for d in more]
            for star, name, n in decls:
                fields.append((name, _c_class(base + star), int(n) if n else None))
        out[m.group(1)] = fields
    return out


def test_prototype_table_matches_the_policy_header():
    """fused.ATR_PROTOTYPES is include/atr_policy.h's ABI: every declared function, with the header's parameter count and,
    per parameter and result, the same class (pointer / int / unsigned / long long / unsigned long long / float / double).
    ctypes converts silently, so a wrong entry would shift the kernel's argument list without any error."""
    from active_tracking_rl_amd import fused
    funcs = _header_functions(_policy_header())
    assert sorted(funcs) == _header_symbols("atr_policy.h", "atr_") == sorted(fused.ATR_PROTOTYPES) and len(funcs) == 54
    for name, (res, params) in funcs.items():
        restype, argtypes = fused.ATR_PROTOTYPES[name][:2]
        assert _py_class(restype) == res, name
        assert len(argtypes) == len(params), name
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _py_class(a) == c, (name, i)


def test_structures_match_the_policy_header():
    """Every typedef struct of include/atr_policy.h has its ctypes.Structure in fused.ATR_STRUCTS with the same field names,
    order, array lengths and classes."""
    from active_tracking_rl_amd import fused
    structs = _header_structs(_policy_header())
    assert sorted(structs) == sorted(fused.ATR_STRUCTS) and len(structs) == 8
    for name, fields in structs.items():
        got = []
        for fname, t in fused.ATR_STRUCTS[name]._fields_:
            arr = issubclass(t, ctypes.Array)
            got.append((fname, _py_class(t._type_ if arr else t), t._length_ if arr else None))
        assert got == fields, name


def test_launch_status_is_checked_in_one_place():
    """A status-returning entry point gets the table's errcheck: non-zero raises RuntimeError naming the entry point that
    failed, 0 comes back as 0. The int results that are values (or that the caller handles) are the ones marked VALUE."""
    from active_tracking_rl_amd import fused
    for name in ("atr_embed_add_ld", "atr_rollout_end2", "atr_lstm_cell_forward_act1", "atr_lstm_bptt_pre2"):
        check = fused._errcheck(name)
        assert check(0, None, ()) == 0
        with pytest.raises(RuntimeError, match=r"^%s failed \(-2\)$" % name):
            check(-2, None, ())
    unchecked = sorted(n for n, e in fused.ATR_PROTOTYPES.items() if e[0] is ctypes.c_int and fused.VALUE in e[2:])
    assert unchecked == ["atr_gate_cell_workgroups", "atr_gemm_tn_set_corun", "atr_linear_kernel_name", "atr_linear_plan_info",
                         "atr_linear_set_choice", "atr_lt_init", "atr_lt_library_info"]
    assert all(e[0] is ctypes.c_int for e in fused.ATR_PROTOTYPES.values() if fused.VALUE in e[2:])
    assert sorted(fused._ERROR_DETAIL) == ["atr_act_env_step", "atr_coop_env_step", "atr_linear"]


def test_library_binding_applies_the_table():
    """fused.lib() on the built library: every entry point carries the table's prototype, the checked ones the errcheck (with
    the library's own error text where it keeps one), the VALUE ones none."""
    from active_tracking_rl_amd import build, fused
    build.build()
    L = fused.lib()
    for name, (restype, argtypes, *value) in fused.ATR_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes or []) == list(argtypes), name
        assert (f.errcheck is not None) == (restype is ctypes.c_int and not value), name
    assert L.atr_gemm_tn.errcheck(0, None, ()) == 0
    with pytest.raises(RuntimeError, match=r"^atr_linear failed \(-1\): "):
        L.atr_linear.errcheck(-1, None, ())
    with pytest.raises(RuntimeError, match=r"^atr_coop_env_step failed \(-3\): "):
        L.atr_coop_env_step.errcheck(-3, None, ())


def test_registry_matches_reference():
    from active_tracking_rl_amd import registry
    rows = np.load(os.path.join(GOLDEN, "registry.npz"))["rows"]
    assert len(rows) == 72 == len(registry.REGISTRY)
    for env_id, mp, ob, lvl, tgt, mx in rows:
        r = registry.REGISTRY[str(env_id)]
        assert (r["map_type"], r["obs_type"], str(r["level"]), r["target_mode"], str(r["max_episode_steps"])) == \
            (str(mp), str(ob), str(lvl), str(tgt), str(mx))
    assert registry.spec("Track2D-BlockPartialPZR-v0")["target_mode"] == "PZR"
    assert registry.spec("Track2D-BlockFullPZR-v0")["obs_type"] == "Full"
    assert registry.spec("Track2D-BlockPartialRPF-v0")["target_mode"] == "RPF"
    for env_id in registry.REGISTRY:                       # all 72 ids resolve
        assert registry.spec(env_id)["max_episode_steps"] == 500
    with pytest.raises(KeyError):
        registry.spec("Track2D-Nope-v0")


def test_no_cpu_fallback():
    import torch
    from active_tracking_rl_amd import vec_env
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(vec_env.T2DError):
        vec_env.VecTrack2D("Track2D-BlockPartialPZR-v0", num_envs=4)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "active_tracking_rl_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f
                assert "libtrack2d_oracle" not in txt, f


def test_evaluator_train_mode_schedule_follows_the_reference():
    """test.py:84-92 restated (active_tracking_rl_amd.test.schedule_train_modes): expected values derived by hand from the
    reference's branch order — below --init-step: 0; --train-mode 2 and more than iter_th iterations since the last flip:
    1 - mode, then iter_th = --init-step if the new mode is 0 else --adv-step; otherwise --train-mode."""
    import argparse
    from active_tracking_rl_amd.test import schedule_train_modes
    args = argparse.Namespace(init_step=10, adv_step=5, train_mode=2)
    modes, st = [0, 0], {}
    seen = []
    for n_iter in (5, 12, 13, 18, 20, 24):
        schedule_train_modes(args, modes, n_iter, st)
        seen.append(list(modes))
    # 5 < 10 -> 0 | 12 - 0 > 10: rank 0 flips 0 -> 1 (last_iter = 12, iter_th = 5), rank 1 then sees 12 - 12 > 5 false -> 2
    # 13: 1 > 5 false -> 2 | 18: 6 > 5: rank 0 flips 2 -> -1, rank 1 -> 2 | 20 -> 2 | 24: rank 0 flips 2 -> -1
    assert seen == [[0, 0], [1, 2], [2, 2], [-1, 2], [2, 2], [-1, 2]]
    # the ordinary schedule (--init-step warm-up, then --train-mode)
    args = argparse.Namespace(init_step=10, adv_step=None, train_mode=-1)
    modes, st = [0], {}
    assert [list(schedule_train_modes(args, modes, n, st)) for n in (0, 9, 10, 500)] == [[0], [0], [-1], [-1]]
    # --train-mode 2 without --adv-step: the reference stops with AttributeError at its first flip away from the tracker
    args = argparse.Namespace(init_step=3, train_mode=2)
    with pytest.raises(AttributeError):
        schedule_train_modes(args, [0], 7, {})


def test_cooperative_step_shape_limits_match_the_kernel():
    """fused.coop_step_supported (what model._act_step asks before it takes the two-launch step) restates the limits
    atr_coop_env_step enforces (csrc/coop_gemm.h: 16 tiles per layer and 8 env pairs per workgroup, whole 16-row tiles per XCD)."""
    from active_tracking_rl_amd import fused
    ok = lambda n, wg: fused.coop_step_supported(n, 256, 128, wg)
    assert ok(512, 256) and ok(1024, 256) and ok(2048, 256) and ok(128, 256)
    assert not ok(4096, 256)            # 32 gate tiles per workgroup
    assert ok(512, 128) and ok(1024, 128) and not ok(2048, 128)
    assert not ok(500, 256) and not ok(512, 100) and not ok(512, 4)
    assert not fused.coop_step_supported(512, 250, 128, 256) and not fused.coop_step_supported(512, 256, 64, 256)
