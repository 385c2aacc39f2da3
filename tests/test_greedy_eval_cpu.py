"""CPU-side checks of the graphed greedy evaluation: the new header include/atr_eval.h against the built library and against
the evaluator's own prototype table and structure (the parsing of tests/test_abi_cpu.py, applied to the new header); the host
model of the kernel's episode accounting; the policy fixture of the GPU tests on the reference path alone; and no CPU fallback."""
import ctypes
import os
import re

import numpy as np
import pytest

import greedy_eval_spec as gs
from conftest import ROOT
from test_abi_cpu import _c_class, _header_functions, _header_structs, _py_class


def _eval_header():
    """include/atr_eval.h without comments and preprocessor lines."""
    txt = open(os.path.join(ROOT, "include", "atr_eval.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    return "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", txt).split("\n") if not ln.lstrip().startswith("#"))


def test_library_exports_every_function_of_the_eval_header():
    from active_tracking_rl_amd import build, vec_env
    build.build()
    assert os.path.join("..", "..", "include", "atr_eval.h") in build.HEADERS
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    funcs = _header_functions(_eval_header())
    assert sorted(funcs) == ["atr_eval_act_env_step"]
    for name in funcs:
        assert hasattr(lib, name), name


def test_eval_prototypes_and_struct_match_the_header():
    """evaluator.EVAL_PROTOTYPES / EVAL_STRUCTS are include/atr_eval.h's ABI: every declared function with the header's
    parameter count and class per parameter, the struct field by field; the struct parameters are bound as pointers to the
    matching ctypes.Structure (atr_act_step: fused.ActStepArgs, which test_abi_cpu.py holds to include/atr_policy.h)."""
    from active_tracking_rl_amd import evaluator, fused
    txt = _eval_header()
    funcs = _header_functions(txt)
    assert sorted(funcs) == sorted(evaluator.EVAL_PROTOTYPES)
    for name, (res, params) in funcs.items():
        restype, argtypes = evaluator.EVAL_PROTOTYPES[name]
        assert _py_class(restype) == res == ctypes.c_int, name
        assert len(argtypes) == len(params), name
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _py_class(a) == c, (name, i)
    m = re.search(r"atr_eval_act_env_step\s*\(([^()]*)\)", txt)
    kinds = [re.sub(r"\w+$", "", p.strip()).strip() for p in m.group(1).split(",")]
    at = evaluator.EVAL_PROTOTYPES["atr_eval_act_env_step"][1]
    assert kinds[1] == "const atr_act_step *" and at[1]._type_ is fused.ActStepArgs
    assert kinds[2] == "const atr_eval_out *" and at[2]._type_ is evaluator.EvalOut
    structs = _header_structs(txt)
    assert sorted(structs) == sorted(evaluator.EVAL_STRUCTS) == ["atr_eval_out"]
    for name, fields in structs.items():
        got = [(f, _py_class(t), None) for f, t in evaluator.EVAL_STRUCTS[name]._fields_]
        assert got == fields, name
    assert _c_class("float *") == "ptr"


def test_eval_binding_checks_status():
    """evaluator.lib() binds the table on the built library with an errcheck that raises like fused._errcheck does."""
    from active_tracking_rl_amd import build, evaluator
    build.build()
    f = evaluator.lib().atr_eval_act_env_step
    assert f.restype is ctypes.c_int and list(f.argtypes) == evaluator.EVAL_PROTOTYPES["atr_eval_act_env_step"][1]
    assert f.errcheck(0, None, ()) == 0
    with pytest.raises(RuntimeError, match=r"^atr_eval_act_env_step failed \(-1\): "):
        f.errcheck(-1, None, ())
    # no device is touched by a refused call: the handle check comes first
    with pytest.raises(RuntimeError, match="needs an env handle"):
        f(None, None, None, None, 1, None, None, None)


def test_accounting_host_model():
    """evaluator.account on synthetic rew [T,N,2] / done [T,N] against a per-env Python loop in the issue's words:
    rsum += alive ? rew : 0 (float32, step order); length += alive; alive &= !done. Continuing from given accounts equals
    running the steps in one go."""
    from active_tracking_rl_amd import evaluator
    rs = np.random.RandomState(3)
    T, N = 57, 19
    rew = rs.randn(T, N, 2).astype(np.float32)
    done = (rs.rand(T, N) < 0.04).astype(np.uint8)
    done[:, 0] = 0                                    # one env never finishes
    done[0, 1] = 1                                    # one finishes at once
    rsum, length, alive = evaluator.account(rew, done)
    assert rsum.dtype == np.float32 and length.dtype == np.int32 and alive.dtype == np.uint8
    for e in range(N):
        s, ln, al = np.zeros(2, np.float32), 0, True
        for t in range(T):
            if al:
                s = (s + rew[t, e]).astype(np.float32)
                ln += 1
            al = al and not done[t, e]
        assert np.array_equal(rsum[e], s) and length[e] == ln and bool(alive[e]) == al, e
    assert length[0] == T and alive[0] == 1 and length[1] == 1 and alive[1] == 0
    first = evaluator.account(rew[:20], done[:20])
    again = evaluator.account(rew[20:], done[20:], *first)
    assert all(np.array_equal(a, b) for a, b in zip(again, (rsum, length, alive)))


def test_fixture_policy_meets_the_near_tie_cap_on_the_reference_path():
    """The GPU tests' fixture (seeded initial weights, actor rows x 100) on the reference path alone — the eager model on the
    CPU over the oracle, test.evaluate's env ids — yields a near-tie share under the cap (observed: 0 of 306 alive rows on
    Track2D-BlockPartialNav-v0, 0 of 1142 on Track2D-BlockPartialPZR-v0, 6 episodes each; 0 of 4284 and 0 of 17392 at 100)."""
    for env_id in ("Track2D-BlockPartialNav-v0", "Track2D-BlockPartialPZR-v0"):
        args = gs.fixture_args(env_id, 6)
        model = gs.fixture_model(args)
        model.eval()
        ref = gs.reference_round(model, env_id, 6)
        assert ref["rows"] >= 2 * 6 * 11 and ref["near_ties"] <= gs.CAP * ref["rows"], (env_id, ref["near_ties"], ref["rows"])
        assert ref["rsum"].shape == (6, 2) and (ref["length"] >= 11).all()


def test_graphed_evaluation_has_no_cpu_fallback():
    """evaluate(..., graphed=True) without a GPU raises the T2DError the eager evaluator raises; supported() is False for
    anything that is not the fused-step VecEnv."""
    import torch
    from active_tracking_rl_amd import evaluator, vec_env
    from active_tracking_rl_amd.test import evaluate
    args = gs.fixture_args("Track2D-BlockPartialNav-v0", 4)
    model = gs.fixture_model(args)
    assert not evaluator.supported(object(), model)
    if torch.cuda.is_available():
        return
    for graphed in (False, True):
        with pytest.raises(vec_env.T2DError):
            evaluate(model, "Track2D-BlockPartialNav-v0", args, torch.device("cuda:0"), 4, graphed=graphed)
    with pytest.raises(vec_env.T2DError):
        evaluator.GreedyEvaluator(model, "Track2D-BlockPartialNav-v0", args, torch.device("cuda:0"), 4)
