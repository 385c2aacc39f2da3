"""CPU checks of the GRU cores' opt-in fused step (--fused-gru; include/atr_gru_step.h):
  * model.gru_step_consts: ONE 4R-wide product over [features | k h_prev] rows + the cell expression of tests/gru_fused_spec.py
    = torch.nn.GRUCell in float64, with non-zero biases, masked rows and the tracker-action embedding;
  * the switch: off by default, never on with CPU tensors, accepted by both parsers;
  * the new header against the built library and fused.GRU_STEP_PROTOTYPES (the parsing of tests/test_abi_cpu.py);
  * the single-launch cases of tests/test_gru_fused_gpu.py meet their 0.9 clear-row condition on the float64 spec alone."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import gru_fused_spec as spec
from conftest import ROOT
from test_abi_cpu import _header_functions, _py_class


@pytest.mark.parametrize("tat", [False, True])
def test_one_product_step_equals_grucell_in_float64(tat):
    from active_tracking_rl_amd import model as M
    torch.manual_seed(5 + tat)
    N, Fd, R, A = 9, 256, 128, 4
    cells = [nn.GRUCell(Fd, R).double() for _ in range(2)]
    fa = nn.Linear(A, Fd).double() if tat else None
    with torch.no_grad():
        for c in cells:
            c.bias_ih.normal_(0, 0.5)
            c.bias_hh.normal_(0, 0.5)
    W4, b4, E4 = M.gru_step_consts(cells, fa)
    assert W4.shape == (2, 4 * R, Fd + R) and b4.shape == (2, 4 * R) and W4.dtype == torch.float64
    assert (E4 is None) == (not tat)
    if tat:
        assert E4.shape == (A, 4 * R) and float(E4[:, 3 * R:].abs().max()) == 0.0 and float(E4[:, :3 * R].abs().max()) > 0.0
    assert float(W4[:, 2 * R:3 * R, Fd:].abs().max()) == 0.0 and float(W4[:, 3 * R:, :Fd].abs().max()) == 0.0
    f = torch.randn(2, N, Fd, dtype=torch.float64)
    h = torch.randn(2, N, R, dtype=torch.float64)
    k = (torch.arange(N) % 3 != 0).double().view(1, N, 1)
    a = torch.randint(0, A, (N,))
    with torch.no_grad():
        for p in range(2):
            rows = torch.cat([f[p], k[0] * h[p]], 1)
            g = rows @ W4[p].t()
            emb = E4[a].numpy() if (tat and p == 1) else None
            got, acts = spec.cell(g.numpy(), b4[p].numpy(), (k[0] * h[p]).numpy(), emb)
            x = f[p] + fa(nn.functional.one_hot(a, A).double()) if (tat and p == 1) else f[p]
            want = cells[p](x, k[0] * h[p]).numpy()
            assert np.abs(got - want).max() <= 1e-12
            assert acts.shape == (N, 4 * R) and np.abs(acts[:, :2 * R]).max() <= 1.0


def test_switch_is_off_by_default_and_never_on_for_cpu_tensors(monkeypatch):
    from active_tracking_rl_amd.environment import _spaces
    from active_tracking_rl_amd.model import build_model
    from active_tracking_rl_amd.train import default_args
    obs, act = _spaces()
    monkeypatch.delenv("ATR_FUSED_GRU", raising=False)
    m = build_model(obs, act, default_args(network="tat-maze-gru"), torch.device("cpu"))
    assert m.fused_gru_step is False and m.cacheable_core is False and m.gru_core is True
    on = build_model(obs, act, default_args(network="tat-maze-gru", fused_gru=True), torch.device("cpu"))
    assert on.fused_gru_step is True and on.cacheable_core is False
    st = torch.zeros((4, 2, 1, 1, 13, 13))
    assert on.new_cache(3, st, env_fused=True) is None and m.new_cache(3, st, env_fused=True) is None
    monkeypatch.setenv("ATR_FUSED_GRU", "1")
    env_on = build_model(obs, act, default_args(network="maze-gru"), torch.device("cpu"))
    assert env_on.fused_gru_step is True and env_on.cacheable_core is False
    lstm = build_model(obs, act, default_args(network="tat-maze-lstm", fused_gru=True), torch.device("cpu"))
    assert lstm.cacheable_core is True and lstm.gru_core is False


@pytest.mark.parametrize("script", ["main.py", "gym_eval.py"])
def test_parsers_accept_the_switch(script):
    code = ("import sys, runpy; sys.argv = [%r, '--fused-gru']; ns = runpy.run_path(%r, run_name='not_main'); "
            "a = ns['parser'].parse_args(); b = ns['parser'].parse_args([]); print(a.fused_gru, b.fused_gru)"
            % (script, os.path.join(ROOT, script)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "True False"


def test_step_header_library_and_prototype_table_agree():
    from active_tracking_rl_amd import build, fused, vec_env
    build.build()
    assert os.path.join("..", "..", "include", "atr_gru_step.h") in build.HEADERS
    txt = open(os.path.join(ROOT, "include", "atr_gru_step.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", txt).split("\n") if not ln.lstrip().startswith("#"))
    funcs = _header_functions(txt)
    lib = ctypes.CDLL(vec_env.LIB_PATH)
    assert sorted(funcs) == sorted(fused.GRU_STEP_PROTOTYPES) == ["atr_gru_act_env_step", "atr_gru_eval_act_env_step"]
    L = fused.lib()
    for name, (res, params) in funcs.items():
        assert hasattr(lib, name), name
        restype, argtypes = fused.GRU_STEP_PROTOTYPES[name]
        assert _py_class(restype) == res == ctypes.c_int and len(argtypes) == len(params), name
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _py_class(a) == c, (name, i)
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes and f.errcheck is not None
    assert not set(fused.GRU_STEP_PROTOTYPES) & (set(fused.ATR_PROTOTYPES) | set(fused.GRU_PROTOTYPES))
    # a refusal is raised from the table's errcheck with the library's own text
    with pytest.raises(RuntimeError, match=r"^atr_gru_act_env_step failed \(-?\d+\): atr_gru_act_env_step: null argument"):
        L.atr_gru_act_env_step(None, None, None, None, 0, None, 0, None, None, None)
    with pytest.raises(RuntimeError, match=r"atr_gru_eval_act_env_step: needs an env handle"):
        L.atr_gru_eval_act_env_step(None, None, None, None, 0, None, None, 0, None, None, None)


@pytest.mark.parametrize("n", [33, 64])
@pytest.mark.parametrize("tat", [True, False])
def test_single_launch_cases_meet_the_clear_row_share_on_the_spec_alone(n, tat):
    """The condition tests/test_gru_fused_gpu.py puts on its action checks — at least 0.9 of the rows are clear — holds for the
    chosen seeds on the float64 spec alone (draw margins under an arbitrary counter value: they barely depend on it)."""
    case = spec.launch_case(n, tat)
    for t in range(spec.T):
        for kind in ("draw", "greedy"):
            for p, (h, acts, logits, clear, act) in enumerate(spec.step_model(case, t, kind, ordinal=2 * t + 1)):
                assert clear.mean() >= 0.9, (t, kind, p, clear.mean())
                assert np.isfinite(h).all() and (case["hp"][t][p].abs().sum(1) == 0).any()


def test_build_refuses_scratch_in_the_gru_step():
    """build.scratch_users reads the compiler's resource remarks: a k_gru_step instantiation with scratch is reported, other
    kernels' scratch is not its business, and remarks that name no such kernel are an error (nothing would be checked)."""
    from active_tracking_rl_amd import build
    assert build.NO_SCRATCH == {"track2d_hip.hip": "k_gru_step"} and "track2d_hip.hip" in build.SOURCES
    rem = lambda name, scratch: ("a.hip:1:1: remark: Function Name: %s [%s]\n 1 | {\n   | ^\na.hip:1:1: remark:     VGPRs: 126 [%s]\n"
                                 "a.hip:1:1: remark:     ScratchSize [bytes/lane]: %d [%s]\n" % (name, build.REMARKS, build.REMARKS,
                                                                                               scratch, build.REMARKS))
    clean = rem("_Z10k_gru_stepILi4EEvv", 0) + rem("_Z7k_step2v", 24) + rem("_Z10k_gru_stepILi8EEvv", 0)
    assert build.scratch_users(clean, "k_gru_step") == []
    assert build.scratch_users(clean + rem("_Z10k_gru_stepILi2EEvv", 16), "k_gru_step") == [("_Z10k_gru_stepILi2EEvv", 16)]
    with pytest.raises(RuntimeError, match="nothing to check"):
        build.scratch_users(rem("_Z7k_step2v", 0), "k_gru_step")
