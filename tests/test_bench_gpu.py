"""bench.py end to end on the GPU. With --full (small shard, no CPU baseline) the JSON line carries both schedules, the
shards, the roofline of the timed region's env kernel — and the run comes back. A plain run (the driver's flags) measures
the headline alone and computes what the --full run computes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_with_the_drivers_flags(tmp_path):
    out = str(tmp_path / "outputs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                        "--envs-per-gpu", "512", "--global-envs", "1024", "--full", "--no-cpu-baseline", "--dump-outputs", out],
                       capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"].startswith("env steps/sec") and line["unit"] == "env steps/s" and line["n_gpus"] == 1
    assert line["steps"] == 20 and line["higher_is_better"] is True and line["scaling"] == "weak" and line["full"] is True
    assert line["schedule"] in ("pipelined", "synchronous")
    other = "synchronous" if line["schedule"] == "pipelined" else "pipelined"
    assert other in line and "error" not in line[other] and line[other]["value"] > 0
    assert line["value"] >= line[other]["value"]                       # value = the faster schedule's
    assert abs(line["value"] - 20 * 512 / (line["ms_per_step"] * 20 * 1e-3)) / line["value"] < 1e-6
    # --steps is the number of timed steps: ONE region of exactly the 20 requested env steps, ms_per_step = its time / 20
    assert line["repeats_run"] == 1 and line["steps_requested"] == 20
    assert abs(line["timed_gpu_seconds"] - line["ms_per_step"] * 20 * 1e-3) <= 1e-9 * line["timed_gpu_seconds"]
    sizes = line["shards"]["sizes"]
    assert set(sizes) == {"128", "256", "512"} and all(v["value"] > 0 for v in sizes.values())
    roof = line["roofline"]
    assert roof["bound"] == "hbm" and roof["in_timed_region"] is True and 0.0 < roof["frac"] < 1.0
    assert roof["variant"] == "act_step" and "k_act_step" in roof["kernel"]
    # SURVEY 8(d)'s figure: 709 B per env-step (byte observations) over the kernel's in-situ duration; the wider byte count
    # (policy state the fused kernel also moves) only under its own name
    assert roof["bytes_per_env_step"] == 709 and roof["frac"] == roof["frac_8d"]
    assert roof["in_situ"] is not None and roof["avg_launch_us"] > 0 and roof["alone_us"] > 0
    assert roof["policy_state_included"]["bytes_per_env_step"] > 709
    assert "step_f32" in roof["other_variants"] and line["ranks"] == 1
    assert line["config"]["schedule"] == line["schedule"] and "workload" in line["config"]
    # --dump-outputs: both schedules' last step, float32 (float64 for the env index), 512 envs, at most 64 MB in all
    names = ("obs", "reward", "done", "actions", "hxs", "cxs", "eps_len", "env_index", "policy_loss", "value_loss",
             "entropy", "pred_loss", "weights", "grad")
    want = {"%s_%s.npy" % (s, n) for s in ("synchronous", "pipelined") for n in names}
    assert set(os.listdir(out)) == want
    arrays = {f: np.load(os.path.join(out, f)) for f in want}
    assert sum(x.nbytes for x in arrays.values()) <= 64 << 20
    for f, x in arrays.items():
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), f
    for s in ("synchronous", "pipelined"):
        assert np.array_equal(arrays[s + "_env_index.npy"], np.arange(512))
        assert arrays[s + "_obs.npy"].shape[0] == 512 and arrays[s + "_actions.npy"].shape == (512, 2)
        assert arrays[s + "_weights.npy"].shape == arrays[s + "_grad.npy"].shape and arrays[s + "_grad.npy"].any()


@pytest.mark.gpu
def test_bench_watchdog_prints_the_synchronous_line_when_the_pipelined_part_does_not_come_back():
    """--pipelined-timeout far below what the pipelined measurements need: the watchdog fires, rank 0 prints the line as
    assembled so far (the synchronous numbers) and the process leaves with exit code 0 — an N>1 run must never hang the driver."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                        "--envs-per-gpu", "512", "--full", "--no-shards", "--no-cpu-baseline", "--pipelined-timeout", "0.01"],
                       capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["schedule"] == "synchronous" and line["value"] > 0
    assert "did not complete" in line["pipelined"]["error"]
    assert line["roofline"]["in_timed_region"] is True


@pytest.mark.gpu
def test_dumped_outputs_are_the_same_in_every_run_with_the_same_arguments(tmp_path):
    """--dump-outputs exists so that two builds can be compared output for output: with the same arguments the timed path
    must start from the same state and compute the same arrays. Two runs, every array bit for bit; --steps 40 times 40 steps."""
    lines = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "20",
                            "--envs-per-gpu", "512", "--no-shards", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / run)],
                           capture_output=True, text=True, cwd=ROOT, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert all(x["steps"] == 40 and x["repeats_run"] == 1 for x in lines)
    files = sorted(os.listdir(str(tmp_path / "a")))
    assert files == sorted(os.listdir(str(tmp_path / "b"))) and len(files) == 28
    for f in files:
        x, y = np.load(str(tmp_path / "a" / f)), np.load(str(tmp_path / "b" / f))
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), f


@pytest.mark.gpu
def test_a_plain_run_measures_the_headline_alone_and_computes_what_a_full_run_computes(tmp_path):
    """Without --full the run sets up, warms up, times both schedules' regions, dumps and prints: no shard sweep, no kernel
    figures, no CPU baseline. What moved behind --full runs outside the headline regions, so the two runs' last timed steps
    must agree array for array."""
    lines = {}
    for run, extra in (("plain", []), ("full", ["--full", "--global-envs", "1024", "--no-cpu-baseline"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                            "--envs-per-gpu", "512", "--dump-outputs", str(tmp_path / run)] + extra,
                           capture_output=True, text=True, cwd=ROOT, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        lines[run] = json.loads(r.stdout.strip().splitlines()[-1])
    line = lines["plain"]
    assert line["full"] is False and line["steps"] == 20 and line["repeats_run"] == 1 and line["value"] > 0
    assert line["metric"] == lines["full"]["metric"] and line["unit"] == "env steps/s" and line["higher_is_better"] is True
    assert line["dtype"] == lines["full"]["dtype"]
    assert abs(line["value"] - 20 * 512 / (line["ms_per_step"] * 20 * 1e-3)) / line["value"] < 1e-6
    other = "synchronous" if line["schedule"] == "pipelined" else "pipelined"
    assert "error" not in line[other] and 0 < line[other]["value"] <= line["value"]
    assert line["shards"] is None and line[other]["shards"] is None
    for key in ("roofline", "env_only", "policy_stem", "kernel_sum_per_iteration", "cpu_baseline", "cpu_baselines"):
        assert key not in line, key
    assert lines["full"]["full"] is True and set(lines["full"]["shards"]["sizes"]) == {"128", "256", "512"}
    assert "roofline" in lines["full"] and "env_only" in lines["full"] and "policy_stem" in lines["full"]
    files = sorted(os.listdir(str(tmp_path / "plain")))
    assert files == sorted(os.listdir(str(tmp_path / "full"))) and len(files) == 28
    for f in files:
        x, y = np.load(str(tmp_path / "plain" / f)), np.load(str(tmp_path / "full" / f))
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), f
