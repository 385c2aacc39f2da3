"""In-tree build of the HIP extension (gfx950 only). `python -m active_tracking_rl_amd.build [--force]`.

Every source is compiled to an object of its own (in parallel; only the ones older than their source or any header are
redone) under csrc/_obj/, then linked into libtrack2d_hip.so next to this file."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
LIB = os.path.join(HERE, "libtrack2d_hip.so")
SOURCES = ["track2d_hip.hip", "stem_hip.hip", "policy_hip.hip", "lstm_hip.hip", "heads_hip.hip", "gemm_tn_hip.hip",
           "actor_step_hip.hip", "pair_gemm_hip.hip", "bptt_hip.hip", "driver_hip.hip", "gate_cell_hip.hip", "episode_stats_hip.hip",
           "gru_hip.hip", "render_hip.hip", "tracking_stats_hip.hip", "state_hip.hip", "stem_full_hip.hip", "heuristic_hip.hip",
           "sight_stats_hip.hip", "occlusion_hip.hip", "fov_hip.hip", "footprints_hip.hip", "ego_hip.hip", "memory_hip.hip",
           "noise_hip.hip", "view_hip.hip", "np_mode.cpp", "lt_gemm.cpp"]
HEADERS = ["t2d_device.h", "t2d_rooms_rule.h", "atr_fov_rule.h", "atr_footprint_rule.h", "atr_ego_rule.h", "atr_memory_rule.h",
           "atr_noise_rule.h", "atr_view_rule.h",
           os.path.join("..", "..", "include", "track2d.h"),
           os.path.join("..", "..", "include", "atr_policy.h"), "atr_sample.h", "atr_cell.h",
           os.path.join("..", "..", "include", "track2d_np.h"), os.path.join("..", "..", "include", "atr_eval.h"),
           os.path.join("..", "..", "include", "atr_stats.h"), os.path.join("..", "..", "include", "atr_gru.h"),
           os.path.join("..", "..", "include", "atr_gru_step.h"), os.path.join("..", "..", "include", "atr_gru_sums.h"),
           os.path.join("..", "..", "include", "track2d_trace.h"), "t2d_trace_view.h",
           os.path.join("..", "..", "include", "atr_track_stats.h"),
           os.path.join("..", "..", "include", "track2d_state.h"), "t2d_state_view.h",
           os.path.join("..", "..", "include", "atr_stem_full.h"), os.path.join("..", "..", "include", "track2d_heuristic.h"),
           os.path.join("..", "..", "include", "atr_sight.h"), os.path.join("..", "..", "include", "atr_occlusion.h"),
           os.path.join("..", "..", "include", "track2d_bank.h"), os.path.join("..", "..", "include", "track2d_bank_prio.h"), os.path.join("..", "..", "include", "atr_fov.h"),
           os.path.join("..", "..", "include", "atr_footprints.h"), os.path.join("..", "..", "include", "atr_ego.h"),
           os.path.join("..", "..", "include", "atr_memory.h"), os.path.join("..", "..", "include", "atr_noise.h"),
           os.path.join("..", "..", "include", "atr_view.h")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-unused-result"]
LDFLAGS = ["--offload-arch=gfx950", "-fPIC", "-shared", "-ldl"]
# kernels that must not spill (source -> a part of their mangled names): the compiler's resource remarks are read when the source is
# compiled, and scratch > 0 bytes per lane in one of them fails the build (k_gru_step: the LSTM forms of the step have none)
NO_SCRATCH = {"track2d_hip.hip": "k_gru_step"}
# ... and the learner's: every k_gru_bptt instantiation (W_hh lives in 96 of its VGPRs; the by-action sums add 12 accumulators)
NO_SCRATCH_LEARNER = {"gru_hip.hip": "k_gru_bptt"}
# ... and the trace / render kernels (k_trace_begin, k_trace_append, k_render_cells, k_render_rgb)
NO_SCRATCH_RENDER = {"render_hip.hip": "k_"}
# ... and the tracking statistics (k_track_stats<uint8_t>, k_track_stats<float>, k_track_stats_drain: a chunk of steps lives in registers)
NO_SCRATCH_STATS = {"tracking_stats_hip.hip": "k_track_stats"}
# ... and the snapshot copy (k_state_copy: at most three 16-byte pieces per lane in flight)
NO_SCRATCH_STATE = {"state_hip.hip": "k_state_copy"}
# ... and the whole-map stem (k_stem_full_fwd, k_stem_full_bwd, k_stem_full_reduce: w2's MFMA fragments live in 36 / 72 VGPRs)
NO_SCRATCH_STEM_FULL = {"stem_full_hip.hip": "k_stem_full"}
# ... and the heuristic players (k_heuristic: the map's bit rows, two frontier sets and the direction planes live in registers)
NO_SCRATCH_HEURISTIC = {"heuristic_hip.hip": "k_heuristic"}
# ... and the sight statistics (k_sight_stats<uint8_t>, k_sight_stats<float>, k_sight_drain: a chunk of steps and each lane's bitboard,
# free cells and flood frontier live in registers)
NO_SCRATCH_SIGHT = {"sight_stats_hip.hip": "k_sight"}
# ... and the occluded observations (k_occlude<uint8_t>, k_occlude<float>: three cells and the window's three wall words per lane)
NO_SCRATCH_OCCLUSION = {"occlusion_hip.hip": "k_occlude"}
# ... and the field of view (k_fov<uint8_t>, k_fov<float>: three cells per lane)
NO_SCRATCH_FOV = {"fov_hip.hip": "k_fov"}
# ... and the footprints (k_footprints<uint8_t>, k_footprints<float>: one trail entry and one window cell per lane)
NO_SCRATCH_FOOTPRINTS = {"footprints_hip.hip": "k_footprints"}
# ... and the egocentric view (k_ego_actions, k_ego<uint8_t>, k_ego<float>: three cells per lane, parked in LDS)
NO_SCRATCH_EGO = {"ego_hip.hip": "k_ego"}
# ... and the map memory (k_memory<uint8_t>, k_memory<float>: three cells, four seen words and the 169-bit visible mask per lane; the
# tiles the paint reads are staged in LDS)
NO_SCRATCH_MEMORY = {"memory_hip.hip": "k_memory"}
# ... and the sensor noise (k_noise<uint8_t>, k_noise<float>: three cells and two Philox blocks per lane)
NO_SCRATCH_NOISE = {"noise_hip.hip": "k_noise"}
# ... and the player views (k_view_cells, k_view_rgb, each for uint8_t and float windows: the tile, the windows' codes and a band's
# colours are staged in LDS)
NO_SCRATCH_VIEW = {"view_hip.hip": "k_view"}
REMARKS = "-Rpass-analysis=kernel-resource-usage"


def _newest_header():
    return max(os.path.getmtime(os.path.join(CSRC, h)) for h in HEADERS)


def _obj(src):
    return os.path.join(OBJ, os.path.splitext(src)[0] + ".o")


def _stale(src, hdr_time):
    o = _obj(src)
    return not os.path.exists(o) or os.path.getmtime(o) < max(os.path.getmtime(os.path.join(CSRC, src)), hdr_time)


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in SOURCES + HEADERS)


def scratch_users(remarks, part):
    """The (mangled name, bytes per lane) of every kernel whose name holds `part` and that uses scratch memory, read from the
    compiler's kernel-resource-usage remarks; an error if the remarks name no such kernel (the check would check nothing)."""
    name, seen, bad = None, 0, []
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen += part in name
            continue
        m = re.search(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name is not None and part in name and int(m.group(1)) != 0:
            bad.append((name, int(m.group(1))))
    if not seen:
        raise RuntimeError("no resource remark names a %s kernel: the scratch check found nothing to check" % part)
    return bad


def build(force=False, verbose=False):
    """Compile csrc/*.hip into libtrack2d_hip.so next to this file (hipcc cross-compiles without a GPU)."""
    if not force and not needs_build():
        return LIB
    os.makedirs(OBJ, exist_ok=True)
    hdr_time = _newest_header()
    todo = [s for s in SOURCES if force or _stale(s, hdr_time)]

    def compile_one(src):
        cmd = [HIPCC] + CFLAGS + ["-c", os.path.join(CSRC, src), "-o", _obj(src)]
        if verbose:
            print(" ".join(cmd), flush=True)
        part = NO_SCRATCH.get(src) or NO_SCRATCH_LEARNER.get(src) or NO_SCRATCH_RENDER.get(src) or NO_SCRATCH_STATS.get(src)
        part = part or NO_SCRATCH_STATE.get(src) or NO_SCRATCH_STEM_FULL.get(src) or NO_SCRATCH_HEURISTIC.get(src)
        part = part or NO_SCRATCH_SIGHT.get(src) or NO_SCRATCH_OCCLUSION.get(src) or NO_SCRATCH_FOV.get(src)
        part = part or NO_SCRATCH_FOOTPRINTS.get(src) or NO_SCRATCH_EGO.get(src) or NO_SCRATCH_MEMORY.get(src)
        part = part or NO_SCRATCH_NOISE.get(src) or NO_SCRATCH_VIEW.get(src)
        if part is None:
            subprocess.check_call(cmd)
            return
        r = subprocess.run(cmd + [REMARKS], stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            raise subprocess.CalledProcessError(r.returncode, cmd)
        sys.stderr.write("".join(l + "\n" for l in r.stderr.splitlines() if "warning:" in l))
        bad = scratch_users(r.stderr, part)
        if bad:
            os.remove(_obj(src))
            raise RuntimeError("%s: scratch memory in %s" % (src, ", ".join("%s (%d bytes per lane)" % b for b in bad)))
    with ThreadPoolExecutor(max_workers=min(len(todo), os.cpu_count() or 4) or 1) as pool:
        list(pool.map(compile_one, todo))
    cmd = [HIPCC] + LDFLAGS + ["-o", LIB] + [_obj(s) for s in SOURCES]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
