// t2d_state_view.h — the one internal seam between csrc/track2d_hip.hip (which owns t2d_handle) and csrc/state_hip.hip
// (env shard snapshots, include/track2d_state.h): the state arrays of a handle in the blob's payload order, the fields a
// snapshot is compared by, and the host counter a full restore reinstates. Not part of the public ABI.
#pragma once
#include <stdint.h>

#include "../../include/track2d.h"

namespace t2d {

// Every state array is u32 [planes][N][words]; element (k, e) starts at ((size_t)k * N + e) * words — the indexing of the
// generator and step kernels (next-episode slots: plane = slot; plan queues: pq_index = ((ep % 3) * 2 + q) * N + e; ring: ep % 4).
struct StateArray { const char *name; int planes, words; };
constexpr int kStateCore = 19, kStateNav = 6, kStateRing = 2, kStateArrays = kStateCore + kStateNav + kStateRing;
constexpr StateArray kStateArray[kStateArrays] = {
    {"maps", 1, 256}, {"pos", 1, 1}, {"goals", 1, 1}, {"cnt", 1, 1}, {"episode", 1, 1}, {"plan", 1, 1}, {"tctr", 1, 1},
    {"navgoal", 1, 1}, {"nav2", 1, 1}, {"d2", 1, 1},
    {"n_maps", 2, 256}, {"n_pos", 2, 1}, {"n_goals", 2, 1}, {"n_plan", 2, 1}, {"n_tctr", 2, 1}, {"n_navgoal", 2, 1},
    {"n_nav2", 2, 1}, {"n_d2", 2, 1}, {"n_win", 2, 32},
    // the Nav arrays (handles with a Nav or RPF target, else null)
    {"dirf", 1, 512}, {"n_dirf", 2, 512}, {"p_field", 6, 768}, {"p_goal", 6, 1}, {"p_tctr", 6, 1}, {"p_state", 3, 1},
    // the grown-ahead maze ring (handles with Maze envs and 'Partial' observations, else null)
    {"g_maps", 4, 256}, {"g_ep", 4, 1},
};

}  // namespace t2d

struct t2d_state_view {
    int device, n, auto_reset, max_steps, obs_full, amask;
    uint32_t env_base, k0, k1;
    int ready;                  // every env has a current episode and, with auto_reset, valid next slots
    int np_attached;            // t2d_np_attach was called
    int trace_attached;         // t2d_trace_attach was called
    int prio_enabled;           // t2d_bank_prio_enable was called (the index ring and the table are not part of a snapshot)
    const uint32_t *cfg;        // [N] per-env configuration words (device)
    uint32_t *random_step;      // the handle's t2d_step_random counter (host)
    uint32_t *arr[t2d::kStateArrays];   // device arrays in kStateArray order
};

extern "C" int t2d_state_view_get(t2d_handle *h, t2d_state_view *out);
