/*
 * track2d_state.h — env shard snapshots: save, restore and rewind the device-resident env state of a t2d_handle
 * (include/track2d.h), and carry it through host memory as one blob.
 *
 * In the reference the env is a Python object, so copy.deepcopy(env) or a pickle is a snapshot of a running env
 * (G/envs/track_1v1.py holds all of it in attributes). Here the state is a structure of arrays in HBM behind the handle;
 * a t2d_snapshot is a second set of those arrays, laid out like the handle's own, that one kernel launch (csrc/state_hip.hip:
 * k_state_copy) fills from the handle or writes back to it.
 *
 * What a snapshot holds, per env: every array a step or generator pass reads as state —
 *   the current episode (map tile, positions, goals, counters, episode number, scripted-target plan, TARGET stream counter,
 *   Nav goal, RPF patrol word, last squared distance, Nav direction planes), both pre-generated next-episode slots (the same
 *   fields and the window rows of their first observation), the Nav plan queues, the grown-ahead maze ring — and the handle's
 *   host counter of t2d_step_random.
 * What it does not hold: the per-env configuration word (compared, never restored), the sticky fault word and the pregrow
 *   statistics (left alone), the reward table, and the slot request stamps: t2d_snapshot_save and t2d_snapshot_restore begin
 *   with what t2d_flush does on `stream` (forked generator and pregrow launches joined, consumed slots regenerated, stamps back
 *   to 0), so every slot is valid on both sides of the copy.
 *
 * Rewinding. A generated episode is a pure function of (seed, global env id, episode number): an env put back to an earlier
 * state of ITSELF reproduces its future bit for bit under the same actions, whatever the other envs of the handle did in
 * between. Copying one env's state into another env is not offered: generation is keyed by the global env id.
 *
 * Streams. Save and restore are asynchronous on `stream` apart from the flush; export and import synchronise it. None of
 * the calls may be captured into a hipGraph (they launch a generator pass that depends on host-side stamps, and restore
 * writes a host counter). A restore BETWEEN two replays of a captured rollout is fine: the handle's arrays keep their
 * addresses, and a captured rollout starts at stamp 0. A t2d_pregrow(T2D_PREGROW_INLINE) launch on another stream is not
 * ordered against save / restore by the library: the caller orders it.
 *
 * Masks. mask_dev: NULL = every env, else N bytes on the device, non-zero = take part. A masked save overwrites only those
 * envs' rows of the snapshot, a masked restore only those envs of the handle. The t2d_step_random counter is recorded and
 * reinstated only by calls with a NULL mask. The first save into a snapshot must cover every env (until then, or until an
 * import, its contents are undefined and a restore is refused with T2D_ERR_STATE).
 *
 * Refusals (T2D_ERR_INVALID; t2d_last_error() names the field):
 *   - a snapshot used with a handle other than the one it was created for ("handle");
 *   - a blob whose header differs from the snapshot's handle in N ("num_envs"), "env_id_base", "seed", "max_episode_steps",
 *     "auto_reset", "obs_type", "action_type", any env's configuration word ("cfg"), or the optional "sections";
 *   - a handle with numpy-legacy streams attached (t2d_np_attach, include/track2d_np.h): the reference-exact mode keeps per-env
 *     MT19937 state and host-driven targets that a snapshot does not hold — out of scope here;
 *   - a handle with a trace store attached (t2d_trace_attach, include/track2d_trace.h): the position record of the running
 *     episode is not part of a snapshot, so a rewound env would disagree with its own trace — out of scope here.
 *
 * Host blob (little-endian throughout; a reader needs no library):
 *   offset  size  field
 *        0     8  magic "T2DSNAP\0"
 *        8     4  u32 format version (T2D_SNAPSHOT_VERSION = 1)
 *       12     4  u32 header size in bytes (T2D_SNAPSHOT_HEADER_BYTES = 96)
 *       16     4  u32 num_envs (N)
 *       20     4  u32 env_id_base
 *       24     8  u64 seed
 *       32     4  i32 max_episode_steps
 *       36     4  i32 auto_reset
 *       40     4  u32 obs_type
 *       44     4  u32 action_type
 *       48     8  u64 hash of the N configuration words: FNV-1a 64 (offset basis 0xcbf29ce484222325, prime 0x100000001b3) over
 *                 their 4 N bytes in memory order
 *       56     4  u32 sections: bit 0 the Nav arrays are present, bit 1 the maze ring is present
 *       60     4  u32 t2d_step_random counter
 *       64     8  u64 payload size in bytes
 *       72    24  reserved, zero
 *   The payload follows the header: u32 arrays, each whole and in the handle's own layout [planes][N][words], in this order
 *   (planes x words per env):
 *     maps 1x256, pos 1x1, goals 1x1, cnt 1x1, episode 1x1, plan 1x1, tctr 1x1, navgoal 1x1, nav2 1x1, d2 1x1,
 *     n_maps 2x256, n_pos 2x1, n_goals 2x1, n_plan 2x1, n_tctr 2x1, n_navgoal 2x1, n_nav2 2x1, n_d2 2x1, n_win 2x32,
 *     [sections bit 0] dirf 1x512, n_dirf 2x512, p_field 6x768, p_goal 6x1, p_tctr 6x1, p_state 3x1,
 *     [sections bit 1] g_maps 4x256, g_ep 4x1
 *   (next-episode slot p of env e is plane p; plan queue slot q of episode ep is plane (ep % 3) * 2 + q, its state word plane
 *   ep % 3; ring entry of episode ep is plane ep % 4). t2d_snapshot_import checks magic, version, sizes and every compared field
 *   before it touches the device; the payload's contents are taken as they are (a blob is trusted like a checkpoint file).
 */
#ifndef TRACK2D_STATE_H
#define TRACK2D_STATE_H

#include <stdint.h>

#include "track2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define T2D_SNAPSHOT_VERSION 1
#define T2D_SNAPSHOT_HEADER_BYTES 96
#define T2D_SNAPSHOT_SECTION_NAV 1u
#define T2D_SNAPSHOT_SECTION_RING 2u

typedef struct t2d_snapshot t2d_snapshot;          /* device-resident copy of the state of every env of one handle */

/* Arrays sized like the handle's own; contents undefined until the first save or import. */
int t2d_snapshot_create(t2d_handle *h, t2d_snapshot **out);
int t2d_snapshot_destroy(t2d_snapshot *s);
/* handle -> snapshot for the masked envs (mask_dev NULL: all). Flushes first; not capturable. */
int t2d_snapshot_save(t2d_handle *h, t2d_snapshot *s, const uint8_t *mask_dev, void *stream);
/* snapshot -> handle for the masked envs (mask_dev NULL: all, and the t2d_step_random counter). Flushes first; not capturable. */
int t2d_snapshot_restore(t2d_handle *h, const t2d_snapshot *s, const uint8_t *mask_dev, void *stream);
/* Size of the host blob (header + payload). */
long long t2d_snapshot_bytes(const t2d_snapshot *s);
/* Snapshot -> blob_host[bytes] (bytes == t2d_snapshot_bytes). Synchronises the stream. */
int t2d_snapshot_export(const t2d_snapshot *s, void *blob_host, long long bytes, void *stream);
/* blob_host[bytes] -> snapshot, after validating the header against the snapshot's handle. Synchronises the stream. */
int t2d_snapshot_import(t2d_snapshot *s, const void *blob_host, long long bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
