/*
 * track2d_bank.h — map banks: the envs of a handle run on fixed, caller-supplied maps (csrc/track2d_hip.hip).
 *
 * Every generated episode of a handle starts by filling the wave's 1 KiB map tile: grown (Maze), scattered (Block) or empty.
 * A map bank is a fourth source for that tile: K maps held on the device, bit-packed as the env tiles are, with an optional
 * fixed start position per map. Attached before the handle's first reset, it replaces the map generators for every episode
 * the handle generates from then on (both pre-generated slots, every generator kernel form, the forced pass of the first
 * reset). Everything else about an episode is unchanged, draw for draw: goal and spawn sampling (SPAWN stream), scripted
 * targets (TARGET stream), rewards, time limit. The step kernels read slots and never see the difference.
 *
 * The selection rule. Let genv = env_id_base + e, and ep the episode number the slot is generated for: the number
 * t2d_get_state reports as `episode` while the env runs it. K = the bank's count.
 *   T2D_BANK_CYCLE    idx = ((uint64)genv + ep) mod K
 *   T2D_BANK_RANDOM   idx = Stream(k0, k1, ep, genv, STREAM_MAP, ctr = 0).bounded(K - 1), the Stream of csrc/t2d_device.h:
 *                     word i is component (i & 3) of philox4x32_10(key (k0, k1), counter (i >> 2, ep, genv, 0)), k0 / k1 the
 *                     low / high 32 bits of the seed; bounded(m) uses mask = the smallest 2^b - 1 >= m and takes words from
 *                     i = 0 until (word & mask) <= m. K = 1 draws nothing.
 * The MAP stream has no other consumer on a banked handle, and the SPAWN and TARGET streams are untouched: an env whose bank
 * map equals the map the generator would have produced for (genv, ep) gets exactly the episode the generator would have
 * produced. The handle's `level` is ignored.
 *
 * A map with a spawn row starts tracker and target on the row's cells: sample_goal(2) still draws first and the goal-test
 * loop still runs, the tracker draw and the get_around draw are skipped. A row of four -1 samples as usual.
 *
 * Conventions as in track2d.h (status codes, t2d_last_error, `stream` = hipStream_t as void *).
 */
#ifndef TRACK2D_BANK_H
#define TRACK2D_BANK_H

#include <stdint.h>

#include "track2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define T2D_BANK_CYCLE 0
#define T2D_BANK_RANDOM 1
#define T2D_BANK_MAX_MAPS 65536

/* Attach a bank of `count` maps to a handle that has not been reset yet. maps_host: [count][side*side] u8, 0 free / 1 wall,
 * row-major; spawns_host: NULL or [count][4] = {tracker r, c, target r, c}, a row of four -1 = "sample as usual". Packs on the
 * host, copies to a device buffer the handle owns (freed by t2d_destroy), synchronises.
 * T2D_ERR_STATE: after the handle's first t2d_reset / t2d_inject, or on a second attach.
 * T2D_ERR_INVALID (before any device work; t2d_last_error names the map and the reason): null handle or maps; count outside
 * 1 .. T2D_BANK_MAX_MAPS; select outside 0 .. 1; side different from the side of any env of the handle (82 Block / Empty, 81
 * Maze); a handle with numpy streams (t2d_np_attach) or with T2D_TGT_RPF / T2D_TGT_EXT envs; a map cell other than 0 / 1; a
 * map whose border is not all wall; a map with fewer than 3 free cells; a spawn row that is neither all -1 nor two free
 * in-map cells. */
int t2d_map_bank_attach(t2d_handle *h, const uint8_t *maps_host, const int32_t *spawns_host, int count, int side, int select,
                        void *stream);

/* The bank index of every env's current episode, by the rule above from episode[e]: idx_dev [N] i32. One launch on `stream`:
 * no synchronisation, no allocation, capturable. T2D_ERR_STATE without a bank or before the first reset. (On a handle with
 * priorities, track2d_bank_prio.h, the index is what the table drew for the episode, read from the handle's index ring.) */
int t2d_map_bank_index(t2d_handle *h, int32_t *idx_dev, void *stream);

/* K, or 0 without a bank. */
int t2d_map_bank_count(const t2d_handle *h);

#ifdef __cplusplus
}
#endif
#endif
