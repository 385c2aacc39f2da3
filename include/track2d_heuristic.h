/*
 * track2d_heuristic.h — C ABI of the heuristic players in libtrack2d_hip.so: the shortest-path distance between the tracker and
 * the target of every env of a handle, a tracker that walks a shortest path to the target ("pursuit") and a target that steps to
 * the neighbouring cell farthest from the tracker ("evade"), for a whole shard in one launch. The reference has scripted
 * targets only (Ram: a random walk; Nav / RPF: walks to goals that ignore the tracker) and no scripted tracker; window offsets
 * and Euclidean distance do not know that a target two cells away behind a wall is thirty steps away.
 *
 * Per env: map[r][c] is 1 for a wall and 0 for a free cell; a cell outside the env's side x side square counts as a wall. The
 * tracker stands on cell T, the target on cell G. Moves are the VonNeumann table of track_1v1.py:276: action 0 = (-1, 0),
 * 1 = (+1, 0), 2 = (0, -1), 3 = (0, +1); dest(X, a) is the cell an agent on X would move to under action a. Agents are not
 * obstacles. D(X, Y) is the 4-connected breadth-first distance over free cells, INF if Y cannot be reached from X; D(X, X) = 0,
 * and D(X, Y) = INF for X != Y when X or Y is itself a wall (only an RPF env can place an agent on a wall: track_1v1.py:233-236).
 * d = D(T, G).
 *
 *   dist      d, or -1 if d = INF.
 *   hold(X)   the first a in 0, 1, 2, 3 whose dest(X, a) is a wall — the env then leaves the agent where it is
 *             (track_1v1.py:282-283) — or 0 if all four destinations are free.
 *   pursuit   (the tracker's action) if 0 < d < INF: the first a in 0 .. 3 with dest(T, a) free and D(dest(T, a), G) == d - 1;
 *             otherwise hold(T). The first case is what the goal-rooted direction field of the Nav target (csrc/t2d_device.h
 *             bfs_dir_field) stores at T when it is rooted at G.
 *   evade     (the target's action) if d < INF and some a in 0 .. 3 has dest(G, a) free with D(T, dest(G, a)) == d + 1: the first
 *             such a; otherwise hold(G), which covers a dead end and an unreachable tracker. On a 4-connected grid a neighbour's
 *             distance is d - 1 or d + 1, so "the farthest neighbour" and "a neighbour at d + 1" are one rule.
 *
 * Both players act on the current (pre-step) state; neither anticipates the other's simultaneous move.
 *
 * How it is computed: one wavefront per (env, role), the env's 1 KiB map tile as bit rows in registers. Pursuit floods from G and
 * stops at the level that reaches T; the direction planes at T are the answer. Evade floods from T until the level that reaches
 * G and then exactly one level more: the cells of that last frontier are the cells at distance d + 1, and the first neighbour of G
 * among them, in action order, is the answer. Level counters are full ints (a Maze path can be longer than 1024 steps).
 *
 * t2d_heuristic_actions writes act[e][0] (roles bit 0) and / or act[e][1] (roles bit 1) as int64 and, if dist is not null,
 * dist[e] as int32, for e = 0 .. N-1. The column of a role that is not asked for is left untouched, so a caller can hand over
 * the policy's own [N][2] action tensor and have one column overwritten in place. No env state is written; there are no atomics,
 * no allocation and no synchronisation. All pointers are device pointers; `stream` is a hipStream_t. The call enqueues exactly
 * one launch (capturable in a hipGraph) and returns 0 or a T2D_ERR_* code of include/track2d.h, with the text in
 * t2d_last_error(). Refused with T2D_ERR_INVALID before any device work: a null handle or a null act, roles outside 1 .. 3, act
 * not 8-byte aligned or dist not 4-byte aligned, a handle with the Moore action table, a handle whose envs have no current
 * episode yet (t2d_reset for all envs comes first).
 */
#ifndef TRACK2D_HEURISTIC_H
#define TRACK2D_HEURISTIC_H

#include "track2d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define T2D_HEUR_PURSUIT 1   /* roles bit 0: write act[e][0] */
#define T2D_HEUR_EVADE   2   /* roles bit 1: write act[e][1] */

int t2d_heuristic_actions(t2d_handle *h, int roles, long long *act_dev /* [N][2] */, int *dist_dev /* [N] or null */, void *stream);

#ifdef __cplusplus
}
#endif

#endif
