// atr_ego_rule.h — the egocentric view's two tables and its cell map (include/atr_ego.h), plain C++17 with no HIP dependence: the
// kernels (ego_hip.hip k_ego, k_ego_actions) and the host test program (tests/ego_host.cpp) both use it. The heading is the
// facing byte of atr_fov_rule.h and turns by atr_fov::turn, which is not restated here.
//
// A heading is 0 .. 3: the VonNeumann moves 0 = (-1, 0), 1 = (+1, 0), 2 = (0, -1), 3 = (0, +1) as (ur, uc). A relative action k is
// 0 = forward, 1 = back, 2 = left, 3 = right. The egocentric window E of an absolute window W has, for the ego offset
// (er, ec) = (r - 6, c - 6), E[r][c] = W[6 + dr][6 + dc] with (dr, dc) = (-er * ur + ec * uc, -er * uc - ec * ur).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ATR_EGO_HD __host__ __device__ constexpr
#else
#define ATR_EGO_HD constexpr
#endif

namespace atr_ego {

constexpr int kSide = 13, kCentre = 6, kWindow = kSide * kSide;

// Two bits per entry, entry 4 * heading + k at bits 2 * (4 * heading + k): ABS rows 0 1 2 3 / 1 0 3 2 / 2 3 1 0 / 3 2 0 1 and
// their inverses REL rows 0 1 2 3 / 1 0 3 2 / 3 2 0 1 / 2 3 1 0 (a word each: no table in memory on the device).
constexpr unsigned pack4x4(const int (&t)[16])
{
    unsigned w = 0;
    for (int i = 0; i < 16; i++) w |= (unsigned)t[i] << (2 * i);
    return w;
}
constexpr int kAbsRows[16] = {0, 1, 2, 3, 1, 0, 3, 2, 2, 3, 1, 0, 3, 2, 0, 1};
constexpr int kRelRows[16] = {0, 1, 2, 3, 1, 0, 3, 2, 3, 2, 0, 1, 2, 3, 1, 0};
constexpr unsigned kAbsBits = pack4x4(kAbsRows), kRelBits = pack4x4(kRelRows);

// The heading of a facing byte: NONE, and whatever is no facing, looks up.
ATR_EGO_HD int heading_of(int facing) { return facing >= 0 && facing <= 3 ? facing : 0; }

// The absolute action of relative action k under a heading in 0 .. 3; an action outside 0 .. 3 passes through.
ATR_EGO_HD long long abs_of(int heading, long long k)
{
    return k < 0 || k > 3 ? k : (long long)((kAbsBits >> (2 * (4 * heading + (int)k))) & 3u);
}

// The relative action of absolute action a under a heading in 0 .. 3; an action outside 0 .. 3 passes through.
ATR_EGO_HD long long rel_of(int heading, long long a)
{
    return a < 0 || a > 3 ? a : (long long)((kRelBits >> (2 * (4 * heading + (int)a))) & 3u);
}

// The cell of the absolute window that cell `cell` (r * 13 + c) of the egocentric window shows, heading in 0 .. 3.
ATR_EGO_HD int src_cell(int heading, int cell)
{
    const int er = cell / kSide - kCentre, ec = cell % kSide - kCentre;
    const int ur = heading == 0 ? -1 : heading == 1 ? 1 : 0, uc = heading == 2 ? -1 : heading == 3 ? 1 : 0;
    const int dr = -er * ur + ec * uc, dc = -er * uc - ec * ur;
    return (kCentre + dr) * kSide + kCentre + dc;
}

} // namespace atr_ego
