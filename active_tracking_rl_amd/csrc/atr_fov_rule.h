// atr_fov_rule.h — the field-of-view predicate and the turn rule of include/atr_fov.h, plain C++17 with no HIP dependence: the
// kernel (fov_hip.hip k_fov) and the host test program (tests/fov_host.cpp) both use it.
//
// A facing is one byte: 0 .. 3 are the VonNeumann moves 0 = (-1, 0), 1 = (+1, 0), 2 = (0, -1), 3 = (0, +1) as (ur, uc), kNone
// looks all round. For the window cell (r, c), offset (dr, dc) = (r - 6, c - 6): f = dr * ur + dc * uc is how far ahead it lies,
// l = |dr * uc - dc * ur| how far to the side, and it is in the cone of aperture 90 / 180 / 270 iff f >= s * l with s = 1 / 0 / -1.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ATR_FOV_HD __host__ __device__ inline
#else
#define ATR_FOV_HD inline
#endif

namespace atr_fov {

constexpr int kSide = 13, kCentre = 6, kMaxNear = 6;
constexpr int kNone = 255;                   // ATR_FOV_NONE

ATR_FOV_HD bool aperture_ok(int aperture) { return aperture == 90 || aperture == 180 || aperture == 270 || aperture == 360; }

// Is cell (r, c) of a window visible to a player of this facing, aperture (one of aperture_ok) and near radius?
ATR_FOV_HD bool visible(int facing, int aperture, int near, int r, int c)
{
    if (facing < 0 || facing > 3 || aperture == 360) return true;            // kNone (and what is no facing): all round
    const int dr = r - kCentre, dc = c - kCentre;
    const int ar = dr < 0 ? -dr : dr, ac = dc < 0 ? -dc : dc;
    if ((ar > ac ? ar : ac) <= near) return true;
    const int ur = facing == 0 ? -1 : facing == 1 ? 1 : 0, uc = facing == 2 ? -1 : facing == 3 ? 1 : 0;
    const int f = dr * ur + dc * uc, x = dr * uc - dc * ur, l = x < 0 ? -x : x;
    const int s = aperture == 90 ? 1 : aperture == 180 ? 0 : -1;
    return f >= s * l;
}

// The facing after a step: NONE where the episode turned over, else the action where one in 0 .. 3 is given, else what it was.
ATR_FOV_HD int turn(int facing, bool has_done, int done, bool has_action, long long action)
{
    if (has_done && done != 0) return kNone;
    if (has_action && action >= 0 && action <= 3) return (int)action;
    return facing;
}

} // namespace atr_fov
