// atr_footprint_rule.h — the recording rule and the paint predicate of include/atr_footprints.h, plain C++17 with no HIP
// dependence: the kernel (footprints_hip.hip k_footprints) and the host test program (tests/footprints_host.cpp) both use it.
//
// A cell is r | c << 8 (16 bits), kEmpty holds none. A trail row is [standing cell, print 1 (newest), ..., print K].
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ATR_FOOTPRINT_HD __host__ __device__ inline
#else
#define ATR_FOOTPRINT_HD inline
#endif

namespace atr_footprint {

constexpr int kSide = 13, kCentre = 6, kWindow = kSide * kSide;
constexpr int kEmpty = 0xFFFF, kMaxK = 63, kValue = 6;
constexpr int kPeek = 0, kStep = 1, kBegin = 2;                  // ATR_FOOTPRINT_PEEK / STEP / BEGIN
constexpr int kKeep = 0, kShift = 1, kRestart = 2;               // what a recording call does to a row

// The cell of player p (0 tracker, 1 target) in a handle's position word r0 | c0 << 8 | r1 << 16 | c1 << 24.
ATR_FOOTPRINT_HD int cell_of(unsigned pos, int p) { return (int)((pos >> (p ? 16 : 0)) & 0xFFFFu); }

// What a call of this mode does to the row whose entry 0 is s0, for a player now standing on `cur`.
ATR_FOOTPRINT_HD int record_kind(int mode, bool has_done, int done, int cur, int s0)
{
    if (mode == kPeek) return kKeep;
    if (mode == kBegin || (has_done && done != 0)) return kRestart;
    return cur != s0 ? kShift : kKeep;
}

// Entry j of the row after the call: `own` is entry j before it, `prev` entry j - 1 before it (not looked at for j = 0).
ATR_FOOTPRINT_HD int record_entry(int kind, int j, int cur, int own, int prev)
{
    if (kind == kKeep) return own;
    if (j == 0) return cur;
    return kind == kRestart ? kEmpty : prev;
}

// The window cell (0 .. 168) at which a viewer standing on `viewer` sees the print `print`, -1 where it sees none.
ATR_FOOTPRINT_HD int paint_cell(int print, int viewer)
{
    if (print == kEmpty) return -1;
    const int dr = (print & 255) - (viewer & 255), dc = ((print >> 8) & 255) - ((viewer >> 8) & 255);
    const int ar = dr < 0 ? -dr : dr, ac = dc < 0 ? -dc : dc;
    if ((ar > ac ? ar : ac) > kCentre) return -1;
    return (kCentre + dr) * kSide + kCentre + dc;
}

} // namespace atr_footprint
