// atr_memory_rule.h — the arithmetic of include/atr_memory.h, plain C++17 with no HIP dependence: the kernel (memory_hip.hip
// k_memory) and the host test program (tests/memory_host.cpp) both use it.
//
// A seen tile has the layout of a map tile: row r is words 3r .. 3r + 2, column c is bit c & 31 of word c >> 5. A window row's
// visible cells are a 13-bit mask, bit wc for window column wc.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ATR_MEMORY_HD __host__ __device__ inline
#else
#define ATR_MEMORY_HD inline
#endif

namespace atr_memory {

constexpr int kSide = 13, kCentre = 6, kWindow = kSide * kSide;
constexpr int kTileWords = 256, kRowWords = 3, kMaxSide = 82;
constexpr int kHidden = 5, kWall = 7, kFree = 8;
constexpr int kKeep = 0, kStep = 1, kBegin = 2;                  // ATR_MEMORY_KEEP / STEP / BEGIN
constexpr int kLeave = -1;                                       // paint_verdict: the window cell stays as it is
constexpr uint32_t kRowMask = (1u << kSide) - 1u;

// (r, c) of player p (0 tracker, 1 target) in a handle's position word r0 | c0 << 8 | r1 << 16 | c1 << 24.
ATR_MEMORY_HD int row_of(uint32_t pos, int p) { return (int)((pos >> (p ? 16 : 0)) & 255u); }
ATR_MEMORY_HD int col_of(uint32_t pos, int p) { return (int)((pos >> (p ? 24 : 8)) & 255u); }

// Does a call of this mode empty the tiles of an env whose done flag is `done` (has_done: a done array was given)?
ATR_MEMORY_HD bool clears(int mode, bool has_done, int done) { return mode == kBegin || (mode == kStep && has_done && done != 0); }

// The 13-bit slice of window row wr out of the 169-bit mask m0 | m1 << 64 | m2 << 128 (bit 13 wr + wc is window cell (wr, wc)).
ATR_MEMORY_HD uint32_t row_slice(uint64_t m0, uint64_t m1, uint64_t m2, int wr)
{
    const int b = kSide * wr, q = b >> 6, s = b & 63;
    const uint64_t lo = q == 0 ? m0 : q == 1 ? m1 : m2;
    const uint64_t hi = q == 0 ? m1 : q == 1 ? m2 : 0ull;
    const uint64_t v = s == 0 ? lo : (lo >> s) | (hi << (64 - s));
    return (uint32_t)v & kRowMask;
}

// Word k (0 .. 2) of the 96-bit map row that holds the 13-bit window-row mask `slice` of a player in column pc: window column wc
// lands on map column pc - 6 + wc; what falls left of column 0 or on a column >= side is dropped. 0 <= pc < side <= 96.
ATR_MEMORY_HD uint32_t place_word(uint32_t slice, int pc, int side, int k)
{
    slice &= kRowMask;
    const int s = pc - kCentre;                                  // the map column of window column 0
    if (s < 0) slice >>= -s;                                     // (the cells left of the map)
    const int at = (s < 0 ? 0 : s) - 32 * k;                     // where the mask's bit 0 sits relative to this word's bit 0
    uint32_t w = 0u;
    if (at >= 0 && at < 32) w = slice << at;
    else if (at < 0 && at > -kSide) w = slice >> -at;
    const int valid = side - 32 * k;                             // columns of this word inside the square
    const uint32_t keep = valid >= 32 ? 0xFFFFFFFFu : valid <= 0 ? 0u : (1u << valid) - 1u;
    return w & keep;
}

// The three words of that row.
ATR_MEMORY_HD void place_row(uint32_t slice, int pc, int side, uint32_t out[3])
{
    for (int k = 0; k < kRowWords; k++) out[k] = place_word(slice, pc, side, k);
}

// What the paint does to a window cell: kLeave, or the value it is written as. is_hidden: the cell equals `hidden`; inside: its
// map cell lies in the side x side square; seen / wall: that cell's bit of the player's seen tile (after the recording) and of the
// env's map tile.
ATR_MEMORY_HD int paint_verdict(bool is_hidden, bool inside, bool seen, bool wall, int wall_value, int free_value)
{
    if (!is_hidden || !inside || !seen) return kLeave;
    return wall ? wall_value : free_value;
}

} // namespace atr_memory
