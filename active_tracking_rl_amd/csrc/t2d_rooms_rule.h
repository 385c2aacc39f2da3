// t2d_rooms_rule.h — the per-region arithmetic of the Rooms map generator (T2D_MAP_ROOMS, include/track2d.h), plain C++17 with no
// HIP dependence: the generator kernel (t2d_device.h gen_rooms) and the host test program (tests/rooms_host.cpp) both use it.
//
// The map is 82 x 82 with a wall border; a region is a rectangle (r0, c0, r1, c1) of interior cells, bounds inclusive, the root
// is (1, 1, 80, 80). A region's four random words X, Y, Z, W are one Philox4x32-10 block whose counter word 0 is the packed
// region itself (region_word), so the regions of one map are independent of the order they are processed in. One step either
// declares the region final (a room) or lays one wall line across it, on an EVEN row / column, pierced by one or two doors at
// ODD positions, and hands back the two rectangles on either side. Walls on even lines and doors on odd positions mean a later
// perpendicular wall never ends on a door, and the cells on either side of a door are (odd, odd) cells, which no wall covers:
// every region stays 4-connected.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define T2D_ROOMS_HD __host__ __device__ inline
#else
#define T2D_ROOMS_HD inline
#endif

namespace t2d_rooms {

constexpr int kRoot0 = 1, kRoot1 = 80;        // interior rows / columns of the 82 x 82 map
constexpr int kMaxRegions = 337;              // <= 13 x 13 rooms of side >= 5: at most 169 leaves, 168 splits
constexpr uint32_t kParamWord = 0xffffffffu;  // counter word 0 of the per-episode parameter block (level 0: m)

T2D_ROOMS_HD uint32_t region_word(int r0, int c0, int r1, int c1)
{
    return (uint32_t)r0 | ((uint32_t)c0 << 7) | ((uint32_t)r1 << 14) | ((uint32_t)c1 << 21);
}
// (word * n) >> 32: uniform over [0, n) without a rejection loop
T2D_ROOMS_HD uint32_t pick(uint32_t word, uint32_t n) { return (uint32_t)(((uint64_t)word * (uint64_t)n) >> 32); }

// smallest room side: 3 + 2 level, or one of 5, 7, 9, 11 from the parameter block's first word at level 0
T2D_ROOMS_HD int min_side(int level, uint32_t px) { return level >= 1 ? 3 + 2 * level : 5 + 2 * (int)pick(px, 4u); }

struct Split {
    int final_;             // 1: the region is a room, nothing else is set
    int horizontal;         // 1: the wall is row t, spanning columns b0 .. b1; 0: column t, spanning rows b0 .. b1
    int t, b0, b1;
    int door1, door2;       // positions along b0 .. b1 (door2 == door1 where the wall is shorter than 32 cells)
    uint32_t child0, child1; // region words of the rectangles before / after line t
};

T2D_ROOMS_HD Split split(uint32_t region, int m, uint32_t X, uint32_t Y, uint32_t Z, uint32_t W)
{
    const int r0 = (int)(region & 127u), c0 = (int)((region >> 7) & 127u);
    const int r1 = (int)((region >> 14) & 127u), c1 = (int)((region >> 21) & 127u);
    const int h = r1 - r0 + 1, w = c1 - c0 + 1;
    Split s;
    s.final_ = 1; s.horizontal = 0; s.t = 0; s.b0 = 0; s.b1 = 0; s.door1 = 0; s.door2 = 0; s.child0 = 0u; s.child1 = 0u;
    if (h <= 4 * m && w <= 4 * m && ((X >> 8) & 7u) == 0u) return s;      // about one small region in eight stays a hall
    const bool hor = h > w || (h == w && (X & 1u) == 0u);
    const int a0 = hor ? r0 : c0, a1 = hor ? r1 : c1;
    const int b0 = hor ? c0 : r0, b1 = hor ? c1 : r1;
    const int lo = (a0 + m + 1) & ~1, hi = (a1 - m) & ~1;                 // the even t in [a0 + m, a1 - m]
    if (lo > hi) return s;                                                // (the other orientation is not tried)
    const int t = lo + 2 * (int)pick(Y, (uint32_t)((hi - lo) / 2 + 1));
    const int d0 = b0 | 1;                                                // the odd d in [b0, b1]; b0 is odd by construction
    const uint32_t nd = (uint32_t)((b1 - d0) / 2 + 1);
    s.final_ = 0; s.horizontal = hor ? 1 : 0; s.t = t; s.b0 = b0; s.b1 = b1;
    s.door1 = d0 + 2 * (int)pick(Z, nd);
    s.door2 = (b1 - b0 + 1) >= 32 ? d0 + 2 * (int)pick(W, nd) : s.door1;
    s.child0 = hor ? region_word(r0, c0, t - 1, c1) : region_word(r0, c0, r1, t - 1);
    s.child1 = hor ? region_word(t + 1, c0, r1, c1) : region_word(r0, t + 1, r1, c1);
    return s;
}

} // namespace t2d_rooms
