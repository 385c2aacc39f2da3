// atr_noise_rule.h — the arithmetic of include/atr_noise.h, once for host and device: the draw blocks, the threshold test, the
// ghost's cell and the verdict on one cell. Plain C++17 with no HIP dependence where a host compiler reads it: the kernel
// (noise_hip.hip k_noise) and the host test program (tests/noise_host.cpp) both use it. Under hipcc the device side takes its
// Philox from atr_sample.h; the host side restates the ten rounds here.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include "atr_sample.h"
#define ATR_NOISE_HD __host__ __device__ inline
#else
#define ATR_NOISE_HD inline
#endif

namespace atr_noise {

constexpr int kWindow = 169, kCentre = 84, kOne = 1 << 24;
constexpr int kPeek = 0, kAdvance = 1;                           // ATR_NOISE_PEEK / ADVANCE
constexpr uint32_t kTag = 0x4E5E0000u;                           // ATR_NOISE_TAG
constexpr int kZero = 0, kWall = 1, kOther = 2, kElse = 3;       // what a cell reads: 0, 1, the other player's value, anything else
constexpr int kKeep = -1;                                        // a verdict that leaves the cell as it is (it is not stored)

// Philox4x32-10 (Salmon et al., SC'11): counter c[0 .. 3] in, the four output words out.
ATR_NOISE_HD void philox(uint32_t k0, uint32_t k1, uint32_t (&c)[4])
{
#if defined(__HIP_DEVICE_COMPILE__)
    atr::philox4x32_10(k0, k1, c[0], c[1], c[2], c[3]);
#else
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0, c[1] = (uint32_t)p1, c[2] = n2, c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
#endif
}

// Block `block` of window (global env id, player p) at clock value `clock`, under the 64-bit key.
ATR_NOISE_HD void draw_block(unsigned long long key, uint32_t env, uint32_t clock, int p, uint32_t block, uint32_t (&w)[4])
{
    w[0] = env, w[1] = clock, w[2] = (uint32_t)p, w[3] = kTag ^ block;
    philox((uint32_t)key, (uint32_t)(key >> 32), w);
}

// The value the other player has in window p (0 the tracker's, 1 the target's).
ATR_NOISE_HD int other_value(int p) { return p ? 2 : 4; }

// Does the event with draw word w and threshold t (0 .. kOne) happen?
ATR_NOISE_HD bool passes(uint32_t w, int t) { return (w >> 8) < (uint32_t)t; }

// The ghost's cell of block 0's word 2: 0 .. 168.
ATR_NOISE_HD int ghost_cell(uint32_t w2) { return (int)(((uint64_t)w2 * (uint64_t)kWindow) >> 32); }

// The flicker word of cell i lives in block 1 + (i & 63), word i >> 6.
ATR_NOISE_HD uint32_t flicker_block(int i) { return 1u + (uint32_t)(i & 63); }
ATR_NOISE_HD int flicker_word(int i) { return i >> 6; }

// The value cell i of window p is written as, kKeep where it stays: `reads` is what it read before any store of the call (kZero,
// kWall, kOther, kElse), fw its flicker word, miss_hit / ghost_hit the window's two verdicts of block 0, g the ghost's cell.
ATR_NOISE_HD int verdict(int i, int reads, int p, uint32_t fw, int flicker, bool miss_hit, bool ghost_hit, int g)
{
    if (i == kCentre) return kKeep;
    if (ghost_hit && i == g && reads == kZero) return other_value(p);        // (the ghost wins over a flicker)
    if ((reads == kZero || reads == kWall) && passes(fw, flicker)) return 1 - reads;
    if (reads == kOther && miss_hit) return 0;
    return kKeep;
}

} // namespace atr_noise
