// noise_host.cpp — stand-alone host program over csrc/atr_noise_rule.h (tests/test_noise_cpu.py compiles it with
// -fsanitize=address,undefined and runs it as a child process; it is never loaded into Python).
//
//   noise_host kat        prints "kat X0 X1 X2 X3" (hex) for the three Random123 known-answer vectors of Philox4x32-10, through
//                         the header's host rounds
//   noise_host verdicts   for every case of a fixed list prints "case KEY ENV CLOCK P FLICKER MISS GHOST", then "in V0 .. V168"
//                         (the window as it reads, made here from a fixed table) and "out V0 .. V168" (every cell after the
//                         call: the verdict's value, or what it read where the verdict keeps it), and "draw MISS GHOST G" (the
//                         two window verdicts and the ghost's cell)
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "atr_noise_rule.h"

namespace nz = atr_noise;

static int kat()
{
    const uint32_t vec[3][6] = {{0u, 0u, 0u, 0u, 0u, 0u},
                                {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                                {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
    for (const auto &v : vec) {
        uint32_t c[4] = {v[0], v[1], v[2], v[3]};
        nz::philox(v[4], v[5], c);
        std::printf("kat %08x %08x %08x %08x\n", c[0], c[1], c[2], c[3]);
    }
    return 0;
}

static const int kTable[16] = {0, 0, 0, 1, 0, 1, 1, 4, 2, 5, 6, 0, 7, 8, 255, 0};
static const unsigned long long kKeys[] = {0ull, 0x6E6F6973655F7633ull, 0xFFFFFFFFFFFFFFFFull, 0x123456789ull};
static const uint32_t kEnvs[] = {0u, 7u, 1000u, 0xFFFFFFFFu};
static const uint32_t kClocks[] = {0u, 1u, 2u, 0xFFFFFFFFu};
static const int kThresholds[][3] = {{0, 0, 0},
                                     {nz::kOne, 0, 0},
                                     {0, nz::kOne, 0},
                                     {0, 0, nz::kOne},
                                     {0, nz::kOne, nz::kOne},
                                     {nz::kOne, nz::kOne, nz::kOne},
                                     {838861, 1677722, 8388608},
                                     {8388608, 8388608, 8388608},
                                     {1, nz::kOne - 1, nz::kOne - 1}};

static int class_of(int v, int p) { return v == 0 ? nz::kZero : v == 1 ? nz::kWall : v == nz::other_value(p) ? nz::kOther : nz::kElse; }

static int verdicts()
{
    int c = 0;
    for (const auto &t : kThresholds)
        for (int k = 0; k < 4; k++)
            for (int p = 0; p < 2; p++, c++) {
                const unsigned long long key = kKeys[(k + c) & 3];
                const uint32_t env = kEnvs[k], clock = kClocks[(k + (c >> 1)) & 3];
                int win[nz::kWindow], out[nz::kWindow];
                for (int i = 0; i < nz::kWindow; i++) win[i] = kTable[(i * 5 + c * 3 + ((i * i) >> 3)) & 15];
                win[nz::kCentre] = (c % 3 == 0) ? 0 : p ? 4 : 2;        // (a centre that reads 0 must stay as well)
                uint32_t b0[4];
                nz::draw_block(key, env, clock, p, 0u, b0);
                const bool miss_hit = nz::passes(b0[0], t[1]), ghost_hit = nz::passes(b0[1], t[2]);
                const int g = nz::ghost_cell(b0[2]);
                if (g < 0 || g >= nz::kWindow) return 3;
                for (int i = 0; i < nz::kWindow; i++) {
                    uint32_t bl[4];
                    nz::draw_block(key, env, clock, p, nz::flicker_block(i), bl);
                    const int v = nz::verdict(i, class_of(win[i], p), p, bl[nz::flicker_word(i)], t[0], miss_hit, ghost_hit, g);
                    out[i] = v == nz::kKeep ? win[i] : v;
                }
                std::printf("case %llu %u %u %d %d %d %d\nin", key, env, clock, p, t[0], t[1], t[2]);
                for (int i = 0; i < nz::kWindow; i++) std::printf(" %d", win[i]);
                std::printf("\nout");
                for (int i = 0; i < nz::kWindow; i++) std::printf(" %d", out[i]);
                std::printf("\ndraw %d %d %d\n", (int)miss_hit, (int)ghost_hit, g);
            }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && std::strcmp(argv[1], "kat") == 0) return kat();
    if (argc == 2 && std::strcmp(argv[1], "verdicts") == 0) return verdicts();
    std::fprintf(stderr, "usage: noise_host kat | verdicts\n");
    return 2;
}
