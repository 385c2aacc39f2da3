// memory_host.cpp — stand-alone host program over csrc/atr_memory_rule.h (tests/test_memory_cpu.py compiles it with
// -fsanitize=address,undefined and runs it as a child process; it is never loaded into Python).
//
//   memory_host place SIDE   prints, for every pc in 0 .. SIDE - 1 and every 13-bit mask 0 .. 8191 (pc outermost), the line
//                            "W0 W1 W2": the three words of place_row(mask, pc, SIDE); place_word and place_row must agree
//   memory_host slice        prints, for a fixed list of 169-bit masks and every window row, "slice M0 M1 M2 WR BITS" (M2 holds
//                            bits 128 .. 168)
//   memory_host verdict      prints "verdict HIDDEN INSIDE SEEN WALL WV FV RESULT" for every combination of the four flags and two
//                            pairs of values (RESULT -1: the cell stays as it is)
//   memory_host clears       prints "clears MODE DONE RESULT" for every mode and done flag (none "x", 0, 1, 255)
//   memory_host pos          prints "pos WORD P R C" for a fixed list of position words and both players
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "atr_memory_rule.h"

namespace mem = atr_memory;

static int place(int side)
{
    if (side < 1 || side > 96) return 3;
    for (int pc = 0; pc < side; pc++)
        for (uint32_t mask = 0; mask <= mem::kRowMask; mask++) {
            uint32_t w[3];
            mem::place_row(mask, pc, side, w);
            for (int k = 0; k < 3; k++)
                if (w[k] != mem::place_word(mask | 0xFFFFE000u, pc, side, k)) return 4;     // (bits above the 13 are not looked at)
            std::printf("%u %u %u\n", w[0], w[1], w[2]);
        }
    return 0;
}

static int slice()
{
    const uint64_t all = ~0ull, top = (1ull << 41) - 1;
    const uint64_t masks[][3] = {
        {0, 0, 0}, {all, all, top}, {0x1FFFull, 0, 0}, {1ull << 63, 1, 0}, {0, 1ull << 63, 1}, {0, 0, 1ull << 40},
        {0x0123456789ABCDEFull, 0xFEDCBA9876543210ull, 0x155AA55AA55ull & top}, {0xAAAAAAAAAAAAAAAAull, 0x5555555555555555ull, 0x0F0F0F0F0Full},
        {0x8000000000001FFFull, 0x8000000000000001ull, 1ull << 40 | 1ull},
    };
    for (const auto &m : masks)
        for (int wr = 0; wr < mem::kSide; wr++) {
            const uint32_t s = mem::row_slice(m[0], m[1], m[2], wr);
            if (s > mem::kRowMask) return 5;
            std::printf("slice %llu %llu %llu %d %u\n", (unsigned long long)m[0], (unsigned long long)m[1], (unsigned long long)m[2], wr, s);
        }
    return 0;
}

static int verdict()
{
    const int values[][2] = {{mem::kWall, mem::kFree}, {200, 0}};
    for (const auto &v : values)
        for (int f = 0; f < 16; f++) {
            const bool hidden = f & 1, inside = f & 2, seen = f & 4, wall = f & 8;
            std::printf("verdict %d %d %d %d %d %d %d\n", hidden, inside, seen, wall, v[0], v[1],
                        mem::paint_verdict(hidden, inside, seen, wall, v[0], v[1]));
        }
    return 0;
}

static int clears()
{
    for (int mode = mem::kKeep; mode <= mem::kBegin; mode++)
        for (int d = -1; d <= 2; d++) {                     // -1: no done flag given; 2 stands for 255
            const int done = d == 2 ? 255 : d;
            char ds[8] = "x";
            if (d >= 0) std::snprintf(ds, sizeof ds, "%d", done);
            std::printf("clears %d %s %d\n", mode, ds, (int)mem::clears(mode, d >= 0, d >= 0 ? done : 0));
        }
    return 0;
}

static int pos()
{
    const uint32_t words[] = {0u, 0x04030201u, 0x51505150u, 0xfffefdfcu, 0x00510000u};
    for (uint32_t w : words)
        for (int p = 0; p < 2; p++) std::printf("pos %u %d %d %d\n", w, p, mem::row_of(w, p), mem::col_of(w, p));
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && std::strcmp(argv[1], "place") == 0) return place(std::atoi(argv[2]));
    if (argc == 2 && std::strcmp(argv[1], "slice") == 0) return slice();
    if (argc == 2 && std::strcmp(argv[1], "verdict") == 0) return verdict();
    if (argc == 2 && std::strcmp(argv[1], "clears") == 0) return clears();
    if (argc == 2 && std::strcmp(argv[1], "pos") == 0) return pos();
    std::fprintf(stderr, "usage: memory_host place SIDE | slice | verdict | clears | pos\n");
    return 2;
}
