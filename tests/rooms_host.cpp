// rooms_host.cpp — stand-alone host program over csrc/t2d_rooms_rule.h (tests/test_rooms_cpu.py compiles it with
// -fsanitize=address,undefined and runs it as a child process; it is never loaded into Python).
//
//   rooms_host philox K0 K1 C0 C1 C2 C3              prints the four output words of its own Philox4x32-10
//   rooms_host map SEED GENV EPISODE LEVEL [...]     prints, per tuple, "map SEED GENV EPISODE LEVEL m regions deepest" and the
//                                                    82 rows of the map as 0 / 1 characters
// Regions are taken depth first from a fixed stack; every array index is checked before it is used.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "t2d_rooms_rule.h"

static void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c[4])
{
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

static const int kSide = 82, kStack = 64;
static uint8_t g[kSide][kSide];

static int fail(const char *what)
{
    std::fprintf(stderr, "rooms_host: %s\n", what);
    return 2;
}
static bool interior(int v) { return v >= 1 && v <= 80; }

static int one_map(uint64_t seed, uint32_t genv, uint32_t episode, int level)
{
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t p[4] = {t2d_rooms::kParamWord, episode, genv, 3u};
    philox4x32_10(k0, k1, p);
    const int m = t2d_rooms::min_side(level, p[0]);
    std::memset(g, 0, sizeof(g));
    uint32_t stack[kStack];
    int top = 0, regions = 0, deepest = 1;
    stack[top++] = t2d_rooms::region_word(t2d_rooms::kRoot0, t2d_rooms::kRoot0, t2d_rooms::kRoot1, t2d_rooms::kRoot1);
    while (top > 0) {
        const uint32_t reg = stack[--top];
        if (++regions > t2d_rooms::kMaxRegions) return fail("more than kMaxRegions regions");
        uint32_t x[4] = {reg, episode, genv, 3u};
        philox4x32_10(k0, k1, x);
        const t2d_rooms::Split s = t2d_rooms::split(reg, m, x[0], x[1], x[2], x[3]);
        if (s.final_) continue;
        if (!interior(s.t) || !interior(s.b0) || !interior(s.b1) || s.b0 > s.b1) return fail("wall outside the interior");
        if (s.door1 < s.b0 || s.door1 > s.b1 || s.door2 < s.b0 || s.door2 > s.b1) return fail("door outside the wall");
        for (int b = s.b0; b <= s.b1; b++) (s.horizontal ? g[s.t][b] : g[b][s.t]) = 1;
        (s.horizontal ? g[s.t][s.door1] : g[s.door1][s.t]) = 0;
        (s.horizontal ? g[s.t][s.door2] : g[s.door2][s.t]) = 0;
        if (top + 2 > kStack) return fail("stack full");
        stack[top++] = s.child0;
        stack[top++] = s.child1;
        if (top > deepest) deepest = top;
    }
    for (int i = 0; i < kSide; i++) g[0][i] = g[kSide - 1][i] = g[i][0] = g[i][kSide - 1] = 1;
    std::printf("map %llu %u %u %d %d %d %d\n", (unsigned long long)seed, genv, episode, level, m, regions, deepest);
    for (int r = 0; r < kSide; r++) {
        char line[kSide + 1];
        for (int c = 0; c < kSide; c++) line[c] = g[r][c] ? '1' : '0';
        line[kSide] = 0;
        std::puts(line);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 8 && std::strcmp(argv[1], "philox") == 0) {
        uint32_t c[4];
        for (int i = 0; i < 4; i++) c[i] = (uint32_t)std::strtoul(argv[4 + i], nullptr, 0);
        philox4x32_10((uint32_t)std::strtoul(argv[2], nullptr, 0), (uint32_t)std::strtoul(argv[3], nullptr, 0), c);
        std::printf("%u %u %u %u\n", c[0], c[1], c[2], c[3]);
        return 0;
    }
    if (argc >= 6 && (argc - 2) % 4 == 0 && std::strcmp(argv[1], "map") == 0) {
        for (int i = 2; i < argc; i += 4) {
            const int rc = one_map(std::strtoull(argv[i], nullptr, 0), (uint32_t)std::strtoul(argv[i + 1], nullptr, 0),
                                   (uint32_t)std::strtoul(argv[i + 2], nullptr, 0), std::atoi(argv[i + 3]));
            if (rc != 0) return rc;
        }
        return 0;
    }
    return fail("usage: rooms_host philox K0 K1 C0 C1 C2 C3 | rooms_host map SEED GENV EPISODE LEVEL [...]");
}
