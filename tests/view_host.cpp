// view_host.cpp — stand-alone host program over csrc/atr_view_rule.h (tests/test_view_cpu.py compiles it with
// -fsanitize=address,undefined and runs it as a child process; it is never loaded into Python).
//
//   view_host codes     "known V CODE" for the integers -2 .. 300 and "knownf X CODE" for a list of floats (X printed with %a; a NaN
//                       and the infinities among them); then "truth BIT TRACKER TARGET T" for all eight cases; then
//                       "code INSIDE T W CODE" for every (band, T, w): inside 0 / 1, T in 0 1 2 4, w = known(v) of v in 0 .. 15
//   view_host colours   "rgb CODE RRGGBB" (the macro form r | g << 8 | b << 16, hex) for every code 0 .. 255
//   view_host unturn    "unturn TURNED H CELL DST" for turned 0 / 1, the four headings and all 169 cells; the program itself holds
//                       DST against atr_ego::src_cell (exit code 3 on a difference) and checks that each map is a bijection (4)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "atr_view_rule.h"

namespace vw = atr_view;

static_assert(vw::known(3) == vw::kUnknown && vw::known(8) == 8 && vw::known(0.5f) == vw::kUnknown && vw::known(7.0f) == 7 &&
              vw::map_code(4, false, 0) == 36 && vw::map_code(1, true, 5) == 17 && vw::map_code(1, true, 6) == 6 &&
              vw::code_rgb(255) == vw::kRgbBackground && vw::unturn_cell(true, 0, 17) == 17,
              "the rule is constexpr");

static int codes()
{
    for (int v = -2; v <= 300; v++) std::printf("known %d %d\n", v, vw::known(v));
    const float fl[] = {0.0f, -0.0f, 1.0f, 2.0f, 3.0f, 4.0f, 5.0f, 6.0f, 7.0f, 8.0f, 9.0f, 0.5f, 1.0000001f, 4.9999995f, -1.0f, 255.0f,
                        1e-45f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                        -std::numeric_limits<float>::infinity()};
    for (float x : fl) std::printf("knownf %a %d\n", (double)x, vw::known(x));
    for (int bit = 0; bit < 2; bit++)
        for (int a = 0; a < 2; a++)
            for (int b = 0; b < 2; b++) std::printf("truth %d %d %d %d\n", bit, a, b, vw::truth(bit, a != 0, b != 0));
    const int ts[4] = {0, 1, 2, 4};
    for (int inside = 0; inside < 2; inside++)
        for (int t : ts)
            for (int v = 0; v < 16; v++) std::printf("code %d %d %d %d\n", inside, t, vw::known(v), vw::map_code(t, inside != 0, vw::known(v)));
    return 0;
}

static int colours()
{
    for (int c = 0; c < 256; c++) std::printf("rgb %d %06x\n", c, vw::code_rgb(c));
    return 0;
}

static int unturn()
{
    for (int turned = 0; turned < 2; turned++)
        for (int h = 0; h < 4; h++) {
            bool hit[vw::kWindow];
            std::memset(hit, 0, sizeof hit);
            for (int cell = 0; cell < vw::kWindow; cell++) {
                const int dst = vw::unturn_cell(turned != 0, h, cell);
                if (dst != (turned ? atr_ego::src_cell(h, cell) : cell)) return 3;
                if (dst < 0 || dst >= vw::kWindow || hit[dst]) return 4;
                hit[dst] = true;
                std::printf("unturn %d %d %d %d\n", turned, h, cell, dst);
            }
        }
    // in_window / window_index over the offsets a map cell can have
    for (int dr = -81; dr <= 81; dr++)
        for (int dc = -81; dc <= 81; dc++) {
            const bool in = vw::in_window(dr, dc);
            if (in != (std::abs(dr) <= 6 && std::abs(dc) <= 6)) return 5;
            if (in && (vw::window_index(dr, dc) < 0 || vw::window_index(dr, dc) >= vw::kWindow)) return 6;
        }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && std::strcmp(argv[1], "codes") == 0) return codes();
    if (argc == 2 && std::strcmp(argv[1], "colours") == 0) return colours();
    if (argc == 2 && std::strcmp(argv[1], "unturn") == 0) return unturn();
    std::fprintf(stderr, "usage: view_host codes | colours | unturn\n");
    return 2;
}
