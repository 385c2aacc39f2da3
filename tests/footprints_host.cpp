// footprints_host.cpp — stand-alone host program over csrc/atr_footprint_rule.h (tests/test_footprints_cpu.py compiles it with
// -fsanitize=address,undefined and runs it as a child process; it is never loaded into Python).
//
//   footprints_host record   prints, for every mode (0 .. 2), done flag (none, 0, 1, 255), current cell and row of a fixed list
//                            (K = 3), the line "rec MODE DONE CUR S0 S1 S2 S3 N0 N1 N2 N3": the row before and after the call,
//                            with "x" for a done flag that is not given
//   footprints_host paint    prints, for every viewer cell of a fixed list and every print at an offset of -8 .. 8 rows and
//                            columns that is a cell of the map, and for the EMPTY entry, the line "cell PRINT VIEWER CELL"
//                            (CELL -1: not seen)
//   footprints_host pos      prints "pos WORD P CELL" for a fixed list of position words and both players
#include <cstdio>
#include <cstring>

#include "atr_footprint_rule.h"

namespace fp = atr_footprint;

constexpr int kK = 3;
static const int kRows[][kK + 1] = {
    {0x0503, 0x0403, 0x0303, 0x0203}, {fp::kEmpty, fp::kEmpty, fp::kEmpty, fp::kEmpty}, {0x0503, fp::kEmpty, fp::kEmpty, fp::kEmpty},
    {0x0503, 0x0403, 0x0503, 0x0403}, {fp::kEmpty, 0x0101, 0x0101, fp::kEmpty},         {0x5150, 0x0000, 0x5150, 0x5051},
};
static const int kCurs[] = {0x0503, 0x0603, 0x0000, 0x5150};

static int record()
{
    for (int mode = fp::kPeek; mode <= fp::kBegin; mode++)
        for (int d = -1; d <= 2; d++)                       // -1: no done flag given; 2 stands for 255
            for (int cur : kCurs)
                for (const auto &row : kRows) {
                    const int done = d == 2 ? 255 : d;
                    int now[kK + 1];
                    const int kind = fp::record_kind(mode, d >= 0, d >= 0 ? done : 0, cur, row[0]);
                    for (int j = 0; j <= kK; j++) now[j] = fp::record_entry(kind, j, cur, row[j], j ? row[j - 1] : row[0]);
                    char ds[8] = "x";
                    if (d >= 0) std::snprintf(ds, sizeof ds, "%d", done);
                    std::printf("rec %d %s %d %d %d %d %d %d %d %d %d\n", mode, ds, cur, row[0], row[1], row[2], row[3], now[0], now[1],
                                now[2], now[3]);
                }
    return 0;
}

static const int kViewers[][2] = {{0, 0}, {5, 3}, {40, 41}, {80, 81}, {81, 0}, {7, 6}};

static int paint()
{
    for (const auto &v : kViewers) {
        const int viewer = v[0] | v[1] << 8;
        std::printf("cell %d %d %d\n", fp::kEmpty, viewer, fp::paint_cell(fp::kEmpty, viewer));
        for (int dr = -8; dr <= 8; dr++)
            for (int dc = -8; dc <= 8; dc++) {
                const int r = v[0] + dr, c = v[1] + dc;
                if (r < 0 || c < 0 || r > 255 || c > 255) continue;
                const int print = r | c << 8;
                const int cell = fp::paint_cell(print, viewer);
                if (cell < -1 || cell >= fp::kWindow) return 3;
                std::printf("cell %d %d %d\n", print, viewer, cell);
            }
    }
    return 0;
}

static int pos()
{
    const unsigned words[] = {0u, 0x04030201u, 0x51505150u, 0xfffefdfcu, 0x00510000u};
    for (unsigned w : words)
        for (int p = 0; p < 2; p++) std::printf("pos %u %d %d\n", w, p, fp::cell_of(w, p));
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && std::strcmp(argv[1], "record") == 0) return record();
    if (argc == 2 && std::strcmp(argv[1], "paint") == 0) return paint();
    if (argc == 2 && std::strcmp(argv[1], "pos") == 0) return pos();
    std::fprintf(stderr, "usage: footprints_host record | paint | pos\n");
    return 2;
}
