// ego_host.cpp — stand-alone host program over csrc/atr_ego_rule.h (tests/test_ego_cpu.py compiles it with
// -fsanitize=address,undefined and runs it as a child process; it is never loaded into Python).
//
//   ego_host tables    prints, for every facing byte (0 .. 3, 255, 7) and action (-1 .. 8), the line
//                      "act FACING ACTION ABS REL": the absolute action of that relative action and the relative action of
//                      that absolute action under the byte's heading
//   ego_host cells     prints, for every facing byte and cell (0 .. 168), the line "cell FACING CELL SOURCE": the cell of the
//                      absolute window that the egocentric window shows there; every source is also written into a 169-element
//                      array at its own index, so that an index outside the window is an error the sanitizer reports
#include <cstdio>
#include <cstring>

#include "atr_ego_rule.h"

static const int kFacings[6] = {0, 1, 2, 3, 255, 7};

static int tables()
{
    for (int facing : kFacings)
        for (long long k = -1; k <= 8; k++) {
            const int h = atr_ego::heading_of(facing);
            std::printf("act %d %lld %lld %lld\n", facing, k, atr_ego::abs_of(h, k), atr_ego::rel_of(h, k));
        }
    return 0;
}

static int cells()
{
    for (int facing : kFacings) {
        int hits[atr_ego::kWindow];
        std::memset(hits, 0, sizeof hits);
        for (int cell = 0; cell < atr_ego::kWindow; cell++) {
            const int s = atr_ego::src_cell(atr_ego::heading_of(facing), cell);
            hits[s]++;
            std::printf("cell %d %d %d\n", facing, cell, s);
        }
        for (int cell = 0; cell < atr_ego::kWindow; cell++)
            if (hits[cell] != 1) return 3;                   // (every heading's map is a permutation of the window)
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && std::strcmp(argv[1], "tables") == 0) return tables();
    if (argc == 2 && std::strcmp(argv[1], "cells") == 0) return cells();
    std::fprintf(stderr, "usage: ego_host tables | ego_host cells\n");
    return 2;
}
