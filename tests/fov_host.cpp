// fov_host.cpp — stand-alone host program over csrc/atr_fov_rule.h (tests/test_fov_cpu.py compiles it with
// -fsanitize=address,undefined and runs it as a child process; it is never loaded into Python).
//
//   fov_host table     prints, for every facing (0 .. 3, 255), aperture (90, 180, 270, 360) and near (0 .. 6), the line
//                      "vis FACING APERTURE NEAR" and the 13 rows of the window as 1 (visible) / 0 (hidden) characters
//   fov_host turn      prints, for every facing (0 .. 3, 255), action (none, -1 .. 8) and done (none, 0, 1), the line
//                      "turn FACING ACTION DONE NEW", with "x" for an action / a done flag that is not given
#include <cstdio>
#include <cstring>

#include "atr_fov_rule.h"

static const int kFacings[5] = {0, 1, 2, 3, atr_fov::kNone};
static const int kApertures[4] = {90, 180, 270, 360};

static int table()
{
    for (int facing : kFacings)
        for (int aperture : kApertures) {
            if (!atr_fov::aperture_ok(aperture)) return 2;
            for (int near = 0; near <= atr_fov::kMaxNear; near++) {
                std::printf("vis %d %d %d\n", facing, aperture, near);
                for (int r = 0; r < atr_fov::kSide; r++) {
                    char line[atr_fov::kSide + 1];
                    for (int c = 0; c < atr_fov::kSide; c++) line[c] = atr_fov::visible(facing, aperture, near, r, c) ? '1' : '0';
                    line[atr_fov::kSide] = 0;
                    std::puts(line);
                }
            }
        }
    return 0;
}

static int turns()
{
    for (int facing : kFacings)
        for (int action = -2; action <= 8; action++)          // -2: no action given
            for (int done = -1; done <= 1; done++) {          // -1: no done flag given
                const int nf = atr_fov::turn(facing, done >= 0, done >= 0 ? done : 0, action >= -1, action >= -1 ? action : 0);
                char a[8] = "x", d[8] = "x";
                if (action >= -1) std::snprintf(a, sizeof a, "%d", action);
                if (done >= 0) std::snprintf(d, sizeof d, "%d", done);
                std::printf("turn %d %s %s %d\n", facing, a, d, nf);
            }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && std::strcmp(argv[1], "table") == 0) return table();
    if (argc == 2 && std::strcmp(argv[1], "turn") == 0) return turns();
    std::fprintf(stderr, "usage: fov_host table | fov_host turn\n");
    return 2;
}
