// pairwise_geom.cpp — the geometry part of imagestitch_amd/csrc/pairwise.hpp on its own (plain C++, no HIP), for tests/test_pairwise_geom.py.
// Reads cases "x1 y1 w1 h1 x2 y2 w2 h2" from standard input, one per line; prints per case "empty", or the roi (x y w h) followed by the
// padded grid (rw rh hp wp oy1 ox1 oy2 ox2).
#define ISX_PAIRWISE_GEOMETRY_ONLY
#include "../../imagestitch_amd/csrc/pairwise.hpp"

#include <cstdio>

int main() {
    int tl1[2], tl2[2], w1, h1, w2, h2;
    while (std::scanf("%d %d %d %d %d %d %d %d", &tl1[0], &tl1[1], &w1, &h1, &tl2[0], &tl2[1], &w2, &h2) == 8) {
        int r[4];
        isx::PairGrid g;
        const bool roi = isx::overlap_roi(tl1, w1, h1, tl2, w2, h2, r), grid = isx::pair_grid(tl1, w1, h1, tl2, w2, h2, g);
        if (roi != grid) return 1;
        if (!roi) { std::puts("empty"); continue; }
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", r[0], r[1], r[2], r[3], g.rw, g.rh, g.hp, g.wp, g.oy1, g.ox1, g.oy2, g.ox2);
    }
    return 0;
}
