// blocks_gain_host.cpp — the host arithmetic of BlocksGainCompensator (imagestitch_amd/csrc/blocks_gain_host.hpp) as a stand-alone program,
// built by tests/test_blocks_gain_model.py with the host compiler under AddressSanitizer and UBSan and compared with the NumPy model.
// One command per line of stdin, one line of stdout each (floats as C99 hex):
//   grid cols rows blw blh                                   -> nx ny bw bh, then every block's x y w h
//   pairs xi yi colsi rowsi xj yj colsj rowsj blw blh        -> count, then bi bj xi yi xj yj w h per pair (image j's blocks follow i's)
//   smooth ny nx v...                                        -> the map smoothed twice
//   tables src_w src_h dst_w dst_h                           -> sx a1 per column, then sy0 sy1 fy per row
#define ISX_PAIRWISE_GEOMETRY_ONLY
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../../imagestitch_amd/csrc/blocks_gain_host.hpp"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "grid") {
            int cols, rows, blw, blh;
            in >> cols >> rows >> blw >> blh;
            const isx::BlockGrid g = isx::block_grid(cols, rows, blw, blh, 0);
            printf("%d %d %d %d", g.nx, g.ny, g.bw, g.bh);
            for (int by = 0; by < g.ny; ++by)
                for (int bx = 0; bx < g.nx; ++bx) {
                    const isx::BlockRect r = isx::block_rect(g, bx, by);
                    printf(" %d %d %d %d", r.x, r.y, r.w, r.h);
                }
            printf("\n");
        } else if (cmd == "pairs") {
            int ci[2], cj[2], wi, hi, wj, hj, blw, blh;
            in >> ci[0] >> ci[1] >> wi >> hi >> cj[0] >> cj[1] >> wj >> hj >> blw >> blh;
            const isx::BlockGrid gi = isx::block_grid(wi, hi, blw, blh, 0);
            const isx::BlockGrid gj = isx::block_grid(wj, hj, blw, blh, gi.nx * gi.ny);
            std::vector<isx::BlockPair> out;
            isx::block_pairs(ci, gi, cj, gj, [&](const isx::BlockPair& p) { out.push_back(p); });
            printf("%zu", out.size());
            for (const isx::BlockPair& p : out) printf(" %d %d %d %d %d %d %d %d", p.bi, p.bj, p.xi, p.yi, p.xj, p.yj, p.w, p.h);
            printf("\n");
        } else if (cmd == "smooth") {
            int ny, nx;
            in >> ny >> nx;
            std::vector<float> m((size_t)ny * nx);
            for (float& v : m) { std::string t; in >> t; v = strtof(t.c_str(), nullptr); }
            isx::smooth_gain_map(m, ny, nx);
            for (size_t k = 0; k < m.size(); ++k) printf("%s%a", k ? " " : "", (double)m[k]);
            printf("\n");
        } else if (cmd == "tables") {
            int sw, sh, dw, dh;
            in >> sw >> sh >> dw >> dh;
            std::vector<isx::ColTap> c;
            std::vector<isx::RowTap> r;
            isx::resize_tables(sw, sh, dw, dh, c, r);
            for (const isx::ColTap& t : c) printf("%d %a ", t.sx, (double)t.a1);
            for (const isx::RowTap& t : r) printf("%d %d %a ", t.sy0, t.sy1, (double)t.fy);
            printf("\n");
        } else if (!cmd.empty()) {
            return 2;
        }
    }
    return 0;
}
