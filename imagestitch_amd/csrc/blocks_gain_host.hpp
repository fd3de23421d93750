// blocks_gain_host.hpp — the host arithmetic of BlocksGainCompensator (blocks_gain.hip) in plain C++, so that it also builds into a
// stand-alone program under the host compiler's sanitizers (tests/cpp/blocks_gain_host.cpp): the block grid of an image, the overlapping
// block pairs of two images by interval intersection, the smoothing of a gain map and the tables of cv::resize(INTER_LINEAR) on CV_32F (their taps: resize_taps.hpp).
// Restated from OpenCV 3.4.2 (stitching/src/exposure_compensate.cpp, imgproc/src/resize.cpp; neither is in the reference tree).
// Compile with -ffp-contract=off: every float expression below is a rounded multiply, then a rounded add.  Internal, not part of the ABI.
#pragma once
#include <cmath>
#include <vector>

#include "pairwise.hpp"
#include "resize_taps.hpp"

namespace isx {

// ---- the block grid of one image -----------------------------------------------------------------------------------------------------------
// nx = ceil(cols / bl_width) blocks of bw = ceil(cols / nx) columns (the last one narrower), the same in y; never an empty block:
// bw <= bl_width, so (nx - 1) bw <= (nx - 1) bl_width < cols.  `first` numbers the image's blocks among all, by outer, bx inner.
struct BlockGrid { int cols, rows, nx, ny, bw, bh, first; };
inline BlockGrid block_grid(int cols, int rows, int bl_width, int bl_height, int first) {
    BlockGrid g{cols, rows, 0, 0, 1, 1, first};
    if (cols > 0) { g.nx = (cols + bl_width - 1) / bl_width; g.bw = (cols + g.nx - 1) / g.nx; }
    if (rows > 0) { g.ny = (rows + bl_height - 1) / bl_height; g.bh = (rows + g.ny - 1) / g.ny; }
    if (g.nx == 0 || g.ny == 0) g.nx = g.ny = 0;
    return g;
}
struct BlockRect { int x, y, w, h; };          // inside the image
inline BlockRect block_rect(const BlockGrid& g, int bx, int by) {
    const int x = bx * g.bw, y = by * g.bh;
    return BlockRect{x, y, std::min(x + g.bw, g.cols) - x, std::min(y + g.bh, g.rows) - y};
}

// ---- the overlapping block pairs of two images ---------------------------------------------------------------------------------------------
// Every (block of image i, block of image j) whose rectangles meet, with the meeting rectangle as offsets into either image: the blocks of
// i that reach into overlapRoi(i, j), and for each the blocks of j its part of the roi falls on - index ranges by division, no loop over
// all pairs.  Emitted by block of i ascending, then block of j ascending.  In 64 bits: corner + size may pass INT_MAX.
struct BlockPair { int bi, bj, xi, yi, xj, yj, w, h; };   // global block numbers; the overlap's top-left in image i and in image j; its size
template <class Emit>
void block_pairs(const int ci[2], const BlockGrid& gi, const int cj[2], const BlockGrid& gj, Emit&& emit) {
    int roi[4];
    if (gi.nx == 0 || gj.nx == 0 || !overlap_roi(ci, gi.cols, gi.rows, cj, gj.cols, gj.rows, roi)) return;
    // the roi in each image's coordinates (inside the image, so they fit an int)
    const int rxi = (int)((long long)roi[0] - ci[0]), ryi = (int)((long long)roi[1] - ci[1]);
    const int rxj = (int)((long long)roi[0] - cj[0]), ryj = (int)((long long)roi[1] - cj[1]);
    const int rw = roi[2], rh = roi[3];
    for (int byi = ryi / gi.bh; byi <= (ryi + rh - 1) / gi.bh; ++byi)
        for (int bxi = rxi / gi.bw; bxi <= (rxi + rw - 1) / gi.bw; ++bxi) {
            const BlockRect a = block_rect(gi, bxi, byi);
            // block a cut to the roi, in image i's coordinates: [x0, x1) x [y0, y1), never empty
            const int x0 = std::max(a.x, rxi), x1 = std::min(a.x + a.w, rxi + rw);
            const int y0 = std::max(a.y, ryi), y1 = std::min(a.y + a.h, ryi + rh);
            const int dx = rxj - rxi, dy = ryj - ryi;      // image i's coordinates to image j's
            for (int byj = (y0 + dy) / gj.bh; byj <= (y1 - 1 + dy) / gj.bh; ++byj)
                for (int bxj = (x0 + dx) / gj.bw; bxj <= (x1 - 1 + dx) / gj.bw; ++bxj) {
                    const BlockRect c = block_rect(gj, bxj, byj);
                    const int u0 = std::max(x0 + dx, c.x), u1 = std::min(x1 + dx, c.x + c.w);
                    const int v0 = std::max(y0 + dy, c.y), v1 = std::min(y1 + dy, c.y + c.h);
                    if (u0 >= u1 || v0 >= v1) continue;    // (cannot happen: the ranges above are exact)
                    emit(BlockPair{gi.first + byi * gi.nx + bxi, gj.first + byj * gj.nx + bxj, u0 - dx, v0 - dy, u0, v0, u1 - u0, v1 - v0});
                }
        }
}

// ---- the gain map's smoothing ---------------------------------------------------------------------------------------------------------------
// sepFilter2D(map, map, CV_32F, ker, ker) with ker = [0.25, 0.5, 0.25], BORDER_REFLECT_101, TWICE: the row pass x[0] * 0.5 + (x[-1] + x[1])
// * 0.25 into a temporary, then the column pass of the same form.  A dimension of length 1 maps every index to 0.
inline int reflect101_host(int p, int n) {
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}
inline void smooth_gain_map(std::vector<float>& m, int ny, int nx) {
    std::vector<float> t((size_t)ny * nx);
    for (int pass = 0; pass < 2; ++pass) {
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const float* r = &m[(size_t)y * nx];
                const float side = r[reflect101_host(x - 1, nx)] + r[reflect101_host(x + 1, nx)];
                t[(size_t)y * nx + x] = r[x] * 0.5f + side * 0.25f;
            }
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const float side = t[(size_t)reflect101_host(y - 1, ny) * nx + x] + t[(size_t)reflect101_host(y + 1, ny) * nx + x];
                m[(size_t)y * nx + x] = t[(size_t)y * nx + x] * 0.5f + side * 0.25f;
            }
    }
}

// ---- cv::resize(map, image.size(), 0, 0, INTER_LINEAR) on CV_32F: the tables -------------------------------------------------------------------
// The taps are resize_taps.hpp's (col_tap, row_tap: what isx_resize computes per pixel): h = S[sx] (1 - fx) + S[sx + 1] fx where sx + 1 < src_w,
// else S[sx]; g = h_sy0 (1 - fy) + h_sy1 fy.
inline void resize_tables(int src_w, int src_h, int dst_w, int dst_h, std::vector<ColTap>& cols, std::vector<RowTap>& rows) {
    const double scale_x = resize_scale(src_w, dst_w), scale_y = resize_scale(src_h, dst_h);
    cols.resize((size_t)dst_w);
    rows.resize((size_t)dst_h);
    for (int dx = 0; dx < dst_w; ++dx) cols[(size_t)dx] = col_tap(dx, scale_x, src_w);
    for (int dy = 0; dy < dst_h; ++dy) rows[(size_t)dy] = row_tap(dy, scale_y, src_h);
}

}  // namespace isx
