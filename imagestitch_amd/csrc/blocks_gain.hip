// blocks_gain.hip — BlocksGainCompensator (OpenCV 3.4.2 stitching/src/exposure_compensate.cpp), what
// ExposureCompensator::createDefault(ExposureCompensator::GAIN_BLOCKS) returns, on gfx950:
//   isx_blocks_gain_create / _destroy                                                             W:238-239
//   isx_blocks_gain_feed      compensator->feed(corners, images_warped, masks_warped)             W:238-240, S:1165-1167, B:117-119
//   isx_blocks_gain_apply     compensator->apply(i, corners[i], images_warped[i], masks_warped[i]) W:241-244
//   isx_selftest_lu_solve     the dense solver alone
//
// feed, restated from OpenCV 3.4.2 (the source is not in the reference tree; DESIGN.md §8 "BlocksGainCompensator"):
//   every image is cut into a grid of blocks (blocks_gain_host.hpp), GainCompensator::feed runs on all blocks as if each were an image
//   (gain.hip's header states it), and the gains become one CV_32F map per image, smoothed twice with [0.25, 0.5, 0.25].
// Blocks of one image never overlap, so the N and I of GainCompensator are sparse: one record per pair of blocks of DIFFERENT images whose
// rectangles meet, found from the two grids by interval intersection, plus the diagonal N.  The pixel part is gain.hip's one launch over a
// table of work items, with its exact sums (I stays math.fsum of the terms).  The contributions to A and b are computed from the records
// on the host in OpenCV's loop order (for i, for j ascending), the dense A is zeroed and scattered into ON THE DEVICE, and solved there:
//
// hal::LU, as lu_solve (gain.hip) states it, one column at a time: k_lu_pivot (one workgroup) finds the first row of largest |value| at
// or below the diagonal (strict >), fails below 100 DBL_EPSILON, and leaves d = -1 / pivot; k_lu_update (the whole grid) gives every row
// j below   A[j][c] += (A[j][i] d) A[i][c]   for c > i, and the same to b, which rides as column n of the matrix.  A row permutation
// stands in for the swaps (it only moves values).  Column i is read by the update and never written by it; the pivot row is read only.
// No FMA (-ffp-contract=off): every entry goes through the operations of hal::LU in its order, so the upper triangle has OpenCV's bits.
// A singular flag turns every later launch into a no-op; the host reads it once, with the solution.  Back substitution is one workgroup
// walking the rows upwards with a dot product each (its additions are a tree, not OpenCV's order).  The matrix is freed when feed returns.
//
// apply: cv::resize(gain_map, image.size(), 0, 0, INTER_LINEAR) on CV_32F fused with the float multiply and the saturating store: a lane
// owns four pixels of four rows; it holds the horizontally interpolated taps of the two map rows a row needs and recomputes them only
// when the map rows change (every bl_height rows or so), so a pixel costs its 3 bytes in and 3 out.  A map of the image's size is used
// as it is.  Twelve bytes per lane go as one load and one store at whatever alignment the rows have; a row's last, partial group byte
// by byte.
#include "isx_device.hpp"
#include "pairwise.hpp"
#include "scratch.hpp"
#include "gain_stats.hpp"
#include "blocks_gain_host.hpp"

#include <chrono>
#include <cmath>
#include <memory>

using namespace isx;
using namespace isxd;

namespace {

constexpr int BG_MAX_BLOCKS = 16384;       // a 2 GiB matrix
constexpr double LU_EPS = 2.220446049250313e-16 * 100;

// ---- the solver ----------------------------------------------------------------------------------------------------------------------------
struct LuState {
    int singular;      // a pivot below LU_EPS: every later launch returns at once
    int swaps;         // row exchanges so far
    double d;          // -1 / pivot of the current column
};

constexpr int LU_PNT = 1024;               // k_lu_pivot, k_lu_backsub: one workgroup
constexpr int LU_NT = 256, LU_RB = 8;      // k_lu_update: 256 columns x 8 rows per workgroup

__global__ __launch_bounds__(256) void k_lu_init(int* perm, int n, LuState* s) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < n) perm[r] = r;
    if (r == 0) { s->singular = 0; s->swaps = 0; s->d = 0.0; }
}

// the dense system from its sparse form: the diagonal, b (column n) and the off-diagonal entries into a zeroed matrix
struct OffDiag { int r, c; double v; };
__global__ __launch_bounds__(256) void k_bg_scatter(double* __restrict__ A, size_t lda, int n, const double* __restrict__ diag, const double* __restrict__ b,
                                                    const OffDiag* __restrict__ off, int noff) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n) { A[(size_t)t * lda + t] = diag[t]; A[(size_t)t * lda + n] = b[t]; }
    if (t < noff) A[(size_t)off[t].r * lda + off[t].c] = off[t].v;
}

// larger |value| wins, the smaller row among equals: the first row of the largest |value|
__device__ __forceinline__ void pick(double& v, int& k, double ov, int ok) {
    if (ov > v || (ov == v && ok < k)) { v = ov; k = ok; }
}

__global__ __launch_bounds__(LU_PNT) void k_lu_pivot(const double* __restrict__ A, size_t lda, int n, int i, int* perm, LuState* s) {
    if (s->singular) return;
    double v = -1.0;
    int k = INT_MAX;
    for (int r = i + (int)threadIdx.x; r < n; r += LU_PNT) pick(v, k, fabs(A[(size_t)perm[r] * lda + i]), r);
    for (int o = 32; o > 0; o >>= 1) pick(v, k, __shfl_xor(v, o), __shfl_xor(k, o));
    __shared__ double sv[LU_PNT / WAVE];
    __shared__ int sk[LU_PNT / WAVE];
    if ((threadIdx.x & (WAVE - 1)) == 0) { sv[threadIdx.x / WAVE] = v; sk[threadIdx.x / WAVE] = k; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < LU_PNT / WAVE; ++w) pick(v, k, sv[w], sk[w]);
        if (v < LU_EPS) { s->singular = 1; return; }
        const int pi = perm[i], pk = perm[k];
        if (k != i) { perm[i] = pk; perm[k] = pi; s->swaps += 1; }
        s->d = -1.0 / A[(size_t)pk * lda + i];
    }
}

__global__ __launch_bounds__(LU_NT) void k_lu_update(double* A, size_t lda, int n, int i, const int* __restrict__ perm, const LuState* __restrict__ s) {
    if (s->singular) return;
    const int c = i + 1 + (int)blockIdx.x * LU_NT + (int)threadIdx.x;      // up to n: column n is b
    if (c > n) return;
    const int r0 = i + 1 + (int)blockIdx.y * LU_RB;
    const double d = s->d;
    const double pv = A[(size_t)perm[i] * lda + c];
#pragma unroll
    for (int k = 0; k < LU_RB; ++k) {
        const int r = r0 + k;
        if (r >= n) break;
        double* row = A + (size_t)perm[r] * lda;
        const double alpha = row[i] * d;
        row[c] += alpha * pv;
    }
}

__global__ __launch_bounds__(LU_PNT) void k_lu_backsub(const double* __restrict__ A, size_t lda, int n, const int* __restrict__ perm, const LuState* __restrict__ s, double* x) {
    if (s->singular) return;
    __shared__ double part[LU_PNT / WAVE];
    for (int i = n - 1; i >= 0; --i) {
        const double* row = A + (size_t)perm[i] * lda;
        double acc = 0.0;
        for (int c = i + 1 + (int)threadIdx.x; c < n; c += LU_PNT) acc += row[c] * x[c];
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int w = 0; w < LU_PNT / WAVE; ++w) t += part[w];
            x[i] = (row[n] - t) / row[i];
        }
        __syncthreads();       // x[i] is visible to the workgroup, part[] is free again
    }
}

// everything the solve keeps on the device beside the matrix
struct LuAux {
    DevBuf buf;
    int* perm = nullptr;
    LuState* state = nullptr;
    double* x = nullptr;
    int reserve(int n) {
        const size_t xb = round256((size_t)n * sizeof(double)), pb = round256((size_t)n * sizeof(int));
        ISX_TRY(buf.reserve(xb + pb + 256));
        x = (double*)buf.p; perm = (int*)((char*)buf.p + xb); state = (LuState*)((char*)buf.p + xb + pb);
        return ISX_OK;
    }
};

// the elimination of the n x (n + 1) system at dA (row pitch lda doubles): 2 n launches, nothing read back
int lu_factor_device(double* dA, size_t lda, int n, LuAux& aux, hipStream_t st) {
    ISX_LAUNCH("lu_init", 0.0, st, k_lu_init, dim3(cdiv(n, 256)), dim3(256), 0, aux.perm, n, aux.state);
    for (int i = 0; i < n; ++i) {
        ISX_LAUNCH("lu_pivot", 8.0 * (n - i), st, k_lu_pivot, dim3(1), dim3(LU_PNT), 0, (const double*)dA, lda, n, i, aux.perm, aux.state);
        if (i + 1 < n)
            ISX_LAUNCH("lu_update", 16.0 * (n - i) * (n - 1 - i), st, k_lu_update, dim3(cdiv(n - i, LU_NT), cdiv(n - 1 - i, LU_RB)), dim3(LU_NT), 0,
                       dA, lda, n, i, (const int*)aux.perm, (const LuState*)aux.state);
    }
    return ISX_OK;
}
int lu_backsub_device(const double* dA, size_t lda, int n, LuAux& aux, hipStream_t st) {
    ISX_LAUNCH("lu_backsub", 4.0 * n * n, st, k_lu_backsub, dim3(1), dim3(LU_PNT), 0, dA, lda, n, (const int*)aux.perm, (const LuState*)aux.state, aux.x);
    return ISX_OK;
}
// the solution and the state to the host: synchronises st
int lu_read_back(int n, LuAux& aux, hipStream_t st, std::vector<double>& x, LuState& state) {
    x.assign((size_t)n, 0.0);
    ISX_HIP(hipMemcpyAsync(&state, aux.state, sizeof(LuState), hipMemcpyDeviceToHost, st));
    ISX_HIP(hipMemcpyAsync(x.data(), aux.x, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    ISX_HIP(hipStreamSynchronize(st));
    return ISX_OK;
}

// ---- apply ---------------------------------------------------------------------------------------------------------------------------------
constexpr int BA_PX = 4;                   // pixels per lane and row
constexpr int BA_ROWS = 4;                 // rows per lane; a workgroup of 4 waves covers 256 pixels x 16 rows
typedef unsigned u32x3 __attribute__((ext_vector_type(3), aligned(1)));

// saturate_cast<uchar>(cvRound((float)p * g)): the product in float, ties to even, clamped
__device__ __forceinline__ unsigned bg_byte(unsigned p, float g) { return (unsigned)sat_u8(cvround_x86((float)p * g)); }

// one map row interpolated at a column: S[sx] (1 - fx) + S[sx + 1] fx, and S[sx] alone where no tap lies to the right
__device__ __forceinline__ float bg_htap(const float* __restrict__ row, ColTap t, int mw) {
    return t.sx + 1 < mw ? row[t.sx] * (1.f - t.a1) + row[t.sx + 1] * t.a1 : row[t.sx];
}

template <bool COPY>
__global__ __launch_bounds__(256) void k_blocks_gain_apply(unsigned char* img, size_t step, int rows, int cols, const float* __restrict__ map, int mw,
                                                           const ColTap* __restrict__ ct, const RowTap* __restrict__ rt) {
    const int x = ((int)blockIdx.x * WAVE + (int)(threadIdx.x & (WAVE - 1))) * BA_PX;
    const int y0 = ((int)blockIdx.y * 4 + (int)(threadIdx.x / WAVE)) * BA_ROWS;
    if (x >= cols || y0 >= rows) return;
    const int np = min(BA_PX, cols - x);           // pixels of this group inside the row
    const int nr = min(BA_ROWS, rows - y0);
    // all of the group's loads first
    u32x3 v[BA_ROWS];
#pragma unroll
    for (int r = 0; r < BA_ROWS; ++r) {
        v[r] = (u32x3){0u, 0u, 0u};
        if (r < nr) {
            const unsigned char* p = img + (size_t)(y0 + r) * step + 3 * (size_t)x;
            if (np == BA_PX) v[r] = *(const u32x3*)p;
            else for (int k = 0; k < 3 * np; ++k) v[r][k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
        }
    }
    ColTap t[BA_PX];
    if constexpr (!COPY) {
#pragma unroll
        for (int k = 0; k < BA_PX; ++k) t[k] = ct[min(x + k, cols - 1)];
    }
    int sy0 = -1, sy1 = -1;
    float h0[BA_PX], h1[BA_PX];
#pragma unroll
    for (int r = 0; r < BA_ROWS; ++r) {
        if (r >= nr) break;
        const int y = y0 + r;
        float g[BA_PX];
        if constexpr (COPY) {
#pragma unroll
            for (int k = 0; k < BA_PX; ++k) g[k] = map[(size_t)y * mw + min(x + k, cols - 1)];
        } else {
            const RowTap q = rt[y];
            if (q.sy0 != sy0) {                    // uniform over the wave: a row is a wave's
                sy0 = q.sy0;
#pragma unroll
                for (int k = 0; k < BA_PX; ++k) h0[k] = bg_htap(map + (size_t)sy0 * mw, t[k], mw);
            }
            if (q.sy1 != sy1) {
                sy1 = q.sy1;
#pragma unroll
                for (int k = 0; k < BA_PX; ++k) h1[k] = bg_htap(map + (size_t)sy1 * mw, t[k], mw);
            }
            const float b0 = 1.f - q.fy;
#pragma unroll
            for (int k = 0; k < BA_PX; ++k) g[k] = h0[k] * b0 + h1[k] * q.fy;
        }
        // byte j of the twelve belongs to pixel j / 3
        u32x3 o;
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            unsigned d = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) d |= bg_byte((v[r][w] >> (8 * e)) & 255u, g[(4 * w + e) / 3]) << (8 * e);
            o[w] = d;
        }
        unsigned char* p = img + (size_t)y * step + 3 * (size_t)x;
        if (np == BA_PX) *(u32x3*)p = o;
        else for (int k = 0; k < 3 * np; ++k) p[k] = (unsigned char)((o[k >> 2] >> (8 * (k & 3))) & 255u);
    }
}

// the tables of one (map size, image size), on the device
struct ResizeTables {
    int mw, mh, w, h;
    DevBuf buf;
    const ColTap* cols = nullptr;
    const RowTap* rows = nullptr;
};

}  // namespace

struct isx_blocks_gain {
    int device = 0, bl_w = 32, bl_h = 32;
    bool fed = false;
    std::vector<BlockGrid> grids;              // of the images fed
    std::vector<double> gains;                 // one per block
    std::vector<std::vector<float>> maps;      // smoothed, ny x nx per image
    std::vector<size_t> map_off;               // of each map in maps_dev, in floats
    DevBuf maps_dev;
    std::vector<isx_block_pair> recs;          // the off-diagonal statistics
    std::vector<long long> diag_n;
    std::vector<std::unique_ptr<ResizeTables>> tables;   // never dropped: a captured apply may point at them
    double ms[4] = {0, 0, 0, 0};               // of the last feed: statistics, assembly, LU, back substitution
    MatStages stages;
};

namespace {

// the tables of (map mw x mh -> image w x h): cached, else built and uploaded (synchronises st; not on a capturing stream)
int tables_for(isx_blocks_gain* h, int mw, int mh, int w, int hh, hipStream_t st, const ResizeTables** out) {
    for (const auto& t : h->tables)
        if (t->mw == mw && t->mh == mh && t->w == w && t->h == hh) { *out = t.get(); return ISX_OK; }
    bool capturing = false;
    ISX_TRY(is_capturing(st, capturing));
    ISX_CHECK_ARG(!capturing, ISX_ERR_STATE,
                  "blocks_gain_apply: the stream is capturing and the tables of a %d x %d map for a %d x %d image are not built yet (apply once before the capture)", mw, mh, w, hh);
    std::vector<ColTap> c;
    std::vector<RowTap> r;
    resize_tables(mw, mh, w, hh, c, r);
    std::unique_ptr<ResizeTables> t(new ResizeTables());
    t->mw = mw; t->mh = mh; t->w = w; t->h = hh;
    const size_t cb = round256(c.size() * sizeof(ColTap));
    ISX_TRY(t->buf.reserve(cb + r.size() * sizeof(RowTap)));
    ISX_HIP(hipMemcpyAsync(t->buf.p, c.data(), c.size() * sizeof(ColTap), hipMemcpyHostToDevice, st));
    ISX_HIP(hipMemcpyAsync((char*)t->buf.p + cb, r.data(), r.size() * sizeof(RowTap), hipMemcpyHostToDevice, st));
    ISX_HIP(hipStreamSynchronize(st));         // c and r go out of scope
    t->cols = (const ColTap*)t->buf.p;
    t->rows = (const RowTap*)((char*)t->buf.p + cb);
    *out = t.get();
    h->tables.push_back(std::move(t));
    return ISX_OK;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

extern "C" {

int isx_blocks_gain_create(int bl_width, int bl_height, int device, isx_blocks_gain** out) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(out != nullptr, ISX_ERR_INVALID, "blocks_gain_create: null out");
    *out = nullptr;
    ISX_CHECK_ARG(bl_width >= 1 && bl_height >= 1, ISX_ERR_INVALID, "blocks_gain_create: blocks of %d x %d", bl_width, bl_height);
    ISX_CHECK_ARG(device >= 0, ISX_ERR_INVALID, "blocks_gain_create: device %d", device);
    isx_blocks_gain* h = new isx_blocks_gain();
    h->device = device; h->bl_w = bl_width; h->bl_h = bl_height;
    *out = h;
    return ISX_OK;
} ISX_EXIT("isx_blocks_gain_create")

int isx_blocks_gain_destroy(isx_blocks_gain* h) ISX_ENTRY {
    clear_error();
    if (!h) return ISX_OK;
    (void)hipSetDevice(h->device);
    delete h;
    return ISX_OK;
} ISX_EXIT("isx_blocks_gain_destroy")

int isx_blocks_gain_feed(isx_blocks_gain* h, int num_images, const int* corners_xy, const isx_mat* images, const isx_mat* masks, void* hip_stream) ISX_ENTRY {
    clear_error();
    const char* who = "blocks_gain_feed";
    ISX_CHECK_ARG(h != nullptr, ISX_ERR_INVALID, "%s: null handle", who);
    ISX_CHECK_ARG(num_images >= 1, ISX_ERR_INVALID, "%s: num_images = %d (at least one image)", who, num_images);
    ISX_CHECK_ARG(corners_xy && images && masks, ISX_ERR_INVALID, "%s: null argument", who);
    const int n = num_images;
    ISX_TRY(check_tiles(n, images, masks, false, who));
    std::vector<BlockGrid> grids((size_t)n);
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        grids[(size_t)i] = block_grid(images[i].cols, images[i].rows, h->bl_w, h->bl_h, (int)total);
        total += (long long)grids[(size_t)i].nx * grids[(size_t)i].ny;
        ISX_CHECK_ARG(total <= BG_MAX_BLOCKS, ISX_ERR_UNSUPPORTED, "%s: more than %d blocks (%d x %d blocks, image %d of %d x %d): the dense system would pass 2 GiB",
                      who, BG_MAX_BLOCKS, h->bl_w, h->bl_h, i, images[i].cols, images[i].rows);
    }
    const int B = (int)total;
    ISX_HIP(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    ISX_TRY(refuse_capture(st, who, "feed reads the statistics and the gains back to the host"));
    h->fed = false;
    auto t0 = std::chrono::steady_clock::now();

    // ---- statistics: the work table of every block (its own mask) and of every pair of blocks that meet
    h->stages.use_device(h->device);
    std::vector<isx_mat> simg((size_t)n), smsk((size_t)n);
    for (int i = 0; i < n; ++i) ISX_TRY(h->stages.stage((size_t)i, &masks[i], false, st, who, smsk[(size_t)i]));
    std::vector<BlockPair> bp;
    std::vector<char> need_img((size_t)n, 0);
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const size_t before = bp.size();
            block_pairs(corners_xy + 2 * i, grids[(size_t)i], corners_xy + 2 * j, grids[(size_t)j], [&](const BlockPair& p) { bp.push_back(p); });
            if (bp.size() != before) need_img[(size_t)i] = need_img[(size_t)j] = 1;
        }
    // the records go out by block_i, then block_j: the loop above gives that order within a pair of images, not across three images that
    // all meet (image 0's blocks against image 2's come after all of image 0's against image 1's)
    std::sort(bp.begin(), bp.end(), [](const BlockPair& a, const BlockPair& c) { return a.bi != c.bi ? a.bi < c.bi : a.bj < c.bj; });
    for (int i = 0; i < n; ++i)
        if (need_img[(size_t)i]) ISX_TRY(h->stages.stage((size_t)(n + i), &images[i], false, st, who, simg[(size_t)i]));
    // the image of a global block number
    std::vector<int> img_of((size_t)B);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < grids[(size_t)i].nx * grids[(size_t)i].ny; ++k) img_of[(size_t)(grids[(size_t)i].first + k)] = i;
    const auto px = [](const isx_mat& m) { return (const unsigned char*)m.data; };
    std::vector<GainItem> items;
    std::vector<int> first((size_t)B + bp.size() + 1);
    double bytes = 0.0;
    for (int i = 0; i < n; ++i) {
        const BlockGrid& g = grids[(size_t)i];
        for (int by = 0; by < g.ny; ++by)
            for (int bx = 0; bx < g.nx; ++bx) {
                const BlockRect r = block_rect(g, bx, by);
                first[(size_t)(g.first + by * g.nx + bx)] = (int)items.size();
                const int band = std::max(1, gain_item_size(true) / r.w);
                for (int y = 0; y < r.h; y += band) {
                    GainItem it{};
                    it.m0 = px(smsk[(size_t)i]) + (size_t)(r.y + y) * smsk[(size_t)i].step + r.x; it.sm0 = smsk[(size_t)i].step;
                    it.rows = std::min(band, r.h - y); it.cols = r.w; it.diag = 1;
                    items.push_back(it);
                }
                bytes += (double)r.w * r.h;
            }
    }
    for (size_t k = 0; k < bp.size(); ++k) {
        const BlockPair& p = bp[k];
        const int i = img_of[(size_t)p.bi], j = img_of[(size_t)p.bj];
        first[(size_t)B + k] = (int)items.size();
        const int band = std::max(1, gain_item_size(false) / p.w);
        for (int y = 0; y < p.h; y += band) {
            GainItem it{};
            it.m0 = px(smsk[(size_t)i]) + (size_t)(p.yi + y) * smsk[(size_t)i].step + p.xi; it.sm0 = smsk[(size_t)i].step;
            it.m1 = px(smsk[(size_t)j]) + (size_t)(p.yj + y) * smsk[(size_t)j].step + p.xj; it.sm1 = smsk[(size_t)j].step;
            it.p0 = px(simg[(size_t)i]) + (size_t)(p.yi + y) * simg[(size_t)i].step + 3 * (size_t)p.xi; it.sp0 = simg[(size_t)i].step;
            it.p1 = px(simg[(size_t)j]) + (size_t)(p.yj + y) * simg[(size_t)j].step + 3 * (size_t)p.xj; it.sp1 = simg[(size_t)j].step;
            it.rows = std::min(band, p.h - y); it.cols = p.w; it.diag = 0;
            items.push_back(it);
        }
        bytes += 8.0 * p.w * p.h;
    }
    first[(size_t)B + bp.size()] = (int)items.size();
    std::vector<GainPartial> part;
    ISX_TRY(gain_feed_items(items, bytes, h->device, st, part));
    std::vector<long long> diag_n((size_t)B);
    std::vector<isx_block_pair> recs(bp.size());
    for (size_t k = 0; k < (size_t)B + bp.size(); ++k) {
        unsigned long long cnt;
        unsigned __int128 s0, s1;
        gain_partial_total(part, first[k], first[k + 1] - first[k], cnt, s0, s1);
        const long long nn = std::max<long long>(1, (long long)cnt);
        if (k < (size_t)B) { diag_n[k] = nn; continue; }
        isx_block_pair& r = recs[k - (size_t)B];
        r.block_i = bp[k - (size_t)B].bi; r.block_j = bp[k - (size_t)B].bj; r.n = nn;
        r.i_ij = ((double)s0 * 0x1p-52) / (double)nn;       // one rounding (to nearest), an exact scaling, one division: gain.hip's
        r.i_ji = ((double)s1 * 0x1p-52) / (double)nn;
    }
    h->ms[0] = ms_since(t0);
    t0 = std::chrono::steady_clock::now();

    // ---- assembly: row i's terms in OpenCV's order, j ascending over the blocks that meet block i (i itself among them)
    struct Adj { int j; double n, iij, iji; };
    std::vector<int> deg((size_t)B + 1, 0);
    for (const isx_block_pair& r : recs) { ++deg[(size_t)r.block_i + 1]; ++deg[(size_t)r.block_j + 1]; }
    for (int i = 0; i < B; ++i) deg[(size_t)i + 1] += deg[(size_t)i] + 1;       // + the diagonal
    std::vector<Adj> adj((size_t)deg[(size_t)B]);
    std::vector<int> fill(deg.begin(), deg.end() - 1);
    for (int i = 0; i < B; ++i) adj[(size_t)fill[(size_t)i]++] = Adj{i, (double)diag_n[(size_t)i], 0.0, 0.0};
    for (const isx_block_pair& r : recs) {
        adj[(size_t)fill[(size_t)r.block_i]++] = Adj{r.block_j, (double)r.n, r.i_ij, r.i_ji};
        adj[(size_t)fill[(size_t)r.block_j]++] = Adj{r.block_i, (double)r.n, r.i_ji, r.i_ij};
    }
    const double alpha = 0.01, beta = 100;
    std::vector<double> diag((size_t)B, 0.0), bvec((size_t)B, 0.0);
    std::vector<OffDiag> off;
    off.reserve(2 * recs.size());
    for (int i = 0; i < B; ++i) {
        std::sort(adj.begin() + deg[(size_t)i], adj.begin() + deg[(size_t)i + 1], [](const Adj& a, const Adj& c) { return a.j < c.j; });
        for (int k = deg[(size_t)i]; k < deg[(size_t)i + 1]; ++k) {
            const Adj& a = adj[(size_t)k];
            bvec[(size_t)i] += beta * a.n;
            diag[(size_t)i] += beta * a.n;
            if (a.j == i) continue;
            diag[(size_t)i] += 2 * alpha * a.iij * a.iij * a.n;
            double v = 0.0;
            v -= 2 * alpha * a.iij * a.iji * a.n;
            off.push_back(OffDiag{i, a.j, v});
        }
    }
    const size_t lda = (size_t)B + 1;
    DevBuf mat, sys;                           // freed on return
    LuAux aux;
    ISX_TRY(mat.reserve((size_t)B * lda * sizeof(double)));
    ISX_TRY(aux.reserve(B));
    const size_t db = round256((size_t)B * sizeof(double));
    ISX_TRY(sys.reserve(2 * db + std::max<size_t>(off.size(), 1) * sizeof(OffDiag)));
    double* d_diag = (double*)sys.p;
    double* d_b = (double*)((char*)sys.p + db);
    OffDiag* d_off = (OffDiag*)((char*)sys.p + 2 * db);
    double* dA = (double*)mat.p;
    ISX_HIP(hipMemsetAsync(dA, 0, (size_t)B * lda * sizeof(double), st));
    ISX_HIP(hipMemcpyAsync(d_diag, diag.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
    ISX_HIP(hipMemcpyAsync(d_b, bvec.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
    if (!off.empty()) ISX_HIP(hipMemcpyAsync(d_off, off.data(), off.size() * sizeof(OffDiag), hipMemcpyHostToDevice, st));
    ISX_LAUNCH("blocks_gain_scatter", 16.0 * B + 16.0 * off.size(), st, k_bg_scatter, dim3(cdiv((int)std::max<size_t>((size_t)B, off.size()), 256)), dim3(256), 0,
               dA, lda, B, (const double*)d_diag, (const double*)d_b, (const OffDiag*)d_off, (int)off.size());
    ISX_HIP(hipStreamSynchronize(st));         // the host vectors are consumed; the stage times are those of the stages
    h->ms[1] = ms_since(t0);
    t0 = std::chrono::steady_clock::now();

    // ---- the solve
    ISX_TRY(lu_factor_device(dA, lda, B, aux, st));
    ISX_HIP(hipStreamSynchronize(st));
    h->ms[2] = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    ISX_TRY(lu_backsub_device(dA, lda, B, aux, st));
    std::vector<double> x;
    LuState state{};
    ISX_TRY(lu_read_back(B, aux, st, x, state));
    h->ms[3] = ms_since(t0);
    ISX_CHECK_ARG(!state.singular, ISX_ERR_INTERNAL, "%s: the system is singular", who);

    // ---- the maps: (float)gain per block, smoothed twice, on the host and on the device
    std::vector<std::vector<float>> maps((size_t)n);
    std::vector<size_t> map_off((size_t)n);
    std::vector<float> all((size_t)B);
    for (int i = 0; i < n; ++i) {
        const BlockGrid& g = grids[(size_t)i];
        std::vector<float>& m = maps[(size_t)i];
        m.resize((size_t)g.nx * g.ny);
        for (size_t k = 0; k < m.size(); ++k) m[k] = (float)x[(size_t)g.first + k];
        smooth_gain_map(m, g.ny, g.nx);
        map_off[(size_t)i] = (size_t)g.first;
        std::copy(m.begin(), m.end(), all.begin() + g.first);
    }
    ISX_TRY(h->maps_dev.reserve((size_t)B * sizeof(float)));
    ISX_HIP(hipMemcpyAsync(h->maps_dev.p, all.data(), (size_t)B * sizeof(float), hipMemcpyHostToDevice, st));
    ISX_HIP(hipStreamSynchronize(st));
    h->grids = grids; h->gains = x; h->maps.swap(maps); h->map_off = map_off; h->recs.swap(recs); h->diag_n.swap(diag_n);
    h->fed = true;
    // the tables of the sizes fed, so that an apply on them uploads nothing (and can be captured)
    for (int i = 0; i < n; ++i) {
        const BlockGrid& g = grids[(size_t)i];
        if (g.nx == g.cols && g.ny == g.rows) continue;
        const ResizeTables* t;
        ISX_TRY(tables_for(h, g.nx, g.ny, g.cols, g.rows, st, &t));
    }
    return ISX_OK;
} ISX_EXIT("isx_blocks_gain_feed")

int isx_blocks_gain_apply(isx_blocks_gain* h, int index, isx_mat* image, void* hip_stream) ISX_ENTRY {
    clear_error();
    const char* who = "blocks_gain_apply";
    ISX_CHECK_ARG(h != nullptr, ISX_ERR_INVALID, "%s: null handle", who);
    ISX_CHECK_ARG(h->fed, ISX_ERR_STATE, "%s: feed has not run", who);
    ISX_CHECK_ARG(index >= 0 && (size_t)index < h->grids.size(), ISX_ERR_INVALID, "%s: index %d of %zu images", who, index, h->grids.size());
    ISX_TRY(check_mat(image, who));
    ISX_CHECK_ARG(image->type == ISX_8UC3, ISX_ERR_TYPE, "%s: image must be CV_8UC3, got %s", who, type_name(image->type));
    ISX_HIP(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const BlockGrid& g = h->grids[(size_t)index];
    const float* map = (const float*)h->maps_dev.p + h->map_off[(size_t)index];
    const int rows = image->rows, cols = image->cols;
    const bool copy = g.nx == cols && g.ny == rows;
    const ResizeTables* t = nullptr;
    if (!copy) ISX_TRY(tables_for(h, g.nx, g.ny, cols, rows, st, &t));
    MatStage si;
    isx_mat view = *image;
    if (image->device < 0) {
        ISX_TRY(si.use_in(image, st, who));
        si.host = image;
        view = si.d;
    }
    const dim3 grid(cdiv(cdiv(cols, BA_PX), WAVE), cdiv(rows, 4 * BA_ROWS));
    const double bytes = 6.0 * rows * cols;
    if (copy) ISX_LAUNCH("blocks_gain_apply", bytes + 4.0 * rows * cols, st, (k_blocks_gain_apply<true>), grid, dim3(256), 0, (unsigned char*)view.data, view.step, rows, cols, map, g.nx,
                         (const ColTap*)nullptr, (const RowTap*)nullptr);
    else ISX_LAUNCH("blocks_gain_apply", bytes, st, (k_blocks_gain_apply<false>), grid, dim3(256), 0, (unsigned char*)view.data, view.step, rows, cols, map, g.nx, t->cols, t->rows);
    if (image->device < 0) ISX_TRY(si.finish_out(st));     // copies back and synchronises: the staging buffer is freed on return
    return ISX_OK;
} ISX_EXIT("isx_blocks_gain_apply")

int isx_blocks_gain_num_images(const isx_blocks_gain* h, int* num_images, int* num_blocks) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(h != nullptr, ISX_ERR_INVALID, "blocks_gain_num_images: null handle");
    ISX_CHECK_ARG(h->fed, ISX_ERR_STATE, "blocks_gain_num_images: feed has not run");
    if (num_images) *num_images = (int)h->grids.size();
    if (num_blocks) *num_blocks = (int)h->gains.size();
    return ISX_OK;
} ISX_EXIT("isx_blocks_gain_num_images")

int isx_blocks_gain_block_counts(const isx_blocks_gain* h, int* nx_ny) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(h != nullptr && nx_ny != nullptr, ISX_ERR_INVALID, "blocks_gain_block_counts: null argument");
    ISX_CHECK_ARG(h->fed, ISX_ERR_STATE, "blocks_gain_block_counts: feed has not run");
    for (size_t i = 0; i < h->grids.size(); ++i) { nx_ny[2 * i] = h->grids[i].nx; nx_ny[2 * i + 1] = h->grids[i].ny; }
    return ISX_OK;
} ISX_EXIT("isx_blocks_gain_block_counts")

int isx_blocks_gain_gains(const isx_blocks_gain* h, double* gains) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(h != nullptr && gains != nullptr, ISX_ERR_INVALID, "blocks_gain_gains: null argument");
    ISX_CHECK_ARG(h->fed, ISX_ERR_STATE, "blocks_gain_gains: feed has not run");
    std::copy(h->gains.begin(), h->gains.end(), gains);
    return ISX_OK;
} ISX_EXIT("isx_blocks_gain_gains")

int isx_blocks_gain_map(const isx_blocks_gain* h, int index, isx_mat* out, void* hip_stream) ISX_ENTRY {
    clear_error();
    const char* who = "blocks_gain_map";
    ISX_CHECK_ARG(h != nullptr, ISX_ERR_INVALID, "%s: null handle", who);
    ISX_CHECK_ARG(h->fed, ISX_ERR_STATE, "%s: feed has not run", who);
    ISX_CHECK_ARG(index >= 0 && (size_t)index < h->grids.size(), ISX_ERR_INVALID, "%s: index %d of %zu images", who, index, h->grids.size());
    ISX_TRY(check_mat(out, who));
    ISX_CHECK_ARG(out->type == ISX_32FC1, ISX_ERR_TYPE, "%s: out must be CV_32FC1, got %s", who, type_name(out->type));
    const BlockGrid& g = h->grids[(size_t)index];
    ISX_CHECK_ARG(out->cols == g.nx && out->rows == g.ny, ISX_ERR_SIZE, "%s: out is %dx%d, the map %dx%d", who, out->cols, out->rows, g.nx, g.ny);
    const std::vector<float>& m = h->maps[(size_t)index];
    const size_t row = (size_t)g.nx * sizeof(float);
    if (out->device < 0) {
        for (int y = 0; y < g.ny; ++y) std::memcpy((char*)out->data + (size_t)y * out->step, &m[(size_t)y * g.nx], row);
        return ISX_OK;
    }
    ISX_HIP(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)hip_stream;
    ISX_HIP(hipMemcpy2DAsync(out->data, out->step, (const float*)h->maps_dev.p + h->map_off[(size_t)index], row, row, (size_t)g.ny, hipMemcpyDeviceToDevice, st));
    return ISX_OK;
} ISX_EXIT("isx_blocks_gain_map")

int isx_blocks_gain_stats(const isx_blocks_gain* h, long long* num_pairs, isx_block_pair* pairs, long long capacity, long long* diag_n) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(h != nullptr, ISX_ERR_INVALID, "blocks_gain_stats: null handle");
    ISX_CHECK_ARG(h->fed, ISX_ERR_STATE, "blocks_gain_stats: feed has not run");
    if (num_pairs) *num_pairs = (long long)h->recs.size();
    if (pairs) {
        ISX_CHECK_ARG(capacity >= (long long)h->recs.size(), ISX_ERR_SIZE, "blocks_gain_stats: room for %lld of %zu records", capacity, h->recs.size());
        std::copy(h->recs.begin(), h->recs.end(), pairs);
    }
    if (diag_n) std::copy(h->diag_n.begin(), h->diag_n.end(), diag_n);
    return ISX_OK;
} ISX_EXIT("isx_blocks_gain_stats")

int isx_blocks_gain_feed_times(const isx_blocks_gain* h, double* ms4) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(h != nullptr && ms4 != nullptr, ISX_ERR_INVALID, "blocks_gain_feed_times: null argument");
    ISX_CHECK_ARG(h->fed, ISX_ERR_STATE, "blocks_gain_feed_times: feed has not run");
    std::copy(h->ms, h->ms + 4, ms4);
    return ISX_OK;
} ISX_EXIT("isx_blocks_gain_feed_times")

int isx_selftest_lu_solve(int n, const double* A, const double* b, double* x, int* swaps, int where, int device) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(n >= 1 && n <= BG_MAX_BLOCKS, ISX_ERR_INVALID, "selftest_lu_solve: n = %d (1 to %d)", n, BG_MAX_BLOCKS);
    ISX_CHECK_ARG(A && b && x, ISX_ERR_INVALID, "selftest_lu_solve: null argument");
    ISX_CHECK_ARG(where == 0 || where == 1, ISX_ERR_INVALID, "selftest_lu_solve: where = %d (0 the device, 1 the host's lu_solve)", where);
    if (where == 1) {
        std::vector<double> a(A, A + (size_t)n * n), v(b, b + n);
        ISX_CHECK_ARG(lu_solve(a, v, n), ISX_ERR_INTERNAL, "selftest_lu_solve: the system is singular");
        std::copy(v.begin(), v.end(), x);
        if (swaps) *swaps = -1;
        return ISX_OK;
    }
    ISX_HIP(hipSetDevice(device));
    hipStream_t st = nullptr;
    const size_t lda = (size_t)n + 1;
    DevBuf mat;
    LuAux aux;
    ISX_TRY(mat.reserve((size_t)n * lda * sizeof(double)));
    ISX_TRY(aux.reserve(n));
    double* dA = (double*)mat.p;
    {
        std::vector<double> aug((size_t)n * lda);      // b rides as column n
        for (int r = 0; r < n; ++r) {
            std::copy(A + (size_t)r * n, A + (size_t)(r + 1) * n, aug.begin() + (size_t)r * lda);
            aug[(size_t)r * lda + n] = b[r];
        }
        ISX_HIP(hipMemcpyAsync(dA, aug.data(), aug.size() * sizeof(double), hipMemcpyHostToDevice, st));
        ISX_HIP(hipStreamSynchronize(st));
    }
    ISX_TRY(lu_factor_device(dA, lda, n, aux, st));
    ISX_TRY(lu_backsub_device(dA, lda, n, aux, st));
    std::vector<double> v;
    LuState state{};
    ISX_TRY(lu_read_back(n, aux, st, v, state));
    if (swaps) *swaps = state.swaps;
    ISX_CHECK_ARG(!state.singular, ISX_ERR_INTERNAL, "selftest_lu_solve: the system is singular");
    std::copy(v.begin(), v.end(), x);
    return ISX_OK;
} ISX_EXIT("isx_selftest_lu_solve")

}  // extern "C"
