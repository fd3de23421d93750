// graphcut.hip — GraphCutSeamFinder(COST_COLOR | COST_COLOR_GRAD) (OpenCV 3.4.2 stitching/src/seam_finders.cpp) on gfx950:
//   isx_graphcut_seam_find        seam_finder = new GraphCutSeamFinder(GraphCutSeamFinder::COST_COLOR);  W:257
//                                 seam_finder->find(images_warped_f, corners, masks_warped)             W:264
//   isx_graphcut_seam_find_pair   one pair, optionally with a certificate of its maximum flow (int32 residuals: COST_COLOR)
//   isx_graphcut_seam_find_pair64 the same with int64 residuals, either cost type
//
// The specification (DESIGN.md §8 "graph-cut seam finder"; OpenCV parity unpinned): for i < j with a non-empty overlapRoi, a padded grid
// of (roi.h + 20) x (roi.w + 20) nodes (gap 10; outside a tile: image 0, mask 0); mask1 only -> source 10000, mask2 only -> sink 10000;
// every right / down edge w = |d(p)|^2 + |d(q)|^2 + 1 (+ 1000 when a mask byte of p or q is 0) both ways; write-back over the roi from
// the MAXIMAL source side (the nodes that cannot reach the sink in the residual graph of a maximum flow - unique, whatever the schedule).
// With CV_8UC3 tiles, or CV_32FC3 tiles holding integers in [0, 255], every w is an integer below 2^24: the flow is exact in int32.
// COST_COLOR_GRAD (setGraphWeightsColorGrad; CV_32FC3 tiles only) changes the edge weight alone: w = (|d(p)|^2 + |d(q)|^2) / grad + 1.f
// (+ 1000.f), grad = dx1(p) + dx1(q) + dx2(p) + dx2(q) + 1.f for a right edge (dy for a down edge), dx_ / dy_ the squared norm over the three
// channels of the tile's 3 x 3 Sobel derivatives (BORDER_REFLECT_101 at the tile's edges, 0 outside the tile).  On integer tiles numerator and
// grad are exact integers below 2^24, so w is one correctly rounded float division and one or two rounded float additions: a float >= 1,
// hence a multiple of 2^-23.  Capacities are w * 2^23 as int64 (Q23, below 2^42), terminals 10000 * 2^23: the flow is exact in int64.
//
// The max-flow kernels are templates on the capacity type CapT (int, or long long for Q23); heights are int in both.  A node may read an
// edge word its neighbour writes in the same launch, which is harmless only when the word is read whole (a stale value understates the
// excess, a torn one could overstate it): every 64-bit residual goes through GcCap<long long>::ld / st, relaxed atomic accesses of
// single-thread scope, each one naturally aligned global_load / global_store_dwordx2.
//
// The max-flow is push-relabel over the 4-connected grid, one node per thread, launch boundaries the only cross-block synchronisation:
//   k_gc_relabel   an active node (excess > 0, height finite) takes 1 + the lowest height over its residual out-edges (in place: heights
//                  only rise, so a neighbour read old or new keeps the labelling valid)
//   k_gc_push      an active node pushes along admissible edges (the sink when its height is 1, a neighbour one lower).  Residuals are
//                  stored once per undirected edge by its left / upper node (r(v -> v+1) = rR[v], r(v+1 -> v) = 2 capR[v] - rR[v]), so a push
//                  writes one edge word, and the two ends of an edge cannot push across it in the same launch (their heights would have to
//                  differ by +1 and -1): no atomics, no lost updates.  A node's excess is not stored: it follows from its terminal and
//                  edge residuals, and a neighbour's concurrent push into it can only raise what it reads.
//   global relabel every GC_SWEEPS sweeps: heights = BFS distance to the sink over residual edges (k_gc_bfs_init, then k_gc_bfs_tile:
//                  64 x 16 node tiles relaxed in LDS for up to GC_BFS_ITERS steps per launch, in place - distances only fall), with the
//                  active-node count (k_gc_count) read back once per batch of GC_BFS_BATCH launches.
// It ends when no node with a finite height holds excess: the preflow is then maximal and the nodes of infinite height are exactly those
// that cannot reach the sink.  Every device loop has a fixed trip count; the host loops are capped (GC_MAX_ROUNDS rounds, GC_MAX_BFS_BATCHES
// batches per global relabel) and the call fails past them with the pair's masks untouched.
#include "isx_device.hpp"
#include "pairwise.hpp"
#include "scratch.hpp"

using namespace isx;
using namespace isxd;

namespace {

constexpr int GC_GAP = isx::PAIR_GAP;
constexpr int GC_TERM = 10000;
constexpr int GC_PENALTY = 1000;
constexpr int GC_INF = 1 << 30;
constexpr int GC_SWEEPS = 16;            // push-relabel sweeps between global relabels
constexpr int GC_MAX_ROUNDS = 4096;      // rounds of (GC_SWEEPS sweeps, global relabel) per pair
constexpr int GC_BFS_BATCH = 4;          // BFS tile launches per read-back
constexpr int GC_MAX_BFS_BATCHES = 8192; // read-backs per global relabel
constexpr int GC_BFS_ITERS = 64;         // relaxation steps in LDS per BFS tile launch
constexpr int GC_TW = 64, GC_TH = 16;    // BFS tile (256 threads, 4 rows each)
constexpr int GC_NT = 256;

struct GcGeom {
    const unsigned char* i1; size_t s1;
    const unsigned char* i2; size_t s2;
    unsigned char* m1; size_t sm1;
    unsigned char* m2; size_t sm2;
    int r1, c1, r2, c2;                  // tile sizes
    int oy1, ox1, oy2, ox2;              // tile coordinates of grid node (0, 0)
    int hp, wp;                          // padded grid
    int rh, rw;                          // the roi
};

constexpr int GC_Q = 23;                 // COST_COLOR_GRAD capacities are multiples of 2^-23

template <typename CapT>
struct GcArr {
    CapT* capR; CapT* capD; int* term; CapT* rR; CapT* rD; CapT* rT; int* h;   // term: +-GC_TERM or 0, unscaled
    int hp, wp;
};

// how a residual word is read and written, and the scale of the terminal links
template <typename CapT> struct GcCap;
template <> struct GcCap<int> {
    static constexpr int SHIFT = 0;
    static __device__ __forceinline__ int ld(const int* p) { return *p; }
    static __device__ __forceinline__ void st(int* p, int v) { *p = v; }
};
template <> struct GcCap<long long> {
    static constexpr int SHIFT = GC_Q;
    static __device__ __forceinline__ long long ld(const long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SINGLETHREAD); }
    static __device__ __forceinline__ void st(long long* p, long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SINGLETHREAD); }
};
template <typename CapT> constexpr CapT gc_term() { return (CapT)GC_TERM * ((CapT)1 << GcCap<CapT>::SHIFT); }
template <typename T> __device__ __forceinline__ T gc_min(T a, T b) { return a < b ? a : b; }

template <bool U8>
__device__ __forceinline__ void gc_pixel(const unsigned char* p, size_t step, int y, int x, int& b, int& g, int& r) {
    if constexpr (U8) {
        const unsigned char* q = p + (size_t)y * step + (size_t)x * 3;
        b = q[0]; g = q[1]; r = q[2];
    } else {
        const float* q = (const float*)(p + (size_t)y * step) + (size_t)x * 3;
        b = (int)q[0]; g = (int)q[1]; r = (int)q[2];    // integers in [0, 255]: checked before the first pair
    }
}

// |img1 - img2|^2 at grid node (y, x) and whether both masks are set there
template <bool U8>
__device__ __forceinline__ int gc_node(const GcGeom& G, int y, int x, bool& m1, bool& m2) {
    int b1 = 0, g1 = 0, r1 = 0, b2 = 0, g2 = 0, r2 = 0;
    const int y1 = G.oy1 + y, x1 = G.ox1 + x, y2 = G.oy2 + y, x2 = G.ox2 + x;
    m1 = m2 = false;
    if ((unsigned)y1 < (unsigned)G.r1 && (unsigned)x1 < (unsigned)G.c1) {
        gc_pixel<U8>(G.i1, G.s1, y1, x1, b1, g1, r1);
        m1 = G.m1[(size_t)y1 * G.sm1 + x1] != 0;
    }
    if ((unsigned)y2 < (unsigned)G.r2 && (unsigned)x2 < (unsigned)G.c2) {
        gc_pixel<U8>(G.i2, G.s2, y2, x2, b2, g2, r2);
        m2 = G.m2[(size_t)y2 * G.sm2 + x2] != 0;
    }
    const int db = b1 - b2, dg = g1 - g2, dr = r1 - r2;
    return db * db + dg * dg + dr * dr;
}

// setGraphWeightsColor: terminal and edge capacities, the residuals at zero flow, heights to be set by the first global relabel
template <bool U8>
__global__ __launch_bounds__(GC_NT) void k_gc_build(GcGeom G, GcArr<int> a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= G.wp || y >= G.hp) return;
    const size_t v = (size_t)y * G.wp + x;
    bool p1, p2;
    const int dp = gc_node<U8>(G, y, x, p1, p2);
    int cr = 0, cd = 0;
    if (x + 1 < G.wp) {
        bool q1, q2;
        const int dq = gc_node<U8>(G, y, x + 1, q1, q2);
        cr = dp + dq + 1 + ((p1 && p2 && q1 && q2) ? 0 : GC_PENALTY);
    }
    if (y + 1 < G.hp) {
        bool q1, q2;
        const int dq = gc_node<U8>(G, y + 1, x, q1, q2);
        cd = dp + dq + 1 + ((p1 && p2 && q1 && q2) ? 0 : GC_PENALTY);
    }
    const int t = (p1 && !p2) ? GC_TERM : (p2 && !p1) ? -GC_TERM : 0;
    a.capR[v] = cr; a.rR[v] = cr;
    a.capD[v] = cd; a.rD[v] = cd;
    a.term[v] = t; a.rT[v] = t < 0 ? GC_TERM : 0;
}

// one CV_32FC3 tile at (y, x) inside it: the pixel, and the squared norms over the channels of Sobel(src, CV_32F, 1, 0) and (0, 1) (3 x 3,
// BORDER_REFLECT_101; a dimension of size 1 reads index 0).  Integers throughout: |derivative| <= 1020, a norm <= 3 * 1020^2.
__device__ __forceinline__ void gc_sobel_sq(const unsigned char* p, size_t step, int rows, int cols, int y, int x, int c[3], int& gx, int& gy) {
    const int ym = y > 0 ? y - 1 : (rows > 1 ? 1 : 0), yp = y + 1 < rows ? y + 1 : (rows > 1 ? rows - 2 : 0);
    const int xm = x > 0 ? x - 1 : (cols > 1 ? 1 : 0), xp = x + 1 < cols ? x + 1 : (cols > 1 ? cols - 2 : 0);
    const float* r0 = (const float*)(p + (size_t)ym * step);
    const float* r1 = (const float*)(p + (size_t)y * step);
    const float* r2 = (const float*)(p + (size_t)yp * step);
    gx = gy = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int a00 = (int)r0[(size_t)xm * 3 + ch], a01 = (int)r0[(size_t)x * 3 + ch], a02 = (int)r0[(size_t)xp * 3 + ch];
        const int a10 = (int)r1[(size_t)xm * 3 + ch], a11 = (int)r1[(size_t)x * 3 + ch], a12 = (int)r1[(size_t)xp * 3 + ch];
        const int a20 = (int)r2[(size_t)xm * 3 + ch], a21 = (int)r2[(size_t)x * 3 + ch], a22 = (int)r2[(size_t)xp * 3 + ch];
        const int dx = (a02 - a00) + 2 * (a12 - a10) + (a22 - a20);
        const int dy = (a20 - a00) + 2 * (a21 - a01) + (a22 - a02);
        gx += dx * dx; gy += dy * dy;
        c[ch] = a11;
    }
}

// grid node (y, x) for COST_COLOR_GRAD: |img1 - img2|^2, dx1 + dx2, dy1 + dy2 (a tile that does not cover the node adds 0) and the masks
__device__ __forceinline__ int gc_node_grad(const GcGeom& G, int y, int x, int& gx, int& gy, bool& m1, bool& m2) {
    int c1[3] = {0, 0, 0}, c2[3] = {0, 0, 0}, gx1 = 0, gy1 = 0, gx2 = 0, gy2 = 0;
    const int y1 = G.oy1 + y, x1 = G.ox1 + x, y2 = G.oy2 + y, x2 = G.ox2 + x;
    m1 = m2 = false;
    if ((unsigned)y1 < (unsigned)G.r1 && (unsigned)x1 < (unsigned)G.c1) {
        gc_sobel_sq(G.i1, G.s1, G.r1, G.c1, y1, x1, c1, gx1, gy1);
        m1 = G.m1[(size_t)y1 * G.sm1 + x1] != 0;
    }
    if ((unsigned)y2 < (unsigned)G.r2 && (unsigned)x2 < (unsigned)G.c2) {
        gc_sobel_sq(G.i2, G.s2, G.r2, G.c2, y2, x2, c2, gx2, gy2);
        m2 = G.m2[(size_t)y2 * G.sm2 + x2] != 0;
    }
    gx = gx1 + gx2; gy = gy1 + gy2;
    const int db = c1[0] - c2[0], dg = c1[1] - c2[1], dr = c1[2] - c2[2];
    return db * db + dg * dg + dr * dr;
}

// (num / grad + 1.f [+ 1000.f]) * 2^23: num and grad exact in float, the division correctly rounded, the additions rounded one by one
// (-ffp-contract=off); the result is a float >= 1, so the scaling and the conversion are exact
__device__ __forceinline__ long long gc_weight_q23(int num, int grad, bool ok) {
    float w = (float)num / (float)grad + 1.f;
    if (!ok) w += (float)GC_PENALTY;
    return (long long)(w * (float)(1 << GC_Q));
}

// setGraphWeightsColorGrad in Q23.  A node's right and lower neighbours are computed again by this thread rather than shared through LDS:
// the launch runs once per pair, against thousands of sweep launches, and stays free of barriers next to its bounds exit.
__global__ __launch_bounds__(GC_NT) void k_gc_build_grad(GcGeom G, GcArr<long long> a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= G.wp || y >= G.hp) return;
    const size_t v = (size_t)y * G.wp + x;
    bool p1, p2;
    int pgx, pgy;
    const int dp = gc_node_grad(G, y, x, pgx, pgy, p1, p2);
    long long cr = 0, cd = 0;
    if (x + 1 < G.wp) {
        bool q1, q2;
        int qgx, qgy;
        const int dq = gc_node_grad(G, y, x + 1, qgx, qgy, q1, q2);
        cr = gc_weight_q23(dp + dq, pgx + qgx + 1, p1 && p2 && q1 && q2);
    }
    if (y + 1 < G.hp) {
        bool q1, q2;
        int qgx, qgy;
        const int dq = gc_node_grad(G, y + 1, x, qgx, qgy, q1, q2);
        cd = gc_weight_q23(dp + dq, pgy + qgy + 1, p1 && p2 && q1 && q2);
    }
    const int t = (p1 && !p2) ? GC_TERM : (p2 && !p1) ? -GC_TERM : 0;
    a.capR[v] = cr; a.rR[v] = cr;
    a.capD[v] = cd; a.rD[v] = cd;
    a.term[v] = t; a.rT[v] = t < 0 ? gc_term<long long>() : 0;
}

// a CV_32FC3 value that is not an integer in [0, 255] (NaN included) raises the flag
__global__ __launch_bounds__(GC_NT) void k_gc_check_f32(const unsigned char* p, size_t step, int rows, int cols, int* flag) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= cols || y >= rows) return;
    const float* q = (const float*)(p + (size_t)y * step) + (size_t)x * 3;
    bool bad = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float f = q[c];
        bad |= !(f >= 0.f && f <= 255.f && f == floorf(f));
    }
    if (bad) *flag = 1;
}

// excess of node v: source inflow - sink outflow + net inflow over its four edges (all from the residuals)
template <typename CapT>
__device__ __forceinline__ CapT gc_excess(const GcArr<CapT>& a, int y, int x, size_t v) {
    using C = GcCap<CapT>;
    const CapT t = (CapT)a.term[v] * ((CapT)1 << C::SHIFT);
    CapT e = (t > 0 ? t : 0) - ((t < 0 ? -t : 0) - C::ld(a.rT + v));
    e -= a.capR[v] - C::ld(a.rR + v);
    e -= a.capD[v] - C::ld(a.rD + v);
    if (x > 0) e += a.capR[v - 1] - C::ld(a.rR + (v - 1));
    if (y > 0) e += a.capD[v - a.wp] - C::ld(a.rD + (v - a.wp));
    return e;
}

// residuals of v's out-edges: right, left, down, up
template <typename CapT>
__device__ __forceinline__ void gc_res4(const GcArr<CapT>& a, int y, int x, size_t v, CapT r[4]) {
    using C = GcCap<CapT>;
    r[0] = C::ld(a.rR + v);
    r[1] = x > 0 ? 2 * a.capR[v - 1] - C::ld(a.rR + (v - 1)) : 0;
    r[2] = C::ld(a.rD + v);
    r[3] = y > 0 ? 2 * a.capD[v - a.wp] - C::ld(a.rD + (v - a.wp)) : 0;
}

template <typename CapT>
__global__ __launch_bounds__(GC_NT) void k_gc_relabel(GcArr<CapT> a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.wp || y >= a.hp) return;
    const size_t v = (size_t)y * a.wp + x;
    const int h = a.h[v];
    if (h >= GC_INF || gc_excess(a, y, x, v) <= 0) return;
    CapT r[4];
    gc_res4(a, y, x, v, r);
    int m = GcCap<CapT>::ld(a.rT + v) > 0 ? 0 : GC_INF;
    if (r[0] > 0) m = min(m, a.h[v + 1]);
    if (r[1] > 0) m = min(m, a.h[v - 1]);
    if (r[2] > 0) m = min(m, a.h[v + a.wp]);
    if (r[3] > 0) m = min(m, a.h[v - a.wp]);
    const int nh = m >= GC_INF - 1 ? GC_INF : m + 1;
    if (nh > h) a.h[v] = nh;
}

// every residual word is read once into a register and written once
template <typename CapT>
__global__ __launch_bounds__(GC_NT) void k_gc_push(GcArr<CapT> a) {
    using C = GcCap<CapT>;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.wp || y >= a.hp) return;
    const size_t v = (size_t)y * a.wp + x;
    const int h = a.h[v];
    if (h >= GC_INF) return;
    CapT e = gc_excess(a, y, x, v);
    if (e <= 0) return;
    if (h == 1) {
        const CapT rt = C::ld(a.rT + v);
        if (rt > 0) {
            const CapT d = gc_min(e, rt);
            C::st(a.rT + v, rt - d); e -= d;
        }
    }
    if (e > 0 && x + 1 < a.wp && a.h[v + 1] == h - 1) {
        const CapT rr = C::ld(a.rR + v);
        if (rr > 0) {
            const CapT d = gc_min(e, rr);
            C::st(a.rR + v, rr - d); e -= d;
        }
    }
    if (e > 0 && x > 0 && a.h[v - 1] == h - 1) {
        const CapT cl = a.capR[v - 1], rl = C::ld(a.rR + (v - 1));
        const CapT d = gc_min(e, 2 * cl - rl);
        if (d > 0) { C::st(a.rR + (v - 1), rl + d); e -= d; }
    }
    if (e > 0 && y + 1 < a.hp && a.h[v + a.wp] == h - 1) {
        const CapT rd = C::ld(a.rD + v);
        if (rd > 0) {
            const CapT d = gc_min(e, rd);
            C::st(a.rD + v, rd - d); e -= d;
        }
    }
    if (e > 0 && y > 0 && a.h[v - a.wp] == h - 1) {
        const CapT cu = a.capD[v - a.wp], ru = C::ld(a.rD + (v - a.wp));
        const CapT d = gc_min(e, 2 * cu - ru);
        if (d > 0) C::st(a.rD + (v - a.wp), ru + d);
    }
}

template <typename CapT>
__global__ __launch_bounds__(GC_NT) void k_gc_bfs_init(GcArr<CapT> a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.wp || y >= a.hp) return;
    const size_t v = (size_t)y * a.wp + x;
    a.h[v] = GcCap<CapT>::ld(a.rT + v) > 0 ? 1 : GC_INF;
}

// one 64 x 16 tile: heights with a one-node halo in LDS, relaxed h(v) = min(h(v), 1 + h(w)) over residual v -> w until nothing changes
// (at most GC_BFS_ITERS steps); lowered heights are written back and raise *changed
template <typename CapT>
__global__ __launch_bounds__(GC_NT) void k_gc_bfs_tile(GcArr<CapT> a, int* changed) {
    __shared__ int sh[GC_TH + 2][GC_TW + 2];
    const int x0 = blockIdx.x * GC_TW, y0 = blockIdx.y * GC_TH;
    for (int k = threadIdx.x; k < (GC_TH + 2) * (GC_TW + 2); k += GC_NT) {
        const int ly = k / (GC_TW + 2), lx = k - ly * (GC_TW + 2);
        const int y = y0 + ly - 1, x = x0 + lx - 1;
        sh[ly][lx] = ((unsigned)y < (unsigned)a.hp && (unsigned)x < (unsigned)a.wp) ? a.h[(size_t)y * a.wp + x] : GC_INF;
    }
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    unsigned dirs[4];                   // residual out-edges of this thread's four nodes: bit 0 right, 1 left, 2 down, 3 up
    int h0[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = y0 + ty + 4 * k, x = x0 + tx;
        dirs[k] = 0;
        h0[k] = GC_INF;
        if (y < a.hp && x < a.wp) {
            const size_t v = (size_t)y * a.wp + x;
            CapT r[4];
            gc_res4(a, y, x, v, r);
            dirs[k] = (r[0] > 0 ? 1u : 0u) | (r[1] > 0 ? 2u : 0u) | (r[2] > 0 ? 4u : 0u) | (r[3] > 0 ? 8u : 0u);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) h0[k] = sh[ty + 4 * k + 1][tx + 1];
    for (int it = 0; it < GC_BFS_ITERS; ++it) {
        int ch = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ly = ty + 4 * k + 1, lx = tx + 1;
            const int cur = sh[ly][lx];
            int m = GC_INF;
            if (dirs[k] & 1u) m = min(m, sh[ly][lx + 1]);
            if (dirs[k] & 2u) m = min(m, sh[ly][lx - 1]);
            if (dirs[k] & 4u) m = min(m, sh[ly + 1][lx]);
            if (dirs[k] & 8u) m = min(m, sh[ly - 1][lx]);
            if (m < GC_INF && m + 1 < cur) { sh[ly][lx] = m + 1; ch = 1; }
        }
        if (!__syncthreads_or(ch)) break;
    }
    int any = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = y0 + ty + 4 * k, x = x0 + tx;
        const int hn = sh[ty + 4 * k + 1][tx + 1];
        if (y < a.hp && x < a.wp && hn < h0[k]) {
            a.h[(size_t)y * a.wp + x] = hn;
            any = 1;
        }
    }
    if (__syncthreads_or(any) && threadIdx.x == 0) *changed = 1;
}

// out[0] += active nodes (excess > 0 and a finite height); with flow != nullptr also *flow += sum of the sink links' flow
template <typename CapT>
__global__ __launch_bounds__(GC_NT) void k_gc_count(GcArr<CapT> a, int* out, unsigned long long* flow) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    int act = 0;
    CapT f = 0;
    if (x < a.wp && y < a.hp) {
        const size_t v = (size_t)y * a.wp + x;
        act = (a.h[v] < GC_INF && gc_excess(a, y, x, v) > 0) ? 1 : 0;
        if (a.term[v] < 0) f = gc_term<CapT>() - GcCap<CapT>::ld(a.rT + v);
    }
    __shared__ int sa[GC_NT / WAVE];
    __shared__ unsigned long long sf[GC_NT / WAVE];
    unsigned long long fl = (unsigned long long)f;
    for (int o = 32; o > 0; o >>= 1) { act += __shfl_xor(act, o); fl += __shfl_xor(fl, o); }
    if ((threadIdx.x & (WAVE - 1)) == 0) { sa[threadIdx.x / WAVE] = act; sf[threadIdx.x / WAVE] = fl; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        unsigned long long t = 0;
        for (int w = 0; w < GC_NT / WAVE; ++w) { s += sa[w]; t += sf[w]; }
        if (s) atomicAdd(out, s);
        if (flow && t) atomicAdd(flow, t);
    }
}

// findInPair's write-back over the roi: source side and mask1 set -> mask2 = 0; sink side and mask2 set -> mask1 = 0
__global__ __launch_bounds__(GC_NT) void k_gc_write_back(GcGeom G, const int* h) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= G.rw || y >= G.rh) return;
    const int gy = y + GC_GAP, gx = x + GC_GAP;
    unsigned char* p1 = G.m1 + (size_t)(G.oy1 + gy) * G.sm1 + (G.ox1 + gx);
    unsigned char* p2 = G.m2 + (size_t)(G.oy2 + gy) * G.sm2 + (G.ox2 + gx);
    if (h[(size_t)gy * G.wp + gx] >= GC_INF) {
        if (*p1) *p2 = 0;
    } else {
        if (*p2) *p1 = 0;
    }
}

// the certificate: per node (right, left, down, up, source, sink) residuals and the label (1 = source side)
template <typename CapT, typename OutT>
__global__ __launch_bounds__(GC_NT) void k_gc_cert(GcArr<CapT> a, OutT* res, unsigned char* labels) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.wp || y >= a.hp) return;
    const size_t v = (size_t)y * a.wp + x;
    CapT r[4];
    gc_res4(a, y, x, v, r);
    OutT* o = res + 6 * v;
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3];
    o[4] = 0;                           // every source link stays saturated (the preflow never returns excess to the source)
    o[5] = GcCap<CapT>::ld(a.rT + v);
    labels[v] = a.h[v] >= GC_INF ? 1 : 0;
}

// per calling thread, kept between calls: the graph arrays, the counters (device and pinned), staged host images and masks
struct GcScratch {
    DevBuf graph, cert;
    int device = -1;
    PinBuf pin;                          // 64 ints: the counters read back
    MatStages stages;                    // slot 2 i: image i, slot 2 i + 1: mask i
};

enum { GC_C_CHANGED = 0, GC_C_COUNT = GC_BFS_BATCH, GC_C_FLAG, GC_C_FLOW, GC_C_WORDS = GC_C_FLOW + 2 };
enum GcMode { GC_MODE_U8, GC_MODE_F32, GC_MODE_F32_GRAD };   // tile depth and cost type of a call

struct PairOut {
    long long flow = 0;
    int rounds = 0, launches = 0, hp = 0, wp = 0;
};

inline dim3 gc_grid(int w, int h) { return dim3((unsigned)cdiv(w, 64), (unsigned)cdiv(h, 4)); }

inline int gc_launch_build(const GcGeom& G, const GcArr<int>& a, GcMode mode, double bytes, dim3 grid, hipStream_t st) {
    if (mode == GC_MODE_U8) ISX_LAUNCH("graphcut_build", bytes, st, (k_gc_build<true>), grid, dim3(GC_NT), 0, G, a);
    else ISX_LAUNCH("graphcut_build", bytes, st, (k_gc_build<false>), grid, dim3(GC_NT), 0, G, a);
    return ISX_OK;
}
inline int gc_launch_build(const GcGeom& G, const GcArr<long long>& a, GcMode, double bytes, dim3 grid, hipStream_t st) {
    ISX_LAUNCH("graphcut_build_grad", bytes, st, k_gc_build_grad, grid, dim3(GC_NT), 0, G, a);
    return ISX_OK;
}

// the max-flow of one pair's graph and its write-back; cert_res / cert_lab (device, may be null) receive the certificate.  CapT int:
// COST_COLOR; long long: COST_COLOR_GRAD in Q23 (flow and residuals in units of 2^-23)
template <typename CapT, typename OutT>
int gc_solve_pair(GcScratch& s, const GcGeom& G, GcMode mode, hipStream_t st, PairOut& out, OutT* cert_res, unsigned char* cert_lab) {
    const size_t n = (size_t)G.hp * G.wp;
    Bump lay;                            // five arrays of CapT, two of int, the counters
    size_t o_cap[5];
    for (size_t& o : o_cap) o = lay.take(n * sizeof(CapT));
    const size_t o_i0 = lay.take(n * sizeof(int)), o_i1 = lay.take(n * sizeof(int)), o_cnt = lay.take(256);
    ISX_TRY(s.graph.reserve(lay.at));
    char* base = (char*)s.graph.p;
    GcArr<CapT> a{(CapT*)(base + o_cap[0]), (CapT*)(base + o_cap[1]), (int*)(base + o_i0), (CapT*)(base + o_cap[2]), (CapT*)(base + o_cap[3]),
                  (CapT*)(base + o_cap[4]), (int*)(base + o_i1), G.hp, G.wp};
    int* cnt = (int*)(base + o_cnt);     // GC_C_WORDS ints: changed flags, active count, (unused) flag, flow (8-byte aligned)
    int* const pin = (int*)s.pin.p;
    const dim3 grid = gc_grid(G.wp, G.hp), tiles((unsigned)cdiv(G.wp, GC_TW), (unsigned)cdiv(G.hp, GC_TH));
    const double nb = (double)n * sizeof(CapT);
    out.hp = G.hp; out.wp = G.wp; out.rounds = 0; out.launches = 0;
    ISX_TRY(gc_launch_build(G, a, mode, nb * 7, grid, st));
    ++out.launches;
    // global relabel, then the active count; returns the count in *active
    auto global_relabel = [&](int* active) -> int {
        ISX_LAUNCH("graphcut_bfs_init", nb * 2, st, k_gc_bfs_init<CapT>, grid, dim3(GC_NT), 0, a);
        ++out.launches;
        for (int b = 0; b < GC_MAX_BFS_BATCHES; ++b) {
            ISX_HIP(hipMemsetAsync(cnt, 0, (GC_C_COUNT + 1) * sizeof(int), st));
            for (int k = 0; k < GC_BFS_BATCH; ++k) {
                ISX_LAUNCH("graphcut_bfs", nb * 6, st, k_gc_bfs_tile<CapT>, tiles, dim3(GC_NT), 0, a, cnt + GC_C_CHANGED + k);
                ++out.launches;
            }
            ISX_LAUNCH("graphcut_count", nb * 7, st, k_gc_count<CapT>, grid, dim3(GC_NT), 0, a, cnt + GC_C_COUNT, (unsigned long long*)nullptr);
            ++out.launches;
            ISX_HIP(hipMemcpyAsync(pin, cnt, (GC_C_COUNT + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
            ISX_HIP(hipStreamSynchronize(st));
            if (pin[GC_C_CHANGED + GC_BFS_BATCH - 1] == 0) { *active = pin[GC_C_COUNT]; return ISX_OK; }
        }
        return fail(ISX_ERR_UNSUPPORTED, "graphcut: the global relabel did not settle within %d launches", GC_MAX_BFS_BATCHES * GC_BFS_BATCH);
    };
    int active = 0;
    ISX_TRY(global_relabel(&active));
    while (active > 0) {
        if (out.rounds == GC_MAX_ROUNDS)
            return fail(ISX_ERR_UNSUPPORTED, "graphcut: the max-flow of a %d x %d grid did not finish within %d rounds (%d nodes still active); "
                        "the pair's masks are unchanged", G.hp, G.wp, GC_MAX_ROUNDS, active);
        ++out.rounds;
        for (int k = 0; k < GC_SWEEPS; ++k) {
            ISX_LAUNCH("graphcut_relabel", nb * 11, st, k_gc_relabel<CapT>, grid, dim3(GC_NT), 0, a);
            ISX_LAUNCH("graphcut_push", nb * 12, st, k_gc_push<CapT>, grid, dim3(GC_NT), 0, a);
            out.launches += 2;
        }
        ISX_TRY(global_relabel(&active));
    }
    unsigned long long* flow = (unsigned long long*)(cnt + GC_C_FLOW);
    ISX_HIP(hipMemsetAsync(cnt, 0, GC_C_WORDS * sizeof(int), st));
    ISX_LAUNCH("graphcut_count", nb * 7, st, k_gc_count<CapT>, grid, dim3(GC_NT), 0, a, cnt + GC_C_COUNT, flow);
    ++out.launches;
    if (cert_res) {
        ISX_LAUNCH("graphcut_cert", nb * 30, st, (k_gc_cert<CapT, OutT>), grid, dim3(GC_NT), 0, a, cert_res, cert_lab);
        ++out.launches;
    }
    ISX_LAUNCH("graphcut_write_back", (double)G.rw * G.rh * 8.0, st, k_gc_write_back, gc_grid(G.rw, G.rh), dim3(GC_NT), 0, G, (const int*)a.h);
    ++out.launches;
    ISX_HIP(hipMemcpyAsync(pin, cnt, GC_C_WORDS * sizeof(int), hipMemcpyDeviceToHost, st));
    ISX_HIP(hipStreamSynchronize(st));
    unsigned long long f;
    memcpy(&f, pin + GC_C_FLOW, sizeof(f));
    out.flow = (long long)f;
    return ISX_OK;
}

constexpr long long GC_MAX_NODES_Q23 = 1ll << 26;   // past this a Q23 flow total is no longer provably below 2^63

inline GcMode gc_mode(int cost_type, int image_type) {
    return cost_type == ISX_GC_COST_COLOR_GRAD ? GC_MODE_F32_GRAD : image_type == ISX_8UC3 ? GC_MODE_U8 : GC_MODE_F32;
}

// one pair by the solver of its cost type; OutT is the certificate's word (int: COST_COLOR only)
template <typename OutT>
int gc_solve(GcScratch& s, const GcGeom& G, GcMode mode, hipStream_t st, PairOut& out, OutT* cert_res, unsigned char* cert_lab) {
    if (mode != GC_MODE_F32_GRAD) return gc_solve_pair<int, OutT>(s, G, mode, st, out, cert_res, cert_lab);
    if constexpr (sizeof(OutT) == sizeof(long long)) return gc_solve_pair<long long, long long>(s, G, mode, st, out, cert_res, cert_lab);
    else return gc_solve_pair<long long, long long>(s, G, mode, st, out, nullptr, nullptr);   // no int32 certificate of a Q23 flow: refused by the entry
}

struct GcCall { std::vector<isx_mat> img, msk; };   // device views

int gc_check_args(int n, const isx_mat* images, const isx_mat* masks, int cost_type, const char* who) {
    ISX_CHECK_ARG(cost_type == ISX_GC_COST_COLOR || cost_type == ISX_GC_COST_COLOR_GRAD, ISX_ERR_INVALID, "%s: cost_type %d", who, cost_type);
    ISX_CHECK_ARG(cost_type == ISX_GC_COST_COLOR || !(n > 0 && images && images[0].type == ISX_8UC3), ISX_ERR_UNSUPPORTED,
                  "%s: COST_COLOR_GRAD takes CV_32FC3 tiles only (OpenCV's finder reads Point3f)", who);
    return check_tiles(n, images, masks, true, who);
}

// COST_COLOR_GRAD: no pair's padded grid may exceed 2^26 nodes - checked over every pair before anything is launched
int gc_check_size(int n, const isx_mat* images, const int* corners_xy, int cost_type, const char* who) {
    if (cost_type != ISX_GC_COST_COLOR_GRAD) return ISX_OK;
    for (int i = 0; i + 1 < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            PairGrid p;
            if (!pair_grid(corners_xy + 2 * i, images[i].cols, images[i].rows, corners_xy + 2 * j, images[j].cols, images[j].rows, p)) continue;
            ISX_CHECK_ARG((long long)p.hp * p.wp <= GC_MAX_NODES_Q23, ISX_ERR_UNSUPPORTED, "%s: COST_COLOR_GRAD on a %d x %d grid (more than 2^26 nodes: "
                          "the flow total is no longer provably below 2^63)", who, p.hp, p.wp);
        }
    return ISX_OK;
}

// capture check, device views of every image and mask, and the CV_32FC3 value check - all before the first pair writes
int gc_prepare(GcScratch& s, int n, const isx_mat* images, isx_mat* masks, int device, hipStream_t st, GcCall& c, const char* who) {
    ISX_TRY(refuse_capture(st, who, "the finder reads counters back to the host"));
    if (s.device != device) { s.graph.release(); s.cert.release(); s.device = device; }
    s.stages.use_device(device);
    ISX_TRY(s.pin.reserve(64 * sizeof(int), 64 * sizeof(int)));
    c.img.resize(n);
    c.msk.resize(n);
    for (int i = 0; i < n; ++i) {
        ISX_TRY(s.stages.stage(2 * i, &images[i], false, st, who, c.img[i]));
        ISX_TRY(s.stages.stage(2 * i + 1, &masks[i], true, st, who, c.msk[i]));
    }
    if (images[0].type == ISX_32FC3) {
        ISX_TRY(s.graph.reserve(256));
        int* flag = (int*)s.graph.p;
        ISX_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
        for (int i = 0; i < n; ++i)
            ISX_LAUNCH("graphcut_check", (double)c.img[i].rows * c.img[i].cols * 12.0, st, k_gc_check_f32, gc_grid(c.img[i].cols, c.img[i].rows), dim3(GC_NT), 0,
                       (const unsigned char*)c.img[i].data, c.img[i].step, c.img[i].rows, c.img[i].cols, flag);
        ISX_HIP(hipMemcpyAsync(s.pin.p, flag, sizeof(int), hipMemcpyDeviceToHost, st));
        ISX_HIP(hipStreamSynchronize(st));
        ISX_CHECK_ARG(*(const int*)s.pin.p == 0, ISX_ERR_UNSUPPORTED, "%s: a CV_32FC3 value is not an integer in [0, 255] (the capacities would not be exact)", who);
    }
    return ISX_OK;
}

bool gc_geom(const isx_mat& i1, const isx_mat& i2, isx_mat& m1, isx_mat& m2, const int tl1[2], const int tl2[2], GcGeom& G) {
    PairGrid p;
    if (!pair_grid(tl1, i1.cols, i1.rows, tl2, i2.cols, i2.rows, p)) return false;
    G.i1 = (const unsigned char*)i1.data; G.s1 = i1.step;
    G.i2 = (const unsigned char*)i2.data; G.s2 = i2.step;
    G.m1 = (unsigned char*)m1.data; G.sm1 = m1.step;
    G.m2 = (unsigned char*)m2.data; G.sm2 = m2.step;
    G.r1 = i1.rows; G.c1 = i1.cols; G.r2 = i2.rows; G.c2 = i2.cols;
    G.rw = p.rw; G.rh = p.rh; G.hp = p.hp; G.wp = p.wp;
    G.oy1 = p.oy1; G.ox1 = p.ox1; G.oy2 = p.oy2; G.ox2 = p.ox2;
    return true;
}

// isx_graphcut_seam_find_pair (OutT int) and isx_graphcut_seam_find_pair64 (OutT long long)
template <typename OutT>
int gc_find_pair(const isx_mat* image1, const isx_mat* image2, const int* corners_xy, isx_mat* mask1, isx_mat* mask2, int cost_type, long long* flow,
                 OutT* residuals, unsigned char* labels, long long cert_nodes, int* info, int device, void* hip_stream, const char* who) {
    clear_error();
    ISX_CHECK_ARG(image1 && image2 && corners_xy && mask1 && mask2, ISX_ERR_INVALID, "%s: null argument", who);
    ISX_CHECK_ARG((residuals == nullptr) == (labels == nullptr), ISX_ERR_INVALID, "%s: residuals and labels go together", who);
    const isx_mat im[2] = {*image1, *image2};
    isx_mat mk[2] = {*mask1, *mask2};
    ISX_TRY(gc_check_args(2, im, mk, cost_type, who));
    ISX_CHECK_ARG(sizeof(OutT) == sizeof(long long) || residuals == nullptr || cost_type == ISX_GC_COST_COLOR, ISX_ERR_INVALID,
                  "%s: COST_COLOR_GRAD residuals are 64-bit (Q23): use isx_graphcut_seam_find_pair64", who);
    ISX_TRY(gc_check_size(2, im, corners_xy, cost_type, who));
    ISX_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)hip_stream;
    GcScratch& s = per_thread<GcScratch>();
    GcCall c;
    ISX_TRY(gc_prepare(s, 2, im, mk, device, st, c, who));   // host masks: copied back through mk, views of the same data
    GcGeom G{};
    PairOut po;
    if (flow) *flow = 0;
    if (!gc_geom(c.img[0], c.img[1], c.msk[0], c.msk[1], corners_xy, corners_xy + 2, G)) {
        if (info) { info[0] = info[1] = info[2] = info[3] = 0; }
        return ISX_OK;
    }
    const long long n = (long long)G.hp * G.wp;
    ISX_CHECK_ARG(residuals == nullptr || cert_nodes >= n, ISX_ERR_SIZE, "%s: the certificate needs %lld nodes (%d x %d), %lld given", who, n, G.hp, G.wp,
                  cert_nodes);
    OutT* dres = nullptr;
    unsigned char* dlab = nullptr;
    if (residuals) {
        const size_t rb = round256((size_t)n * 6 * sizeof(OutT));
        ISX_TRY(s.cert.reserve(rb + (size_t)n));
        dres = (OutT*)s.cert.p;
        dlab = (unsigned char*)s.cert.p + rb;
    }
    ISX_TRY(gc_solve<OutT>(s, G, gc_mode(cost_type, im[0].type), st, po, dres, dlab));
    if (residuals) {
        ISX_HIP(hipMemcpyAsync(residuals, dres, (size_t)n * 6 * sizeof(OutT), hipMemcpyDeviceToHost, st));
        ISX_HIP(hipMemcpyAsync(labels, dlab, (size_t)n, hipMemcpyDeviceToHost, st));
        ISX_HIP(hipStreamSynchronize(st));
    }
    if (flow) *flow = po.flow;
    if (info) { info[0] = po.hp; info[1] = po.wp; info[2] = po.rounds; info[3] = po.launches; }
    return s.stages.finish(st);
}

}  // namespace

extern "C" {

int isx_graphcut_seam_release(void) ISX_ENTRY {
    clear_error();
    GcScratch& s = per_thread<GcScratch>();
    s.graph.release();
    s.cert.release();
    s.stages.clear();
    s.device = -1;
    return s.pin.release();
} ISX_EXIT("isx_graphcut_seam_release")

int isx_graphcut_seam_find(int num_images, const isx_mat* images, const int* corners_xy, isx_mat* masks, int cost_type, int device,
                           void* hip_stream) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(num_images >= 0 && (num_images == 0 || (images && corners_xy && masks)), ISX_ERR_INVALID, "graphcut_seam_find: null argument");
    ISX_TRY(gc_check_args(num_images, images, masks, cost_type, "graphcut_seam_find"));
    if (num_images < 2) return ISX_OK;     // PairwiseSeamFinder::run visits no pair
    ISX_TRY(gc_check_size(num_images, images, corners_xy, cost_type, "graphcut_seam_find"));
    ISX_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)hip_stream;
    GcScratch& s = per_thread<GcScratch>();
    GcCall c;
    ISX_TRY(gc_prepare(s, num_images, images, masks, device, st, c, "graphcut_seam_find"));
    const GcMode mode = gc_mode(cost_type, images[0].type);
    for (int i = 0; i + 1 < num_images; ++i)
        for (int j = i + 1; j < num_images; ++j) {
            GcGeom G{};
            if (!gc_geom(c.img[i], c.img[j], c.msk[i], c.msk[j], corners_xy + 2 * i, corners_xy + 2 * j, G)) continue;
            PairOut po;
            const int rc = gc_solve<int>(s, G, mode, st, po, nullptr, nullptr);
            if (rc != ISX_OK) {
                (void)s.stages.finish(st);     // the pairs before this one keep their edits, host masks as device ones
                return rc;
            }
        }
    return s.stages.finish(st);
} ISX_EXIT("isx_graphcut_seam_find")

int isx_graphcut_seam_find_pair(const isx_mat* image1, const isx_mat* image2, const int* corners_xy, isx_mat* mask1, isx_mat* mask2,
                                int cost_type, long long* flow, int* residuals, unsigned char* labels, long long cert_nodes, int* info,
                                int device, void* hip_stream) ISX_ENTRY {
    return gc_find_pair<int>(image1, image2, corners_xy, mask1, mask2, cost_type, flow, residuals, labels, cert_nodes, info, device, hip_stream,
                             "graphcut_seam_find_pair");
} ISX_EXIT("isx_graphcut_seam_find_pair")

int isx_graphcut_seam_find_pair64(const isx_mat* image1, const isx_mat* image2, const int* corners_xy, isx_mat* mask1, isx_mat* mask2,
                                  int cost_type, long long* flow, long long* residuals, unsigned char* labels, long long cert_nodes, int* info,
                                  int device, void* hip_stream) ISX_ENTRY {
    return gc_find_pair<long long>(image1, image2, corners_xy, mask1, mask2, cost_type, flow, residuals, labels, cert_nodes, info, device, hip_stream,
                                   "graphcut_seam_find_pair64");
} ISX_EXIT("isx_graphcut_seam_find_pair64")

}  // extern "C"
