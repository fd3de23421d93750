// estimator.hip — HomographyBasedEstimator1 of the reference's 恢复相机内参数 demo (C = its 恢复相机内参数.cpp) on gfx950:
//   isx_estimate_cameras    estimator(features, pairwise_matches, cameras) (C:313-321): focalsFromHomography1 (C:26-54), estimateFocal1
//                           (C:55-105), findMaxSpanningTree (C:145-213), CalcRotation (C:215-243), estimate (C:246-284) and the float32 K()
//                           and R of C:329-334 and C:385-386, for every rig of a matcher call, reading H and stats where
//                           isx_find_homography left them
//   isx_estimator_release   returns the per-thread scratch
//
// The specification is tests/helpers/estimator_np.py (DESIGN.md §8 "Camera estimator"): float64 in + - * / sqrt only, every sum in the order
// written; Mat::inv() and Mat * Mat of 3 x 3, CameraParams and Graph::walkBreadthFirst are restated there (unpinned); edges of equal weight
// sort by i * num_images + j.
//
// ONE launch per call: k_es_rigs, one block of ES_THREADS per rig.  The work is small and latency-bound; the launch stays in stream order
// behind the homography launch and nothing is read back.  Inside the block:
//   1  a thread per pair: the dual inverse (kept in the call's scratch), focalsFromHomography of both directions, the candidates;
//   2  a bitonic sort of the candidates' bits in LDS (they are positive doubles or +inf: their bits order as they do), the median;
//   3  a bitonic sort of the edge keys (weight descending) << 12 | i * 64 + j, which orders as i * n + j does;
//   4  Kruskal by wave 0: lane v holds the component of image v, an edge costs three lane reads and a select - no union-find chain in LDS;
//   5  the leaf walks, a lane per leaf (queue and distances in LDS), max_dists by LDS atomics, the centers;
//   6  the walk from the root by one lane (parent, depth), every edge's rotation by a thread of its own, then R level by level.
#include "isx_device.hpp"
#include "mat3.hpp"
#include "pairwise.hpp"
#include "scratch.hpp"

#include <algorithm>

using namespace isx;
using namespace isxd;

namespace {

constexpr int ES_MAXN = ISX_ESTIMATOR_MAX_IMAGES;            // images a rig = lanes of the wave that runs Kruskal and the leaf walks
constexpr int ES_THREADS = 256;
constexpr int ES_MAXPAIRS = ES_MAXN * (ES_MAXN - 1) / 2;     // 2016
constexpr int ES_SORT = 4096;                                // >= 2 * ES_MAXPAIRS, a power of two
constexpr int ES_ST_MEDIAN = ISX_ESTIMATOR_MEDIAN, ES_ST_ASSERT = ISX_ESTIMATOR_ASSERT, ES_ST_UNREACHED = ISX_ESTIMATOR_UNREACHED;
static_assert(ES_MAXN == WAVE, "one image per lane of one wave");
static_assert(2 * ES_MAXPAIRS <= ES_SORT && ES_MAXN * ES_MAXN <= 4096, "the pair index has 12 bits of the edge key");
static_assert(ES_SORT / 2 % ES_THREADS == 0, "a sort step is a whole number of compare-exchanges a thread");
// (float)num_inliers (C:158) is compared as the integer: exact while a float32 holds it.  num_inliers <= the rows of both images.
static_assert(2ll * ISX_MATCH_MAX_ROWS <= (1ll << 24), "num_inliers must stay exact in float32");

struct EsRig { int img_first, n, pair_first, pair_count; };
struct EsPair { int from, to, row, pad; };                   // local image indices; row: the pair's index in H / stats

struct EsCall {
    const EsRig* rigs; const EsPair* pairs; const int* sizes;
    const double* H; long long H_step;
    const int* stats; long long stats_step;
    const double* fin; long long fin_step;                   // null: is_focals_estimated = false
    double* dual;                                            // 9 doubles per table pair
    double* cams; long long cams_step;
    float* kr; long long kr_step;
    int* tree; long long tree_step;
    int* rs; long long rs_step;
};

// C:35-43 and C:45-53 share their tail
__device__ bool es_pick(double d1, double d2, double v1, double v2, double& f) {
    if (v1 < v2) { const double t = v1; v1 = v2; v2 = t; }
    if (v1 > 0 && v2 > 0) f = sqrt(fabs(d1) > fabs(d2) ? v1 : v2);
    else if (v1 > 0) f = sqrt(v1);
    else return false;
    return true;
}

// focalsFromHomography1 (C:26-54) and the candidate of C:75-76: its bits, or all ones where a focal is not ok
__device__ unsigned long long es_candidate(const double* h) {
    double f0 = 0.0, f1 = 0.0;
    double d1 = h[6] * h[7];
    double d2 = (h[7] - h[6]) * (h[7] + h[6]);
    double v1 = (-((h[0] * h[1]) + (h[3] * h[4]))) / d1;
    double v2 = ((((h[0] * h[0]) + (h[3] * h[3])) - (h[1] * h[1])) - (h[4] * h[4])) / d2;
    const bool f1_ok = es_pick(d1, d2, v1, v2, f1);
    d1 = (h[0] * h[3]) + (h[1] * h[4]);
    d2 = (((h[0] * h[0]) + (h[1] * h[1])) - (h[3] * h[3])) - (h[4] * h[4]);
    v1 = ((-h[2]) * h[5]) / d1;
    v2 = ((h[5] * h[5]) - (h[2] * h[2])) / d2;
    const bool f0_ok = es_pick(d1, d2, v1, v2, f0);
    if (!(f0_ok && f1_ok)) return ~0ull;
    return (unsigned long long)__double_as_longlong(sqrt(f0 * f1));
}

// keys[0, P) ascending, P a power of two >= 2, by the whole block.  A thread's compare-exchanges of one step touch disjoint pairs: it
// loads them all, then stores, so that the LDS latencies overlap.
__device__ void es_sort(unsigned long long* keys, int P, int tid) {
    constexpr int PER = ES_SORT / 2 / ES_THREADS;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            unsigned long long a[PER], b[PER];
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                const int t = tid + u * ES_THREADS;
                if (t < (P >> 1)) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    a[u] = keys[i]; b[u] = keys[i | j];
                }
            }
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                const int t = tid + u * ES_THREADS;
                if (t < (P >> 1)) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    if ((a[u] > b[u]) == ((i & k) == 0)) { keys[i] = b[u]; keys[i | j] = a[u]; }
                }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ void es_K(const double* cam, int i, double* k) {      // C:224-234, CameraParams::K()
    k[0] = cam[4 * i]; k[1] = 0.0; k[2] = cam[4 * i + 2];
    k[3] = 0.0; k[4] = cam[4 * i] * cam[4 * i + 1]; k[5] = cam[4 * i + 3];
    k[6] = 0.0; k[7] = 0.0; k[8] = 1.0;
}

__global__ __launch_bounds__(ES_THREADS) void k_es_rigs(EsCall c) {
    // the sort buffer; after Kruskal its bytes hold the queues and distances of the leaf walks
    __shared__ __attribute__((aligned(16))) unsigned long long keys[ES_SORT];
    __shared__ short slot[ES_MAXN * ES_MAXN];                // [i * 64 + j], i < j: the pair's place in the rig's table, -1 without H
    __shared__ unsigned char adj[ES_MAXN * ES_MAXN];         // the tree's adjacency lists in insertion order
    __shared__ double cam[ES_MAXN * 4];                      // focal, aspect, ppx, ppy
    __shared__ double R[ES_MAXN * 9];
    __shared__ int deg[ES_MAXN], maxd[ES_MAXN], par[ES_MAXN], dep[ES_MAXN];
    __shared__ int sh[8];                                    // 0 candidates, 1 pairs with H, 2 tree edges, 3 status, 4 5 centers, 6 their number, 7 the deepest level
    __shared__ int sh2[2];                                   // 0 the min-max distance, 1 cameras reached
    unsigned char* const bq = (unsigned char*)keys;          // [leaf lane][64]
    unsigned char* const bd = bq + ES_MAXN * ES_MAXN;        // [leaf lane][64]

    const int tid = (int)threadIdx.x;
    const EsRig rig = c.rigs[blockIdx.x];
    const int n = rig.n, pc = rig.pair_count;
    const EsPair* const prs = c.pairs + rig.pair_first;
    double* const dual = c.dual + 9ll * rig.pair_first;
    const int* const sizes = c.sizes + 2ll * rig.img_first;
    const bool given = c.fin != nullptr;

    for (int i = tid; i < ES_MAXN * ES_MAXN; i += ES_THREADS) slot[i] = -1;
    if (tid < 8) sh[tid] = 0;
    if (tid < ES_MAXN) { maxd[tid] = 0; deg[tid] = 0; par[tid] = -2; dep[tid] = -1; }
    int P = 2;
    while (P < 2 * pc) P <<= 1;
    __syncthreads();

    // ---- 1: the dual of every pair with H, the candidates of both directions ----
    for (int k = tid; k < (P >> 1); k += ES_THREADS) {
        unsigned long long k0 = ~0ull, k1 = ~0ull;
        if (k < pc) {
            const EsPair p = prs[k];
            const int st = row_ptr(c.stats, p.row, c.stats_step)[0];
            if (st & ISX_HOMOGRAPHY_H) {
                double h[9], hd[9];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double* src = row_ptr(c.H, 3ll * p.row + r, c.H_step);
                    h[3 * r] = src[0]; h[3 * r + 1] = src[1]; h[3 * r + 2] = src[2];
                }
                es_inv3(h, hd);
#pragma unroll
                for (int e = 0; e < 9; ++e) dual[9ll * k + e] = hd[e];
                slot[p.from * ES_MAXN + p.to] = (short)k;
                atomicAdd(&sh[1], 1);
                if (!given) {
                    k0 = es_candidate(h);
                    k1 = es_candidate(hd);
                    const int add = (k0 != ~0ull) + (k1 != ~0ull);
                    if (add) atomicAdd(&sh[0], add);
                }
            }
        }
        keys[2 * k] = k0; keys[2 * k + 1] = k1;
    }
    __syncthreads();

    // ---- 2: the focal (C:84-104), or the caller's cameras (C:264-268) ----
    if (!given) {
        es_sort(keys, P, tid);
        if (tid == 0) {
            const int cnt = sh[0];
            double f;
            if (cnt >= n - 1) {
                if (cnt & 1) f = __longlong_as_double((long long)keys[cnt >> 1]);
                else f = (__longlong_as_double((long long)keys[(cnt >> 1) - 1]) + __longlong_as_double((long long)keys[cnt >> 1])) * 0.5;
                sh[3] |= ES_ST_MEDIAN;
            } else {
                double s = 0.0;
                for (int i = 0; i < n; ++i) s = s + (double)(sizes[2 * i] + sizes[2 * i + 1]);
                f = s / (double)n;
            }
            R[0] = f;                                        // handed to the block through LDS
        }
        __syncthreads();
        const double f = R[0];
        __syncthreads();
        if (tid < n) { cam[4 * tid] = f; cam[4 * tid + 1] = 1.0; cam[4 * tid + 2] = 0.0; cam[4 * tid + 3] = 0.0; }
    } else if (tid < n) {
        const double* fi = row_ptr(c.fin, rig.img_first + tid, c.fin_step);
        cam[4 * tid] = fi[0]; cam[4 * tid + 1] = fi[1];
        cam[4 * tid + 2] = fi[2] - (0.5 * (double)sizes[2 * tid]);
        cam[4 * tid + 3] = fi[3] - (0.5 * (double)sizes[2 * tid + 1]);
    }
    __syncthreads();

    // ---- 3: the edges (C:152-162) sorted as C:169 with the tie rule ----
    for (int k = tid; k < (P >> 1); k += ES_THREADS) {
        unsigned long long k0 = ~0ull, k1 = ~0ull;
        if (k < pc) {
            const EsPair p = prs[k];
            if (slot[p.from * ES_MAXN + p.to] >= 0) {
                const unsigned w = ~((unsigned)row_ptr(c.stats, p.row, c.stats_step)[1] ^ 0x80000000u);      // ascending = weight descending
                k0 = ((unsigned long long)w << 12) | (unsigned)(p.from * ES_MAXN + p.to);      // i * 64 + j orders as i * n + j does: j < n <= 64
                k1 = ((unsigned long long)w << 12) | (unsigned)(p.to * ES_MAXN + p.from);
            }
        }
        keys[2 * k] = k0; keys[2 * k + 1] = k1;
    }
    __syncthreads();
    es_sort(keys, P, tid);

    // ---- 4: Kruskal (C:164-182) by wave 0, lane v = image v ----
    if (tid < WAVE) {
        const int lane = tid, E = 2 * sh[1];
        int comp = lane, dg = 0, te = 0;
        for (int base = 0; base < E && te < n - 1; base += WAVE) {
            const int mine = base + lane < E ? (int)(keys[base + lane] & 0xFFFull) : 0;
            const int m = min(WAVE, E - base);
            for (int e = 0; e < m && te < n - 1; ++e) {
                const int idx = __builtin_amdgcn_readlane(mine, e);      // e, a and b are uniform: scalar reads of a lane, no LDS crossbar
                const int a = idx >> 6, b = idx & (ES_MAXN - 1);
                const int ca = __builtin_amdgcn_readlane(comp, a), cb = __builtin_amdgcn_readlane(comp, b);
                if (ca != cb) {
                    if (comp == cb) comp = ca;
                    if (lane == a) adj[a * ES_MAXN + dg++] = (unsigned char)b;      // span_tree.addEdge(from, to), C:177
                    if (lane == b) adj[b * ES_MAXN + dg++] = (unsigned char)a;      // span_tree.addEdge(to, from), C:178
                    ++te;
                }
            }
        }
        deg[lane] = dg;
        if (lane == 0) sh[2] = te;
    }
    __syncthreads();

    // ---- 5: a breadth-first walk from every leaf (C:184-199), a lane each ----
    if (tid < n && deg[tid] == 1) {
        unsigned char* const q = bq + tid * ES_MAXN;
        unsigned char* const d = bd + tid * ES_MAXN;
        for (int j = 0; j < n; ++j) d[j] = 0;
        unsigned long long was = 1ull << tid;
        int head = 0, tail = 0;
        q[tail++] = (unsigned char)tid;
        while (head < tail) {
            const int v = q[head++];
            const int dv = deg[v];
            for (int e = 0; e < dv; ++e) {
                const int to = adj[v * ES_MAXN + e];
                if (!((was >> to) & 1ull)) {
                    d[to] = (unsigned char)(d[v] + 1);
                    was |= 1ull << to;
                    q[tail++] = (unsigned char)to;
                }
            }
        }
        for (int j = 0; j < n; ++j) atomicMax(&maxd[j], (int)d[j]);
    }
    __syncthreads();

    // ---- the centers (C:201-212) and the walk from the first (C:275): parent and depth ----
    if (tid == 0) {
        int mm = maxd[0];
        for (int i = 1; i < n; ++i) mm = min(mm, maxd[i]);
        int nc = 0, c0 = -1, c1 = -1;
        for (int i = 0; i < n; ++i)
            if (maxd[i] == mm) { if (nc == 0) c0 = i; else if (nc == 1) c1 = i; ++nc; }
        sh[4] = c0; sh[5] = c1; sh[6] = nc; sh2[0] = mm;
        int reached = 0, deepest = 0, status = sh[3];
        if (nc >= 1 && nc <= 2) {
            unsigned char* const q = bq;                     // the leaf walks are done with it
            unsigned long long was = 1ull << c0;
            int head = 0, tail = 0;
            q[tail++] = (unsigned char)c0;
            par[c0] = -1; dep[c0] = 0;
            while (head < tail) {
                const int v = q[head++];
                const int dv = deg[v];
                for (int e = 0; e < dv; ++e) {
                    const int to = adj[v * ES_MAXN + e];
                    if (!((was >> to) & 1ull)) {
                        par[to] = v; dep[to] = dep[v] + 1;
                        deepest = max(deepest, dep[to]);
                        was |= 1ull << to;
                        q[tail++] = (unsigned char)to;
                    }
                }
            }
            reached = tail;
            if (reached < n) status |= ES_ST_UNREACHED;
        } else {
            status |= ES_ST_ASSERT;
        }
        sh[3] = status; sh[7] = deepest; sh2[1] = reached;
    }
    __syncthreads();

    // ---- 6: CalcRotation (C:220-238): every edge's R by its own thread, then cameras[to].R = cameras[from].R * R level by level ----
    if (tid < n) {
#pragma unroll
        for (int e = 0; e < 9; ++e) R[9 * tid + e] = (e == 0 || e == 4 || e == 8) ? 1.0 : 0.0;
    }
    double re[9];
    const int my_par = tid < n ? par[tid] : -2, my_dep = tid < n ? dep[tid] : -1;
    if (my_par >= 0) {
        const int from = my_par, to = tid;
        const int k = slot[min(from, to) * ES_MAXN + max(from, to)];
        double h[9], hi[9], kf[9], kfi[9], kt[9], t[9];
        if (from < to) {
            const int row = prs[k].row;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double* src = row_ptr(c.H, 3ll * row + r, c.H_step);
                h[3 * r] = src[0]; h[3 * r + 1] = src[1]; h[3 * r + 2] = src[2];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 9; ++e) h[e] = dual[9ll * k + e];
        }
        es_inv3(h, hi);
        es_K(cam, from, kf);
        es_K(cam, to, kt);
        es_inv3(kf, kfi);
        es_mul3(kfi, hi, t);
        es_mul3(t, kt, re);
    }
    const int deepest = sh[7];
    __syncthreads();
    for (int lvl = 1; lvl <= deepest; ++lvl) {
        if (my_dep == lvl) {
            double rf[9], o[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) rf[e] = R[9 * my_par + e];
            es_mul3(rf, re, o);
#pragma unroll
            for (int e = 0; e < 9; ++e) R[9 * tid + e] = o[e];
        }
        __syncthreads();
    }

    // ---- the outputs: C:278-282, CameraParams::K() and the float32 of C:332 and C:386 ----
    if (tid < n) {
        const long long img = rig.img_first + tid;
        const double focal = cam[4 * tid], aspect = cam[4 * tid + 1];
        const double ppx = cam[4 * tid + 2] + (0.5 * (double)sizes[2 * tid]);
        const double ppy = cam[4 * tid + 3] + (0.5 * (double)sizes[2 * tid + 1]);
        double* const co = row_ptr(c.cams, img, c.cams_step);
        float* const ko = row_ptr(c.kr, img, c.kr_step);
        co[0] = focal; co[1] = aspect; co[2] = ppx; co[3] = ppy;
#pragma unroll
        for (int e = 0; e < 9; ++e) { const double v = R[9 * tid + e]; co[4 + e] = v; ko[9 + e] = (float)v; }
        co[13] = 0.0; co[14] = 0.0; co[15] = 0.0;
        ko[0] = (float)focal; ko[1] = 0.f; ko[2] = (float)ppx;
        ko[3] = 0.f; ko[4] = (float)(focal * aspect); ko[5] = (float)ppy;
        ko[6] = 0.f; ko[7] = 0.f; ko[8] = 1.f;
        int* const to = row_ptr(c.tree, img, c.tree_step);
        to[0] = my_par; to[1] = my_dep;
    }
    if (tid < 8) {
        int v = sh[3];
        v = tid == 1 ? sh[0] : v; v = tid == 2 ? sh[4] : v; v = tid == 3 ? sh[5] : v; v = tid == 4 ? sh[2] : v;
        v = tid == 5 ? sh2[1] : v; v = tid == 6 ? sh[6] : v; v = tid == 7 ? sh2[0] : v;
        row_ptr(c.rs, (long long)blockIdx.x, c.rs_step)[tid] = v;
    }
}

struct EsScratch : UploadScratch {};     // pin: the tables and the staged rows of host input mats (scratch.hpp)

int es_call(int num_images, const int* image_sizes_wh, int num_pairs, const int* pairs_from_to, int num_rigs, const int* rig_first, const isx_mat* H,
            const isx_mat* stats, const isx_mat* conf, const isx_mat* focals_in, isx_mat* cameras, isx_mat* kr32, isx_mat* tree, isx_mat* rig_stats,
            int* info, int device, void* hip_stream) {
    const char* who = "estimate_cameras";
    // ---- checks: all of them before anything is written or enqueued ----
    ISX_CHECK_ARG(image_sizes_wh && H && stats && conf && cameras && kr32 && tree && rig_stats, ISX_ERR_INVALID,
                  "%s: null image_sizes_wh, H, stats, conf, cameras, kr32, tree or rig_stats", who);
    ISX_CHECK_ARG(num_pairs >= 0 && (num_pairs == 0 || pairs_from_to), ISX_ERR_INVALID, "%s: %d pairs, or null pairs_from_to", who, num_pairs);
    ISX_CHECK_ARG(num_rigs >= 1 && (rig_first || num_rigs == 1), ISX_ERR_INVALID, "%s: %d rigs, or more than one without rig_first", who, num_rigs);
    ISX_CHECK_ARG(num_images >= 2, ISX_ERR_INVALID, "%s: %d images (C:84 indexes all_focals[-1] with one)", who, num_images);
    std::vector<int> first((size_t)num_rigs + 1);
    for (int r = 0; r <= num_rigs; ++r) first[r] = rig_first ? rig_first[r] : (r == 0 ? 0 : num_images);
    ISX_CHECK_ARG(first[0] == 0 && first[num_rigs] == num_images, ISX_ERR_INVALID, "%s: rig_first runs from %d to %d, not from 0 to %d", who, first[0],
                  first[num_rigs], num_images);
    for (int r = 0; r < num_rigs; ++r) {
        ISX_CHECK_ARG(first[r + 1] > first[r], ISX_ERR_INVALID, "%s: rig_first does not increase at rig %d", who, r);
        ISX_CHECK_ARG(first[r + 1] - first[r] >= 2, ISX_ERR_INVALID, "%s: rig %d has one image", who, r);
    }
    for (int r = 0; r < num_rigs; ++r)
        ISX_CHECK_ARG(first[r + 1] - first[r] <= ES_MAXN, ISX_ERR_UNSUPPORTED, "%s: rig %d has %d images, more than %d", who, r, first[r + 1] - first[r], ES_MAXN);
    std::vector<int> rig_of((size_t)num_images);
    for (int r = 0; r < num_rigs; ++r)
        for (int i = first[r]; i < first[r + 1]; ++i) rig_of[i] = r;
    std::vector<long long> seen((size_t)num_pairs);
    for (int p = 0; p < num_pairs; ++p) {
        const int a = pairs_from_to[2 * p], b = pairs_from_to[2 * p + 1];
        ISX_CHECK_ARG(a >= 0 && b >= 0 && a < num_images && b < num_images, ISX_ERR_INVALID, "%s: pair %d (%d, %d) is out of range", who, p, a, b);
        ISX_CHECK_ARG(a < b, ISX_ERR_INVALID, "%s: pair %d (%d, %d): from >= to", who, p, a, b);
        ISX_CHECK_ARG(rig_of[a] == rig_of[b], ISX_ERR_INVALID, "%s: pair %d (%d, %d) crosses rigs %d and %d", who, p, a, b, rig_of[a], rig_of[b]);
        seen[p] = (long long)a * num_images + b;
    }
    std::sort(seen.begin(), seen.end());
    ISX_CHECK_ARG(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), ISX_ERR_INVALID, "%s: a pair is listed twice", who);
    ISX_TRY(check_mat_holds(*H, ISX_64FC1, 3ll * num_pairs, 3, 8, STOP_NO_ROW_WANTED, device, who, "H", 0));
    ISX_TRY(check_mat_holds(*stats, ISX_32SC1, num_pairs, 2, 4, STOP_NO_ROW_WANTED, device, who, "stats", 0));
    ISX_TRY(check_mat_holds(*conf, ISX_64FC1, num_pairs > 0 ? 1 : 0, num_pairs, 8, STOP_NO_ROW_WANTED, device, who, "conf", 0));
    if (focals_in) ISX_TRY(check_mat_holds(*focals_in, ISX_64FC1, num_images, 4, 8, STOP_NO_ROW_WANTED, device, who, "focals_in", 0));
    ISX_TRY(check_mat_holds(*cameras, ISX_64FC1, num_images, 16, 8, STOP_NO_ROW_WANTED, device, who, "cameras", 0));
    ISX_TRY(check_mat_holds(*kr32, ISX_32FC1, num_images, 18, 4, STOP_NO_ROW_WANTED, device, who, "kr32", 0));
    ISX_TRY(check_mat_holds(*tree, ISX_32SC1, num_images, 2, 4, STOP_NO_ROW_WANTED, device, who, "tree", 0));
    ISX_TRY(check_mat_holds(*rig_stats, ISX_32SC1, num_rigs, 8, 4, STOP_NO_ROW_WANTED, device, who, "rig_stats", 0));
    ISX_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)hip_stream;
    ISX_TRY(refuse_capture(st, who, "the call uploads its tables and may stage host mats"));

    // ---- one buffer: [upload: rigs | pairs | sizes | staged host H, stats, focals_in] [the duals] [staged host outputs] ----
    std::vector<EsRig> rigs((size_t)num_rigs);
    std::vector<EsPair> prs((size_t)std::max(num_pairs, 1));
    for (int r = 0; r < num_rigs; ++r) rigs[r] = EsRig{first[r], first[r + 1] - first[r], 0, 0};
    for (int p = 0; p < num_pairs; ++p) ++rigs[rig_of[pairs_from_to[2 * p]]].pair_count;
    for (int r = 1; r < num_rigs; ++r) rigs[r].pair_first = rigs[r - 1].pair_first + rigs[r - 1].pair_count;
    std::vector<int> fill((size_t)num_rigs, 0);
    for (int p = 0; p < num_pairs; ++p) {                   // the caller's order inside each rig
        const int a = pairs_from_to[2 * p], b = pairs_from_to[2 * p + 1], r = rig_of[a];
        prs[(size_t)rigs[r].pair_first + fill[r]++] = EsPair{a - first[r], b - first[r], p, 0};
    }
    StagedMat m_H, m_stats, m_fin, m_cams, m_kr, m_tree, m_rs;
    Bump lay;
    const size_t o_rigs = lay.take(rigs.size() * sizeof(EsRig));
    const size_t o_prs = lay.take(prs.size() * sizeof(EsPair));
    const size_t o_sizes = lay.take((size_t)num_images * 8);
    m_H.plan(lay, *H, 3ll * num_pairs, 24);
    m_stats.plan(lay, *stats, num_pairs, 8);
    if (focals_in) m_fin.plan(lay, *focals_in, num_images, 32);
    const size_t upload_bytes = lay.at;
    const size_t o_dual = lay.take((size_t)std::max(num_pairs, 1) * 72);
    m_cams.plan(lay, *cameras, num_images, 128);
    m_kr.plan(lay, *kr32, num_images, 72);
    m_tree.plan(lay, *tree, num_images, 8);
    m_rs.plan(lay, *rig_stats, num_rigs, 32);

    EsScratch& s = per_thread<EsScratch>();
    ISX_TRY(s.begin(device, st, lay.at, upload_bytes));
    char* const dev = (char*)s.work.p;
    char* const pin = (char*)s.pin.p;
    std::memcpy(pin + o_rigs, rigs.data(), rigs.size() * sizeof(EsRig));
    std::memcpy(pin + o_prs, prs.data(), prs.size() * sizeof(EsPair));
    std::memcpy(pin + o_sizes, image_sizes_wh, (size_t)num_images * 8);
    m_H.fill(pin);
    m_stats.fill(pin);
    m_fin.fill(pin);
    ISX_TRY(s.upload(st, upload_bytes));

    // ---- one launch ----
    EsCall c;
    c.rigs = (const EsRig*)(dev + o_rigs); c.pairs = (const EsPair*)(dev + o_prs); c.sizes = (const int*)(dev + o_sizes);
    m_H.bind(dev, c.H, c.H_step);
    m_stats.bind(dev, c.stats, c.stats_step);
    c.fin = nullptr; c.fin_step = 0;
    if (focals_in) m_fin.bind(dev, c.fin, c.fin_step);
    c.dual = (double*)(dev + o_dual);
    m_cams.bind(dev, c.cams, c.cams_step);
    m_kr.bind(dev, c.kr, c.kr_step);
    m_tree.bind(dev, c.tree, c.tree_step);
    m_rs.bind(dev, c.rs, c.rs_step);
    ISX_LAUNCH("estimator_rigs", (double)num_pairs * 88.0 + (double)num_images * 216.0, st, k_es_rigs, dim3((unsigned)num_rigs), dim3(ES_THREADS), 0, c);
    ISX_TRY(s.ran(st));

    // ---- host outputs ----
    if (m_cams.staged || m_kr.staged || m_tree.staged || m_rs.staged) {
        ISX_TRY(m_cams.back(dev, num_images, st));
        ISX_TRY(m_kr.back(dev, num_images, st));
        ISX_TRY(m_tree.back(dev, num_images, st));
        ISX_TRY(m_rs.back(dev, num_rigs, st));
        ISX_HIP(hipStreamSynchronize(st));
    }
    if (info) { info[0] = num_rigs; info[1] = 1; }
    return ISX_OK;
}

}  // namespace

extern "C" {

int isx_estimator_release(void) ISX_ENTRY {
    clear_error();
    return per_thread<EsScratch>().release();
} ISX_EXIT("isx_estimator_release")

int isx_estimate_cameras(int num_images, const int* image_sizes_wh, int num_pairs, const int* pairs_from_to, int num_rigs, const int* rig_first,
                         const isx_mat* H, const isx_mat* stats, const isx_mat* conf, const isx_mat* focals_in, isx_mat* cameras, isx_mat* kr32,
                         isx_mat* tree, isx_mat* rig_stats, int* info, int device, void* hip_stream) ISX_ENTRY {
    clear_error();
    return es_call(num_images, image_sizes_wh, num_pairs, pairs_from_to, num_rigs, rig_first, H, stats, conf, focals_in, cameras, kr32, tree, rig_stats,
                   info, device, hip_stream);
} ISX_EXIT("isx_estimate_cameras")

}  // extern "C"
