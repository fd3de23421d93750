// match.hip — the features matcher of the M demo (the reference's 特征点匹配/特征点匹配/特征点匹配.cpp) on gfx950:
//   isx_match_features   BestOf2NearestMatcher1 matcher(false, 0.3f, 6, 6); matcher(features, pairwise_matches)      M:307-308
//                        = near_pairs M:131-135, CpuMatcher1::match M:232-289 per pair, the point gather M:164-179
//   isx_match_features_f32   the same over CV_32F descriptors of 1 .. 128 columns (M:237): exact L2 2-NN (DESIGN.md §8 "Features matcher,
//                        float descriptors"; tests/helpers/match_f32_np.py) - the kernels k_mf_pack / k_mf_search and the second
//                        instantiation of k_mt_finalise, the host code one template for both
//   isx_match_release    returns the per-thread scratch
//
// The specification (DESIGN.md §8 "Features matcher"; tests/helpers/match_np.py): exact 2-nearest neighbours by (Hamming distance, row)
// in both directions, the ratio test (float)d0 < k * (float)d1 with k = 1.f - match_conf, 1->2 matches in query order, then the 2->1
// matches 1->2 did not accept.  An accepted match has a unique nearest neighbour, so the list is that of any exact brute-force matcher;
// the FLANN LSH index of M:241-250 is not reproduced.
//
// At most three launches per call, however many pairs, no atomics, nothing read back on device mats:
//   k_mt_pack      the descriptors of every DEVICE mat, byte loads (any pointer and step), into one dense array of 8 dwords per row; host
//                  mats are packed on the host into the upload that carries the tables.  Every image is packed once, not once per pair.
//   k_mt_search    one block per work item (pair, direction, query block, train chunk): a thread owns one query row in 8 registers, the
//                  chunk's train rows pass through an LDS tile that every lane reads at the same address (a broadcast), a candidate costs
//                  8 xor + 8 accumulating popcounts and the update of the two smallest keys distance << 22 | row; the two keys of the
//                  chunk go to the partials.  Keys are unique per query, so the later merge is exact whatever the chunking.
//   k_mt_finalise  one block per pair: merges the partials, writes knn, runs the ratio test and - for 2->1 - the lookup "1->2 accepted
//                  this row with that neighbour", compacts in order with a ballot prefix scan and writes matches, points and the count.
#include <type_traits>

#include "isx_device.hpp"
#include "pairwise.hpp"
#include "scratch.hpp"

using namespace isx;
using namespace isxd;

namespace {

constexpr int MT_Q = ISX_MATCH_QUERY_BLOCK;      // queries (threads) per search block
constexpr int MT_T = ISX_MATCH_TRAIN_TILE;       // train rows per LDS tile
constexpr int MT_CHUNK = ISX_MATCH_TRAIN_CHUNK;  // train rows per work item (times a factor once an image passes MT_CHUNK * MT_MAX_SPLIT rows)
constexpr int MT_MAX_SPLIT = 32;                 // chunks per (pair, direction) at most: bounds the partials at 256 B per query
constexpr int MT_KEY_SHIFT = 22;
constexpr unsigned MT_IDX_MASK = (1u << MT_KEY_SHIFT) - 1u;
constexpr unsigned MT_NONE = 0xFFFFFFFFu;        // "no neighbour": above every key (a key is at most 256 << 22 | 2^22 - 1)
constexpr int MT_FIN_NT = 256;
constexpr int MT_PACK_ROWS = 32;                 // rows per block of k_mt_pack (8 threads a row)
static_assert(MT_T == MT_Q, "a thread of the search block stages one train row per tile");
static_assert(MT_CHUNK % MT_T == 0, "a chunk is whole tiles");
static_assert(ISX_MATCH_MAX_TOTAL_ROWS <= (1 << MT_KEY_SHIFT) && (256u << MT_KEY_SHIFT) < MT_NONE, "the packed key");

struct MtImage {
    const unsigned char* desc; long long desc_step;   // the caller's device mat (k_mt_pack); unused for a host mat
    const unsigned char* kp; long long kp_step;       // n x 2 floats: the caller's device mat or the staged copy of a host mat
    int rows, off;                                    // off: first row in the packed array
    float half_w, half_h;                             // img_size * 0.5f
};

struct MtPair {
    int from, to;                        // images
    int nchunks[2], chunk_rows[2];       // per direction (0: 1->2, the train set is image `to`)
    long long part_off[2];               // first entry (uint2; ulonglong2 for float descriptors) of the direction's partials: [query][chunk]
    long long acc_off;                   // n_from ints: the row 1->2 accepted for each query, or -1
    int* matches; long long matches_step;
    float* points; long long points_step;
    int* knn[2]; long long knn_step[2];
    int* count;
};

// blocks: (image, first row) per block
__global__ __launch_bounds__(MT_PACK_ROWS * 8) void k_mt_pack(const MtImage* __restrict__ imgs, const int2* __restrict__ blocks, unsigned* __restrict__ packed) {
    imgs = as_global(imgs); blocks = as_global(blocks); packed = as_global(packed);
    const int2 b = blocks[blockIdx.x];
    const MtImage& I = imgs[b.x];
    const int row = b.y + (int)(threadIdx.x >> 3), w = (int)(threadIdx.x & 7);
    if (row >= I.rows) return;
    const unsigned char* p = as_global(I.desc) + (long long)row * I.desc_step + 4 * w;
    const unsigned v = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
    packed[((size_t)I.off + row) * 8 + w] = v;
}

template <class K>
__device__ __forceinline__ void mt_update(K key, K& k0, K& k1) {
    k1 = min(k1, max(k0, key));
    k0 = min(k0, key);
}

// What k_mt_finalise needs of a key: the partials' type, "no neighbour", the train row, the int32 that knn and matches carry as the
// distance, and that distance as the float of the ratio test.
struct HamKey {                                      // distance << 22 | row
    typedef unsigned key_t;
    typedef uint2 part_t;
    static constexpr key_t NONE = MT_NONE;
    static __device__ __forceinline__ int row(key_t k) { return (int)(k & MT_IDX_MASK); }
    static __device__ __forceinline__ int carried(key_t k) { return (int)(k >> MT_KEY_SHIFT); }
    static __device__ __forceinline__ float dist(int carried) { return (float)carried; }
};
struct L2Key {                                       // bits(s) << 32 | row, s the squared distance (>= +0, so its bits order as an integer)
    typedef unsigned long long key_t;
    typedef ulonglong2 part_t;
    static constexpr key_t NONE = ~0ull;
    static __device__ __forceinline__ int row(key_t k) { return (int)(unsigned)k; }
    static __device__ __forceinline__ int carried(key_t k) { return __float_as_int(sqrtf(__uint_as_float((unsigned)(k >> 32)))); }      // bits(d), d = sqrtf(s) correctly rounded
    static __device__ __forceinline__ float dist(int carried) { return __int_as_float(carried); }
};

// work: (pair, direction, query block, train chunk) per block
__global__ __launch_bounds__(MT_Q) void k_mt_search(const MtPair* __restrict__ pairs, const MtImage* __restrict__ imgs, const int4* __restrict__ work,
                                                    const uint4* __restrict__ packed, uint2* __restrict__ partial) {
    __shared__ uint4 s_tile[2 * MT_T];
    pairs = as_global(pairs); imgs = as_global(imgs); work = as_global(work); packed = as_global(packed); partial = as_global(partial);
    const int4 wi = work[blockIdx.x];
    const MtPair& P = pairs[wi.x];
    const int dir = wi.y, t = (int)threadIdx.x;
    const MtImage& Q = imgs[dir ? P.to : P.from];
    const MtImage& R = imgs[dir ? P.from : P.to];
    const int nq = Q.rows, nt = R.rows, nch = P.nchunks[dir], crows = P.chunk_rows[dir];
    const int q = wi.z * MT_Q + t;
    uint4 qa = make_uint4(0u, 0u, 0u, 0u), qb = qa;
    if (q < nq) { qa = packed[2 * ((size_t)Q.off + q)]; qb = packed[2 * ((size_t)Q.off + q) + 1]; }
    const int t0 = wi.w * crows, t1 = min(nt, t0 + crows);       // t0 < nt: the host makes no empty chunk
    unsigned k0 = MT_NONE, k1 = MT_NONE;
    for (int tb = t0; tb < t1; tb += MT_T) {
        __syncthreads();                                          // the previous tile's readers are done
        if (tb + t < t1) { s_tile[2 * t] = packed[2 * ((size_t)R.off + tb + t)]; s_tile[2 * t + 1] = packed[2 * ((size_t)R.off + tb + t) + 1]; }
        __syncthreads();
        const int n = min(MT_T, t1 - tb);
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const uint4 a = s_tile[2 * j], b = s_tile[2 * j + 1];
            unsigned d = __popc(qa.x ^ a.x);
            d += __popc(qa.y ^ a.y); d += __popc(qa.z ^ a.z); d += __popc(qa.w ^ a.w);
            d += __popc(qb.x ^ b.x); d += __popc(qb.y ^ b.y); d += __popc(qb.z ^ b.z); d += __popc(qb.w ^ b.w);
            mt_update((d << MT_KEY_SHIFT) | (unsigned)(tb + j), k0, k1);
        }
    }
    if (q < nq) partial[P.part_off[dir] + (long long)q * nch + wi.w] = make_uint2(k0, k1);
}

// ---- float descriptors: rows of W floats (64 where cols <= 64, else 128), zero-padded - s + 0 * 0 is s, so the padding changes no bit ----
constexpr int MF_T = ISX_MATCH_F32_TRAIN_TILE;   // train rows per LDS tile: 8 / 16 KiB, so that several blocks share a CU's LDS
constexpr int MF_U = 4;                          // candidates in flight: independent chains of sub, mul, add hide the add's latency
constexpr int MF_G = 2;                          // float4s of a candidate read from the LDS ahead of their arithmetic
static_assert(MT_CHUNK % MF_T == 0 && MF_T % MF_U == 0, "a chunk is whole tiles, a tile whole groups of candidates");

// blocks: (image, first row) per block, as for k_mt_pack; a wave copies a row, dword loads at any 4-aligned step
__global__ __launch_bounds__(MT_PACK_ROWS * 8) void k_mf_pack(const MtImage* __restrict__ imgs, const int2* __restrict__ blocks, float* __restrict__ packed, int cols, int W) {
    imgs = as_global(imgs); blocks = as_global(blocks); packed = as_global(packed);
    const int2 b = blocks[blockIdx.x];
    const MtImage& I = imgs[b.x];
    for (int r = (int)(threadIdx.x >> 6); r < MT_PACK_ROWS; r += (MT_PACK_ROWS * 8) >> 6) {
        const int row = b.y + r;
        if (row >= I.rows) break;
        const float* p = (const float*)(as_global(I.desc) + (long long)row * I.desc_step);
        for (int c = (int)(threadIdx.x & 63); c < W; c += 64) packed[((size_t)I.off + row) * W + c] = c < cols ? p[c] : 0.f;
    }
}

// work: (pair, direction, query block, train chunk) per block, as for k_mt_search.  A thread owns one query row in W registers; the tile's
// rows are read by all lanes at one address (ds_read_b128 broadcasts).  s = 0, then s = s + e * e for c = 0 .. W - 1 in that order, e =
// a[c] - b[c], every operation rounded on its own (-ffp-contract=off); an s that is not finite becomes +inf.
template <int W>
__global__ __launch_bounds__(MT_Q) void k_mf_search(const MtPair* __restrict__ pairs, const MtImage* __restrict__ imgs, const int4* __restrict__ work,
                                                    const float4* __restrict__ packed, ulonglong2* __restrict__ partial) {
    constexpr int V = W / 4;                                      // float4s a row
    __shared__ float4 s_tile[MF_T * V];
    pairs = as_global(pairs); imgs = as_global(imgs); work = as_global(work); packed = as_global(packed); partial = as_global(partial);
    const int4 wi = work[blockIdx.x];
    const MtPair& P = pairs[wi.x];
    const int dir = wi.y, t = (int)threadIdx.x;
    const MtImage& Q = imgs[dir ? P.to : P.from];
    const MtImage& R = imgs[dir ? P.from : P.to];
    const int nq = Q.rows, nt = R.rows, nch = P.nchunks[dir], crows = P.chunk_rows[dir];
    const int q = wi.z * MT_Q + t;
    float4 qv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) qv[v] = q < nq ? packed[((size_t)Q.off + q) * V + v] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int t0 = wi.w * crows, t1 = min(nt, t0 + crows);       // t0 < nt: the host makes no empty chunk
    unsigned long long k0 = L2Key::NONE, k1 = L2Key::NONE;
    for (int tb = t0; tb < t1; tb += MF_T) {
        __syncthreads();                                          // the previous tile's readers are done
        for (int i = t; i < MF_T * V; i += MT_Q)                  // rows past the chunk's end are zeros: computed, never kept
            s_tile[i] = tb + i / V < t1 ? packed[((size_t)R.off + tb) * V + i] : make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
        const int n = min(MF_T, t1 - tb);
#pragma unroll 1
        for (int j = 0; j < n; j += MF_U) {
            float s[MF_U];
#pragma unroll
            for (int u = 0; u < MF_U; ++u) s[u] = 0.f;
            // groups of MF_G float4s a candidate: the next group's LDS reads are issued before this group's arithmetic and no further
            // ahead (the fence), so the tile's values in flight stay at 2 * MF_U * MF_G float4s beside the query row - no spill
            float4 cur[MF_U][MF_G], nxt[MF_U][MF_G];
#pragma unroll
            for (int u = 0; u < MF_U; ++u)
#pragma unroll
                for (int g = 0; g < MF_G; ++g) cur[u][g] = s_tile[(j + u) * V + g];
#pragma unroll
            for (int v0 = 0; v0 < V; v0 += MF_G) {
                if (v0 + MF_G < V) {
#pragma unroll
                    for (int u = 0; u < MF_U; ++u)
#pragma unroll
                        for (int g = 0; g < MF_G; ++g) nxt[u][g] = s_tile[(j + u) * V + v0 + MF_G + g];
                }
#pragma unroll
                for (int g = 0; g < MF_G; ++g) {
#pragma unroll
                    for (int u = 0; u < MF_U; ++u) {
                        const float4 a = cur[u][g], b = qv[v0 + g];
                        float e;
                        e = b.x - a.x; s[u] = s[u] + e * e;
                        e = b.y - a.y; s[u] = s[u] + e * e;
                        e = b.z - a.z; s[u] = s[u] + e * e;
                        e = b.w - a.w; s[u] = s[u] + e * e;
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < MF_U; ++u)
#pragma unroll
                    for (int g = 0; g < MF_G; ++g) cur[u][g] = nxt[u][g];
            }
#pragma unroll
            for (int u = 0; u < MF_U; ++u) {
                const float sv = s[u] <= 3.402823466e38f ? s[u] : __uint_as_float(0x7F800000u);      // NaN and overflow: +inf
                const unsigned long long key = ((unsigned long long)__float_as_uint(sv) << 32) | (unsigned)(tb + j + u);
                mt_update(j + u < n ? key : L2Key::NONE, k0, k1);      // a select, not a branch: the MF_U chains stay interleaved
            }
        }
    }
    if (q < nq) partial[P.part_off[dir] + (long long)q * nch + wi.w] = make_ulonglong2(k0, k1);
}

template <class K>
__global__ __launch_bounds__(MT_FIN_NT) void k_mt_finalise(const MtPair* __restrict__ pairs, const MtImage* __restrict__ imgs,
                                                           const typename K::part_t* __restrict__ partial,
                                                           int* acc, float k) {
    __shared__ int s_cnt[MT_FIN_NT / WAVE];
    pairs = as_global(pairs); imgs = as_global(imgs); partial = as_global(partial); acc = as_global(acc);
    const MtPair& P = pairs[blockIdx.x];
    const MtImage& F = imgs[P.from];
    const MtImage& T = imgs[P.to];
    const int t = (int)threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
    if (F.rows == 0 || T.rows == 0) {                            // M:134: not a near pair
        if (t == 0) *as_global(P.count) = 0;
        return;
    }
    int* accp = acc + P.acc_off;
    int* const mrows = as_global(P.matches);
    float* const prows = as_global(P.points);
    const unsigned char* const kpf = as_global(F.kp);
    const unsigned char* const kpt = as_global(T.kp);
    int base = 0;
    for (int dir = 0; dir < 2; ++dir) {
        const int nq = dir ? T.rows : F.rows, nt = dir ? F.rows : T.rows, nch = P.nchunks[dir];
        const typename K::part_t* part = partial + P.part_off[dir];
        int* knn = as_global(P.knn[dir]);
        for (int q0 = 0; q0 < nq; q0 += MT_FIN_NT) {
            const int q = q0 + t;
            bool ok = false;
            int i0 = -1, d0 = -1;
            if (q < nq) {
                typename K::key_t k0 = K::NONE, k1 = K::NONE;
                for (int c = 0; c < nch; ++c) {
                    const typename K::part_t p = part[(long long)q * nch + c];
                    mt_update<typename K::key_t>(p.x, k0, k1); mt_update<typename K::key_t>(p.y, k0, k1);
                }
                const int i1 = k1 == K::NONE ? -1 : K::row(k1), d1 = k1 == K::NONE ? -1 : K::carried(k1);
                i0 = k0 == K::NONE ? -1 : K::row(k0); d0 = k0 == K::NONE ? -1 : K::carried(k0);
                if (knn) {
                    int* o = (int*)((char*)knn + (long long)q * P.knn_step[dir]);
                    o[0] = i0; o[1] = d0; o[2] = i1; o[3] = d1;
                }
                if (nt >= 2) ok = K::dist(d0) < k * K::dist(d1); // M:260, M:267 (-ffp-contract=off: one rounded multiply)
                if (dir == 0) accp[q] = ok ? i0 : -1;
                else if (ok) ok = accp[i0] != q;                 // M:285
            }
            const unsigned long long bal = __ballot(ok);
            if (lane == 0) s_cnt[wv] = __popcll(bal);
            __syncthreads();
            int pos = base + __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
            for (int i = 0; i < MT_FIN_NT / WAVE; ++i) { pos += i < wv ? s_cnt[i] : 0; total += s_cnt[i]; }
            base += total;
            if (ok) {
                const int a = dir ? i0 : q, b = dir ? q : i0;    // rows of `from` and of `to`: M:270, M:286
                int* o = (int*)((char*)mrows + (long long)pos * P.matches_step);
                o[0] = a; o[1] = b; o[2] = d0;
                if (prows) {
                    const float* pa = (const float*)(kpf + (long long)a * F.kp_step);
                    const float* pb = (const float*)(kpt + (long long)b * T.kp_step);
                    float* op = (float*)((char*)prows + (long long)pos * P.points_step);
                    op[0] = pa[0] - F.half_w; op[1] = pa[1] - F.half_h;      // M:170-173
                    op[2] = pb[0] - T.half_w; op[3] = pb[1] - T.half_h;      // M:175-178
                }
            }
            __syncthreads();                                      // s_cnt is rewritten by the next step; acc is complete before 2->1 reads it
        }
    }
    if (t == 0) *as_global(P.count) = base;
}

struct MtScratch : UploadScratch {};      // pin: the tables, staged keypoints and packed descriptors of host mats (scratch.hpp)

// Both entries: K = HamKey over n x 32 CV_8UC1 rows (32 bytes a packed row), K = L2Key over n x cols CV_32FC1 rows (W floats a packed row).
template <class K>
int match_entry(const char* who, int num_images, const isx_mat* descriptors, const isx_mat* keypoints, const int* image_sizes_wh,
                int num_pairs, const int* pairs_ij, float match_conf, isx_mat* matches, isx_mat* points, isx_mat* counts,
                isx_mat* knn, int* info, int device, void* hip_stream) {
    constexpr bool F32 = std::is_same<K, L2Key>::value;
    // ---- checks: all of them before anything is written or enqueued ----
    ISX_CHECK_ARG(num_images >= 0 && num_pairs >= 0, ISX_ERR_INVALID, "%s: %d images, %d pairs", who, num_images, num_pairs);
    ISX_CHECK_ARG(num_images == 0 || descriptors, ISX_ERR_INVALID, "%s: null descriptors", who);
    ISX_CHECK_ARG(num_pairs == 0 || (pairs_ij && matches && counts), ISX_ERR_INVALID, "%s: null pairs, matches or counts", who);
    ISX_CHECK_ARG(!keypoints || image_sizes_wh, ISX_ERR_INVALID, "%s: keypoints without image sizes", who);
    ISX_CHECK_ARG(!points || keypoints, ISX_ERR_INVALID, "%s: points without keypoints", who);
    ISX_CHECK_ARG(match_conf >= 0.f && match_conf < 1.f, ISX_ERR_INVALID, "%s: match_conf %g is not in [0, 1)", who, (double)match_conf);
    for (int p = 0; p < num_pairs; ++p) {
        const int i = pairs_ij[2 * p], j = pairs_ij[2 * p + 1];
        ISX_CHECK_ARG(i >= 0 && i < j && j < num_images, ISX_ERR_INVALID, "%s: pair %d is (%d, %d) of %d images (from < to)", who, p, i, j, num_images);
    }
    long long total_rows = 0;
    int cols = 0;                                                 // of the images with rows (float descriptors: one width a call)
    for (int i = 0; i < num_images; ++i) {
        const isx_mat& m = descriptors[i];
        ISX_CHECK_ARG(m.type == (F32 ? ISX_32FC1 : ISX_8UC1), ISX_ERR_TYPE, "%s: descriptors %d are %s (%s)", who, i, type_name(m.type), F32 ? "CV_32FC1" : "CV_8UC1");
        ISX_CHECK_ARG(m.rows >= 0, ISX_ERR_INVALID, "%s: descriptors %d have %d rows", who, i, m.rows);
        if (m.rows > 0) {
            if (F32) {
                ISX_CHECK_ARG(m.cols >= 1, ISX_ERR_INVALID, "%s: descriptors %d have %d columns", who, i, m.cols);
                ISX_CHECK_ARG(m.cols <= ISX_MATCH_F32_MAX_COLS, ISX_ERR_UNSUPPORTED, "%s: descriptors %d have %d columns (at most %d)", who, i, m.cols, ISX_MATCH_F32_MAX_COLS);
                ISX_CHECK_ARG(cols == 0 || m.cols == cols, ISX_ERR_SIZE, "%s: descriptors %d have %d columns, those before %d", who, i, m.cols, cols);
                cols = m.cols;
            } else {
                // binary descriptors of another length are not built
                ISX_CHECK_ARG(m.cols == 32, ISX_ERR_UNSUPPORTED, "%s: descriptors %d have %d columns (32-byte ORB descriptors only)", who, i, m.cols);
                cols = 32;
            }
            ISX_CHECK_ARG(m.rows <= ISX_MATCH_MAX_ROWS, ISX_ERR_UNSUPPORTED, "%s: descriptors %d have %d rows (at most %d)", who, i, m.rows, ISX_MATCH_MAX_ROWS);
            ISX_CHECK_ARG(m.data != nullptr, ISX_ERR_INVALID, "%s: descriptors %d have a null data pointer", who, i);
            ISX_CHECK_ARG(m.step >= (size_t)cols * (F32 ? 4 : 1) || m.rows == 1, ISX_ERR_INVALID, "%s: descriptors %d: step %zu smaller than a row", who, i, m.step);
            if (F32)
                ISX_CHECK_ARG(((uintptr_t)m.data & 3) == 0 && (m.step & 3) == 0, ISX_ERR_INVALID, "%s: descriptors %d are not 4-byte aligned in pointer and step", who, i);
            ISX_CHECK_ARG(m.device < 0 || m.device == device, ISX_ERR_INVALID, "%s: descriptors %d live on device %d, the call runs on %d", who, i, m.device, device);
        }
        total_rows += m.rows;
        if (keypoints) {
            const isx_mat& kp = keypoints[i];
            ISX_CHECK_ARG(kp.type == ISX_32FC1, ISX_ERR_TYPE, "%s: keypoints %d are %s (CV_32FC1)", who, i, type_name(kp.type));
            ISX_CHECK_ARG(kp.rows == m.rows && (m.rows == 0 || kp.cols == 2), ISX_ERR_SIZE, "%s: keypoints %d are %d x %d, the descriptors have %d rows", who, i,
                          kp.rows, kp.cols, m.rows);
            if (m.rows > 0) {
                ISX_CHECK_ARG(kp.data != nullptr && (kp.step >= 8 || kp.rows == 1), ISX_ERR_INVALID, "%s: keypoints %d: null data or a step smaller than a row", who, i);
                ISX_CHECK_ARG(((uintptr_t)kp.data & 3) == 0 && (kp.step & 3) == 0, ISX_ERR_INVALID, "%s: keypoints %d are not 4-byte aligned in pointer and step", who, i);
                ISX_CHECK_ARG(kp.device < 0 || kp.device == device, ISX_ERR_INVALID, "%s: keypoints %d live on device %d, the call runs on %d", who, i, kp.device, device);
            }
        }
    }
    ISX_CHECK_ARG(total_rows <= ISX_MATCH_MAX_TOTAL_ROWS, ISX_ERR_UNSUPPORTED, "%s: %lld descriptor rows in all (at most %d)", who, total_rows, ISX_MATCH_MAX_TOTAL_ROWS);
    int searched = 0;
    if (num_pairs > 0) ISX_TRY(check_mat_holds(*counts, ISX_32SC1, 1, num_pairs, 4, STOP_NO_ROW_WANTED, device, who, "counts", 0));
    for (int p = 0; p < num_pairs; ++p) {
        const int nf = descriptors[pairs_ij[2 * p]].rows, nt = descriptors[pairs_ij[2 * p + 1]].rows;
        const bool run = nf > 0 && nt > 0;
        const long long rows = run ? (long long)nf + nt : 0;
        searched += run;
        ISX_TRY(check_mat_holds(matches[p], ISX_32SC1, rows, 3, 4, STOP_NO_ROW_WANTED, device, who, "matches", p));
        if (points) ISX_TRY(check_mat_holds(points[p], ISX_32FC1, rows, 4, 4, STOP_NO_ROW_WANTED, device, who, "points", p));
        if (knn)
            for (int d = 0; d < 2; ++d)
                ISX_TRY(check_mat_holds(knn[2 * p + d], ISX_32SC1, run ? (d ? nt : nf) : 0, 4, 4, STOP_NO_ROW_WANTED, device, who, "knn", 2 * p + d));
    }
    ISX_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)hip_stream;
    ISX_TRY(refuse_capture(st, who, "the call uploads its tables and may stage host mats"));
    if (num_pairs == 0) {
        if (info) { info[0] = 0; info[1] = 0; }
        return ISX_OK;
    }

    // ---- the plan: packed rows (host mats first: they travel in the upload), chunking, work items ----
    const int W = cols <= 64 ? 64 : 128;                          // floats a packed row (float descriptors)
    const size_t row_bytes = F32 ? (size_t)W * 4 : 32;
    std::vector<MtImage> imgs((size_t)num_images);
    int host_rows = 0, dev_rows = 0;
    for (int i = 0; i < num_images; ++i)
        if (descriptors[i].rows > 0 && descriptors[i].device < 0) { imgs[i].off = host_rows; host_rows += descriptors[i].rows; }
    std::vector<int2> pack_blocks;
    for (int i = 0; i < num_images; ++i) {
        const isx_mat& m = descriptors[i];
        MtImage& I = imgs[i];
        I.rows = m.rows; I.desc = nullptr; I.desc_step = 0; I.kp = nullptr; I.kp_step = 0; I.half_w = I.half_h = 0.f;
        if (m.rows == 0) { I.off = 0; continue; }
        if (m.device >= 0) {
            I.off = host_rows + dev_rows; dev_rows += m.rows;
            I.desc = (const unsigned char*)m.data; I.desc_step = (long long)m.step;
            for (int r = 0; r < m.rows; r += MT_PACK_ROWS) pack_blocks.push_back(make_int2(i, r));
        }
        if (keypoints) { I.half_w = (float)image_sizes_wh[2 * i] * 0.5f; I.half_h = (float)image_sizes_wh[2 * i + 1] * 0.5f; }
    }
    std::vector<MtPair> prs((size_t)num_pairs);
    std::vector<int4> work;
    long long part_count = 0, acc_count = 0;
    for (int p = 0; p < num_pairs; ++p) {
        MtPair& P = prs[p];
        std::memset(&P, 0, sizeof(P));
        P.from = pairs_ij[2 * p]; P.to = pairs_ij[2 * p + 1];
        const int n[2] = {imgs[P.from].rows, imgs[P.to].rows};
        if (n[0] == 0 || n[1] == 0) continue;
        P.acc_off = acc_count; acc_count += n[0];
        for (int d = 0; d < 2; ++d) {
            const int nq = n[d], nt = n[1 - d];
            // MT_CHUNK rows a work item until an image passes MT_CHUNK * MT_MAX_SPLIT rows, whole multiples of it from there
            P.chunk_rows[d] = MT_CHUNK * cdiv(nt, MT_CHUNK * MT_MAX_SPLIT);
            P.nchunks[d] = cdiv(nt, P.chunk_rows[d]);
            P.part_off[d] = part_count; part_count += (long long)nq * P.nchunks[d];
            for (int qb = 0; qb < cdiv(nq, MT_Q); ++qb)
                for (int c = 0; c < P.nchunks[d]; ++c) work.push_back(make_int4(p, d, qb, c));
        }
    }
    ISX_CHECK_ARG(work.size() <= (size_t)INT_MAX, ISX_ERR_UNSUPPORTED, "%s: %zu work items", who, work.size());

    // ---- one buffer: [upload: tables | staged keypoints of host mats | packed rows of host mats] [packed rows of device mats] [partials] [acc]
    //      [staged host outputs]
    Bump lay;
    const size_t o_imgs = lay.take(imgs.size() * sizeof(MtImage)), o_prs = lay.take(prs.size() * sizeof(MtPair));
    const size_t o_work = lay.take(work.size() * sizeof(int4)), o_pblk = lay.take(pack_blocks.size() * sizeof(int2));
    std::vector<StagedMat> m_kp((size_t)num_images);
    if (keypoints)
        for (int i = 0; i < num_images; ++i) m_kp[i].plan(lay, keypoints[i], imgs[i].rows, 8);
    const size_t o_packed = lay.take(0);
    const size_t upload_bytes = o_packed + (size_t)host_rows * row_bytes;
    lay.take((size_t)(host_rows + dev_rows) * row_bytes);
    const size_t o_part = lay.take((size_t)part_count * sizeof(typename K::part_t)), o_acc = lay.take((size_t)acc_count * sizeof(int));
    StagedMat m_counts;
    m_counts.plan(lay, *counts, 1, (size_t)num_pairs * 4);
    std::vector<StagedMat> m_m((size_t)num_pairs), m_p((size_t)num_pairs), m_k((size_t)2 * num_pairs);
    bool any_host_out = m_counts.staged;
    for (int p = 0; p < num_pairs; ++p) {
        const int nf = imgs[prs[p].from].rows, nt = imgs[prs[p].to].rows;
        if (nf == 0 || nt == 0) continue;
        m_m[p].plan(lay, matches[p], nf + nt, 12);
        if (points) m_p[p].plan(lay, points[p], nf + nt, 16);
        if (knn)
            for (int d = 0; d < 2; ++d) m_k[2 * p + d].plan(lay, knn[2 * p + d], d ? nt : nf, 16);
        any_host_out |= m_m[p].staged || m_p[p].staged || m_k[2 * p].staged || m_k[2 * p + 1].staged;
    }

    MtScratch& s = per_thread<MtScratch>();
    ISX_TRY(s.begin(device, st, lay.at, upload_bytes));
    char* const dev = (char*)s.work.p;
    char* const pin = (char*)s.pin.p;

    // ---- fill the upload ----
    for (int i = 0; i < num_images; ++i) {
        MtImage& I = imgs[i];
        if (I.rows == 0) continue;
        const isx_mat& m = descriptors[i];
        if (m.device < 0)
            for (int r = 0; r < m.rows; ++r) {
                char* const row = pin + o_packed + ((size_t)I.off + r) * row_bytes;
                const size_t have = F32 ? (size_t)cols * 4 : 32;
                std::memcpy(row, (const char*)m.data + (size_t)r * m.step, have);
                std::memset(row + have, 0, row_bytes - have);
            }
        if (!keypoints) continue;
        m_kp[i].fill(pin);
        m_kp[i].bind(dev, I.kp, I.kp_step);
    }
    int* d_counts;
    m_counts.bind(dev, d_counts);
    for (int p = 0; p < num_pairs; ++p) {
        MtPair& P = prs[p];
        P.count = d_counts + p;
        if (imgs[P.from].rows == 0 || imgs[P.to].rows == 0) continue;
        m_m[p].bind(dev, P.matches, P.matches_step);
        if (points) m_p[p].bind(dev, P.points, P.points_step);
        if (knn)
            for (int d = 0; d < 2; ++d) m_k[2 * p + d].bind(dev, P.knn[d], P.knn_step[d]);
    }
    std::memcpy(pin + o_imgs, imgs.data(), imgs.size() * sizeof(MtImage));
    std::memcpy(pin + o_prs, prs.data(), prs.size() * sizeof(MtPair));
    std::memcpy(pin + o_work, work.data(), work.size() * sizeof(int4));
    std::memcpy(pin + o_pblk, pack_blocks.data(), pack_blocks.size() * sizeof(int2));
    ISX_TRY(s.upload(st, upload_bytes));

    // ---- at most three launches ----
    const MtImage* d_imgs = (const MtImage*)(dev + o_imgs);
    const MtPair* d_prs = (const MtPair*)(dev + o_prs);
    int launches = 0;
    if (!pack_blocks.empty()) {
        if (F32)
            ISX_LAUNCH("match_f32_pack", (double)dev_rows * (cols * 4.0 + (double)row_bytes), st, k_mf_pack, dim3((unsigned)pack_blocks.size()), dim3(MT_PACK_ROWS * 8), 0,
                       d_imgs, (const int2*)(dev + o_pblk), (float*)(dev + o_packed), cols, W);
        else
            ISX_LAUNCH("match_pack", (double)dev_rows * 64.0, st, k_mt_pack, dim3((unsigned)pack_blocks.size()), dim3(MT_PACK_ROWS * 8), 0, d_imgs,
                       (const int2*)(dev + o_pblk), (unsigned*)(dev + o_packed));
        ++launches;
    }
    if (!work.empty()) {
        if (!F32)
            ISX_LAUNCH("match_search", (double)work.size() * (MT_Q + MT_CHUNK) * 32.0, st, k_mt_search, dim3((unsigned)work.size()), dim3(MT_Q), 0, d_prs, d_imgs,
                       (const int4*)(dev + o_work), (const uint4*)(dev + o_packed), (uint2*)(dev + o_part));
        else if (W == 64)
            ISX_LAUNCH("match_f32_search", (double)work.size() * (MT_Q + MT_CHUNK) * 256.0, st, k_mf_search<64>, dim3((unsigned)work.size()), dim3(MT_Q), 0, d_prs,
                       d_imgs, (const int4*)(dev + o_work), (const float4*)(dev + o_packed), (ulonglong2*)(dev + o_part));
        else
            ISX_LAUNCH("match_f32_search", (double)work.size() * (MT_Q + MT_CHUNK) * 512.0, st, k_mf_search<128>, dim3((unsigned)work.size()), dim3(MT_Q), 0, d_prs,
                       d_imgs, (const int4*)(dev + o_work), (const float4*)(dev + o_packed), (ulonglong2*)(dev + o_part));
        ++launches;
    }
    const float k = 1.f - match_conf;
    ISX_LAUNCH(F32 ? "match_f32_finalise" : "match_finalise", (double)part_count * sizeof(typename K::part_t), st, k_mt_finalise<K>, dim3((unsigned)num_pairs),
               dim3(MT_FIN_NT), 0, d_prs, d_imgs, (const typename K::part_t*)(dev + o_part), (int*)(dev + o_acc), k);
    ++launches;
    ISX_TRY(s.ran(st));

    // ---- host outputs: the counts first, then the rows they name ----
    if (any_host_out) {
        std::vector<int> cnt_tmp(m_counts.staged ? 0 : (size_t)num_pairs);      // a host counts mat takes them itself
        int* const cnt = m_counts.staged ? (int*)counts->data : cnt_tmp.data();
        ISX_TRY(counts_to_host(cnt, d_counts, num_pairs, st));
        for (int p = 0; p < num_pairs; ++p) {
            ISX_TRY(m_m[p].back(dev, cnt[p], st));
            ISX_TRY(m_p[p].back(dev, cnt[p], st));
            for (int d = 0; d < 2; ++d) ISX_TRY(m_k[2 * p + d].back(dev, m_k[2 * p + d].rows, st));
        }
        ISX_HIP(hipStreamSynchronize(st));
    }
    if (info) { info[0] = searched; info[1] = launches; }
    return ISX_OK;
}

}  // namespace

extern "C" {

int isx_match_release(void) ISX_ENTRY {
    clear_error();
    return per_thread<MtScratch>().release();
} ISX_EXIT("isx_match_release")

int isx_match_features(int num_images, const isx_mat* descriptors, const isx_mat* keypoints, const int* image_sizes_wh,
                       int num_pairs, const int* pairs_ij, float match_conf, isx_mat* matches, isx_mat* points, isx_mat* counts,
                       isx_mat* knn, int* info, int device, void* hip_stream) ISX_ENTRY {
    clear_error();
    return match_entry<HamKey>("match_features", num_images, descriptors, keypoints, image_sizes_wh, num_pairs, pairs_ij, match_conf, matches, points, counts, knn,
                               info, device, hip_stream);
} ISX_EXIT("isx_match_features")

int isx_match_features_f32(int num_images, const isx_mat* descriptors, const isx_mat* keypoints, const int* image_sizes_wh,
                           int num_pairs, const int* pairs_ij, float match_conf, isx_mat* matches, isx_mat* points, isx_mat* counts,
                           isx_mat* knn, int* info, int device, void* hip_stream) ISX_ENTRY {
    clear_error();
    return match_entry<L2Key>("match_features_f32", num_images, descriptors, keypoints, image_sizes_wh, num_pairs, pairs_ij, match_conf, matches, points, counts,
                              knn, info, device, hip_stream);
} ISX_EXIT("isx_match_features_f32")

}  // extern "C"
