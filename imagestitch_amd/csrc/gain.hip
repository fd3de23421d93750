// gain.hip — GainCompensator::feed (OpenCV 3.4.2 stitching/src/exposure_compensate.cpp) on gfx950:
//   isx_gain_compensator_feed   compensator->feed(corners, images_warped, masks_warped)   W:238-240, S:1165-1167, B:117-119
//
// What feed computes, restated from OpenCV 3.4.2 (the source is not in the reference tree; DESIGN.md §1 "exposure compensation"):
//   for every pair i <= j (i == j included) with a non-empty overlapRoi(corners[i], corners[j], sizes):
//     intersect = (mask_i == 255) & (mask_j == 255) over the overlap       (the public feed wraps every mask as pair(mask, 255))
//     N(i,j) = N(j,i) = max(1, countNonZero(intersect))
//     I(i,j) = sum over intersect of sqrt((double)(r^2 + g^2 + b^2)) of image i / N(i,j);  I(j,i) the same of image j
//   N and I start at 0, so a pair whose overlapRoi is empty keeps N = 0, I = 0 (an empty intersect inside a non-empty overlap gives
//   N = 1, I = 0).  Then, alpha = 0.01, beta = 100, for every i, j:
//     b(i) += beta N(i,j);  A(i,i) += beta N(i,j);  and for j != i:  A(i,i) += 2 alpha I(i,j)^2 N(i,j);  A(i,j) -= 2 alpha I(i,j) I(j,i) N(i,j)
//   gains = solve(A, b, DECOMP_LU).
//
// The pixel part is ONE launch over a table of work items (a band of rows of one pair's overlap).  A diagonal pair only needs N(i,i)
// (I(i,i) never enters A or b): its items read the mask alone, in aligned 16-byte chunks.  An off-diagonal item reads both masks and
// both CV_8UC3 tiles, four pixels per lane, from the enclosing aligned dwords (v_alignbyte), so a view may start anywhere and have any
// pitch.  Every load is of an aligned dword or 16-byte chunk that holds at least one byte of the view: it never leaves the view's pages.
//
// The sums are exact and order-free: a term other than 0 lies in [1, 2^9), so term * 2^52 is an integer below 2^61 (its last 52 - 8
// bits may be set, none below 2^0).  It is split into two limbs, q >> 30 and q & (2^30 - 1), and each limb summed in uint64 - exact
// for up to 2^31 pixels per item - then by wave, by block, and per item into a partial record; the host adds the records of a pair
// in unsigned __int128 and rounds once.  Isum is therefore math.fsum of the terms, bit for bit, whatever the block shape or order.
#include "isx_device.hpp"
#include "pairwise.hpp"
#include "scratch.hpp"
#include "gain_stats.hpp"

#include <cmath>

using namespace isx;
using namespace isxd;

namespace {

constexpr int GF_NT = 256;                 // threads per block: one block per work item
constexpr int GF_DIAG_BYTES = 16384;       // mask bytes per diagonal item (about 4 chunks of 16 B per lane)
constexpr int GF_PAIR_PIXELS = 4096;       // overlap pixels per off-diagonal item (4 groups of 4 pixels per lane)
constexpr unsigned long long GF_LO_MASK = (1ull << 30) - 1ull;

// bytes equal to 0xFF in a dword: their high bits (exact, no carry between bytes)
__device__ __forceinline__ unsigned ff_bytes(unsigned d) {
    const unsigned x = ~d;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// term * 2^52 of one pixel: sqrt of the integer r^2 + g^2 + b^2 (<= 195075), correctly rounded in double (IEEE sqrt, no fast math).
// t is 0 or in [1, 2^9): t * 2^52 = (1.mantissa) * 2^(52 + e), e = exponent in [0, 8], an integer read off the bits without a conversion
__device__ __forceinline__ unsigned long long term_q(unsigned px) {
    const unsigned b = px & 0xFFu, g = (px >> 8) & 0xFFu, r = (px >> 16) & 0xFFu;
    const unsigned s = b * b + g * g + r * r;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(sqrt((double)s));
    const unsigned long long m = (bits & ((1ull << 52) - 1ull)) | (1ull << 52);
    return s ? m << ((unsigned)(bits >> 52) - 1023u) : 0ull;
}

// the 4-byte group at byte offset `off` of a row that starts at `row` and holds `len` bytes (bytes past len are don't-care): loads only
// the aligned dwords that hold one of the wanted bytes [off, min(off + 4, len))
__device__ __forceinline__ unsigned load4(const unsigned char* row, int off, int len) {
    const uintptr_t a = (uintptr_t)row + (uintptr_t)off;
    const unsigned* A = (const unsigned*)(a & ~(uintptr_t)3);
    const unsigned sh = (unsigned)(a & 3u);
    const unsigned lo = A[0];
    const unsigned hi = (sh != 0 && (int)(4 - sh) < len - off) ? A[1] : 0u;
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
}
// 12 bytes (four BGR pixels) at byte offset `off` of a row of `len` bytes, as three dwords
__device__ __forceinline__ void load12(const unsigned char* row, int off, int len, unsigned& w0, unsigned& w1, unsigned& w2) {
    const uintptr_t a = (uintptr_t)row + (uintptr_t)off;
    const unsigned* A = (const unsigned*)(a & ~(uintptr_t)3);
    const unsigned sh = (unsigned)(a & 3u);
    const int have = len - off;                               // wanted bytes: [0, min(12, have)) from a
    const int need = (int)sh + (have < 12 ? have : 12);       // bytes from A
    const unsigned d0 = A[0];
    const unsigned d1 = need > 4 ? A[1] : 0u;
    const unsigned d2 = need > 8 ? A[2] : 0u;
    const unsigned d3 = need > 12 ? A[3] : 0u;
    w0 = __builtin_amdgcn_alignbyte(d1, d0, sh);
    w1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
    w2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Every lane takes GF_U units (a 16-byte mask chunk, or a group of four pixels) per round and issues all of their loads before it uses
// any: an item is sized to one round, so a block waits for memory once.  One block per item: measured against grids capped at 2048,
// 1024 and 512 blocks that loop over the items (config 2: 18.8 / 20.7 / 26.4 us against 18.8; 64 x 4K tiles: 569 / 632 / 825 against
// 491), and against quarter-size items with one unit per lane (32 us), it is the fastest form.
constexpr int GF_U = 4;

__global__ __launch_bounds__(GF_NT) void k_gain_feed(const GainItem* __restrict__ items, GainPartial* __restrict__ out) {
    const GainItem it = items[blockIdx.x];
    unsigned long long n = 0, hi0 = 0, lo0 = 0, hi1 = 0, lo1 = 0;
    if (it.diag) {
        // 16-byte aligned chunks of each row; a row has at most cols / 16 + 2 of them (its start is anywhere in the first)
        const int cpr = it.cols / 16 + 2;
        const int total = it.rows * cpr;
        for (int g0 = threadIdx.x; g0 < total; g0 += GF_U * GF_NT) {
            uint4 v[GF_U];
            int b0[GF_U], b1[GF_U];
#pragma unroll
            for (int u = 0; u < GF_U; ++u) {
                const int g = g0 + u * GF_NT;
                const int y = g / cpr, k = g - y * cpr;
                const uintptr_t a = (uintptr_t)(it.m0 + (size_t)y * it.sm0);
                const uintptr_t c = (a & ~(uintptr_t)15) + (uintptr_t)k * 16u;
                const uintptr_t e = a + (uintptr_t)it.cols;
                const bool live = g < total && c < e;
                v[u] = live ? *(const uint4*)c : make_uint4(0, 0, 0, 0);
                // keep the bytes of [a, e) inside [c, c + 16)
                b0[u] = a > c ? (int)(a - c) : 0;
                b1[u] = live ? (e < c + 16 ? (int)(e - c) : 16) : 0;
            }
#pragma unroll
            for (int u = 0; u < GF_U; ++u) {
                const unsigned d[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    unsigned keep = 0;
#pragma unroll
                    for (int t = 0; t < 4; ++t) keep |= (unsigned)(q * 4 + t >= b0[u] && q * 4 + t < b1[u]) << (8 * t + 7);
                    n += __popc(ff_bytes(d[q]) & keep);
                }
            }
        }
    } else {
        const int gpr = (it.cols + 3) >> 2;                   // groups of four pixels per row
        const int total = it.rows * gpr;
        const int mlen = it.cols, plen = 3 * it.cols;
        for (int g0 = threadIdx.x; g0 < total; g0 += GF_U * GF_NT) {
            unsigned both[GF_U], a0[GF_U], a1[GF_U], a2[GF_U], c0[GF_U], c1[GF_U], c2[GF_U];
#pragma unroll
            for (int u = 0; u < GF_U; ++u) {
                const int g = g0 + u * GF_NT;
                both[u] = 0; a0[u] = a1[u] = a2[u] = c0[u] = c1[u] = c2[u] = 0;
                if (g >= total) continue;
                const int y = g / gpr, x = (g - y * gpr) * 4;
                const unsigned k0 = load4(it.m0 + (size_t)y * it.sm0, x, mlen);
                const unsigned k1 = load4(it.m1 + (size_t)y * it.sm1, x, mlen);
                load12(it.p0 + (size_t)y * it.sp0, 3 * x, plen, a0[u], a1[u], a2[u]);
                load12(it.p1 + (size_t)y * it.sp1, 3 * x, plen, c0[u], c1[u], c2[u]);
                const int left = it.cols - x;
                both[u] = ff_bytes(k0) & ff_bytes(k1) & (left < 4 ? (1u << (8 * left)) - 1u : 0xFFFFFFFFu);   // not past the right edge
            }
#pragma unroll
            for (int u = 0; u < GF_U; ++u) {
                if (!both[u]) continue;
                // the four pixels as the low 24 bits of a dword each
                const unsigned pa[4] = {a0[u] & 0xFFFFFFu, __builtin_amdgcn_alignbyte(a1[u], a0[u], 3) & 0xFFFFFFu,
                                        __builtin_amdgcn_alignbyte(a2[u], a1[u], 2) & 0xFFFFFFu, a2[u] >> 8};
                const unsigned pb[4] = {c0[u] & 0xFFFFFFu, __builtin_amdgcn_alignbyte(c1[u], c0[u], 3) & 0xFFFFFFu,
                                        __builtin_amdgcn_alignbyte(c2[u], c1[u], 2) & 0xFFFFFFu, c2[u] >> 8};
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (!((both[u] >> (8 * t + 7)) & 1u)) continue;
                    const unsigned long long qa = term_q(pa[t]), qb = term_q(pb[t]);
                    n += 1;
                    hi0 += qa >> 30; lo0 += qa & GF_LO_MASK;
                    hi1 += qb >> 30; lo1 += qb & GF_LO_MASK;
                }
            }
        }
    }
    // wave, then block: integer sums, exact in any order
    __shared__ unsigned long long red[GF_NT / WAVE][GP_COUNT];
    n = wave_sum(n); hi0 = wave_sum(hi0); lo0 = wave_sum(lo0); hi1 = wave_sum(hi1); lo1 = wave_sum(lo1);
    const int wv = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        red[wv][GP_N] = n; red[wv][GP_HI0] = hi0; red[wv][GP_LO0] = lo0; red[wv][GP_HI1] = hi1; red[wv][GP_LO1] = lo1;
    }
    __syncthreads();
    if (threadIdx.x < GP_COUNT) {
        unsigned long long s = 0;
        for (int w = 0; w < GF_NT / WAVE; ++w) s += red[w][threadIdx.x];
        out[blockIdx.x].v[threadIdx.x] = s;
    }
}

// per calling thread, kept between calls: the work table and the partials on the device, and their pinned host mirrors
struct FeedScratch {
    DevBuf dev;
    int device = -1;
    PinBuf pin;
};

}  // namespace

namespace isx {

int gain_item_size(bool diag) { return diag ? GF_DIAG_BYTES : GF_PAIR_PIXELS; }

int gain_feed_items(const std::vector<GainItem>& items, double alg_bytes, int device, hipStream_t st, std::vector<GainPartial>& part) {
    const size_t ni = items.size();
    const size_t tab_bytes = round256(ni * sizeof(GainItem)), part_bytes = ni * sizeof(GainPartial);
    FeedScratch& fs = per_thread<FeedScratch>();
    if (fs.device != device) { fs.dev.release(); fs.device = device; }
    ISX_TRY(fs.dev.reserve(tab_bytes + part_bytes));
    ISX_TRY(fs.pin.reserve(tab_bytes + part_bytes, std::max<size_t>(tab_bytes + part_bytes, 1u << 16)));      // (the call ends synchronised: nothing reads the old one)
    GainItem* htab = (GainItem*)fs.pin.p;
    const GainPartial* hpart = (const GainPartial*)((char*)fs.pin.p + tab_bytes);
    std::copy(items.begin(), items.end(), htab);
    GainItem* dtab = (GainItem*)fs.dev.p;
    GainPartial* dpart = (GainPartial*)((char*)fs.dev.p + tab_bytes);
    ISX_HIP(hipMemcpyAsync(dtab, htab, ni * sizeof(GainItem), hipMemcpyHostToDevice, st));
    ISX_LAUNCH("gain_feed", alg_bytes, st, k_gain_feed, dim3((unsigned)ni), dim3(GF_NT), 0, (const GainItem*)dtab, dpart);
    ISX_HIP(hipMemcpyAsync((void*)hpart, dpart, part_bytes, hipMemcpyDeviceToHost, st));
    ISX_HIP(hipStreamSynchronize(st));       // host values come back (and the staging buffers of host mats are freed on return)
    part.assign(hpart, hpart + ni);
    return ISX_OK;
}

// OpenCV's hal::LU and its back substitution on the host (gain_stats.hpp states the contract; blocks_gain.hip runs the same operations
// on the device)
bool lu_solve(std::vector<double>& A, std::vector<double>& b, int n) {
    const double eps = 2.220446049250313e-16 * 100;
    for (int i = 0; i < n; ++i) {
        int k = i;
        for (int j = i + 1; j < n; ++j)
            if (std::fabs(A[(size_t)j * n + i]) > std::fabs(A[(size_t)k * n + i])) k = j;
        if (std::fabs(A[(size_t)k * n + i]) < eps) return false;
        if (k != i) {
            for (int j = i; j < n; ++j) std::swap(A[(size_t)i * n + j], A[(size_t)k * n + j]);
            std::swap(b[i], b[k]);
        }
        const double d = -1.0 / A[(size_t)i * n + i];
        for (int j = i + 1; j < n; ++j) {
            const double alpha = A[(size_t)j * n + i] * d;
            for (int c = i + 1; c < n; ++c) A[(size_t)j * n + c] += alpha * A[(size_t)i * n + c];
            b[j] += alpha * b[i];
        }
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = b[i];
        for (int c = i + 1; c < n; ++c) s -= A[(size_t)i * n + c] * b[c];
        b[i] = s / A[(size_t)i * n + i];
    }
    return true;
}

}  // namespace isx

extern "C" {

int isx_gain_compensator_feed(int num_images, const int* corners_xy, const isx_mat* images, const isx_mat* masks, double* gains,
                              long long* n_out, double* i_out, int device, void* hip_stream) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(num_images >= 1, ISX_ERR_INVALID, "gain_feed: num_images = %d (at least one image)", num_images);
    ISX_CHECK_ARG(corners_xy && images && masks && gains, ISX_ERR_INVALID, "gain_feed: null argument");
    const int n = num_images;
    ISX_TRY(check_tiles(n, images, masks, false, "gain_feed"));
    ISX_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)hip_stream;

    // overlapRoi of every pair i <= j, and the work table
    struct PairRoi { int i, j, x, y, w, h, first, count; };
    std::vector<PairRoi> pairs;
    std::vector<GainItem> items;
    for (int i = 0; i < n; ++i)
        for (int j = i; j < n; ++j) {
            int r[4];
            if (!overlap_roi(corners_xy + 2 * i, images[i].cols, images[i].rows, corners_xy + 2 * j, images[j].cols, images[j].rows, r)) continue;
            pairs.push_back(PairRoi{i, j, r[0], r[1], r[2], r[3], 0, 0});
        }
    MatStages stages;                        // of this call: slot i mask i, slot n + i image i
    std::vector<isx_mat> simg(n), smsk(n);   // device views
    for (int i = 0; i < n; ++i) ISX_TRY(stages.stage(i, &masks[i], false, st, "gain_feed", smsk[i]));
    // images are read by off-diagonal pairs only: a tile that overlaps no other is never staged
    std::vector<char> need_img(n, 0);
    for (const PairRoi& pr : pairs) if (pr.i != pr.j) need_img[pr.i] = need_img[pr.j] = 1;
    for (int i = 0; i < n; ++i)
        if (need_img[i]) ISX_TRY(stages.stage(n + i, &images[i], false, st, "gain_feed", simg[i]));
    const auto px = [](const isx_mat& m) { return (const unsigned char*)m.data; };
    double bytes = 0.0;
    for (PairRoi& pr : pairs) {
        const int i = pr.i, j = pr.j;
        const int oxi = pr.x - corners_xy[2 * i], oyi = pr.y - corners_xy[2 * i + 1];
        const int oxj = pr.x - corners_xy[2 * j], oyj = pr.y - corners_xy[2 * j + 1];
        const bool diag = i == j;
        const int per = diag ? GF_DIAG_BYTES : GF_PAIR_PIXELS;
        const int band = std::max(1, per / pr.w);
        pr.first = (int)items.size();
        for (int y = 0; y < pr.h; y += band) {
            GainItem it{};
            const int ri = oyi + y, rj = oyj + y;
            it.m0 = px(smsk[i]) + (size_t)ri * smsk[i].step + oxi; it.sm0 = smsk[i].step;
            if (!diag) {
                it.m1 = px(smsk[j]) + (size_t)rj * smsk[j].step + oxj; it.sm1 = smsk[j].step;
                it.p0 = px(simg[i]) + (size_t)ri * simg[i].step + 3 * (size_t)oxi; it.sp0 = simg[i].step;
                it.p1 = px(simg[j]) + (size_t)rj * simg[j].step + 3 * (size_t)oxj; it.sp1 = simg[j].step;
            }
            it.rows = std::min(band, pr.h - y); it.cols = pr.w; it.diag = diag ? 1 : 0;
            items.push_back(it);
        }
        pr.count = (int)items.size() - pr.first;
        bytes += (double)pr.w * pr.h * (diag ? 1.0 : 8.0);
    }
    std::vector<GainPartial> part;           // items.size() >= n: every image overlaps itself
    ISX_TRY(gain_feed_items(items, bytes, device, st, part));

    // N and I in OpenCV's layout: both start at 0 (Mat_::setTo(0)), so a pair without overlap keeps N = 0, I = 0; a pair with an
    // overlap gets N = max(1, count) - an empty intersect there gives N = 1, I = 0
    std::vector<long long> N((size_t)n * n, 0);
    std::vector<double> I((size_t)n * n, 0.0);
    for (const PairRoi& pr : pairs) {
        unsigned long long cnt;
        unsigned __int128 s0, s1;
        gain_partial_total(part, pr.first, pr.count, cnt, s0, s1);
        const long long nn = std::max<long long>(1, (long long)cnt);
        N[(size_t)pr.i * n + pr.j] = N[(size_t)pr.j * n + pr.i] = nn;
        if (pr.i != pr.j) {
            const double isum0 = (double)s0 * 0x1p-52, isum1 = (double)s1 * 0x1p-52;   // one rounding each (to nearest), then an exact scaling
            I[(size_t)pr.i * n + pr.j] = isum0 / (double)nn;
            I[(size_t)pr.j * n + pr.i] = isum1 / (double)nn;
        }
    }
    // the system in OpenCV's loop order
    const double alpha = 0.01, beta = 100;
    std::vector<double> A((size_t)n * n, 0.0), b(n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double Nij = (double)N[(size_t)i * n + j], Iij = I[(size_t)i * n + j], Iji = I[(size_t)j * n + i];
            b[i] += beta * Nij;
            A[(size_t)i * n + i] += beta * Nij;
            if (j == i) continue;
            A[(size_t)i * n + i] += 2 * alpha * Iij * Iij * Nij;
            A[(size_t)i * n + j] -= 2 * alpha * Iij * Iji * Nij;
        }
    ISX_CHECK_ARG(lu_solve(A, b, n), ISX_ERR_INTERNAL, "gain_feed: the system is singular");
    for (int i = 0; i < n; ++i) gains[i] = b[i];
    if (n_out) std::copy(N.begin(), N.end(), n_out);
    if (i_out) std::copy(I.begin(), I.end(), i_out);
    return ISX_OK;
} ISX_EXIT("isx_gain_compensator_feed")

}  // extern "C"
