// voronoi.hip — VoronoiSeamFinder (OpenCV 3.4.2 stitching/src/seam_finders.cpp) on gfx950:
//   isx_voronoi_seam_find      seam_finder = makePtr<detail::VoronoiSeamFinder>();                       S:1180
//                              seam_finder->find(images_warped_f, corners, masks_seam)                  S:1192
//   isx_voronoi_seam_reserve   sizes the per-thread scratch ahead of a stream capture
//   isx_voronoi_seam_release   returns it
//
// The specification (DESIGN.md §8 "Voronoi seam finder"; OpenCV parity unpinned): for i < j with a non-empty overlapRoi, two submasks of
// (roi.h + 20) x (roi.w + 20) cells (gap 10; outside a tile: 0); unique_k = the cells only tile k covers; dist_k =
// distanceTransform(unique_k == 0, DIST_L1, 3) - the 16.16 chamfer whose one-cell border ring holds INIT_DIST0 = INT_MAX >> 2, so a cell is
// min(65536 d_unique, INIT_DIST0 + 65536 d_ring), converted (float)t * (1 / 65536); over the roi, where dist1 < dist2 (as floats) mask2 = 0,
// elsewhere mask1 = 0.  Pixels are never read.
//
// Three launches per pair, no memset, no atomics, nothing read back:
//   k_vr_rows      one block per submask row: reads both tiles' windows from the callers' mats (aligned dwords, any pointer / step), forms
//                  unique1 / unique2 as two 16-bit words per thread and writes, for both, the distance along the row to the nearest unique
//                  cell (block-wide prefix-max / suffix-min of positions; rows wider than VR_CHUNK take a forward and a backward sweep)
//   k_vr_seg_min   minima of r[k] - k and r[k] + k over VR_SEG-row segments of the roi's columns, both maps
//   k_vr_cols      both min-plus scans down a column in registers, the border-ring term, the float compare and the byte stores into
//                  mask1 / mask2 inside the roi; the distance maps are never written
// A pair writes the masks it reads: k_vr_rows is the only kernel that reads them and k_vr_cols the only one that writes them, in that
// order on one stream.  Every device loop has a trip count fixed by the kernel's arguments.
#include "isx_device.hpp"
#include "pairwise.hpp"
#include "scratch.hpp"

using namespace isx;
using namespace isxd;

namespace {

constexpr int VR_GAP = isx::PAIR_GAP;
constexpr int VR_BIG = 1 << 28;          // "no unique cell in this row"
constexpr int VR_PX = 16;                // cells per thread of the row pass
constexpr int VR_NT = 256;
constexpr int VR_CHUNK = VR_NT * VR_PX;  // 4096 cells per sweep step
constexpr int VR_SEG = 32;               // rows per column segment
constexpr int VR_MAX_SIDE = 32768;       // of a submask: keeps INIT_DIST0 + 65536 (ring + 1) and 65536 d inside 32 bits

struct VrGeom {
    unsigned char* m1; size_t s1;
    unsigned char* m2; size_t s2;
    int r1, c1, r2, c2;                  // tile sizes
    int oy1, ox1, oy2, ox2;              // tile coordinates of submask cell (0, 0)
    int hp, wp;                          // the submasks
    int rh, rw;                          // the roi
    int pitch;                           // ints per row of a row-distance map (a multiple of 4)
    int nseg;
};

// 16 cells of tile row ty starting at tile column tx0 (either may lie outside the tile) -> bit i set when cell i is inside and non-zero.
// The row is read as aligned dwords that each hold at least one byte of it, so any data pointer and step work.
__device__ __forceinline__ unsigned vr_cells16(const unsigned char* base, size_t step, int rows, int cols, int ty, int tx0) {
    if ((unsigned)ty >= (unsigned)rows || tx0 + VR_PX <= 0 || tx0 >= cols) return 0u;
    const unsigned char* row = base + (size_t)ty * step;
    const unsigned mis = (unsigned)(((uintptr_t)row + (uintptr_t)(intptr_t)tx0) & 3);
    const int o0 = tx0 - (int)mis;                  // row + o0 is dword-aligned
    unsigned q[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int o = o0 + 4 * i;                   // the dword covers row bytes o .. o + 3
        q[i] = (o + 3 >= 0 && o < cols) ? *(const unsigned*)(row + o) : 0u;
    }
    unsigned bits = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned w = __builtin_amdgcn_alignbyte(q[k + 1], q[k], mis);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 4 * k + j;
            const bool in = (unsigned)(tx0 + i) < (unsigned)cols;
            bits |= (in && ((w >> (8 * j)) & 255u) != 0u) ? (1u << i) : 0u;
        }
    }
    return bits;
}

__global__ __launch_bounds__(VR_NT) void k_vr_rows(VrGeom G, int* __restrict__ rowd1, int* __restrict__ rowd2) {
    __shared__ int s_wl[2][4], s_wf[2][4];
    const int y = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int* out[2] = {rowd1 + (size_t)y * G.pitch, rowd2 + (size_t)y * G.pitch};
    const int nch = (G.wp + VR_CHUNK - 1) / VR_CHUNK;
    int carry_last[2] = {-VR_BIG, -VR_BIG}, carry_first[2] = {VR_BIG, VR_BIG};
    for (int pass = 0; pass < (nch > 1 ? 2 : 1); ++pass) {
        const bool fwd = pass == 0, bwd = pass == 1 || nch == 1;
        for (int ci = 0; ci < nch; ++ci) {
            const int c = pass == 0 ? ci : nch - 1 - ci;
            const int xb = c * VR_CHUNK, n = min(VR_CHUNK, G.wp - xb);
            const int x0 = VR_PX * t;
            unsigned v1 = vr_cells16(G.m1, G.s1, G.r1, G.c1, G.oy1 + y, G.ox1 + xb + x0);
            unsigned v2 = vr_cells16(G.m2, G.s2, G.r2, G.c2, G.oy2 + y, G.ox2 + xb + x0);
            const unsigned inside = x0 >= n ? 0u : (n - x0 >= VR_PX ? 0xFFFFu : (1u << (n - x0)) - 1u);   // cells of the submask
            v1 &= inside; v2 &= inside;
            const unsigned zb[2] = {v1 & ~v2, v2 & ~v1};          // unique1, unique2: the collision cells belong to neither
            int pl[2], nn[2];
            __syncthreads();                                      // the previous step's readers of s_wl / s_wf are done
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                pl[k] = -VR_BIG; nn[k] = VR_BIG;
                if (fwd) {
                    int v = zb[k] ? xb + x0 + 31 - __clz((int)zb[k]) : -VR_BIG;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o); if (lane >= o) v = max(v, u); }
                    pl[k] = __shfl_up(v, 1);
                    if (lane == 0) pl[k] = -VR_BIG;
                    if (lane == 63) s_wl[k][wv] = v;
                }
                if (bwd) {
                    int v = zb[k] ? xb + x0 + __ffs((int)zb[k]) - 1 : VR_BIG;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_down(v, o); if (lane + o < 64) v = min(v, u); }
                    nn[k] = __shfl_down(v, 1);
                    if (lane == 63) nn[k] = VR_BIG;
                    if (lane == 0) s_wf[k][wv] = v;
                }
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (fwd) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) if (i < wv) pl[k] = max(pl[k], s_wl[k][i]);
                    pl[k] = max(pl[k], carry_last[k]);
                    carry_last[k] = max(max(carry_last[k], max(s_wl[k][0], s_wl[k][1])), max(s_wl[k][2], s_wl[k][3]));
                }
                if (bwd) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) if (i > wv) nn[k] = min(nn[k], s_wf[k][i]);
                    nn[k] = min(nn[k], carry_first[k]);
                    carry_first[k] = min(min(carry_first[k], min(s_wf[k][0], s_wf[k][1])), min(s_wf[k][2], s_wf[k][3]));
                }
#pragma unroll
                for (int q = 0; q < VR_PX / 4; ++q) {
                    const int gx0 = xb + x0 + 4 * q;
                    if (x0 + 4 * q >= n) continue;                // gx0 < wp <= pitch, and pitch is a multiple of 4: the int4 fits the row
                    int d[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = 4 * q + j, gx = gx0 + j;
                        int v = VR_BIG;
                        if (fwd) {
                            const unsigned b = zb[k] & ((2u << i) - 1u);
                            v = gx - (b ? xb + x0 + 31 - __clz((int)b) : pl[k]);
                        }
                        if (bwd) {
                            const unsigned b = zb[k] >> i;
                            v = min(v, (b ? gx + __ffs((int)b) - 1 : nn[k]) - gx);
                        }
                        d[j] = v >= VR_BIG / 2 ? VR_BIG : v;
                    }
                    int4* o4 = (int4*)(out[k] + gx0);
                    if (!fwd) { const int4 e = *o4; d[0] = min(d[0], e.x); d[1] = min(d[1], e.y); d[2] = min(d[2], e.z); d[3] = min(d[3], e.w); }
                    *o4 = make_int4(d[0], d[1], d[2], d[3]);
                }
            }
        }
    }
}

// Column pass over the roi's columns only (submask columns VR_GAP .. VR_GAP + rw - 1; the row pass needed the gap, the write-back does not).
// The chamfer's "+1" sweeps down a column are min-plus scans: forward d_f[y] = y + min_{k<=y}(r[k] - k), backward d_b[y] = -y +
// min_{k>=y}(r[k] + k).  seg holds 4 planes of nseg x rw ints: map 1 forward, map 1 backward, map 2 forward, map 2 backward.
__global__ __launch_bounds__(64) void k_vr_seg_min(VrGeom G, const int* __restrict__ rowd1, const int* __restrict__ rowd2, int* __restrict__ seg) {
    const int xr = blockIdx.x * 64 + threadIdx.x, s = blockIdx.y;
    if (xr >= G.rw) return;
    const int x = xr + VR_GAP, y0 = s * VR_SEG;
    int mf1 = 2 * VR_BIG, mb1 = 2 * VR_BIG, mf2 = 2 * VR_BIG, mb2 = 2 * VR_BIG;
#pragma unroll 8
    for (int j = 0; j < VR_SEG; ++j) {
        const int y = y0 + j;
        if (y < G.hp) {
            const int a = rowd1[(size_t)y * G.pitch + x], b = rowd2[(size_t)y * G.pitch + x];
            mf1 = min(mf1, a - y); mb1 = min(mb1, a + y);
            mf2 = min(mf2, b - y); mb2 = min(mb2, b + y);
        }
    }
    const size_t plane = (size_t)G.nseg * G.rw, at = (size_t)s * G.rw + xr;
    seg[at] = mf1; seg[plane + at] = mb1; seg[2 * plane + at] = mf2; seg[3 * plane + at] = mb2;
}

// the chamfer value (16.16) of every row of segment s in column x of one map
__device__ __forceinline__ void vr_column(const VrGeom& G, const int* __restrict__ rowd, const int* __restrict__ seg_f, const int* __restrict__ seg_b,
                                          int s, int x, int xr, unsigned (&t)[VR_SEG]) {
    const int y0 = s * VR_SEG;
    int run_f = 2 * VR_BIG, run_b = 2 * VR_BIG;
#pragma unroll 4
    for (int i = 0; i < s; ++i) run_f = min(run_f, seg_f[(size_t)i * G.rw + xr]);
#pragma unroll 4
    for (int i = G.nseg - 1; i > s; --i) run_b = min(run_b, seg_b[(size_t)i * G.rw + xr]);
    int r[VR_SEG], db[VR_SEG];
#pragma unroll
    for (int j = 0; j < VR_SEG; ++j) r[j] = y0 + j < G.hp ? rowd[(y0 + j) * G.pitch + x] : VR_BIG;   // hp * pitch <= 2^30: an int index
#pragma unroll
    for (int j = VR_SEG - 1; j >= 0; --j) { run_b = min(run_b, r[j] + (y0 + j)); db[j] = run_b - (y0 + j); }
    const unsigned INIT = (unsigned)(INT_MAX >> 2);
#pragma unroll
    for (int j = 0; j < VR_SEG; ++j) {
        const int y = y0 + j;
        run_f = min(run_f, r[j] - y);
        const int d = min(run_f + y, db[j]);
        // city-block distance to a unique cell, or INIT_DIST0 + distance to the border ring.  A submask side is at most VR_MAX_SIDE, so the
        // ring term stays below 2^31 and any d above 32767 loses to it: clamping d there keeps d << 16 inside 32 bits and changes nothing.
        const unsigned border = INIT + ((unsigned)(1 + min(min(x, G.wp - 1 - x), min(y, G.hp - 1 - y))) << 16);
        t[j] = d >= VR_BIG / 2 ? border : min((unsigned)min(d, 32767) << 16, border);
    }
}

__global__ __launch_bounds__(64) void k_vr_cols(VrGeom G, const int* __restrict__ rowd1, const int* __restrict__ rowd2, const int* __restrict__ seg) {
    const int xr = blockIdx.x * 64 + threadIdx.x, s = blockIdx.y;
    const int y0 = s * VR_SEG;
    if (xr >= G.rw || y0 + VR_SEG <= VR_GAP || y0 >= VR_GAP + G.rh) return;     // no roi cell in this segment
    const int x = xr + VR_GAP;
    const size_t plane = (size_t)G.nseg * G.rw;
    unsigned t1[VR_SEG], t2[VR_SEG];
    vr_column(G, rowd1, seg, seg + plane, s, x, xr, t1);
    vr_column(G, rowd2, seg + 2 * plane, seg + 3 * plane, s, x, xr, t2);
    unsigned seam = 0u;
#pragma unroll
    for (int j = 0; j < VR_SEG; ++j) {
        // seam = dist1 < dist2 on the FLOATS the distance transform returns: past 2^24 two different fixed-point values can round to the
        // same float (INIT_DIST0 + 65536 k and 65536 (8192 + k) do), and the comparison must then say "not less"
        const float d1 = (float)t1[j] * (1.f / 65536.f), d2 = (float)t2[j] * (1.f / 65536.f);
        seam |= d1 < d2 ? 1u << j : 0u;
    }
    // the roi's rows of this segment (rolled: 32 unrolled rows of two mats cost more scalar registers than the wave has)
    const int j0 = max(0, VR_GAP - y0), j1 = min(VR_SEG, VR_GAP + G.rh - y0);
    unsigned char* p1 = G.m1 + (size_t)(G.oy1 + y0 + j0) * G.s1 + (size_t)(G.ox1 + x);
    unsigned char* p2 = G.m2 + (size_t)(G.oy2 + y0 + j0) * G.s2 + (size_t)(G.ox2 + x);
#pragma unroll 1
    for (int j = j0; j < j1; ++j, p1 += G.s1, p2 += G.s2) {
        if ((seam >> j) & 1u) *p2 = 0;
        else *p1 = 0;
    }
}

struct VrScratch {
    DevBuf work;
    int device = -1;
    MatStages msk;                       // host masks (a device of its own: isx_voronoi_seam_reserve moves `work` alone)
};

inline size_t vr_map_bytes(int rw, int rh) {
    const int hp = rh + 2 * VR_GAP, wp = rw + 2 * VR_GAP;
    return round256((size_t)hp * ((wp + 3) & ~3) * sizeof(int));
}
inline size_t vr_bytes(int rw, int rh) {
    const int hp = rh + 2 * VR_GAP;
    return 2 * vr_map_bytes(rw, rh) + (size_t)4 * cdiv(hp, VR_SEG) * rw * sizeof(int);
}

bool vr_geom(const isx_mat& m1, const isx_mat& m2, const int tl1[2], const int tl2[2], VrGeom& G) {
    PairGrid p;
    if (!pair_grid(tl1, m1.cols, m1.rows, tl2, m2.cols, m2.rows, p)) return false;
    G.m1 = (unsigned char*)m1.data; G.s1 = m1.step;
    G.m2 = (unsigned char*)m2.data; G.s2 = m2.step;
    G.r1 = m1.rows; G.c1 = m1.cols; G.r2 = m2.rows; G.c2 = m2.cols;
    G.rw = p.rw; G.rh = p.rh; G.hp = p.hp; G.wp = p.wp;
    G.oy1 = p.oy1; G.ox1 = p.ox1; G.oy2 = p.oy2; G.ox2 = p.ox2;
    G.pitch = (G.wp + 3) & ~3;
    G.nseg = cdiv(G.hp, VR_SEG);
    return true;
}

int vr_pair(const VrGeom& G, void* work, hipStream_t st) {
    int* rowd1 = (int*)work;
    int* rowd2 = (int*)((char*)work + vr_map_bytes(G.rw, G.rh));
    int* seg = (int*)((char*)work + 2 * vr_map_bytes(G.rw, G.rh));
    const double cells = (double)G.hp * G.wp;
    const dim3 cg((unsigned)cdiv(G.rw, 64), (unsigned)G.nseg);
    ISX_LAUNCH("voronoi_rows", cells * 10.0, st, k_vr_rows, dim3((unsigned)G.hp), dim3(VR_NT), 0, G, rowd1, rowd2);
    ISX_LAUNCH("voronoi_seg_min", cells * 8.0, st, k_vr_seg_min, cg, dim3(64), 0, G, (const int*)rowd1, (const int*)rowd2, seg);
    ISX_LAUNCH("voronoi_cols", cells * 9.0, st, k_vr_cols, cg, dim3(64), 0, G, (const int*)rowd1, (const int*)rowd2, (const int*)seg);
    return ISX_OK;
}

}  // namespace

extern "C" {

int isx_voronoi_seam_release(void) ISX_ENTRY {
    clear_error();
    VrScratch& s = per_thread<VrScratch>();
    s.work.release();
    s.msk.clear();
    s.device = -1;
    return ISX_OK;
} ISX_EXIT("isx_voronoi_seam_release")

int isx_voronoi_seam_reserve(int max_roi_width, int max_roi_height, int device) ISX_ENTRY {
    clear_error();
    ISX_CHECK_ARG(max_roi_width > 0 && max_roi_height > 0, ISX_ERR_INVALID, "voronoi_seam_reserve: roi %d x %d", max_roi_width, max_roi_height);
    ISX_CHECK_ARG(max_roi_width + 2 * VR_GAP <= VR_MAX_SIDE && max_roi_height + 2 * VR_GAP <= VR_MAX_SIDE, ISX_ERR_UNSUPPORTED,
                  "voronoi_seam_reserve: a roi of %d x %d passes %d cells a side with its gap", max_roi_width, max_roi_height, VR_MAX_SIDE);
    ISX_HIP(hipSetDevice(device));
    VrScratch& s = per_thread<VrScratch>();
    if (s.device != device) { s.work.release(); s.device = device; }
    return s.work.reserve(vr_bytes(max_roi_width, max_roi_height));
} ISX_EXIT("isx_voronoi_seam_reserve")

int isx_voronoi_seam_find(int num_images, const int* sizes_wh, const int* corners_xy, isx_mat* masks, int device, void* hip_stream) ISX_ENTRY {
    clear_error();
    const char* who = "voronoi_seam_find";
    ISX_CHECK_ARG(num_images >= 0 && (num_images == 0 || (sizes_wh && corners_xy && masks)), ISX_ERR_INVALID, "%s: null argument", who);
    ISX_TRY(check_masks(num_images, sizes_wh, masks, who));
    const bool any_host = std::any_of(masks, masks + num_images, [](const isx_mat& m) { return m.device < 0; });
    if (num_images < 2) return ISX_OK;     // PairwiseSeamFinder::run visits no pair
    // the scratch the largest pair needs (a pair's roi depends on sizes and corners only, not on what earlier pairs wrote)
    size_t need = 0;
    for (int i = 0; i + 1 < num_images; ++i)
        for (int j = i + 1; j < num_images; ++j) {
            VrGeom G{};
            if (!vr_geom(masks[i], masks[j], corners_xy + 2 * i, corners_xy + 2 * j, G)) continue;
            ISX_CHECK_ARG(G.hp <= VR_MAX_SIDE && G.wp <= VR_MAX_SIDE, ISX_ERR_UNSUPPORTED,
                          "%s: the overlap of images %d and %d (%d x %d) passes %d cells a side with its gap", who, i, j, G.rw, G.rh, VR_MAX_SIDE);
            need = std::max(need, vr_bytes(G.rw, G.rh));
        }
    ISX_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)hip_stream;
    bool capturing = false;
    ISX_TRY(is_capturing(st, capturing));
    VrScratch& s = per_thread<VrScratch>();
    if (capturing) {
        ISX_CHECK_ARG(!any_host, ISX_ERR_STATE, "%s: the stream is capturing and a mask is a host mat (staging it synchronises)", who);
        ISX_CHECK_ARG(need == 0 || (s.device == device && s.work.cap >= need), ISX_ERR_STATE,
                      "%s: the stream is capturing and the scratch holds %zu of the %zu bytes this call needs (isx_voronoi_seam_reserve before the capture)",
                      who, s.device == device ? s.work.cap : (size_t)0, need);
    } else {
        if (s.device != device) { s.work.release(); s.device = device; }
        ISX_TRY(s.work.reserve(need));
    }
    if (need == 0) return ISX_OK;          // no two tiles overlap
    std::vector<isx_mat> mk(masks, masks + num_images);       // device views
    if (any_host) {                                            // (never under capture)
        s.msk.use_device(device);
        for (int i = 0; i < num_images; ++i) ISX_TRY(s.msk.stage(i, &masks[i], true, st, who, mk[i]));
    }
    for (int i = 0; i + 1 < num_images; ++i)
        for (int j = i + 1; j < num_images; ++j) {
            VrGeom G{};
            if (!vr_geom(mk[i], mk[j], corners_xy + 2 * i, corners_xy + 2 * j, G)) continue;
            ISX_TRY(vr_pair(G, s.work.p, st));
        }
    return any_host ? s.msk.finish(st) : ISX_OK;
} ISX_EXIT("isx_voronoi_seam_find")

}  // extern "C"
