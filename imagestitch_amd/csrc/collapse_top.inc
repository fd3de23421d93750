// collapse_top.inc — the TOP collapse steps of the deferred cycle in ONE launch (included by blend.hip inside its anonymous namespace).
//
//   out_L     = norm(SUM_t cast(G_{L,t} W_{L,t}))
//   out_{k-1} = sat(pyrUp(out_k) + norm(SUM_t cast((G_{k-1,t} - pyrUp(G_{k,t})) W_{k-1,t})))      k = L .. L - D + 1
//   (MultiBandBlender::blend: normalizeUsingWeightMap + restoreImageFromLaplacePyr, W:313; SURVEY §8(a) A12)
//
// The steps above level 2 of a 4K pair are launches of 36 - 490 workgroups that run 6 - 10 us each at a few percent of the GPU
// (profiles/round4a_bench_kernel_stats.csv): launch, one memory round trip, a barrier, another round trip.  Their outputs out_L ..
// out_{L-D+1} are read by the next step and by nobody else, and a block of the last of them depends on a halo of only one pixel per
// level: here ONE workgroup produces a 64 x 16 block of out_{L-D} from the tiles' Gaussian levels alone, the levels in between living
// in LDS (12 x 6, 20 x 8 and 36 x 12 pixels of out_L, out_{L-1}, out_{L-2} for D = 3; the halos are recomputed by the neighbouring
// blocks - a few hundred pixels).  Per pixel the operations and their order are those of k_collapse_gather (same helpers: pyr_up_2x2 on a
// staged coarse tile, normalise, the accumulate expressions), so the bits are the same; D - 1 launches and their round trips are gone.
constexpr int TOP_DMAX = 3;                 // most steps one launch fuses
constexpr int TOP_BW = 64, TOP_BH = 16;     // the block of out_{L-D} a workgroup produces
struct TopTiles {
    int n, D;                                // tiles, fused steps (2 or 3)
    int x_tl[DEF_MAX], y_tl[DEF_MAX], w[DEF_MAX], h[DEF_MAX];      // tile rectangle at the OUTPUT level (L - D), dst_roi_ coordinates: multiples of 2^D
    const void* g[DEF_MAX][TOP_DMAX + 1];    // G_{L-D+i,t}, i = 0 .. D
};
static_assert(sizeof(TopTiles) + sizeof(LevelBuf) + 64 <= 4096, "k_collapse_top's arguments exceed the kernel-argument limit");
// the same in a device-resident table (more than DEF_MAX tiles, see TileTab in blend.hip): one TopDesc per tile, and per TOP_BW columns of the
// output level the index range of the tiles that can reach a block there (its cone widens by at most 3 * 2^D output-level columns)
struct TopDesc { int x_tl, y_tl, w, h; const void* g[TOP_DMAX + 1]; };
static_assert(sizeof(TopDesc) % 16 == 0, "TopDesc records are loaded in 16-byte pieces");
struct TopGRow {
    const char* row;
    __device__ __forceinline__ const void* operator[](int i) const { return as_global(ld_const<const void*>(row + (size_t)(unsigned)i * sizeof(void*))); }   // a loaded pointer, said to be global (isx_device.hpp: as_global)
};
struct TopGField {
    const char* base;
    __device__ __forceinline__ TopGRow operator[](int t) const { return TopGRow{base + (size_t)(unsigned)t * sizeof(TopDesc) + offsetof(TopDesc, g)}; }
};
template <size_t OFF>
struct TopIField {
    const char* base;
    __device__ __forceinline__ int operator[](int t) const { return ld_const<int>(base + (size_t)(unsigned)t * sizeof(TopDesc) + OFF); }
};
struct TopTab {
    int n, D, nrng, pad_;
    const int2* rng;
    TopIField<offsetof(TopDesc, x_tl)> x_tl;
    TopIField<offsetof(TopDesc, y_tl)> y_tl;
    TopIField<offsetof(TopDesc, w)> w;
    TopIField<offsetof(TopDesc, h)> h;
    TopGField g;
};
// the tiles a block at block column bxa (absolute) has to look at
__device__ __forceinline__ void top_range(const TopTiles& tt, int, int& tb, int& te) { tb = 0; te = tt.n; }
__device__ __forceinline__ void top_range(const TopTab& tt, int bxa, int& tb, int& te) {
    tb = 0; te = tt.n;
    if (tt.nrng <= 0) return;
    const int2 r = ld_const<int2>(tt.rng + min(max(bxa, 0), tt.nrng - 1));
    tb = min(r.x, r.y); te = r.y;
}

// level L - D + i of tile t as a LevelBuf (tile levels halve exactly: the fed rectangles are multiples of 2^L)
template <class TT>
__device__ __forceinline__ LevelBuf top_level(const TT& tt, int t, int i) {
    LevelBuf l;
    l.img = const_cast<void*>(tt.g[t][i]); l.wgt = nullptr; l.rows = tt.h[t] >> i; l.cols = tt.w[t] >> i;
    return l;
}

// pyr_up_2x2 (blend.hip) on a staged tile of row pitch TOP_P: the thread's coarse pixel is ct[wv + 1][lane + 1].  Same expressions, same bits.
constexpr int TOP_P = 40;                   // row pitch of the LDS arrays: the widest region is 36 pixels (+ 2 of halo)
template <int M>
__device__ __forceinline__ Up4<M> top_pyr_up(Px<M> (*ct)[TOP_P], int lane, int wv, int cx, int cw) {
    using WT = typename WorkT<M>::t;
    WT t0[3][3], t1[3][3];  // [row][channel]
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
        const Px<M> sm = ct[wv + rr][lane], sc = ct[wv + rr][lane + 1], sp = ct[wv + rr][lane + 2];
        t0[rr][0] = sm.c0 + sc.c0 * 6 + sp.c0; t1[rr][0] = (sc.c0 + sp.c0) * 4;
        t0[rr][1] = sm.c1 + sc.c1 * 6 + sp.c1; t1[rr][1] = (sc.c1 + sp.c1) * 4;
        t0[rr][2] = sm.c2 + sc.c2 * 6 + sp.c2; t1[rr][2] = (sc.c2 + sp.c2) * 4;
    }
    if (cx == 0 || cx == cw - 1) {   // OpenCV's explicit edge formulas (a different fp32 association)
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {
            const Px<M> sm = ct[wv + rr][lane], sc = ct[wv + rr][lane + 1], sp = ct[wv + rr][lane + 2];
            const WT m[3] = {sm.c0, sm.c1, sm.c2}, c[3] = {sc.c0, sc.c1, sc.c2}, p[3] = {sp.c0, sp.c1, sp.c2};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (cw == 1) { t0[rr][k] = c[k] * 8; t1[rr][k] = c[k] * 8; }
                else if (cx == 0) { t0[rr][k] = c[k] * 6 + p[k] * 2; t1[rr][k] = (c[k] + p[k]) * 4; }
                else { t0[rr][k] = m[k] + c[k] * 7; t1[rr][k] = c[k] * 8; }
            }
        }
    }
    Up4<M> u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        WT e0 = t0[0][k] + t0[1][k] * 6 + t0[2][k], e1 = t1[0][k] + t1[1][k] * 6 + t1[2][k];
        WT o0 = (t0[1][k] + t0[2][k]) * 4, o1 = (t1[1][k] + t1[2][k]) * 4;
        if constexpr (M == M_I16) {   // the clamp of saturate_cast<short> can never act (pyr_up_2x2)
            u.v[0][0][k] = (e0 + 32) >> 6; u.v[0][1][k] = (e1 + 32) >> 6;
            u.v[1][0][k] = (o0 + 32) >> 6; u.v[1][1][k] = (o1 + 32) >> 6;
        } else {
            u.v[0][0][k] = e0 * (1.f / 64.f); u.v[0][1][k] = e1 * (1.f / 64.f);
            u.v[1][0][k] = o0 * (1.f / 64.f); u.v[1][1][k] = o1 * (1.f / 64.f);
        }
    }
    return u;
}

// One step inside the block: out_f (fine, LDS or global) from out_c (coarse, LDS) and the tiles' levels i (fine) and i + 1 (coarse).
//   fine region  [fx0, fx0 + 2 cw) x [fy0, fy0 + 2 ch)  = twice the core coarse region [cx0, cx0 + cw) x [cy0, cy0 + ch), cw * ch <= 256
//   oc : the coarse out level in LDS, oc[r][c] = out_c(cy0 - 1 + r, cx0 - 1 + c) already clamped / row-mapped at the level's borders
//        (what stage_coarse would have put there)
//   ct : scratch of the same shape for the coarse levels of TWO tiles: the tiles that reach the block are taken two at a time, every load
//        of a round (the threads' fine pixels, both staged tiles) in flight together, one barrier pair per round
// (cw, ch are compile-time: the staging index arithmetic divides by them, and a wave of this launch runs nearly alone on its SIMD - every
// instruction of its chain counts)
template <int M, bool LAST, int cw, int ch, class TT>
__device__ __forceinline__ void top_step(const TT& tt, const int tb, const int te, int i, Px<M> (*oc)[TOP_P], Px<M> (*ct)[TOP_BH / 2 + 2][TOP_P], Px<M> (*of)[TOP_P], int of_x0, int of_y0,
                                         const LevelBuf& out_g, int cx0, int cy0, int lev_cw, int lev_ch) {
    using WT = typename WorkT<M>::t;
    constexpr bool OUT_DST = M != M_I16;
    constexpr int G = 2;
    const int tid = threadIdx.x;
    const int lcx_b = tid % cw, lcy_b = tid / cw;              // this thread's coarse pixel inside the core region
    const bool active = tid < cw * ch;
    const int cx = cx0 + lcx_b, cy = cy0 + lcy_b;              // ... at the coarse level (mosaic coordinates)
    const bool mine_out = active && (unsigned)cx < (unsigned)lev_cw && (unsigned)cy < (unsigned)lev_ch;
    WT acc[2][2][3];
    float accw[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) { acc[a][b][0] = 0; acc[a][b][1] = 0; acc[a][b][2] = 0; accw[a][b] = 0.f; }
    constexpr int nstage = (ch + 2) * (cw + 2);
    bool first_round = true;
    for (int t = tb; t < te;) {
        // the next (up to) G tiles, in feed order, whose rectangle at the fine level of this step (level index i) meets the block's fine region
        int sel[G], ns = 0;
        for (; t < te && ns < G; ++t) {
            const int tx = tt.x_tl[t] >> i, ty = tt.y_tl[t] >> i, tw = tt.w[t] >> i, th = tt.h[t] >> i;
            const bool touch = !((2 * cx0 >= tx + tw) | (2 * cx0 + 2 * cw <= tx) | (2 * cy0 >= ty + th) | (2 * cy0 + 2 * ch <= ty));      // block-uniform
            if (touch) sel[ns++] = t;
        }
        if (ns == 0) break;
        Px<M> gg[G][2][2], sv[G][2];
        bool mine[G];
        int lcxs[G], ccols[G];
#pragma unroll
        for (int s = 0; s < G; ++s) {
            mine[s] = false; lcxs[s] = 0; ccols[s] = 1;
            if (s < ns) {
                const int tl = sel[s];
                const LevelBuf fine = top_level(tt, tl, i), coarse = top_level(tt, tl, i + 1);
                const int lx0 = cx0 - ((tt.x_tl[tl] >> i) >> 1), ly0 = cy0 - ((tt.y_tl[tl] >> i) >> 1);      // the core region's origin in the tile's coarse coordinates
                const int lcx = lx0 + lcx_b, lcy = ly0 + lcy_b;
                mine[s] = mine_out && (unsigned)lcx < (unsigned)coarse.cols && (unsigned)lcy < (unsigned)coarse.rows;
                lcxs[s] = lcx; ccols[s] = coarse.cols;
                if (mine[s]) {
#pragma unroll
                    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                        for (int dx = 0; dx < 2; ++dx) gg[s][dy][dx] = load_px<M, false>(fine, 2 * lcx + dx, 2 * lcy + dy);
                }
#pragma unroll
                for (int it = 0; it < 2; ++it) {
                    const int k = tid + 256 * it;
                    if (k < nstage) {
                        const int ry = k / (cw + 2), rx = k - ry * (cw + 2);
                        const int gx = min(max(lx0 - 1 + rx, 0), coarse.cols - 1), gy = up_row_map<M>(ly0 - 1 + ry, coarse.rows);
                        sv[s][it] = load_px_rgb<M, false>(coarse, gx, gy);
                    }
                }
            }
        }
        if (!first_round) __syncthreads();                                       // the previous round's readers are done with ct
        first_round = false;
#pragma unroll
        for (int s = 0; s < G; ++s)
            if (s < ns) {
#pragma unroll
                for (int it = 0; it < 2; ++it) {
                    const int k = tid + 256 * it;
                    if (k < nstage) { const int ry = k / (cw + 2), rx = k - ry * (cw + 2); ct[s][ry][rx] = sv[s][it]; }
                }
            }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < G; ++s) {
            if (!mine[s]) continue;
            const Up4<M> u = top_pyr_up<M>(ct[s], lcx_b, lcy_b, lcxs[s], ccols[s]);
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const Px<M> g = gg[s][dy][dx];
                    if constexpr (M == M_I16) {     // cv::subtract saturates; dst += static_cast<short>(lap * w), wrapping
                        acc[dy][dx][0] = wrap_s16(acc[dy][dx][0] + f2s_x86((float)sat_s16(g.c0 - u.v[dy][dx][0]) * g.w));
                        acc[dy][dx][1] = wrap_s16(acc[dy][dx][1] + f2s_x86((float)sat_s16(g.c1 - u.v[dy][dx][1]) * g.w));
                        acc[dy][dx][2] = wrap_s16(acc[dy][dx][2] + f2s_x86((float)sat_s16(g.c2 - u.v[dy][dx][2]) * g.w));
                    } else {
                        acc[dy][dx][0] = acc[dy][dx][0] + (g.c0 - u.v[dy][dx][0]) * g.w;
                        acc[dy][dx][1] = acc[dy][dx][1] + (g.c1 - u.v[dy][dx][1]) * g.w;
                        acc[dy][dx][2] = acc[dy][dx][2] + (g.c2 - u.v[dy][dx][2]) * g.w;
                    }
                    accw[dy][dx] = accw[dy][dx] + g.w;
                }
        }
    }
    // pyrUp(out_c) + normalised level
    if (!mine_out) return;
    const Up4<M> u = top_pyr_up<M>(oc, lcx_b, lcy_b, cx, lev_cw);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            Px<M> d;
            d.c0 = acc[dy][dx][0]; d.c1 = acc[dy][dx][1]; d.c2 = acc[dy][dx][2]; d.w = accw[dy][dx];
            normalise<M>(d);
            if constexpr (M == M_I16) {      // cv::add saturates
                d.c0 = sat_s16(u.v[dy][dx][0] + d.c0); d.c1 = sat_s16(u.v[dy][dx][1] + d.c1); d.c2 = sat_s16(u.v[dy][dx][2] + d.c2);
            } else {
                d.c0 = u.v[dy][dx][0] + d.c0; d.c1 = u.v[dy][dx][1] + d.c1; d.c2 = u.v[dy][dx][2] + d.c2;
            }
            const int fx = 2 * cx + dx, fy = 2 * cy + dy;
            if constexpr (LAST) store_px<M, OUT_DST>(out_g, fx, fy, d);
            else of[fy - of_y0][fx - of_x0] = d;
        }
}

// the staged form of an out level held in LDS: lv[r][c] = out(y0 + r, x0 + c) for the rows / columns the block computed; what a step reads
// is that level through stage_coarse's border rules (row -1 := row 1 (0 if one row), row h := h - 1; columns clamped), copied into `oc`
template <int M, int cw, int ch>
__device__ __forceinline__ void top_restage(Px<M> (*lv)[TOP_P], int x0, int y0, Px<M> (*oc)[TOP_P], int cx0, int cy0, int lev_cw, int lev_ch) {
    constexpr int nstage = (ch + 2) * (cw + 2);
    for (int k = threadIdx.x; k < nstage; k += blockDim.x) {
        const int ry = k / (cw + 2), rx = k - ry * (cw + 2);
        const int gx = min(max(cx0 - 1 + rx, 0), lev_cw - 1), gy = up_row_map<M>(cy0 - 1 + ry, lev_ch);
        oc[ry][rx] = lv[gy - y0][gx - x0];
    }
}

template <int M, class TT>
__device__ __forceinline__ void collapse_top_body(const TT& tt, const LevelBuf& out_g, int bx0, int top_rows, int top_cols) {
    // LDS: two ping-pong level buffers, the staged coarse out level, a tile's staged coarse level: 4 x 14 x 66 records
    // LDS (34 KB: four workgroups per CU): two ping-pong level buffers, the staged coarse out level, the staged coarse levels of two tiles
    constexpr int LR = TOP_BH / 2 + 4, SR = TOP_BH / 2 + 2;       // rows: a computed level holds at most 12, a staged one 8 + 2
    __shared__ Px<M> lvA[LR][TOP_P], lvB[LR][TOP_P], oc[SR][TOP_P], ct[2][SR][TOP_P];
    const int D = tt.D;
    const int X0 = (blockIdx.x + bx0) * TOP_BW, Y0 = blockIdx.y * TOP_BH;       // the block of the output level (index 0)
    int tb, te;
    top_range(tt, (int)blockIdx.x + bx0, tb, te);
    // core coarse regions of the D steps, finest first: step j produces level j from level j + 1 (level indices relative to the output level)
    //   C[1] = the block / 2;  level j's computed region R_j = C[j] widened by 2 (its halo of 1, rounded to even);  C[j + 1] = R_j / 2
    int ccx[TOP_DMAX + 1], ccy[TOP_DMAX + 1], ccw[TOP_DMAX + 1], cch[TOP_DMAX + 1];
    ccx[1] = X0 / 2; ccy[1] = Y0 / 2; ccw[1] = TOP_BW / 2; cch[1] = TOP_BH / 2;
    for (int j = 2; j <= D; ++j) {
        // step j - 1 reads level j - 1 on its core region widened by one pixel; step j produces whole 2 x 2 blocks: that range rounded out
        // to even bounds, halved, is step j's core region (32 x 8 -> 18 x 6 -> 10 x 4 coarse pixels)
        const int xl = (ccx[j - 1] - 1) & ~1, xh = (ccx[j - 1] + ccw[j - 1] + 2) & ~1, yl = (ccy[j - 1] - 1) & ~1, yh = (ccy[j - 1] + cch[j - 1] + 2) & ~1;
        ccx[j] = xl >> 1; ccw[j] = (xh - xl) >> 1; ccy[j] = yl >> 1; cch[j] = (yh - yl) >> 1;
    }
    // level extents relative to the top: level D has top_rows x top_cols, level j has them shifted up
    auto lev_w = [&](int j) { return top_cols << (D - j); };
    auto lev_h = [&](int j) { return top_rows << (D - j); };
    // ---- the top level out_D on the halo region of C[D]: [ccx[D] - 1, ccx[D] + ccw[D] + 1) x [ccy[D] - 1, ...), clamped to the level
    {
        const int x0 = max(ccx[D] - 1, 0), y0 = max(ccy[D] - 1, 0), x1 = min(ccx[D] + ccw[D] + 1, lev_w(D)), y1 = min(ccy[D] + cch[D] + 1, lev_h(D));
        const int rw = max(x1 - x0, 0), rh = max(y1 - y0, 0);
        for (int k = threadIdx.x; k < rw * rh; k += blockDim.x) {
            const int ry = k / rw, rx = k - ry * rw, x = x0 + rx, y = y0 + ry;
            Px<M> d; d.c0 = 0; d.c1 = 0; d.c2 = 0; d.w = 0.f;
            for (int t = tb; t < te; ++t) {
                const LevelBuf top = top_level(tt, t, D);
                const int lx = x - (tt.x_tl[t] >> D), ly = y - (tt.y_tl[t] >> D);
                if ((unsigned)lx < (unsigned)top.cols && (unsigned)ly < (unsigned)top.rows) {
                    const Px<M> g = load_px<M, false>(top, lx, ly);
                    if constexpr (M == M_I16) {
                        d.c0 = wrap_s16(d.c0 + f2s_x86((float)g.c0 * g.w)); d.c1 = wrap_s16(d.c1 + f2s_x86((float)g.c1 * g.w)); d.c2 = wrap_s16(d.c2 + f2s_x86((float)g.c2 * g.w));
                    } else { d.c0 = d.c0 + g.c0 * g.w; d.c1 = d.c1 + g.c1 * g.w; d.c2 = d.c2 + g.c2 * g.w; }
                    d.w = d.w + g.w;
                }
            }
            normalise<M>(d);
            lvA[ry][rx] = d;
        }
        __syncthreads();
        if (D == 3) top_restage<M, 10, 4>(lvA, x0, y0, oc, ccx[3], ccy[3], lev_w(3), lev_h(3));
        else top_restage<M, 18, 6>(lvA, x0, y0, oc, ccx[2], ccy[2], lev_w(2), lev_h(2));
        __syncthreads();
    }
    // ---- the steps, coarsest first: level j - 1 from level j (core regions 10 x 4, 18 x 6, 32 x 8 coarse pixels)
    Px<M> (*cur)[TOP_P] = lvB;       // where a step writes its fine level (the one before is free again after the restage)
    if (D == 3) {
        top_step<M, false, 10, 4>(tt, tb, te, 2, oc, ct, cur, 2 * ccx[3], 2 * ccy[3], out_g, ccx[3], ccy[3], lev_w(3), lev_h(3));
        __syncthreads();
        top_restage<M, 18, 6>(cur, 2 * ccx[3], 2 * ccy[3], oc, ccx[2], ccy[2], lev_w(2), lev_h(2));
        __syncthreads();
        cur = lvA;
    }
    top_step<M, false, 18, 6>(tt, tb, te, 1, oc, ct, cur, 2 * ccx[2], 2 * ccy[2], out_g, ccx[2], ccy[2], lev_w(2), lev_h(2));
    __syncthreads();
    top_restage<M, 32, 8>(cur, 2 * ccx[2], 2 * ccy[2], oc, ccx[1], ccy[1], lev_w(1), lev_h(1));
    __syncthreads();
    top_step<M, true, 32, 8>(tt, tb, te, 0, oc, ct, cur, 0, 0, out_g, ccx[1], ccy[1], lev_w(1), lev_h(1));
}
template <int M>
__global__ __launch_bounds__(256) void k_collapse_top(TopTiles tt, LevelBuf out_g, int bx0, int top_rows, int top_cols) { collapse_top_body<M>(tt, out_g, bx0, top_rows, top_cols); }
template <int M>
__global__ __launch_bounds__(256) void k_collapse_top_tab(TopTab tt, LevelBuf out_g, int bx0, int top_rows, int top_cols) { collapse_top_body<M>(tt, out_g, bx0, top_rows, top_cols); }
