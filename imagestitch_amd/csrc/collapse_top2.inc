// collapse_top2.inc — k_collapse_top for a PAIR (at most two tiles, three fused steps) with one memory round trip (included by blend.hip).
//
// What the levels >= L - 3 cost a 4K pair's step (profiles/round5_tail_ablation.txt): 34 us for 7 us of pixels - three small pyrDown launches
// and k_collapse_top, each the life of ONE block: launch, a memory round trip, a barrier, an LDS phase, stores; k_collapse_top walks four such
// round trips (the gathered top level, then a step per level, each loading its tiles' Gaussians when it gets there).  None of those loads
// depends on what the step before it computed - they are the tiles' Gaussian levels, known when the block starts.  So for the case that matters
// most (a pair: BASELINE configs 2, 3, 4) a block here
//   0. issues EVERY global load it will ever need before the first barrier: G_{L-1} of both tiles on the 27 x 15 pixels under its top region,
//      G_{L-2} on 36 x 12, its own 2 x 2 pixels of G_{L-3} - each level read exactly once per block, one memory wait;
//   1. rebuilds G_L itself: pyrDown of the staged G_{L-1} (pyr_down_row5 / pyr_down_col5 - the device functions of k_pyr_down_multi, the same
//      REFLECT_101 index maps, the same storage rounding for fp16 levels), 12 x 6 pixels per tile - the launch that produced level L is not
//      issued any more (run_blend_deferred_t skips it), its 5.5 us and its round trip are gone;
//   2. gathers the top level and runs the three steps out of LDS: a step's fine pixels and its coarse 3 x 3 neighbourhoods are read where the
//      loads of phase 0 put them (G_L from phase 1), through the same clamp / row-map rules k_collapse_top's staging applies.
// Per pixel the operations and their order are k_collapse_top's (top_step's accumulate expressions, top_pyr_up's filters, normalise): the same
// bits (the whole GPU suite runs through it).
// LDS: 38.5 KB per block = four blocks per CU: the 748 blocks of a 4K pair are resident at once.
// What it buys, measured (profiles/round5_top2_ab.txt): the step of a 4K pair -1.5 ... -3 us - all of it the launch that is gone (4.4 us); the kernel
// itself takes 17.8 us against k_collapse_top's 16.5 - 17.3.  Phase by phase (timing-only builds, since removed): an empty launch 4.1 us;
// with the loads, the pyrDown phase and the gathered top level still 4.2 (they hide inside the launch's own ramp); the first step + 3.6 us (40
// pixels), the second + 3.7 (108), the last + 6.0 (256 pixels, the stores).  A step costs what it costs whatever was tried on it - packed fp32
// (3 223 -> 2 633 vector instructions per wave), loads issued in the order of use, three or four blocks per CU, other waves of the block doing the
// narrow steps: none moved the launch by 0.2 us.

constexpr int T2_AW = 27, T2_AH = 15;       // G_{L-1} under the top region: 2 * 12 + 3 columns, 2 * 6 + 3 rows
constexpr int T2_FW = 36, T2_FH = 12;       // G_{L-2} on twice the second step's core region
constexpr int T2_TW = 12, T2_TH = 6;        // the top region: the first step's core region (10 x 4) and its halo
constexpr int T2_P = 36;                    // row pitch of the out-level arrays (the widest computed region: 36)

template <int M>
__device__ __forceinline__ Px<M> top2_storage_round(Px<M> p) {       // what store_px + load_px of a tile level do to a value
    if constexpr (M == M_F16) { p.c0 = h2f_bits(f2h_bits(p.c0)); p.c1 = h2f_bits(f2h_bits(p.c1)); p.c2 = h2f_bits(f2h_bits(p.c2)); p.w = h2f_bits(f2h_bits(p.w)); }
    return p;
}

// top_pyr_up (collapse_top.inc) with the 3 x 3 coarse neighbourhood behind a functor: fetch(rr, cc) = the staged coarse pixel of row rr, column cc
// of the neighbourhood (what ct[wv + rr][lane + cc] holds there).  Same expressions, same bits.
template <int M, class F>
__device__ __forceinline__ Up4<M> top2_pyr_up(F fetch, int cx, int cw) {
    using WT = typename WorkT<M>::t;
    WT t0[3][3], t1[3][3];  // [row][channel]
    Px<M> nb[3][3];
#pragma unroll
    for (int rr = 0; rr < 3; ++rr)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) nb[rr][cc] = fetch(rr, cc);
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
        const Px<M> sm = nb[rr][0], sc = nb[rr][1], sp = nb[rr][2];
        t0[rr][0] = sm.c0 + sc.c0 * 6 + sp.c0; t1[rr][0] = (sc.c0 + sp.c0) * 4;
        t0[rr][1] = sm.c1 + sc.c1 * 6 + sp.c1; t1[rr][1] = (sc.c1 + sp.c1) * 4;
        t0[rr][2] = sm.c2 + sc.c2 * 6 + sp.c2; t1[rr][2] = (sc.c2 + sp.c2) * 4;
    }
    if (cx == 0 || cx == cw - 1) {   // OpenCV's explicit edge formulas (a different fp32 association)
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {
            const Px<M> sm = nb[rr][0], sc = nb[rr][1], sp = nb[rr][2];
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

// pyr_up_2x2_pk (blend.hip: the same pyrUp with the fp32 arithmetic on register pairs, each half rounded on its own) behind the same functor
template <int M, class F>
__device__ __forceinline__ UpPk top2_pyr_up_pk(F fetch, int cx, int cw) {
    static_assert(M != M_I16, "packed pyrUp: float work types only");
    f32x2 t0a[3], t1a[3], tc[3];      // tc[rr] = (t0, t1) of the r channel
    const bool edge = cx == 0 || cx == cw - 1;
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
        const Px<M> sm = fetch(rr, 0), sc = fetch(rr, 1), sp = fetch(rr, 2);
        const f32x2 ma = {sm.c0, sm.c1}, ca = {sc.c0, sc.c1}, pa = {sp.c0, sp.c1};
        t0a[rr] = (ma + ca * splat2(6.f)) + pa; t1a[rr] = (ca + pa) * splat2(4.f);
        tc[rr].x = (sm.c2 + sc.c2 * 6.f) + sp.c2; tc[rr].y = (sc.c2 + sp.c2) * 4.f;
        if (edge) {   // OpenCV's explicit edge formulas (a different fp32 association)
            if (cw == 1) { t0a[rr] = ca * splat2(8.f); t1a[rr] = t0a[rr]; tc[rr].x = sc.c2 * 8.f; tc[rr].y = tc[rr].x; }
            else if (cx == 0) { t0a[rr] = ca * splat2(6.f) + pa * splat2(2.f); tc[rr].x = sc.c2 * 6.f + sp.c2 * 2.f; }
            else { t0a[rr] = ma + ca * splat2(7.f); t1a[rr] = ca * splat2(8.f); tc[rr].x = sm.c2 + sc.c2 * 7.f; tc[rr].y = sc.c2 * 8.f; }
        }
    }
    UpPk u;
    const f32x2 s64 = splat2(1.f / 64.f);
    u.a[0][0] = ((t0a[0] + t0a[1] * splat2(6.f)) + t0a[2]) * s64; u.a[0][1] = ((t1a[0] + t1a[1] * splat2(6.f)) + t1a[2]) * s64;
    u.a[1][0] = ((t0a[1] + t0a[2]) * splat2(4.f)) * s64;          u.a[1][1] = ((t1a[1] + t1a[2]) * splat2(4.f)) * s64;
    u.c[0] = ((tc[0] + tc[1] * splat2(6.f)) + tc[2]) * s64;
    u.c[1] = ((tc[1] + tc[2]) * splat2(4.f)) * s64;
    return u;
}

// one tile's uniform description at the four levels (j = 0: the output level L - 3 ... j = 3: the top level L)
struct Top2Tile {
    bool on;
    int tx[4], ty[4], cw[4], ch[4];      // origin in the mosaic and size, per level
};

// One step: out level j - 1 on twice the core region [cx0, +cw) x [cy0, +ch) of level j.  FINE(s, fx, fy) = tile s's Gaussian pixel of level
// j - 1 at tile-local (fx, fy) (inside the tile); COARSE(s, gx, gy) = its pixel of level j at tile-local (gx, gy) (already clamped / row-mapped).
// oc = the staged out level j (top_restage).  The accumulate expressions are top_step's.
template <int M, bool LAST, int cw, int ch, class FINE, class COARSE>
__device__ __forceinline__ void top2_step(const Top2Tile (&T)[2], int j, FINE fine, COARSE coarse, Px<M> (*oc)[T2_P], Px<M> (*of)[T2_P], int of_x0, int of_y0,
                                          const LevelBuf& out_g, int cx0, int cy0, int lev_cw, int lev_ch) {
    using WT = typename WorkT<M>::t;
    constexpr bool OUT_DST = M != M_I16;
    const int tid = threadIdx.x;
    const int lcx_b = tid % cw, lcy_b = tid / cw;
    const bool active = tid < cw * ch;
    const int cx = cx0 + lcx_b, cy = cy0 + lcy_b;
    const bool mine_out = active && (unsigned)cx < (unsigned)lev_cw && (unsigned)cy < (unsigned)lev_ch;
    // float work types: accumulators and stencils on register pairs, as k_collapse_gather's packed form ((b, g) per pixel, r and the weight of the
    // two pixels of a fine row): 3 223 -> 2 633 vector instructions per wave, 112 -> 89 registers; each half is rounded on its own: same bits
    constexpr bool PK = M != M_I16;
    WT acc[2][2][3];
    float accw[2][2];
    f32x2 accA[2][2], accC[2], accW[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) { acc[a][b][0] = 0; acc[a][b][1] = 0; acc[a][b][2] = 0; accw[a][b] = 0.f; accA[a][b] = splat2(0.f); accC[a] = splat2(0.f); accW[a] = splat2(0.f); }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (!T[s].on) continue;
        // the tile's rectangle at the fine level of this step meets the block's fine region? (block-uniform, top_step's test)
        const int tx = T[s].tx[j - 1], ty = T[s].ty[j - 1], tw = T[s].cw[j - 1], th = T[s].ch[j - 1];
        if ((2 * cx0 >= tx + tw) | (2 * cx0 + 2 * cw <= tx) | (2 * cy0 >= ty + th) | (2 * cy0 + 2 * ch <= ty)) continue;
        const int lx0 = cx0 - T[s].tx[j], ly0 = cy0 - T[s].ty[j];       // the core region's origin in the tile's coarse coordinates
        const int lcx = lx0 + lcx_b, lcy = ly0 + lcy_b, ccols = T[s].cw[j], crows = T[s].ch[j];
        if (!(mine_out && (unsigned)lcx < (unsigned)ccols && (unsigned)lcy < (unsigned)crows)) continue;
        auto nbr = [&](int rr, int cc) {
            const int gx = min(max(lcx - 1 + cc, 0), ccols - 1), gy = up_row_map<M>(lcy - 1 + rr, crows);
            return coarse(s, gx, gy);
        };
        if constexpr (PK) {
            const UpPk u = top2_pyr_up_pk<M>(nbr, lcx, ccols);
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {   // acc = acc + (g - pyrUp) * w, accw = accw + w: two values per instruction
                const Px<M> g0 = fine(s, 2 * lcx, 2 * lcy + dy, 0, dy), g1 = fine(s, 2 * lcx + 1, 2 * lcy + dy, 1, dy);
                const f32x2 a0 = {g0.c0, g0.c1}, a1 = {g1.c0, g1.c1}, gc = {g0.c2, g1.c2}, gw = {g0.w, g1.w};
                accA[dy][0] = accA[dy][0] + (a0 - u.a[dy][0]) * splat2(g0.w);
                accA[dy][1] = accA[dy][1] + (a1 - u.a[dy][1]) * splat2(g1.w);
                accC[dy] = accC[dy] + (gc - u.c[dy]) * gw;
                accW[dy] = accW[dy] + gw;
            }
            continue;
        }
        const Up4<M> u = top2_pyr_up<M>(nbr, lcx, ccols);
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const Px<M> g = fine(s, 2 * lcx + dx, 2 * lcy + dy, dx, dy);
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
    // pyrUp(out_j) + normalised level
    if (!mine_out) return;
    if constexpr (PK) {
        const UpPk u = top2_pyr_up_pk<M>([&](int rr, int cc) { return oc[lcy_b + rr][lcx_b + cc]; }, cx, lev_cw);
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const f32x2 den = accW[dy] + splat2(WEIGHT_EPS);                 // normalizeUsingWeightMap: c / (w + 1e-5f), both pixels of the row
            f32x2 n0, n1, nc;
            n0.x = accA[dy][0].x / den.x; n0.y = accA[dy][0].y / den.x; n1.x = accA[dy][1].x / den.y; n1.y = accA[dy][1].y / den.y;
            nc.x = accC[dy].x / den.x; nc.y = accC[dy].y / den.y;
            const f32x2 ra0 = u.a[dy][0] + n0, ra1 = u.a[dy][1] + n1, rc = u.c[dy] + nc;    // restoreImageFromLaplacePyr: pyrUp(out_j) + level
            Px<M> dd[2];
            dd[0].c0 = ra0.x; dd[0].c1 = ra0.y; dd[0].c2 = rc.x; dd[0].w = accW[dy].x;
            dd[1].c0 = ra1.x; dd[1].c1 = ra1.y; dd[1].c2 = rc.y; dd[1].w = accW[dy].y;
            const int fy = 2 * cy + dy;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                if constexpr (LAST) store_px<M, OUT_DST>(out_g, 2 * cx + dx, fy, dd[dx]);
                else of[fy - of_y0][2 * cx + dx - of_x0] = dd[dx];
            }
        }
        return;
    }
    const Up4<M> u = top2_pyr_up<M>([&](int rr, int cc) { return oc[lcy_b + rr][lcx_b + cc]; }, cx, lev_cw);
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

// top_restage (collapse_top.inc) on arrays of pitch T2_P
template <int M, int cw, int ch>
__device__ __forceinline__ void top2_restage(Px<M> (*lv)[T2_P], int x0, int y0, Px<M> (*oc)[T2_P], int cx0, int cy0, int lev_cw, int lev_ch) {
    constexpr int nstage = (ch + 2) * (cw + 2);
    for (int k = threadIdx.x; k < nstage; k += 256) {
        const int ry = k / (cw + 2), rx = k - ry * (cw + 2);
        const int gx = min(max(cx0 - 1 + rx, 0), lev_cw - 1), gy = up_row_map<M>(cy0 - 1 + ry, lev_ch);
        oc[ry][rx] = lv[gy - y0][gx - x0];
    }
}

template <int M>
#ifndef ISX_TOP2_WPE
#define ISX_TOP2_WPE 1       // (no occupancy request: 110 registers, four 4-wave blocks per CU by its 38.5 KB of LDS)
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ISX_TOP2_WPE))) void k_collapse_top2(TopTiles tt, LevelBuf out_g, int bx0, int top_rows, int top_cols) {
    constexpr int D = 3;
    // LDS, 38.5 KB = four blocks per CU, as k_collapse_top has (with every array on its own, 47.6 KB, three fit; measured: the same time): the staged Gaussians of both
    // tiles (A, F); one out-level buffer lv (a step reads the staged copy `oc` of the level before, never the level itself: its own output may
    // overwrite it); the staged out level oc.  Two arrays live where another is not in use yet / any more: the row-filtered G_{L-1} (hb: phase 1
    // only) in oc's place (first written in phase 2), and G_L (g3: phases 1 - first step) in lv's rows 8 .. 11, which only the SECOND step writes.
    constexpr unsigned SZ_A = 2u * T2_AH * T2_AW * 16u, SZ_F = 2u * T2_FH * T2_FW * 16u, SZ_OC = (T2_FH - 2) * T2_P * 16u, SZ_LV = T2_FH * T2_P * 16u;
    static_assert(sizeof(Px<M>) == 16 && SZ_OC >= 2u * T2_AH * T2_TW * 16u && SZ_LV - 8u * T2_P * 16u >= 2u * T2_TH * T2_TW * 16u, "the aliased arrays fit");
    static_assert(SZ_A + SZ_F + SZ_OC + SZ_LV <= 40960u, "four blocks per CU");
    __shared__ __attribute__((aligned(16))) unsigned char smem[SZ_A + SZ_F + SZ_OC + SZ_LV];
    Px<M> (*A)[T2_AH][T2_AW] = reinterpret_cast<Px<M> (*)[T2_AH][T2_AW]>(smem);
    Px<M> (*F)[T2_FH][T2_FW] = reinterpret_cast<Px<M> (*)[T2_FH][T2_FW]>(smem + SZ_A);
    Px<M> (*oc)[T2_P] = reinterpret_cast<Px<M> (*)[T2_P]>(smem + SZ_A + SZ_F);
    Px<M> (*hb)[T2_AH][T2_TW] = reinterpret_cast<Px<M> (*)[T2_AH][T2_TW]>(smem + SZ_A + SZ_F);
    Px<M> (*lv)[T2_P] = reinterpret_cast<Px<M> (*)[T2_P]>(smem + SZ_A + SZ_F + SZ_OC);
    Px<M> (*g3)[T2_TH][T2_TW] = reinterpret_cast<Px<M> (*)[T2_TH][T2_TW]>(smem + SZ_A + SZ_F + SZ_OC + 8u * T2_P * 16u);
    const int tid = threadIdx.x;
    const int X0 = (blockIdx.x + bx0) * TOP_BW, Y0 = blockIdx.y * TOP_BH;
    int ccx[D + 1], ccy[D + 1], ccw[D + 1], cch[D + 1];      // core regions of the steps, as in k_collapse_top
    ccx[1] = X0 / 2; ccy[1] = Y0 / 2; ccw[1] = TOP_BW / 2; cch[1] = TOP_BH / 2;
#pragma unroll
    for (int j = 2; j <= D; ++j) {
        const int xl = (ccx[j - 1] - 1) & ~1, xh = (ccx[j - 1] + ccw[j - 1] + 2) & ~1, yl = (ccy[j - 1] - 1) & ~1, yh = (ccy[j - 1] + cch[j - 1] + 2) & ~1;
        ccx[j] = xl >> 1; ccw[j] = (xh - xl) >> 1; ccy[j] = yl >> 1; cch[j] = (yh - yl) >> 1;
    }
    auto lev_w = [&](int j) { return top_cols << (D - j); };
    auto lev_h = [&](int j) { return top_rows << (D - j); };
    const int Tx0 = ccx[3] - 1, Ty0 = ccy[3] - 1;            // the top region (level L, mosaic coordinates): [Tx0, +12) x [Ty0, +6)
    const int Fx0 = 2 * ccx[2], Fy0 = 2 * ccy[2];            // the staged region of level L - 2: [Fx0, +36) x [Fy0, +12)
    Top2Tile T[2];
    LevelBuf G1[2], G2[2], G0[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        T[s].on = s < tt.n;
        const int t = s < tt.n ? s : 0;
#pragma unroll
        for (int j = 0; j <= D; ++j) { T[s].tx[j] = tt.x_tl[t] >> j; T[s].ty[j] = tt.y_tl[t] >> j; T[s].cw[j] = tt.w[t] >> j; T[s].ch[j] = tt.h[t] >> j; }
        // a tile further than the block's cone from it (less than 24 output-level pixels on either side) takes part in nothing
        T[s].on = T[s].on && !((T[s].tx[0] >= X0 + TOP_BW + 24) | (T[s].tx[0] + T[s].cw[0] <= X0 - 24) | (T[s].ty[0] >= Y0 + TOP_BH + 24) | (T[s].ty[0] + T[s].ch[0] <= Y0 - 24));
        G0[s] = top_level(tt, t, 0); G1[s] = top_level(tt, t, 1); G2[s] = top_level(tt, t, 2);
    }
    // ---- 0. every global load of the block ---------------------------------------------------------------------------------------------------
    // (a) G_{L-1} on tile-local columns ax0 .. ax0 + 26, rows ay0 .. ay0 + 14 through REFLECT_101 (what pyrDown reads for G_L on the top region;
    //     coordinates more than two pixels outside the tile only feed G_L pixels outside it, which nothing reads: clamped first)
    // Issue order = the order of use: G_{L-1} (needed first, 13 KB per block), then G_{L-2} and the thread's pixels of G_{L-3} (46 KB, needed by the
    // last two steps).  The counter of outstanding loads retires them in order, so the LDS copy of G_{L-1} below waits for ITS loads only and the
    // pyrDown / top / first-step phases run while the bulk is still on its way.
    // (no branch around any of these loads, not even the block-uniform 'this tile is far away': a branch between loads makes the compiler drain the
    // ones before it; a tile that takes no part is loaded at clamped addresses and never used - for a single tile s = 1 repeats tile 0)
    Px<M> av[2][2], fv[2][2], gg[2][2][2];
    int ax0[2], ay0[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        ax0[s] = 2 * (Tx0 - T[s].tx[3]) - 2; ay0[s] = 2 * (Ty0 - T[s].ty[3]) - 2;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int k = tid + 256 * it;
            if (k < T2_AW * T2_AH) {
                const int r = k / T2_AW, c = k - r * T2_AW;
                const int gx = reflect101(min(max(ax0[s] + c, -2), T[s].cw[2] + 1), T[s].cw[2]), gy = reflect101(min(max(ay0[s] + r, -2), T[s].ch[2] + 1), T[s].ch[2]);
                av[s][it] = load_px<M, false>(G2[s], gx, gy);
            }
        }
    }
    // (b) G_{L-2} on the mosaic region [Fx0, +36) x [Fy0, +12), where it lies inside the tile
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int k = tid + 256 * it;
            if (k < T2_FW * T2_FH) {
                const int r = k / T2_FW, c = k - r * T2_FW;
                // (entries outside the tile are never read: the load goes to a clamped address instead of sitting behind a per-lane branch - a
                // branch around a load makes the compiler wait for every load before it, one round trip after the other)
                const int fx = min(max(Fx0 + c - T[s].tx[1], 0), T[s].cw[1] - 1), fy = min(max(Fy0 + r - T[s].ty[1], 0), T[s].ch[1] - 1);
                fv[s][it] = load_px<M, false>(G1[s], fx, fy);
            }
        }
    }
    // (c) the thread's own 2 x 2 pixels of G_{L-3} (the last step's fine level)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        // (a thread whose coarse pixel lies outside the tile never uses these: clamped address, no branch)
        const int lcx = min(max(ccx[1] + (tid & 31) - T[s].tx[1], 0), T[s].cw[1] - 1), lcy = min(max(ccy[1] + (tid >> 5) - T[s].ty[1], 0), T[s].ch[1] - 1);
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) gg[s][dy][dx] = load_px<M, false>(G0[s], 2 * lcx + dx, 2 * lcy + dy);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int k = tid + 256 * it;
            if (k < T2_AW * T2_AH) { const int r = k / T2_AW, c = k - r * T2_AW; A[s][r][c] = av[s][it]; }
        }
    }
    __syncthreads();
    // ---- 1. G_L = pyrDown(G_{L-1}) on the top region: row filter, column filter (k_pyr_down_multi's functions and index maps) ------------------
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (!T[s].on) continue;
        const int vt = tid;
        if (vt < T2_AH * T2_TW) {
            const int r = vt / T2_TW, x = vt - r * T2_TW;
            hb[s][r][x] = pyr_down_row5<M>(A[s][r][2 * x + 2], A[s][r][2 * x + 1], A[s][r][2 * x + 3], A[s][r][2 * x], A[s][r][2 * x + 4]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (!T[s].on) continue;
        const int vt = tid;
        if (vt < T2_TH * T2_TW) {
            const int y = vt / T2_TW, x = vt - y * T2_TW;
            g3[s][y][x] = top2_storage_round<M>(pyr_down_col5<M>(hb[s][2 * y][x], hb[s][2 * y + 1][x], hb[s][2 * y + 2][x], hb[s][2 * y + 3][x], hb[s][2 * y + 4][x]));
        }
    }
    __syncthreads();
    // G_L of tile s at tile-local (gx, gy) (inside the tile and - by construction of every reader - inside the top region; the index is clamped
    // for the neighbourhood entries of threads that own no pixel)
    auto top_of = [&](int s, int gx, int gy) -> Px<M> {
        const int ix = min(max(gx + T[s].tx[3] - Tx0, 0), T2_TW - 1), iy = min(max(gy + T[s].ty[3] - Ty0, 0), T2_TH - 1);
        return g3[s][iy][ix];
    };
    // ---- 2. the top level out_L on the halo region of the first step's core, clamped to the level (k_collapse_top's expressions) --------------
    {
        const int x0 = max(ccx[D] - 1, 0), y0 = max(ccy[D] - 1, 0), x1 = min(ccx[D] + ccw[D] + 1, lev_w(D)), y1 = min(ccy[D] + cch[D] + 1, lev_h(D));
        const int rw = max(x1 - x0, 0), rh = max(y1 - y0, 0);
        for (int k = tid; k < rw * rh; k += 256) {
            const int ry = k / rw, rx = k - ry * rw, x = x0 + rx, y = y0 + ry;
            Px<M> d; d.c0 = 0; d.c1 = 0; d.c2 = 0; d.w = 0.f;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (!T[s].on) continue;
                const int lx = x - T[s].tx[3], ly = y - T[s].ty[3];
                if ((unsigned)lx < (unsigned)T[s].cw[3] && (unsigned)ly < (unsigned)T[s].ch[3]) {
                    const Px<M> g = top_of(s, lx, ly);
                    if constexpr (M == M_I16) {
                        d.c0 = wrap_s16(d.c0 + f2s_x86((float)g.c0 * g.w)); d.c1 = wrap_s16(d.c1 + f2s_x86((float)g.c1 * g.w)); d.c2 = wrap_s16(d.c2 + f2s_x86((float)g.c2 * g.w));
                    } else { d.c0 = d.c0 + g.c0 * g.w; d.c1 = d.c1 + g.c1 * g.w; d.c2 = d.c2 + g.c2 * g.w; }
                    d.w = d.w + g.w;
                }
            }
            normalise<M>(d);
            lv[ry][rx] = d;
        }
        __syncthreads();
        top2_restage<M, 10, 4>(lv, x0, y0, oc, ccx[3], ccy[3], lev_w(3), lev_h(3));
        __syncthreads();
    }
    // ---- 3. the three steps, every operand out of LDS / registers --------------------------------------------------------------------------
    // level L - 1 of tile s at tile-local coordinates: the staged A (no reflection inside the tile)
    auto a_of = [&](int s, int gx, int gy) -> Px<M> {
        const int ix = min(max(gx - ax0[s], 0), T2_AW - 1), iy = min(max(gy - ay0[s], 0), T2_AH - 1);
        return A[s][iy][ix];
    };
    auto f_of = [&](int s, int gx, int gy) -> Px<M> {
        const int ix = min(max(gx + T[s].tx[1] - Fx0, 0), T2_FW - 1), iy = min(max(gy + T[s].ty[1] - Fy0, 0), T2_FH - 1);
        return F[s][iy][ix];
    };
    top2_step<M, false, 10, 4>(T, 3, [&](int s, int fx, int fy, int, int) { return a_of(s, fx, fy); }, top_of, oc, lv, 2 * ccx[3], 2 * ccy[3], out_g, ccx[3], ccy[3], lev_w(3), lev_h(3));
    // G_{L-2} goes to LDS now (its loads have had the phases above to arrive); the two barriers before the next step publish it
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int k = tid + 256 * it;
            if (k < T2_FW * T2_FH) { const int r = k / T2_FW, c = k - r * T2_FW; F[s][r][c] = fv[s][it]; }
        }
    }
    __syncthreads();
    top2_restage<M, 18, 6>(lv, 2 * ccx[3], 2 * ccy[3], oc, ccx[2], ccy[2], lev_w(2), lev_h(2));
    __syncthreads();
    top2_step<M, false, 18, 6>(T, 2, [&](int s, int fx, int fy, int, int) { return f_of(s, fx, fy); }, a_of, oc, lv, 2 * ccx[2], 2 * ccy[2], out_g, ccx[2], ccy[2], lev_w(2), lev_h(2));
    __syncthreads();
    top2_restage<M, 32, 8>(lv, 2 * ccx[2], 2 * ccy[2], oc, ccx[1], ccy[1], lev_w(1), lev_h(1));
    __syncthreads();
    top2_step<M, true, 32, 8>(T, 1, [&](int s, int, int, int dx, int dy) { return gg[s][dy][dx]; }, f_of, oc, lv, 0, 0, out_g, ccx[1], ccy[1], lev_w(1), lev_h(1));
}
