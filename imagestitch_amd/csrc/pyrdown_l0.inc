// pyrdown_l0.inc — level 0 -> 1 of the tile pyramids for CV_8UC3 and CV_16SC3 tiles (included by blend.hip inside its anonymous namespace, after
// collapse_roll.inc whose global-pointer types and scalar-base idiom it uses).
//
//   G_1 = pyrDown(G_0),  G_0 = copyMakeBorder(tile, REFLECT) as int16 / fp32, W_0 = copyMakeBorder(mask, CONSTANT 0) * (1 / 255)
//   (MultiBandBlender::feed -> createLaplacePyr / pyrDown of the weight map; SURVEY §8(a) A10, A11)
//
// k_pyr_down_multi<M, SK_U8> is bound by instruction issue (profiles/round3a_pmc_f32.txt: 498 VALU per wave, 76 % VALU-busy): per input
// row a lane tests whether its pair of pixels lies inside the tile, builds two 64-bit addresses, realigns a 12-byte and an 8-byte window
// with v_alignbyte, and fetches its three neighbour taps with twelve v_mov_dpp before twelve packed operations filter them.
// Here a block whose 35 x 128 input pixels all lie inside the tile, off its last row (one scalar test per block; nine blocks in ten of a 4K
// tile) takes a straight-line path: every row base is a scalar, the lane's two offsets are computed once, the six image bytes are ONE
// byte-misaligned global_load_dwordx2 and the two mask bytes ONE global_load_ushort (as in k_collapse_roll), and the neighbour taps are
// DPP operands of the filter's own additions (v_add_f32_dpp wave_shr:1 / wave_shl:1).  Same operations in the same order per pixel as
// pyr_down_block: identical bits.  Blocks on the tile's rim run pyr_down_block itself.
// CV_16SC3 tiles (what Blender::feed receives in the reference, W:294,302): the same path with the pair's 12 bytes as ONE
// global_load_dwordx3 at a 2-byte aligned address (collapse_roll.inc: RollWin).
// o[k] = x[k] + (src[k] of the lane below / above; 0 beyond the wave's ends), four at a time: v_add_*_dpp wave_shr:1 / wave_shl:1 written
// out.  The compiler folds __builtin_amdgcn_update_dpp into the addition only in some of the unrolled rows (the others become v_mov_dpp +
// v_add, 24 more instructions per row and enough live registers to spill); the s_nop covers the two wait states a DPP read needs
// after a VALU write of its source, which nobody inserts around inline assembly.
#define PD0_DPP4(NAME, OP, CTRL, T)                                                                                                      \
    __device__ __forceinline__ void NAME(T (&o)[4], const T (&src)[4], const T (&x)[4]) {                                               \
        asm("s_nop 1\n\t" OP " %0, %4, %8 " CTRL " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" OP " %1, %5, %9 " CTRL                \
            " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" OP " %2, %6, %10 " CTRL " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" OP  \
            " %3, %7, %11 " CTRL " row_mask:0xf bank_mask:0xf bound_ctrl:1"                                                             \
            : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3])                                                                        \
            : "v"(src[0]), "v"(src[1]), "v"(src[2]), "v"(src[3]), "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]));                          \
    }
PD0_DPP4(pd0_add_lower, "v_add_f32_dpp", "wave_shr:1", float)
PD0_DPP4(pd0_add_upper, "v_add_f32_dpp", "wave_shl:1", float)
#undef PD0_DPP4

// One row of pyrDown's row filter for this lane's output column from its level-0 window (w = the six channel values of pixels 2x, 2x + 1;
// mk = their two mask bytes); pixels 2x - 2, 2x - 1 and 2x + 2 are the neighbour lanes'.
// tap5(c = A, l1 = B of the lane below, r1 = B, l2 = A of the lane below, r2 = A of the lane above) = ((c * 6 + (l1 + r1) * 4) + l2) + r2
template <int M>
__device__ __forceinline__ Px<M> pd0_hfilter(const float (&a)[4], const float (&b)[4]) {
    static_assert(M != M_I16, "the int16 arithmetic takes this path as integer-valued floats (k_pyr_down0)");
    Px<M> h;
    float s[4], u[4], v[4];
    pd0_add_lower(s, b, b);
    const f32x2 t0 = f32x2{a[0], a[1]} * splat2(6.f) + f32x2{s[0], s[1]} * splat2(4.f);
    const f32x2 t1 = f32x2{a[2], a[3]} * splat2(6.f) + f32x2{s[2], s[3]} * splat2(4.f);
    const float t[4] = {t0.x, t0.y, t1.x, t1.y};
    pd0_add_lower(u, a, t);
    pd0_add_upper(v, a, u);
    h.c0 = v[0]; h.c1 = v[1]; h.c2 = v[2]; h.w = v[3];
    return h;
}
template <int M, int SK>
__device__ __forceinline__ Px<M> pd0_hrow(const RollWin<SK>& w, unsigned mk) {
    const float inv255 = (float)(1. / 255.);
    int p0[3], p1[3];
    roll_win_decode<SK>(w, false, p0, p1);
    const float a[4] = {(float)p0[0], (float)p0[1], (float)p0[2], (float)(mk & 255u) * inv255};
    const float b[4] = {(float)p1[0], (float)p1[1], (float)p1[2], (float)((mk >> 8) & 255u) * inv255};
    return pd0_hfilter<M>(a, b);
}
// the same from a window on the level's or the tile's rim: the lane's pixels swapped or doubled inside the window (fl bits 1, 2: pixel a / b is
// the window's second), no weight outside the tile (bits 3, 4: a / b inside its columns; wrow: the row inside its rows), the last row's
// CV_8UC3 window loaded two bytes early (`shifted`) - collapse_roll.inc's scheme for copyMakeBorder's reflected columns
template <int M, int SK>
__device__ __forceinline__ Px<M> pd0_hrow_rim(const RollWin<SK>& w, unsigned mk, bool shifted, unsigned fl, bool wrow) {
    const float inv255 = (float)(1. / 255.);
    int p0[3], p1[3];
    roll_win_decode<SK>(w, shifted, p0, p1);
    const bool asec = fl & 2u, bsec = fl & 4u, wa = (fl & 8u) && wrow, wb = (fl & 16u) && wrow;
    const int m0 = mk & 255, m1 = (mk >> 8) & 255;
    const float a[4] = {(float)(asec ? p1[0] : p0[0]), (float)(asec ? p1[1] : p0[1]), (float)(asec ? p1[2] : p0[2]), (float)(wa ? (asec ? m1 : m0) : 0) * inv255};
    const float b[4] = {(float)(bsec ? p1[0] : p0[0]), (float)(bsec ? p1[1] : p0[1]), (float)(bsec ? p1[2] : p0[2]), (float)(wb ? (bsec ? m1 : m0) : 0) * inv255};
    return pd0_hfilter<M>(a, b);
}

// NR input rows from row `row0` of the padded level 0 (all inside the tile, off its last row), for the output column `ox` of this lane
template <int M, int SK, int NR>
__device__ __forceinline__ void pd0_interior_rows(const Src0& s0, int ox, int row0, Px<M> (*hb)[WAVE]) {
    constexpr int RPW = (NR + PD_WAVES - 1) / PD_WAVES;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned xr = (unsigned)(2 * ox - s0.left);                      // the lane's pixels xr, xr + 1 of every row
    const unsigned l_io = xr * roll_px_bytes<SK>(), l_mo = xr;
    const int yr0 = row0 - s0.top;
    const unsigned istep = (unsigned)s0.img_step, mstep = (unsigned)s0.mask_step;
    const gcp img = roll_sgpr((gcp)s0.img), msk = roll_sgpr((gcp)s0.mask);     // the bases once, in scalar registers (not re-read from the arguments per row)
    RollWin<SK> rv[RPW];
    unsigned rm[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {      // every load of the wave before the first use
        const int r = wv + PD_WAVES * i;
        rv[i] = RollWin<SK>{}; rm[i] = 0;
        if (r < NR) {
            const unsigned yr = (unsigned)(yr0 + r);
            if constexpr (SK == SK_S16) {
                const u32x3_a2 t = *(ROLL_G(u32x3_a2))(roll_sgpr(img + (size_t)(yr * istep)) + l_io);
                rv[i].x = t.x; rv[i].y = t.y; rv[i].z = t.z;
            } else {
                const u32x2_a1 t = *(ROLL_G(u32x2_a1))(roll_sgpr(img + (size_t)(yr * istep)) + l_io);
                rv[i].x = t.x; rv[i].y = t.y;
            }
            rm[i] = *(ROLL_G(u16_a1))(roll_sgpr(msk + (size_t)(yr * mstep)) + l_mo);
        }
    }
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const int r = wv + PD_WAVES * i;
        if (r < NR) {
            const Px<M> h = pd0_hrow<M, SK>(rv[i], rm[i]);
            hb[r][lane] = h;
        }
    }
}

// ISX_PREC_I16 on the straight-line path: OpenCV's CV_16S pyrDown - (sum + 128) >> 8 of integer taps - carried on integer-valued floats.
// Every sum is below 2^24 (256 x 32767), so the float row and column filters are exact and the rounding shift is floor(fma(sum, 1 / 256, 0.5));
// the weight plane is fp32 in both arithmetics.  The row phase is then the float modes' (one group of DPP additions for image and weight
// instead of two), the column phase two packed filters + three floors and three conversions.  Same numbers as pyr_down_col5<M_I16>.
__device__ __forceinline__ Px<M_I16> pd0_col5_ix(const Px<M_F32>& r0, const Px<M_F32>& r1, const Px<M_F32>& r2, const Px<M_F32>& r3, const Px<M_F32>& r4) {
    const f32x2 s0 = (((f32x2{r2.c0, r2.c1} * splat2(6.f) + (f32x2{r1.c0, r1.c1} + f32x2{r3.c0, r3.c1}) * splat2(4.f)) + f32x2{r0.c0, r0.c1}) + f32x2{r4.c0, r4.c1});
    const f32x2 s1 = (((f32x2{r2.c2, r2.w} * splat2(6.f) + (f32x2{r1.c2, r1.w} + f32x2{r3.c2, r3.w}) * splat2(4.f)) + f32x2{r0.c2, r0.w}) + f32x2{r4.c2, r4.w});
    const f32x2 q0 = pk_fma(s0, splat2(1.f / 256.f), splat2(0.5f)), q1 = pk_fma(s1, splat2(1.f / 256.f), splat2(0.5f)), w1 = s1 * splat2(1.f / 256.f);
    Px<M_I16> o;
    o.c0 = (int)__builtin_floorf(q0.x); o.c1 = (int)__builtin_floorf(q0.y); o.c2 = (int)__builtin_floorf(q1.x); o.w = w1.y;
    return o;
}
template <int PLD>
__device__ __forceinline__ void pd0_columns_ix(Px<M_F32> (*hb)[WAVE], const LevelBuf& dst, int ox, int oy0, int lane, int wv) {
    const int dw = dst.cols, dh = dst.rows;
    if (lane == 0 || lane == 63 || ox >= dw) return;
#pragma unroll
    for (int i = 0; i < PD_TY / PD_WAVES; ++i) {
        const int ty = wv + PD_WAVES * i, oy = oy0 + ty;
        if (oy >= dh) break;
        const Px<M_I16> o = pd0_col5_ix(hb[2 * ty][lane], hb[2 * ty + 1][lane], hb[2 * ty + 2][lane], hb[2 * ty + 3][lane], hb[2 * ty + 4][lane]);
        if constexpr (PLD) store_px_planar<M_I16>(dst, ox, oy, o);
        else store_px<M_I16, false>(dst, ox, oy, o);
    }
}

// Waves per SIMD the level-0 pyrDown is compiled for.  6 (rounds 3 - 5: three 8-wave blocks per CU) was set when every block took the LDS path;
// since the rim runs as single-wave strips and level 1 leaves as shorts, 8 (64 registers, four blocks per CU; the fp32 / fp16 CV_8UC3 forms
// spill 8 dwords in the rim strips) is 2.2 us faster per launch in five of five same-box alternations (27.9 -> 25.7 us serialised,
// profiles/round6_retune.txt; 7: 27.4; 4: 32.8).
#ifndef ISX_PD0_WPE
#define ISX_PD0_WPE 8
#endif
// PLD: level 1 is written PLANAR (blend.hip, load_px_planar); 2: in Q8 records (fp32 pyramids over CV_8UC3 tiles)
// A RIM block of k_pyr_down0 (the level's REFLECT_101 border, the tile's copyMakeBorder columns and rows) as eight single-wave strips of two output
// rows - k_feed_strip's rim scheme without its copy: the lane's two taps of a row lie in ONE window of two adjacent tile pixels (possibly swapped or
// doubled: flags), the rows go through the same two maps as scalars; every row index is computed BEFORE the first load (control flow between loads
// drains them) and the strip makes one memory round trip, no LDS, no barrier.  The block-wide generic path it replaces (pyr_down_block: per-pixel
// byte loads wherever a window does not fit) made a tenth of the blocks cost a seventh of the launch (a timing-only build that skipped the rim blocks, since removed).
template <int M, int SK, int PLD>
__device__ __forceinline__ void pd0_rim_wave(const Src0& s0, const LevelBuf& dst, int bx, int oy0) {
    constexpr int NO = 2, NR = 2 * NO + 3;
    constexpr int MWK = M == M_I16 ? M_F32 : M;
    const int lane = threadIdx.x & 63;
    const int ox = bx * PD_OW + lane - 1, row0 = 2 * oy0 - 2;
    const unsigned istep = (unsigned)s0.img_step, mstep = (unsigned)s0.mask_step;
    const gcp img = roll_sgpr((gcp)s0.img), msk = roll_sgpr((gcp)s0.mask);
    const bool own = (lane >= 1) & (lane <= PD_OW);
    const int sw = s0.width, sh = s0.height;
    const int oxc = min(max(ox, -1), dst.cols);               // (lanes further out feed nobody)
    int cA = 2 * oxc, cB = 2 * oxc + 1;
    cA = cA < 0 ? -cA : (cA >= sw ? 2 * sw - 2 - cA : cA);
    cB = cB < 0 ? -cB : (cB >= sw ? 2 * sw - 2 - cB : cB);
    const int qa = cA - s0.left, qb = cB - s0.left;
    const int xa = roll_reflect(qa, s0.cols), xb = roll_reflect(qb, s0.cols);
    const int xw = min(min(xa, xb), s0.cols - 2);
    const unsigned fl = (xa != xw ? 2u : 0u) | (xb != xw ? 4u : 0u) | ((unsigned)qa < (unsigned)s0.cols ? 8u : 0u) | ((unsigned)qb < (unsigned)s0.cols ? 16u : 0u);
    const unsigned l_io = (unsigned)xw * roll_px_bytes<SK>(), l_mo = (unsigned)xw;
    int ryv[NR];
    bool wrow[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        int pr = row0 + r;
        pr = pr < 0 ? -pr : (pr >= sh ? 2 * sh - 2 - pr : pr);
        pr = min(max(pr, 0), sh - 1);                            // (a strip below the level's last row: rows nobody stores)
        wrow[r] = (unsigned)(pr - s0.top) < (unsigned)s0.rows;
        ryv[r] = roll_reflect(pr - s0.top, s0.rows);
    }
    RollWin<SK> rv[NR];
    unsigned rm[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int ry = ryv[r];
        if constexpr (SK == SK_S16) {
            const u32x3_a2 t = *(ROLL_G(u32x3_a2))(roll_sgpr(img + (size_t)((unsigned)ry * istep)) + l_io);
            rv[r].x = t.x; rv[r].y = t.y; rv[r].z = t.z;
        } else {
            const unsigned back = ry == s0.rows - 1 ? 2u : 0u;      // the last row's window starts two bytes early (the last pair's would pass the end of the buffer)
            const u32x2_a1 t = *(ROLL_G(u32x2_a1))(roll_sgpr(img + (size_t)((unsigned)ry * istep - back)) + l_io);
            rv[r].x = t.x; rv[r].y = t.y;
        }
        rm[r] = *(ROLL_G(u16_a1))(roll_sgpr(msk + (size_t)((unsigned)ry * mstep)) + l_mo);
    }
    Px<MWK> h[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) h[r] = pd0_hrow_rim<MWK, SK>(rv[r], rm[r], SK != SK_S16 && ryv[r] == s0.rows - 1, fl, wrow[r]);
    if (own && ox < dst.cols) {
#pragma unroll
        for (int i = 0; i < NO; ++i) {
            const int oy = oy0 + i;
            if (oy < dst.rows) {
                if constexpr (M == M_I16) {
                    const Px<M_I16> o = pd0_col5_ix(h[2 * i], h[2 * i + 1], h[2 * i + 2], h[2 * i + 3], h[2 * i + 4]);
                    if constexpr (PLD) store_px_planar<M_I16>(dst, ox, oy, o); else store_px<M_I16, false>(dst, ox, oy, o);
                } else {
                    const Px<M> o = pyr_down_col5<M>(h[2 * i], h[2 * i + 1], h[2 * i + 2], h[2 * i + 3], h[2 * i + 4]);
                    if constexpr (PLD != 0) store_px_planar<M, PLD == 2>(dst, ox, oy, o); else store_px<M, false>(dst, ox, oy, o);
                }
            }
        }
    }
}

template <int M, int SK, int PLD, class TS>
__device__ __forceinline__ void pyr_down0_body(const TS& ts) {
    static_assert(SK == SK_U8 || SK == SK_S16, "CV_8UC3 or CV_16SC3 tiles");
    // blockIdx.z = tile; ts.s0 = the caller's tiles, ts.coarse = level 1 of their pyramids (as k_pyr_down_multi<M, SK>)
    // Workgroups go to the 8 XCDs round robin in dispatch order (x fastest, then y, then z).  A block's rows are 372 image bytes and 124 mask
    // bytes long - no multiple of a 128-byte line - so horizontal neighbours share their boundary lines, vertical neighbours three rows of
    // halo: XCD k takes the k-th eighth of the blocks in (tile, row, column) order, so that neighbours run on the same XCD one after the other
    // and find the shared lines in its L2 instead of fetching them again.
    const unsigned gx = gridDim.x, gxy = gx * gridDim.y, L = gxy * gridDim.z;
    const unsigned lin = blockIdx.z * gxy + blockIdx.y * gx + blockIdx.x;
    const unsigned k = lin & 7u, chunk = L >> 3, rem = L & 7u;
    const unsigned j = k * chunk + (k < rem ? k : rem) + (lin >> 3);
    const int t = (int)(j / gxy);
    const unsigned r = j - (unsigned)t * gxy;
    const int by = (int)(r / gx), bx = (int)(r - (unsigned)by * gx);
    const LevelBuf dst = ts.coarse[t];
    if (bx * PD_OW >= dst.cols || by * PD_TY >= dst.rows || bx < ts.bx_lo[t] || bx >= ts.bx_hi[t]) return;
    __shared__ Px<M> hb[PD_NR][WAVE];
    const Src0& s0 = ts.s0[t];
    // columns of lanes 0 .. 63 and rows 0 .. PD_NR - 1 of the block, in tile coordinates
    const int x_lo = 2 * (bx * PD_OW - 1) - s0.left, x_hi = 2 * (bx * PD_OW + WAVE - 2) + 1 - s0.left;
    const int y_lo = 2 * by * PD_TY - 2 - s0.top, y_hi = y_lo + PD_NR - 1;
    // CV_8UC3: off the tile's last row - a lane's 8-byte window holds 2 bytes of the next pixel (or of the next row); iend != 0: the tile is below 2 GiB
    const bool interior = x_lo >= 0 && x_hi < s0.cols && y_lo >= 0 && y_hi < s0.rows - (SK == SK_S16 ? 0 : 1) && s0.iend != 0u;
    if (!interior) {
        if (s0.iend != 0u && s0.cols >= 2 && s0.rows >= 2 && s0.width >= 4 && s0.height >= 4) {
            static_assert(PD_TY == 2 * PD_WAVES, "eight waves x two output rows = one block");
            pd0_rim_wave<M, SK, PLD>(s0, dst, bx, by * PD_TY + 2 * __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)));
            return;
        }
        pyr_down_block<M, SK, 0, PLD>(s0, ts.fine[t], dst, bx, by, hb);
        return;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if constexpr (M == M_I16) {       // integer-valued floats (pd0_columns_ix); the records in LDS have the size of the integer ones
        static_assert(sizeof(Px<M_F32>) == sizeof(Px<M_I16>), "one LDS array for both forms");
        Px<M_F32>(*hf)[WAVE] = reinterpret_cast<Px<M_F32>(*)[WAVE]>(hb);
        pd0_interior_rows<M_F32, SK, PD_NR>(s0, bx * PD_OW + lane - 1, 2 * by * PD_TY - 2, hf);
        __syncthreads();
        pd0_columns_ix<PLD>(hf, dst, bx * PD_OW + lane - 1, by * PD_TY, lane, wv);
    } else {
        pd0_interior_rows<M, SK, PD_NR>(s0, bx * PD_OW + lane - 1, 2 * by * PD_TY - 2, hb);
        __syncthreads();
        pyr_down_columns<M, PLD>(hb, dst, bx * PD_OW + lane - 1, by * PD_TY, lane, wv);
    }
}
template <int M, int SK, int PLD = 0>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(ISX_PD0_WPE, ISX_PD0_WPE))) void k_pyr_down0(TileSet ts) { pyr_down0_body<M, SK, PLD>(ts); }
// ... the tiles in a device-resident table (more than DEF_MAX of them)
template <int M, int SK, int PLD = 0>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(ISX_PD0_WPE, ISX_PD0_WPE))) void k_pyr_down0_tab(TileTab ts) { pyr_down0_body<M, SK, PLD>(ts); }

// ------------------------------------------------------------------------------------------------------------------------------------
// k_feed_pd0 - feed() of a recorded CV_8UC3 / CV_16SC3 device tile under OpenCV's contract (isx_blender_set_deferred_level0 = 2: the
// caller may release or overwrite the fed mats as soon as feed() returns, W:305-308).  Round 4 made a private copy of image and mask
// (k_copy_rows: 57.5 us per 4K pair of CV_16SC3 tiles) and read it again in blend() for the level-0 pyrDown (43 us).  Here ONE pass per
// tile reads the caller's tile + mask once and writes G_1 = pyrDown(G_0) (exactly k_pyr_down0's arithmetic: same device functions) AND
// the private copy out of the windows it holds in registers anyway: every block stores the pixels of the padded rows [32 by, + 32) x
// columns [124 bx, + 124) it owns that lie inside the tile; blocks on the tile's rim copy theirs pixel by pixel.
// CF_NARROW (CV_16SC3 tiles): the copy is written as CV_8UC3 - what the tile is after convertTo(CV_16S) of a warped CV_8UC3 image
// (W:294) - so that everything downstream takes the CV_8UC3 kernels (the last collapse step reads 3 instead of 6 bytes per pixel).
// A row segment (one wave, one row, 124 pixels) that holds a value outside [0, 255] goes to a CV_16SC3 escape buffer instead and says
// so in a byte map; blend() publishes {violation seen, sequence number} in pinned host memory with its first launch (k_feed_publish) and reads
// it before it picks the last step's kernel (no stream synchronisation: by then that launch is long over).  A violated cycle is widened from
// copy + escape segments (k_feed_widen) and blended by the CV_16SC3 kernels: same bits either way.
// ------------------------------------------------------------------------------------------------------------------------------------
enum { CF_SAME = 0, CF_NARROW = 1 };
// Measured and left out (profiles/round5_feed_ab.txt, same box, alternating): non-temporal loads of the caller's tile (read once by contract) -
// the pass 5-6 us slower per pair (they miss what convertTo just left in the Infinity Cache), the last collapse step 3 us faster (the private
// copies stay cached): level; a lane's 6 copy bytes as ONE overlapping 8-byte store instead of 4 + 2: -1 us, inside the noise.
struct FeedCopy {
    unsigned char* cimg; unsigned cstep;        // the private copy of the image: CV_8UC3 (CF_NARROW, or a CV_8UC3 tile) or CV_16SC3
    unsigned char* wimg; unsigned wstep;        // CF_NARROW: CV_16SC3 escape buffer (row segments that hold a non-byte value)
    unsigned char* cmask; unsigned cmstep;      // the private copy of the mask
    unsigned char* chunk; int nbx;              // CF_NARROW: chunk[yr * nbx + bx] = 1: columns [124 bx - left, + 124) of tile row yr are in the escape buffer
    unsigned* state;                            // CF_NARROW: the tile's device word "a segment escaped" (zero before the launch; k_feed_publish reads and clears it)
};
typedef unsigned u32_a1 __attribute__((aligned(1)));

// one lane's pixel pair of tile row yr (columns xr, xr + 1, both inside the tile) out of its loaded window; uniform `viol` on return
template <int SK, int CF>
__device__ __forceinline__ bool feed_copy_window(const FeedCopy& fc, const RollWin<SK>& w, unsigned mk, unsigned yr, unsigned xr, int bx, bool own, int lane) {
    bool viol = false;
    if constexpr (SK == SK_S16 && CF == CF_NARROW) {
        viol = __builtin_amdgcn_ballot_w64(own & (((w.x | w.y | w.z) & 0xff00ff00u) != 0u)) != 0ull;
        if (!viol) {
            const gp crow = roll_sgpr((gp)fc.cimg + (size_t)(yr * fc.cstep));
            if (own) {
                *(ROLL_GW(u32_a1))(crow + 3u * xr) = __builtin_amdgcn_perm(w.y, w.x, 0x06040200u);
                *(ROLL_GW(u16_a1))(crow + 3u * xr + 4u) = (unsigned short)((w.z & 255u) | ((w.z >> 8) & 0xff00u));
            }
        } else {
            const gp wrow = roll_sgpr((gp)fc.wimg + (size_t)(yr * fc.wstep));
            if (own) *(ROLL_GW(u32x3_a2))(wrow + 6u * xr) = u32x3_a2{w.x, w.y, w.z};
        }
        if (lane == 1) fc.chunk[(size_t)yr * (unsigned)fc.nbx + (unsigned)bx] = viol ? 1 : 0;
    } else if constexpr (SK == SK_S16) {
        const gp crow = roll_sgpr((gp)fc.cimg + (size_t)(yr * fc.cstep));
        if (own) *(ROLL_GW(u32x3_a2))(crow + 6u * xr) = u32x3_a2{w.x, w.y, w.z};
    } else {
        const gp crow = roll_sgpr((gp)fc.cimg + (size_t)(yr * fc.cstep));
        if (own) {
            *(ROLL_GW(u32_a1))(crow + 3u * xr) = w.x;
            *(ROLL_GW(u16_a1))(crow + 3u * xr + 4u) = (unsigned short)(w.y & 0xffffu);
        }
    }
    const gp mrow = roll_sgpr((gp)fc.cmask + (size_t)(yr * fc.cmstep));
    if (own) *(ROLL_GW(u16_a1))(mrow + xr) = (unsigned short)mk;
    return viol;
}

// pd0_interior_rows with the copy of the rows the block owns (local rows 2 .. PD_NR - 2): the windows are in registers already
template <int M, int SK, int CF>
__device__ __forceinline__ bool feed_interior_rows(const Src0& s0, const FeedCopy& fc, int bx, int ox, int row0, Px<M> (*hb)[WAVE]) {
    constexpr int RPW = (PD_NR + PD_WAVES - 1) / PD_WAVES;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned xr = (unsigned)(2 * ox - s0.left);
    const unsigned l_io = xr * roll_px_bytes<SK>(), l_mo = xr;
    const int yr0 = row0 - s0.top;
    const unsigned istep = (unsigned)s0.img_step, mstep = (unsigned)s0.mask_step;
    const gcp img = roll_sgpr((gcp)s0.img), msk = roll_sgpr((gcp)s0.mask);
    const bool own = (lane >= 1) & (lane <= PD_OW);
    RollWin<SK> rv[RPW];
    unsigned rm[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const int r = wv + PD_WAVES * i;
        rv[i] = RollWin<SK>{}; rm[i] = 0;
        if (r < PD_NR) {
            const unsigned yr = (unsigned)(yr0 + r);
            if constexpr (SK == SK_S16) {
                const u32x3_a2 t = *(ROLL_G(u32x3_a2))(roll_sgpr(img + (size_t)(yr * istep)) + l_io);
                rv[i].x = t.x; rv[i].y = t.y; rv[i].z = t.z;
            } else {
                const u32x2_a1 t = *(ROLL_G(u32x2_a1))(roll_sgpr(img + (size_t)(yr * istep)) + l_io);
                rv[i].x = t.x; rv[i].y = t.y;
            }
            rm[i] = *(ROLL_G(u16_a1))(roll_sgpr(msk + (size_t)(yr * mstep)) + l_mo);
        }
    }
    bool viol = false;
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const int r = wv + PD_WAVES * i;
        if (r < PD_NR) {
            if (r >= 2 && r < PD_NR - 1) viol |= feed_copy_window<SK, CF>(fc, rv[i], rm[i], (unsigned)(yr0 + r), xr, bx, own, lane);
            const Px<M> h = pd0_hrow<M, SK>(rv[i], rm[i]);
            hb[r][lane] = h;
        }
    }
    return viol;
}

// the copy of a rim block's owned pixels that lie inside the tile, pixel by pixel (one block in ten of a 4K tile)
template <int SK, int CF>
__device__ __forceinline__ bool feed_copy_rim(const Src0& s0, const FeedCopy& fc, int bx, int by) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int xr = 2 * (bx * PD_OW + lane - 1) - s0.left;
    const bool own = (lane >= 1) & (lane <= PD_OW);
    const bool in0 = own & ((unsigned)xr < (unsigned)s0.cols), in1 = own & ((unsigned)(xr + 1) < (unsigned)s0.cols);
    const unsigned long long any_in = __builtin_amdgcn_ballot_w64(in0 | in1);
    if (any_in == 0ull) return false;
    const int first = __builtin_ctzll(any_in);
    bool viol_any = false;
    for (int r = wv; r < 2 * PD_TY; r += PD_WAVES) {
        const int yr = 2 * by * PD_TY + r - s0.top;
        if ((unsigned)yr >= (unsigned)s0.rows) continue;
        const unsigned char* irow = s0.img + (size_t)yr * s0.img_step;
        const unsigned char* mrow = s0.mask + (size_t)yr * s0.mask_step;
        int v[2][3] = {{0, 0, 0}, {0, 0, 0}};
        unsigned m[2] = {0u, 0u};
#pragma unroll
        for (int p = 0; p < 2; ++p)
            if (p == 0 ? in0 : in1) {
                if constexpr (SK == SK_S16) { const short* q = (const short*)irow + (size_t)(xr + p) * 3; v[p][0] = q[0]; v[p][1] = q[1]; v[p][2] = q[2]; }
                else { const unsigned char* q = irow + (size_t)(xr + p) * 3; v[p][0] = q[0]; v[p][1] = q[1]; v[p][2] = q[2]; }
                m[p] = mrow[xr + p];
            }
        bool viol = false;
        if constexpr (SK == SK_S16 && CF == CF_NARROW) {
            const bool bad = (((unsigned)(v[0][0] | v[0][1] | v[0][2] | v[1][0] | v[1][1] | v[1][2])) & 0xffffff00u) != 0u;       // (a negative value sets the high bits)
            viol = __builtin_amdgcn_ballot_w64(bad) != 0ull;
            if (lane == first) fc.chunk[(size_t)yr * (unsigned)fc.nbx + (unsigned)bx] = viol ? 1 : 0;
        }
        viol_any |= viol;
#pragma unroll
        for (int p = 0; p < 2; ++p)
            if (p == 0 ? in0 : in1) {
                if constexpr (SK == SK_S16) {
                    if (CF == CF_NARROW && !viol) {
                        unsigned char* q = fc.cimg + (size_t)yr * fc.cstep + (size_t)(xr + p) * 3;
                        q[0] = (unsigned char)v[p][0]; q[1] = (unsigned char)v[p][1]; q[2] = (unsigned char)v[p][2];
                    } else {
                        short* q = (short*)((CF == CF_NARROW ? fc.wimg : fc.cimg) + (size_t)yr * (CF == CF_NARROW ? fc.wstep : fc.cstep)) + (size_t)(xr + p) * 3;
                        q[0] = (short)v[p][0]; q[1] = (short)v[p][1]; q[2] = (short)v[p][2];
                    }
                } else {
                    unsigned char* q = fc.cimg + (size_t)yr * fc.cstep + (size_t)(xr + p) * 3;
                    q[0] = (unsigned char)v[p][0]; q[1] = (unsigned char)v[p][1]; q[2] = (unsigned char)v[p][2];
                }
                fc.cmask[(size_t)yr * fc.cmstep + (size_t)(xr + p)] = (unsigned char)m[p];
            }
    }
    return viol_any;
}

template <int M, int SK, int PLD, int CF>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(ISX_PD0_WPE, ISX_PD0_WPE))) void k_feed_pd0(Src0 s0, LevelBuf dst, FeedCopy fc) {
    static_assert(SK == SK_U8 || SK == SK_S16, "CV_8UC3 or CV_16SC3 tiles");
    static_assert(CF == CF_SAME || SK == SK_S16, "only CV_16SC3 tiles are narrowed");
    // the block order of k_pyr_down0 (every XCD one contiguous share of the blocks in row-major order)
    const unsigned gx = gridDim.x, L = gx * gridDim.y;
    const unsigned lin = blockIdx.y * gx + blockIdx.x;
    const unsigned k = lin & 7u, chunk = L >> 3, rem = L & 7u;
    const unsigned j = k * chunk + (k < rem ? k : rem) + (lin >> 3);
    const int by = (int)(j / gx), bx = (int)(j - (unsigned)by * gx);
    __shared__ Px<M> hb[PD_NR][WAVE];
    const int x_lo = 2 * (bx * PD_OW - 1) - s0.left, x_hi = 2 * (bx * PD_OW + WAVE - 2) + 1 - s0.left;
    const int y_lo = 2 * by * PD_TY - 2 - s0.top, y_hi = y_lo + PD_NR - 1;
    const bool interior = x_lo >= 0 && x_hi < s0.cols && y_lo >= 0 && y_hi < s0.rows - (SK == SK_S16 ? 0 : 1) && s0.iend != 0u;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bool viol = false;
    if (!interior) {
        viol = feed_copy_rim<SK, CF>(s0, fc, bx, by);
        pyr_down_block<M, SK, 0, PLD>(s0, dst, dst, bx, by, hb);
    } else if constexpr (M == M_I16) {
        Px<M_F32>(*hf)[WAVE] = reinterpret_cast<Px<M_F32>(*)[WAVE]>(hb);
        viol = feed_interior_rows<M_F32, SK, CF>(s0, fc, bx, bx * PD_OW + lane - 1, 2 * by * PD_TY - 2, hf);
        __syncthreads();
        pd0_columns_ix<PLD>(hf, dst, bx * PD_OW + lane - 1, by * PD_TY, lane, wv);
    } else {
        viol = feed_interior_rows<M, SK, CF>(s0, fc, bx, bx * PD_OW + lane - 1, 2 * by * PD_TY - 2, hb);
        __syncthreads();
        pyr_down_columns<M, PLD>(hb, dst, bx * PD_OW + lane - 1, by * PD_TY, lane, wv);
    }
    if constexpr (CF == CF_NARROW) {
        // a violation is rare (never after W:294): its wave tells the tile's device word; k_feed_publish hands it to the host
        if (viol && lane == 0) __hip_atomic_fetch_or(fc.state, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// blend() of a cycle with narrowed tiles starts with this launch: the tiles' violation words (zeroed for the next cycle) OR-ed into pinned
// host memory under a sequence number, which the host reads after it has enqueued the chain up to the last step - no stream synchronisation.
// (A last-block counter inside k_feed_pd0 would put 3 900 arrivals on one memory-side atomic per tile.)
__global__ __launch_bounds__(64) void k_feed_publish(unsigned* state, int n, int* pin, int seq) {
    unsigned v = 0u;
    for (int i = threadIdx.x; i < n; i += 64) {
        v |= __hip_atomic_load(&state[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&state[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const bool any = __builtin_amdgcn_ballot_w64(v != 0u) != 0ull;
    if (threadIdx.x == 0) {
        __hip_atomic_store(&pin[1], any ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __threadfence_system();
        __hip_atomic_store(&pin[0], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The INTERIOR of the same pass as single-wave workgroups without LDS (round 5).  k_feed_pd0's 512-thread blocks are bound by their own life -
// dispatch of eight waves with 35.8 KB of LDS, a memory round trip, a barrier, an LDS round trip (DESIGN §3, round 3) - and a launch for ONE tile is
// 1 904 of them for 768 resident places: 2.5 rounds cost 3.  Here a wave owns 62 output columns x NO output rows of an interior block's area: it
// loads the 2 NO + 3 input rows' windows (every load before the first use), row-filters each with pd0_hrow (neighbour taps as DPP operands),
// column-filters in registers and stores; the copy of the 2 NO rows it owns goes out of the same windows.  Measured (profiles/round5_feed_strip.txt,
// both tiles of a 4K pair): 69 -> 61 us for CV_16SC3 tiles, 62 -> 53 for CV_8UC3; with its stores switched off one by one the launch is 30 us of
// loads + filters (7 rows read per 4 owned: the vertical halo comes from L2), 10 us of level-1 stores, 14 us of copy stores, one after the other
// in every wave's life; four output rows per wave (11 rows per 8) and the block kernel's 35 per 32 read less and are no faster.  Same device functions per pixel as
// the block kernel: identical bits.  Strips on the rim (the level's REFLECT_101 border, the tile's copyMakeBorder columns and rows) take the
// window-with-flags path of collapse_roll.inc - still one memory round trip - so the whole level is this one launch (a first version left the
// rim to the block kernel behind it: 16 us per tile for a tenth of the blocks, whose byte-wise generic path lives as long as a whole interior
// launch).  grid.x = every strip of level 1, dealt to the XCDs in contiguous ranges of the row-major order (vertical neighbours, which share
// three input rows, meet in one L2).
template <int M, int SK, int PLD, int CF>
__global__ __launch_bounds__(64) void k_feed_strip(Src0 s0, LevelBuf dst, FeedCopy fc) {
    constexpr int NO = 2, NR = 2 * NO + 3;
    constexpr int MWK = M == M_I16 ? M_F32 : M;
    const int lane = threadIdx.x;
    const unsigned gx = (unsigned)((dst.cols + PD_OW - 1) / PD_OW), gy = (unsigned)((dst.rows + NO - 1) / NO), L = gx * gy;
    const unsigned lin = blockIdx.x, k = lin & 7u, chunk = L >> 3, rem = L & 7u;
    const unsigned j = k * chunk + (k < rem ? k : rem) + (lin >> 3);
    if (j >= L) return;
    const int sy = (int)(j / gx), bx = (int)(j - (unsigned)sy * gx);
    const int oy0 = sy * NO;                                      // first output row of the strip
    const int ox = bx * PD_OW + lane - 1;
    const int row0 = 2 * oy0 - 2;                                 // first input row (padded level 0)
    const unsigned istep = (unsigned)s0.img_step, mstep = (unsigned)s0.mask_step;
    const gcp img = roll_sgpr((gcp)s0.img), msk = roll_sgpr((gcp)s0.mask);
    const bool own = (lane >= 1) & (lane <= PD_OW);
    // every pixel of the strip's 64 x NR window inside the tile, off its last row (CV_8UC3: a window holds 2 bytes of the next pixel)?
    const int x_lo = 2 * (bx * PD_OW - 1) - s0.left, x_hi = 2 * (bx * PD_OW + WAVE - 2) + 1 - s0.left;
    const int y_lo = row0 - s0.top, y_hi = y_lo + NR - 1;
    const bool interior = x_lo >= 0 && x_hi < s0.cols && y_lo >= 0 && y_hi < s0.rows - (SK == SK_S16 ? 0 : 1);
    Px<MWK> h[NR];
    bool viol = false;
    if (interior) {
        const unsigned xr = (unsigned)(2 * ox - s0.left);
        const unsigned l_io = xr * roll_px_bytes<SK>(), l_mo = xr;
        RollWin<SK> rv[NR];
        unsigned rm[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const unsigned yr = (unsigned)(y_lo + r);
            if constexpr (SK == SK_S16) {
                const u32x3_a2 t = *(ROLL_G(u32x3_a2))(roll_sgpr(img + (size_t)(yr * istep)) + l_io);
                rv[r].x = t.x; rv[r].y = t.y; rv[r].z = t.z;
            } else {
                const u32x2_a1 t = *(ROLL_G(u32x2_a1))(roll_sgpr(img + (size_t)(yr * istep)) + l_io);
                rv[r].x = t.x; rv[r].y = t.y;
            }
            rm[r] = *(ROLL_G(u16_a1))(roll_sgpr(msk + (size_t)(yr * mstep)) + l_mo);
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            if (r >= 2 && r < NR - 1) viol |= feed_copy_window<SK, CF>(fc, rv[r], rm[r], (unsigned)(y_lo + r), xr, bx, own, lane);
            h[r] = pd0_hrow<MWK, SK>(rv[r], rm[r]);
        }
    } else {
        // a strip on the level's or the tile's rim.  Columns: the lane's two taps are the padded columns REFLECT_101(2 ox), REFLECT_101(2 ox + 1)
        // (pyrDown's own border, pyr_down_rows), which copyMakeBorder(BORDER_REFLECT) maps to tile columns xa, xb - neighbours or one and the same
        // pixel, so both lie in ONE window of two adjacent pixels (collapse_roll.inc); the weight is zero outside the tile.  Rows: the same two
        // maps, scalar.  One memory round trip, as in the interior.
        const int sw = s0.width, sh = s0.height;
        const int oxc = min(max(ox, -1), dst.cols);               // (lanes further out feed nobody)
        int cA = 2 * oxc, cB = 2 * oxc + 1;
        cA = cA < 0 ? -cA : (cA >= sw ? 2 * sw - 2 - cA : cA);
        cB = cB < 0 ? -cB : (cB >= sw ? 2 * sw - 2 - cB : cB);
        const int qa = cA - s0.left, qb = cB - s0.left;
        const int xa = roll_reflect(qa, s0.cols), xb = roll_reflect(qb, s0.cols);
        const int xw = min(min(xa, xb), s0.cols - 2);
        const unsigned fl = (xa != xw ? 2u : 0u) | (xb != xw ? 4u : 0u) | ((unsigned)qa < (unsigned)s0.cols ? 8u : 0u) | ((unsigned)qb < (unsigned)s0.cols ? 16u : 0u);
        const unsigned l_io = (unsigned)xw * roll_px_bytes<SK>(), l_mo = (unsigned)xw;
        // the lane's own pixels (2 ox, 2 ox + 1) as they lie in the tile - not reflected, inside its columns - are the ones it copies
        const bool dir_a = own && ox < dst.cols && cA == 2 * ox && (fl & 8u), dir_b = own && ox < dst.cols && cB == 2 * ox + 1 && (fl & 16u);
        RollWin<SK> rv[NR];
        unsigned rm[NR];
        int ryv[NR];        // the tile rows of the windows, before the first load (copyMakeBorder's reflection is a loop: control flow between loads drains them)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            int pr = row0 + r;
            pr = pr < 0 ? -pr : (pr >= sh ? 2 * sh - 2 - pr : pr);
            pr = min(max(pr, 0), sh - 1);                            // (a strip below the level's last row: rows nobody stores)
            ryv[r] = roll_reflect(pr - s0.top, s0.rows);
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int ry = ryv[r];
            if constexpr (SK == SK_S16) {
                const u32x3_a2 t = *(ROLL_G(u32x3_a2))(roll_sgpr(img + (size_t)((unsigned)ry * istep)) + l_io);
                rv[r].x = t.x; rv[r].y = t.y; rv[r].z = t.z;
            } else {
                const unsigned back = ry == s0.rows - 1 ? 2u : 0u;      // the last row's window starts two bytes early (the last pair's would pass the end of the buffer)
                const u32x2_a1 t = *(ROLL_G(u32x2_a1))(roll_sgpr(img + (size_t)((unsigned)ry * istep - back)) + l_io);
                rv[r].x = t.x; rv[r].y = t.y;
            }
            rm[r] = *(ROLL_G(u16_a1))(roll_sgpr(msk + (size_t)((unsigned)ry * mstep)) + l_mo);
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            int pr = row0 + r;
            const bool row_direct = pr >= 0 && pr < sh && r >= 2 && r < NR - 1;       // an owned row, not a reflection of pyrDown's border
            pr = pr < 0 ? -pr : (pr >= sh ? 2 * sh - 2 - pr : pr);
            pr = min(max(pr, 0), sh - 1);
            const int yr = pr - s0.top, ry = roll_reflect(yr, s0.rows);
            const bool wrow = (unsigned)yr < (unsigned)s0.rows, shifted = SK != SK_S16 && ry == s0.rows - 1;
            if (row_direct && wrow) {       // copy the lane's direct pixels of tile row yr (uniform condition)
                int p0[3], p1[3];
                roll_win_decode<SK>(rv[r], shifted, p0, p1);
                const bool asec = fl & 2u, bsec = fl & 4u;
                const int va[3] = {asec ? p1[0] : p0[0], asec ? p1[1] : p0[1], asec ? p1[2] : p0[2]}, vb[3] = {bsec ? p1[0] : p0[0], bsec ? p1[1] : p0[1], bsec ? p1[2] : p0[2]};
                const unsigned ma = asec ? (rm[r] >> 8) & 255u : rm[r] & 255u, mb = bsec ? (rm[r] >> 8) & 255u : rm[r] & 255u;
                bool v = false;
                if constexpr (SK == SK_S16 && CF == CF_NARROW) {
                    const bool bad = (dir_a && (((unsigned)(va[0] | va[1] | va[2])) & 0xffffff00u) != 0u) || (dir_b && (((unsigned)(vb[0] | vb[1] | vb[2])) & 0xffffff00u) != 0u);
                    v = __builtin_amdgcn_ballot_w64(bad) != 0ull;
                    const unsigned long long anyd = __builtin_amdgcn_ballot_w64(dir_a | dir_b);
                    if (anyd != 0ull && lane == (int)__builtin_ctzll(anyd)) fc.chunk[(size_t)yr * (unsigned)fc.nbx + (unsigned)bx] = v ? 1 : 0;
                    viol |= v;
                }
#pragma unroll
                for (int p = 0; p < 2; ++p)
                    if (p == 0 ? dir_a : dir_b) {
                        const int* vv = p == 0 ? va : vb;
                        const int x = 2 * ox + p - s0.left;
                        if (SK == SK_S16 && !(CF == CF_NARROW && !v)) {
                            short* q = (short*)((CF == CF_NARROW ? fc.wimg : fc.cimg) + (size_t)yr * (CF == CF_NARROW ? fc.wstep : fc.cstep)) + (size_t)x * 3;
                            q[0] = (short)vv[0]; q[1] = (short)vv[1]; q[2] = (short)vv[2];
                        } else {
                            unsigned char* q = fc.cimg + (size_t)yr * fc.cstep + (size_t)x * 3;
                            q[0] = (unsigned char)vv[0]; q[1] = (unsigned char)vv[1]; q[2] = (unsigned char)vv[2];
                        }
                        fc.cmask[(size_t)yr * fc.cmstep + (size_t)x] = (unsigned char)(p == 0 ? ma : mb);
                    }
            }
            h[r] = pd0_hrow_rim<MWK, SK>(rv[r], rm[r], shifted, fl, wrow);
        }
    }
    if (own && ox < dst.cols) {
#pragma unroll
        for (int i = 0; i < NO; ++i) {
            const int oy = oy0 + i;
            if (oy < dst.rows) {
                if constexpr (M == M_I16) {
                    const Px<M_I16> o = pd0_col5_ix(h[2 * i], h[2 * i + 1], h[2 * i + 2], h[2 * i + 3], h[2 * i + 4]);
                    if constexpr (PLD) store_px_planar<M_I16>(dst, ox, oy, o); else store_px<M_I16, false>(dst, ox, oy, o);
                } else {
                    const Px<M> o = pyr_down_col5<M>(h[2 * i], h[2 * i + 1], h[2 * i + 2], h[2 * i + 3], h[2 * i + 4]);
                    if constexpr (PLD != 0) store_px_planar<M, PLD == 2>(dst, ox, oy, o); else store_px<M, false>(dst, ox, oy, o);
                }
            }
        }
    }
    if constexpr (CF == CF_NARROW) {
        if (viol && lane == 0) __hip_atomic_fetch_or(fc.state, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// A violated cycle: every row segment the feed kernel narrowed is widened into the escape buffer, which then IS the CV_16SC3 private copy
// (segments the kernel wrote there itself are left alone).  One thread per pixel pair; rare path.
__global__ __launch_bounds__(256) void k_feed_widen(const unsigned char* cimg, unsigned cstep, unsigned char* wimg, unsigned wstep, const unsigned char* chunk, int nbx,
                                                    int rows, int cols, int left) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    const int bx = (x + left) / (2 * PD_OW);
    if (chunk[(size_t)y * (unsigned)nbx + (unsigned)bx]) return;
    const unsigned char* q = cimg + (size_t)y * cstep + (size_t)x * 3;
    short* d = (short*)(wimg + (size_t)y * wstep) + (size_t)x * 3;
    d[0] = q[0]; d[1] = q[1]; d[2] = q[2];
}
