// collapse_roll.inc — the LAST collapse step of the deferred cycle without LDS (included by blend.hip inside its anonymous namespace).
//
//   out_0 = sat(pyrUp(out_1) + norm(SUM_t cast((G_{0,t} - pyrUp(G_{1,t})) * W_{0,t})))        (MultiBandBlender::blend, W:313; SURVEY §8(a) A10-A12)
//
// k_collapse_gather stages every 6 x 66 coarse tile through LDS (LDS-DMA, a barrier per round); its own ablation
// (profiles/round2_final_kernel_sq.txt) prices the staging at 29 of 63 us in instructions.  Here a WAVE owns 62 coarse columns (lanes
// 1..62; lanes 0 and 63 are halo lanes that only feed their neighbours) and R coarse rows: per source (each tile that reaches the strip,
// and out_1) it loads the R + 2 coarse rows it needs, ONE record per lane and row, and runs pyrUp's row filter on them with the
// neighbour columns as DPP operands of the additions themselves (v_add_f32_dpp wave_shr:1 / wave_shl:1) - no LDS, no barrier, no LDS-DMA
// address set-up, straight-line code with no per-lane branch off the tiles' rims, every address a scalar row base + a per-lane offset.
// The level-0 pixels of a lane (two adjacent CV_8UC3 pixels + their two mask bytes per fine row) are ONE byte-misaligned
// global_load_dwordx2 and ONE global_load_ushort (unaligned access mode is on under amdhsa; tools/probes/valu_probe.hip: right bytes
// at every misalignment, same rate as the aligned 12-byte window + v_alignbyte it replaces, two registers and two VALU less per window).
// Operations per pixel and their order are exactly those of k_collapse_gather (and of the eager path): identical bits.
// ISX_PREC_I16 (OpenCV's CV_16S arithmetic) runs on integer-valued floats here: every number on its path is an integer below 2^22, which
// fp32 carries exactly - the filters as packed adds / FMAs, (sum + 32) >> 6 as floor(fma(sum, 1/64, 0.5)), static_cast<short> of the
// weighted Laplacian as trunc of the same fp32 product, the short accumulator's wrap applied once to the finished (exact) sum.  Same
// numbers as the integer form of k_collapse_gather, the instruction mix of the float modes (roll_vrow_ix).
//
// Why R is 1 or 2 and not large: a first version rolled down 10 - 16 rows per wave (filtered rows kept in registers, then in a
// wave-private LDS ring with a one-row-ahead prefetch of every load).  It issued 28 % fewer vector and 50 % fewer scalar instructions
// than k_collapse_gather and was SLOWER (70 - 80 us against 62): 5 000 waves that each live as long as the kernel cannot keep 4 096
// wave slots busy - a SIMD runs four of them side by side and then a fifth alone at a quarter of its issue rate
// (profiles/round3_roll_pmc.txt: 20 resident waves per SQ against 36).  Short waves, many of them, is what this part schedules well.
//
// Limits (the host falls back to k_collapse_gather otherwise): CV_8UC3 or CV_16SC3 tiles (what Blender::feed receives, W:294,302) at least 2
// columns wide and below 2 GiB, coarse levels
// below 4 GiB and at least 2 columns wide, at most ROLL_MAXT tiles reach any one strip, this is not also the first step (L >= 2).
constexpr int RL_CW = WAVE - 2;       // coarse columns a wave produces
constexpr int ROLL_MAXT = 3;        // most tiles that may reach one strip (kernels are instantiated for 2 and for 3)

template <int M> struct HRow { f32x2 t0a, t1a, tc; };            // float work types: (b, g) of the even- / odd-column result, r = (even, odd)

struct U2u { unsigned x, y; };
// a lane's two adjacent level-0 pixels as loaded: 6 bytes of a CV_8UC3 tile in an 8-byte window, 12 bytes of a CV_16SC3 tile
template <int SK> struct RollWin { unsigned x, y; };
template <> struct RollWin<SK_S16> { unsigned x, y, z; };
template <int SK> constexpr unsigned roll_px_bytes() { return SK == SK_S16 ? 6u : 3u; }
// the six channel values of the pair (first pixel, second pixel) as integers; CV_8UC3: `shifted` = the window was loaded 2 bytes early
// (the tile's last row, see the load)
template <int SK>
__device__ __forceinline__ void roll_win_decode(const RollWin<SK>& w, bool shifted, int (&p0)[3], int (&p1)[3]) {
    if constexpr (SK == SK_S16) {
        p0[0] = (int)(short)(w.x & 0xffffu); p0[1] = (int)(short)(w.x >> 16); p0[2] = (int)(short)(w.y & 0xffffu);
        p1[0] = (int)(short)(w.y >> 16); p1[1] = (int)(short)(w.z & 0xffffu); p1[2] = (int)(short)(w.z >> 16);
    } else {
        unsigned lo = w.x, hi = w.y;
        if (shifted) { lo = __builtin_amdgcn_alignbyte(hi, lo, 2u); hi >>= 16; }
        p0[0] = (int)(lo & 255u); p0[1] = (int)((lo >> 8) & 255u); p0[2] = (int)((lo >> 16) & 255u);
        p1[0] = (int)(lo >> 24); p1[1] = (int)(hi & 255u); p1[2] = (int)((hi >> 8) & 255u);
    }
}
// what travels between memory and registers: built-in vector types (they can be read through address-space pointers), with the
// alignment the ADDRESSES have - 1 for the level-0 window (the compiler emits one misaligned global_load_dwordx2 / _ushort), 4 for records
typedef unsigned u32x2_a1 __attribute__((ext_vector_type(2), aligned(1)));
typedef unsigned u32x3_a2 __attribute__((ext_vector_type(3), aligned(2)));      // a CV_16SC3 pixel pair: 12 bytes at a 2-byte aligned address
typedef unsigned short u16_a1 __attribute__((aligned(1)));
typedef float f32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));
typedef int i32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));
typedef unsigned u32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));
typedef unsigned short u16x4_a8 __attribute__((ext_vector_type(4), aligned(8)));

// pointers into global memory, said so: a pointer that went through an asm statement (roll_sgpr) is a generic pointer to the compiler, and
// generic pointers make FLAT loads (which count on lgkmcnt as well and drew a full s_waitcnt before each window load)
typedef const __attribute__((address_space(1))) char* gcp;
typedef __attribute__((address_space(1))) char* gp;
#define ROLL_G(T) const __attribute__((address_space(1))) T*
#define ROLL_GW(T) __attribute__((address_space(1))) T*

// bytes of one coarse record
template <int M, bool TILE> constexpr unsigned roll_rec() { return (M == M_F16 && TILE) ? 8u : 16u; }

// the image channels of one coarse record (pyrUp never reads the weight of a coarse level): 12 of its 16 bytes, all 8 of an fp16 tile record
template <int M, bool TILE>
__device__ __forceinline__ void roll_load_rgb(gcp row, unsigned off, typename WorkT<M>::t (&c)[3], bool dense = false, bool q8 = false) {
    if constexpr (M == M_I16) {              // tile levels and the out_k levels of the deferred cycle: {int b, g, r; float w} ...
        // ... or, as dense records (planar level 1, OutMat::rec12), three shorts.  ONE load instruction for both forms - 12 bytes at a 2-byte aligned
        // address, of which a dense record is the first 6 (the rest: its neighbour, or the plane behind the last record - inside the allocation) -
        // and a select: a branch around the load, even a uniform one, makes the compiler drain every load before it (measured: a wait per load)
        const u32x3_a2 v = *(ROLL_G(u32x3_a2))(row + off);
        const int d0 = (int)(short)(v.x & 0xffffu), d1 = (int)(short)(v.x >> 16), d2 = (int)(short)(v.y & 0xffffu);
        c[0] = dense ? d0 : (int)v.x; c[1] = dense ? d1 : (int)v.y; c[2] = dense ? d2 : (int)v.z;
    } else if constexpr (M == M_F16 && TILE) {
        const u16x4_a8 v = *(ROLL_G(u16x4_a8))(row + off);
        c[0] = h2f_bits(v.x); c[1] = h2f_bits(v.y); c[2] = h2f_bits(v.z);
    } else if constexpr (M == M_F32 && TILE) {
        // fp32 tile levels: the record's three floats or, of a planar level 1 in Q8 records (blend.hip, load_px_planar), three unsigned shorts =
        // 256 x the value - one load for both forms and a select, as above
        const u32x3_a2 v = *(ROLL_G(u32x3_a2))(row + off);
        c[0] = q8 ? q8_f(v.x & 0xffffu) : __uint_as_float(v.x); c[1] = q8 ? q8_f(v.x >> 16) : __uint_as_float(v.y); c[2] = q8 ? q8_f(v.y & 0xffffu) : __uint_as_float(v.z);
    } else {
        const f32x3_a4 v = *(ROLL_G(f32x3_a4))(row + off);
        c[0] = v.x; c[1] = v.y; c[2] = v.z;
    }
}

// pyrUp's row filter for this lane's coarse column: even result t0 = (s[x-1] + 6 s[x]) + s[x+1], odd result t1 = 4 (s[x] + s[x+1]);
// OpenCV's explicit formulas in the level's first / last column (a different fp32 association).  The neighbours are DPP operands.
template <int M>
__device__ __forceinline__ void roll_hpass(const typename WorkT<M>::t (&c)[3], bool edges, unsigned off, unsigned off_last, HRow<M>& h) {
    using WT = typename WorkT<M>::t;
    WT t0[3], t1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const WT m = dpp_from_lower_lane(c[k]), p = dpp_from_upper_lane(c[k]);
        t0[k] = (m + c[k] * 6) + p;
        t1[k] = (c[k] + p) * 4;
    }
    if (edges) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const WT m = dpp_from_lower_lane(c[k]), p = dpp_from_upper_lane(c[k]);
            if (off == 0u) t0[k] = c[k] * 6 + p * 2;                    // the lane's record offset in its row identifies the level's first / last column
            else if (off == off_last) { t0[k] = m + c[k] * 7; t1[k] = c[k] * 8; }
        }
    }
    h.t0a = f32x2{t0[0], t0[1]}; h.t1a = f32x2{t1[0], t1[1]}; h.tc = f32x2{t0[2], t1[2]};
}

// pyrUp's column filter from three filtered coarse rows (a = row above, b = the output's own coarse row, c = row below)
template <int M>
__device__ __forceinline__ UpPk roll_vpass(const HRow<M>& a, const HRow<M>& b, const HRow<M>& c) {
    UpPk u;
    const f32x2 s64 = splat2(1.f / 64.f);
    u.a[0][0] = ((a.t0a + b.t0a * splat2(6.f)) + c.t0a) * s64; u.a[0][1] = ((a.t1a + b.t1a * splat2(6.f)) + c.t1a) * s64;
    u.a[1][0] = ((b.t0a + c.t0a) * splat2(4.f)) * s64;         u.a[1][1] = ((b.t1a + c.t1a) * splat2(4.f)) * s64;
    u.c[0] = ((a.tc + b.tc * splat2(6.f)) + c.tc) * s64;
    u.c[1] = ((b.tc + c.tc) * splat2(4.f)) * s64;
    return u;
}
// cv::borderInterpolate(BORDER_REFLECT) with the loop inline (isx_device.hpp keeps it out of line: a call inside the row loop costs the
// kernel its scalar registers)
__device__ __forceinline__ int roll_reflect(int p, int n) {
    if (n == 1) return 0;
    while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p - 1 : 2 * n - 1 - p;
    return p;
}

// a uniform row pointer pinned to scalar registers: the access becomes `global_load v, v_off, s[base:base+1]` with the lane's constant
// offset (otherwise the compiler hoists pointer + lane offset into a 64-bit VGPR pair per stream and adds the row offset per load)
template <class T>
__device__ __forceinline__ T* roll_sgpr(T* p) { asm volatile("" : "+s"(p)); return p; }

// up_row_map as scalar arithmetic (borderInterpolate(2 y, 2 h, REFLECT_101) / 2 for y in [-1, h]: -1 -> 1 (0 when h == 1), h -> h - 1; rows
// further out only feed lanes that own no pixel, any valid row will do): the conditional form makes the compiler carry the uniform
// condition as a lane mask and select through the vector unit
__device__ __forceinline__ int roll_row_map(int y, int h) { return min(abs(y), h - 1); }

// a lane's pixel pair of result row fy, zeroed (no weight: Blender::blend zeroes pixels and mask, W:313); l_so = 12 x column pair
__device__ __forceinline__ void roll_zero_pair(const OutMat& out, int fy, unsigned l_so, unsigned l_sm) {
    const gp orow = roll_sgpr((gp)out.img + (size_t)((unsigned)fy * (unsigned)out.img_step));
    if (out.img_f32 == 0) __builtin_nontemporal_store(u32x3_a2{0u, 0u, 0u}, (ROLL_GW(u32x3_a2))(orow + l_so));      // (2-byte aligned: a dense CV_16SC3 row of odd width)
    else if (out.img_f32 == 1) {
        __builtin_nontemporal_store(u32x3_a4{0u, 0u, 0u}, (ROLL_GW(u32x3_a4))(orow + 2u * l_so));
        __builtin_nontemporal_store(u32x3_a4{0u, 0u, 0u}, (ROLL_GW(u32x3_a4))(orow + 2u * l_so + 12u));
    } else {
        typedef unsigned u32_a2 __attribute__((aligned(2)));
        __builtin_nontemporal_store((u32_a2)0u, (ROLL_GW(u32_a2))(orow + (l_so >> 1)));
        __builtin_nontemporal_store((unsigned short)0, (ROLL_GW(unsigned short))(orow + (l_so >> 1) + 4u));
    }
    if (out.mask) __builtin_nontemporal_store((unsigned short)0, (ROLL_GW(unsigned short))(roll_sgpr((gp)out.mask + (size_t)((unsigned)fy * (unsigned)out.mask_step)) + l_sm));
}

// uniform description of one tile slot of a strip
struct RollSlot {
    gcp img, msk, cimg;
    unsigned istep, mstep, crowb;      // row pitches in bytes: tile image, tile mask, coarse level
    int top, rows, crows, tyc;
    unsigned co_last;                  // record offset of the coarse level's last column
    bool hrefl, hedge, hall, cdense;   // cdense: the coarse level holds dense image records (planar level 1)
};

// pyrUp's column filter for ONE of the two fine rows of a coarse row: dy = 0 from (a, b, c) = (row above, own row, row below), dy = 1
// from (b, c).  Float work types: (b, g) of the row's two pixels and r of both; I16: [dx][channel].
struct UpRowPk { f32x2 a[2], c; };
template <int DY, int M>
__device__ __forceinline__ UpRowPk roll_vrow(const HRow<M>& a, const HRow<M>& b, const HRow<M>& c) {
    UpRowPk u;
    const f32x2 s64 = splat2(1.f / 64.f);
    if constexpr (DY == 0) {
        u.a[0] = ((a.t0a + b.t0a * splat2(6.f)) + c.t0a) * s64; u.a[1] = ((a.t1a + b.t1a * splat2(6.f)) + c.t1a) * s64;
        u.c = ((a.tc + b.tc * splat2(6.f)) + c.tc) * s64;
    } else {
        u.a[0] = ((b.t0a + c.t0a) * splat2(4.f)) * s64; u.a[1] = ((b.t1a + c.t1a) * splat2(4.f)) * s64;
        u.c = ((b.tc + c.tc) * splat2(4.f)) * s64;
    }
    return u;
}
// OpenCV's integer pyrUp of a CV_16S level - (sum + 32) >> 6 - on integer-valued floats: every sum is below 2^22 (64 x 32767), so the
// row filter, the column filter, the + 32 and the / 64 are exact in fp32 and floor() is the arithmetic shift; two values per packed
// instruction instead of one per integer instruction (the I16 arithmetic of this kernel runs in this form since round 4: same numbers)
template <int DY>
__device__ __forceinline__ UpRowPk roll_vrow_ix(const HRow<M_F32>& a, const HRow<M_F32>& b, const HRow<M_F32>& c) {
    UpRowPk u;
    f32x2 e0, e1, ec;
    if constexpr (DY == 0) {
        e0 = pk_fma(pk_fma(b.t0a, splat2(6.f), a.t0a) + c.t0a, splat2(1.f / 64.f), splat2(0.5f));
        e1 = pk_fma(pk_fma(b.t1a, splat2(6.f), a.t1a) + c.t1a, splat2(1.f / 64.f), splat2(0.5f));
        ec = pk_fma(pk_fma(b.tc, splat2(6.f), a.tc) + c.tc, splat2(1.f / 64.f), splat2(0.5f));
    } else {
        e0 = pk_fma(b.t0a + c.t0a, splat2(4.f / 64.f), splat2(0.5f));
        e1 = pk_fma(b.t1a + c.t1a, splat2(4.f / 64.f), splat2(0.5f));
        ec = pk_fma(b.tc + c.tc, splat2(4.f / 64.f), splat2(0.5f));
    }
    u.a[0] = f32x2{__builtin_floorf(e0.x), __builtin_floorf(e0.y)}; u.a[1] = f32x2{__builtin_floorf(e1.x), __builtin_floorf(e1.y)};
    u.c = f32x2{__builtin_floorf(ec.x), __builtin_floorf(ec.y)};
    return u;
}
__device__ __forceinline__ f32x2 trunc2(f32x2 v) { return f32x2{__builtin_truncf(v.x), __builtin_truncf(v.y)}; }      // static_cast<short>(float) of a value inside +-32768
__device__ __forceinline__ f32x2 sat16f2(f32x2 v) {      // saturate_cast<short> of an integer-valued float
    return f32x2{__builtin_fminf(__builtin_fmaxf(v.x, -32768.f), 32767.f), __builtin_fminf(__builtin_fmaxf(v.y, -32768.f), 32767.f)};
}
__device__ __forceinline__ f32x2 wrap16f2(f32x2 v) {      // the wrap of a short accumulator, on an integer-valued float below 2^23: v - 65536 floor((v + 32768) / 65536)
    const f32x2 q = pk_fma(v, splat2(1.f / 65536.f), splat2(0.5f));
    return pk_fma(f32x2{__builtin_floorf(q.x), __builtin_floorf(q.y)}, splat2(-65536.f), v);
}
// accumulators of one fine row of a lane (two pixels), packed as in UpRowPk (the int16 arithmetic too: integer-valued floats)
template <int M> struct RollAcc { f32x2 a[2], c, w; };

template <int V> struct IC { static constexpr int value = V; };

// The strip with NS tile slots: R coarse rows starting at cy0, coarse columns scx0 - 1 + lane.  Everything indexed by a slot, a row or
// a fine row is indexed by a constant: registers.
template <int M, int SK, int R, int NS, int MAXT, class TS>
__device__ __forceinline__ void roll_strip(const TS& ts, const LevelBuf& coarse_out, const OutMat& out, const int (&sel)[MAXT],
                                           int scx0, int cy0, int lane) {
    // IX: OpenCV's int16 arithmetic carried on integer-valued floats (exact, see roll_vrow_ix): the registers and the packed instructions of
    // the float modes, the rounding steps of the integer one
    constexpr bool IX = M == M_I16;
    constexpr int MW = IX ? M_F32 : M;
    using WT = typename WorkT<MW>::t;
    constexpr bool BOUNDED = !IX && (SK == SK_U8 || SK == SK_S16);
    constexpr int NSA = NS > 0 ? NS : 1;
    const int ocw = coarse_out.cols, och = coarse_out.rows;
    const int cxl = scx0 - 1 + lane;                         // this lane's coarse column
    const bool prod = (lane >= 1) & (lane <= RL_CW) & (cxl < ocw);
    // every producing lane's 2 x 2 pixels inside the result's columns and the image rows fit the vector stores (4-byte aligned; CV_8UC3 and
    // the mask need no alignment: byte-misaligned stores are legal)
    // (a CV_16SC3 result's 12-byte stores are typed 2-byte aligned: the rows of a dense cv::Mat of odd width - what dst.create() gives the
    // reference's result, W:313 - start on 2-byte boundaries; until round 4 such a result took the per-pixel stores and the step 77 us instead of 58)
    const bool allin_x = (out.img_f32 == 2 || (((size_t)out.img | out.img_step) & (out.img_f32 == 0 ? 1 : 3)) == 0) && __builtin_amdgcn_ballot_w64(prod & !(2 * cxl + 1 < out.cols)) == 0ull;
    const unsigned l_so = (unsigned)cxl * 12u, l_sm = (unsigned)cxl * 2u;      // byte offsets of the lane's pair in a result row / mask row
    if constexpr (NS == 0) {
        // no tile reaches the strip: every weight is zero, Blender::blend zeroes the pixels and the mask (W:313)
        if (!prod) return;
        Px<M> z; z.c0 = 0; z.c1 = 0; z.c2 = 0; z.w = 0.f;
        for (int fy = 2 * cy0; fy < min(2 * (cy0 + R), out.rows); ++fy) {
            if (allin_x) {
                roll_zero_pair(out, fy, l_so, l_sm);
            } else {
                write_final<M, BOUNDED>(out, 2 * cxl, fy, z);
                write_final<M, BOUNDED>(out, 2 * cxl + 1, fy, z);
            }
        }
        return;
    }
    const int ogx = min(max(cxl, 0), ocw - 1);
    const unsigned orec = out.rec12 ? dense_rec<M>() : roll_rec<M, false>();       // out_1 in dense image records (OutMat::rec12): 12 bytes, int16: 6
    const bool odense = out.rec12 != 0;
    const unsigned l_oo = (unsigned)ogx * orec;
    const unsigned ocrowb = (unsigned)ocw * orec;
    const bool oedge = (scx0 <= 1) | (scx0 + RL_CW + 1 >= ocw);

    const bool cq8 = M == M_F32 && ts.q8 != 0;      // the tiles' planar level 1 in Q8 records (uniform)
    RollSlot S[NSA];
    unsigned l_co[NSA], l_io[NSA], l_mo[NSA], l_fl[NSA];      // per lane: coarse record offset, window offsets, flags (bit 0: inside the tile's columns)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int t = sel[s];
        const Src0& q = ts.s0[t];
        const LevelBuf tcl = ts.coarse[t];
        const int tx = ts.x_tl[t], ty = ts.y_tl[t], ccols = tcl.cols, crows = tcl.rows;
        S[s].cimg = (gcp)tcl.img; S[s].crows = crows; S[s].tyc = ty >> 1;
        // a PLANAR level 1 (wgt != null: 12-byte image records + a weight plane this kernel never reads, blend.hip load_px_planar)
        S[s].cdense = M != M_F16 && tcl.wgt != nullptr;
        const unsigned crec = S[s].cdense ? (cq8 ? 6u : dense_rec<M>()) : roll_rec<M, true>();
        S[s].crowb = (unsigned)ccols * crec; S[s].co_last = (unsigned)(ccols - 1) * crec;
        S[s].img = (gcp)q.img; S[s].msk = (gcp)q.mask; S[s].istep = (unsigned)q.img_step; S[s].mstep = (unsigned)q.mask_step;
        S[s].top = q.top; S[s].rows = q.rows;
        const int lx0 = scx0 - (tx >> 1);                   // strip origin in the tile's coarse coordinates
        const int lcx = lx0 - 1 + lane;
        const int gxc = min(max(lcx, 0), ccols - 1);
        l_co[s] = (unsigned)gxc * crec;
        S[s].hedge = (lx0 <= 1) | (lx0 + RL_CW + 1 >= ccols);
        // every producing lane inside the tile's columns?  (strips off the tile's left / right rim: a scalar test, no ballot)
        S[s].hall = (lx0 >= 0) & (lx0 + min(RL_CW, ocw - scx0) <= ccols);
        l_fl[s] = 1u;
        if (!S[s].hall) {
            const bool colin = prod & ((unsigned)lcx < (unsigned)ccols);
            l_fl[s] = colin ? 1u : 0u;
            S[s].hall = __builtin_amdgcn_ballot_w64(prod & !colin) == 0ull;
        }
        // level 0: the lane's two pixels (2 lcx, 2 lcx + 1) of the padded tile are columns xr, xr + 1 of the caller's tile through
        // copyMakeBorder(BORDER_REFLECT): a reflection maps neighbours to neighbours or to the same pixel, so both always lie in ONE
        // window of two adjacent pixels [xw, xw + 1] - possibly swapped, possibly the same one twice (bits 1, 2: pixel a / b is the
        // window's second).  The weight of a column outside the tile is zero (BORDER_CONSTANT; bits 3, 4: a / b inside).
        // Strips whose every lane (halo lanes included) lies inside the tile's own columns skip all of that (scalar test).
        const int xr0 = 2 * (lx0 - 1) - q.left;             // lane 0's first pixel; the lanes' pixels are xr0 + 2 lane, + 1
        const int xr = 2 * gxc - q.left;
        S[s].hrefl = !((lx0 - 1 >= 0) & (lx0 + RL_CW < ccols) & (xr0 >= 0) & (xr0 + 2 * (WAVE - 1) + 1 < q.cols));
        l_io[s] = (unsigned)xr * roll_px_bytes<SK>(); l_mo[s] = (unsigned)xr;
        if (S[s].hrefl) {
            const int xa = roll_reflect(xr, q.cols), xb = roll_reflect(xr + 1, q.cols);
            const int xw = min(min(xa, xb), q.cols - 2);
            const bool asec = xa != xw, bsec = xb != xw, wa = (unsigned)xr < (unsigned)q.cols, wb = (unsigned)(xr + 1) < (unsigned)q.cols;
            l_fl[s] |= (asec ? 2u : 0u) | (bsec ? 4u : 0u) | (wa ? 8u : 0u) | (wb ? 16u : 0u);
            l_io[s] = (unsigned)xw * roll_px_bytes<SK>(); l_mo[s] = (unsigned)xw;
            S[s].hrefl = __builtin_amdgcn_ballot_w64(asec | !bsec | !wa | !wb) != 0ull;
        }
    }

    // the tile rows of the level-0 windows, BEFORE the first load: copyMakeBorder's row reflection is a (uniform) loop, and control flow between
    // two loads makes the compiler wait for the first one (round 5: the windows used to be loaded behind their rows' reflection and behind an
    // `if the tile reaches this coarse row` - two or three drained round trips per wave instead of one).  A coarse row the tile does not reach
    // loads the windows of a clamped row and drops them (live = false): every load of the strip is issued back to back.
    int ryv[NSA][R][2];
    bool live[NSA][R];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int lcy = cy0 + r - S[s].tyc;
            live[s][r] = (unsigned)lcy < (unsigned)S[s].crows;
            const int lcyc = min(max(lcy, 0), S[s].crows - 1);
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const int yr = 2 * lcyc + dy - S[s].top;
                ryv[s][r][dy] = roll_reflect(yr, S[s].rows);                                      // copyMakeBorder(BORDER_REFLECT) of the image rows
            }
        }
    // ---- every load of the strip: R + 2 coarse rows per source, the level-0 pixels of the 2 R fine rows per slot ----
    WT cr[NSA + 1][R + 2][3];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int r = 0; r < R + 2; ++r) {
            const int gy = roll_row_map(cy0 - 1 + r - S[s].tyc, S[s].crows);
            if constexpr (IX) {
                int ci[3];
                roll_load_rgb<M, true>(roll_sgpr(S[s].cimg + (size_t)((unsigned)gy * S[s].crowb)), l_co[s], ci, S[s].cdense);
                cr[s][r][0] = (float)ci[0]; cr[s][r][1] = (float)ci[1]; cr[s][r][2] = (float)ci[2];
            } else roll_load_rgb<M, true>(roll_sgpr(S[s].cimg + (size_t)((unsigned)gy * S[s].crowb)), l_co[s], cr[s][r], false, cq8 && S[s].cdense);
        }
#pragma unroll
    for (int r = 0; r < R + 2; ++r)
    {
        const gcp orow_c = roll_sgpr((gcp)coarse_out.img + (size_t)((unsigned)roll_row_map(cy0 - 1 + r, och) * ocrowb));
        if constexpr (IX) {
            int ci[3];
            roll_load_rgb<M, false>(orow_c, l_oo, ci, odense);
            cr[NSA][r][0] = (float)ci[0]; cr[NSA][r][1] = (float)ci[1]; cr[NSA][r][2] = (float)ci[2];
        } else roll_load_rgb<M, false>(orow_c, l_oo, cr[NSA][r]);
    }
    RollWin<SK> rv[NSA][R][2];
    unsigned rm[NSA][R][2];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            {
#pragma unroll
                for (int dy = 0; dy < 2; ++dy) {
                    const int ry = ryv[s][r][dy];
                    if constexpr (SK == SK_S16) {       // the pair's 12 bytes exactly: one global_load_dwordx3 at a 2-byte aligned address
                        const gcp ip = roll_sgpr(S[s].img + (size_t)((unsigned)ry * S[s].istep));
                        const u32x3_a2 t = *(ROLL_G(u32x3_a2))(ip + l_io[s]); rv[s][r][dy].x = t.x; rv[s][r][dy].y = t.y; rv[s][r][dy].z = t.z;
                    } else {
                        // 8 bytes for the window's 6; in the tile's last row they start 2 bytes early (the last pair's would pass the end of the
                        // buffer) and are shifted back after the load - one load instruction on every path, no branch around a load
                        const unsigned back = ry == S[s].rows - 1 ? 2u : 0u;
                        const gcp ip = roll_sgpr(S[s].img + (size_t)((unsigned)ry * S[s].istep - back));
                        const u32x2_a1 t = *(ROLL_G(u32x2_a1))(ip + l_io[s]); rv[s][r][dy].x = t.x; rv[s][r][dy].y = t.y;
                    }
                    // copyMakeBorder(BORDER_CONSTANT 0) of the weight: the mask byte of a row outside the tile is read from the reflected row
                    // and dropped (wkeep = 0)
                    rm[s][r][dy] = *(ROLL_G(u16_a1))(roll_sgpr(S[s].msk + (size_t)((unsigned)ry * S[s].mstep)) + l_mo[s]);
                }
            }
        }
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) rm[s][r][dy] = live[s][r] ? rm[s][r][dy] : 0u;       // (a select, not a branch)
    // ---- gather the tiles' Laplacians, source by source in feed order ----
    RollAcc<MW> A[R][2];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            A[r][dy].a[0] = splat2(0.f); A[r][dy].a[1] = splat2(0.f); A[r][dy].c = splat2(0.f); A[r][dy].w = splat2(0.f);
        }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        // copyMakeBorder(BORDER_CONSTANT 0) of the weight: the mask bytes of a border row were read from the reflected row; drop them
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const int yr = 2 * (cy0 + r - S[s].tyc) + dy - S[s].top;
                if (!((unsigned)yr < (unsigned)S[s].rows)) rm[s][r][dy] = 0u;
            }
        // A tile whose every weight in this strip is zero adds (g - pyrUp) * 0 = +-0 to sums that are never -0 and 0 to the weight sums: nothing.
        // With seam masks that is one of the two tiles of almost every strip of the overlap (wave-uniform test, one ballot) - its row
        // filters, column filters, decode and accumulate are skipped.  (Level values are finite: pyramids of 8-bit images.)
        unsigned any = 0u;
#pragma unroll
        for (int r = 0; r < R; ++r) any |= rm[s][r][0] | rm[s][r][1];
        if (__builtin_amdgcn_ballot_w64(any != 0u) == 0ull) continue;
        HRow<MW> H[R + 2];        // pyrUp's row filter of the source's coarse rows (a clamped lane outside the level only feeds itself)
#pragma unroll
        for (int r = 0; r < R + 2; ++r) roll_hpass<MW>(cr[s][r], S[s].hedge, l_co[s], S[s].co_last, H[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!((unsigned)(cy0 + r - S[s].tyc) < (unsigned)S[s].crows)) continue;      // the tile does not reach this row
            auto fine = [&](auto DY) {
                constexpr int dy = decltype(DY)::value;
                const unsigned mk = rm[s][r][dy];
                int p0[3], p1[3];
                {
                    bool shifted = false;       // CV_8UC3: the last row's window was loaded 2 bytes early
                    if constexpr (SK != SK_S16) shifted = ryv[s][r][dy] == S[s].rows - 1;
                    roll_win_decode<SK>(rv[s][r][dy], shifted, p0, p1);
                }
                const float inv255 = (float)(1. / 255.);
                Px<MW> ga, gb;
                if (S[s].hrefl) {       // a strip on the tile's reflected columns: the lane's pixels swapped or doubled, no weight outside the tile
                    const bool asec = l_fl[s] & 2u, bsec = l_fl[s] & 4u, wa = l_fl[s] & 8u, wb = l_fl[s] & 16u;
                    const int m0 = mk & 255, m1 = (mk >> 8) & 255;
                    ga.c0 = (WT)(asec ? p1[0] : p0[0]); ga.c1 = (WT)(asec ? p1[1] : p0[1]); ga.c2 = (WT)(asec ? p1[2] : p0[2]);
                    gb.c0 = (WT)(bsec ? p1[0] : p0[0]); gb.c1 = (WT)(bsec ? p1[1] : p0[1]); gb.c2 = (WT)(bsec ? p1[2] : p0[2]);
                    ga.w = (float)(wa ? (asec ? m1 : m0) : 0) * inv255; gb.w = (float)(wb ? (bsec ? m1 : m0) : 0) * inv255;
                } else {                // the window's values converted in place (CV_8UC3: v_cvt_f32_ubyteN)
                    ga.c0 = (WT)p0[0]; ga.c1 = (WT)p0[1]; ga.c2 = (WT)p0[2];
                    gb.c0 = (WT)p1[0]; gb.c1 = (WT)p1[1]; gb.c2 = (WT)p1[2];
                    ga.w = (float)(mk & 255) * inv255;          // mask * (float)(1. / 255.); zero in the constant border (mk = 0)
                    gb.w = (float)((mk >> 8) & 255) * inv255;
                }
                {
                    UpRowPk u;
                    if constexpr (IX) u = roll_vrow_ix<dy>(H[r], H[r + 1], H[r + 2]); else u = roll_vrow<dy, MW>(H[r], H[r + 1], H[r + 2]);
                    const f32x2 a0 = {(float)ga.c0, (float)ga.c1}, a1 = {(float)gb.c0, (float)gb.c1}, gc = {(float)ga.c2, (float)gb.c2};
                    f32x2 gw = {ga.w, gb.w};
                    f32x2 d0 = a0 - u.a[0], d1 = a1 - u.a[1], dc = gc - u.c;
                    if constexpr (IX && SK == SK_S16) { d0 = sat16f2(d0); d1 = sat16f2(d1); dc = sat16f2(dc); }      // cv::subtract of two shorts saturates
                    if (!S[s].hall) {       // a strip on the tile's left / right rim: a lane outside the tile adds exact zeros (0 * 0: a level value may be Inf / NaN)
                        if (!(l_fl[s] & 1u)) { d0 = splat2(0.f); d1 = splat2(0.f); dc = splat2(0.f); gw = splat2(0.f); }
                    }
                    f32x2 t0 = d0 * splat2(gw.x), t1 = d1 * splat2(gw.y), tc = dc * gw;
                    // int16 arithmetic: static_cast<short>(float product) truncates (the product of a short and a weight in [0, 1] stays inside +-32768);
                    // the short accumulator's wrap is applied once, to the finished sum (a sum of wraps is the wrap of the sum)
                    if constexpr (IX) { t0 = trunc2(t0); t1 = trunc2(t1); tc = trunc2(tc); }
                    A[r][dy].a[0] = A[r][dy].a[0] + t0;
                    A[r][dy].a[1] = A[r][dy].a[1] + t1;
                    A[r][dy].c = A[r][dy].c + tc;
                    A[r][dy].w = A[r][dy].w + gw;
                }
            };
            fine(IC<0>{});
            fine(IC<1>{});
        }
    }

    // no weight anywhere in the strip (outside every seam mask): Blender::blend zeroes the pixels and the mask (W:313), whatever out_1 holds
    bool nz = false;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            nz = nz | (A[r][dy].w.x > WEIGHT_EPS) | (A[r][dy].w.y > WEIGHT_EPS);
        }
    const bool all_zero = __builtin_amdgcn_ballot_w64(nz) == 0ull;
    if (all_zero && allin_x) {
        if (!prod) return;
        for (int fy = 2 * cy0; fy < min(2 * (cy0 + R), out.rows); ++fy) {
            roll_zero_pair(out, fy, l_so, l_sm);
        }
        return;
    }
    // ---- normalise, add pyrUp(out_1), convert, store ----
    HRow<MW> H[R + 2];
#pragma unroll
    for (int r = 0; r < R + 2; ++r) roll_hpass<MW>(cr[NSA][r], oedge, l_oo, (unsigned)(ocw - 1) * orec, H[r]);
    if (!prod) return;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        auto fine = [&](auto DY) {
            constexpr int dy = decltype(DY)::value;
            const int fy = 2 * (cy0 + r) + dy;
            if (fy >= out.rows) return;         // crop to dst_roi_final_
            Px<M> d0, d1;
            if constexpr (IX) {
                const UpRowPk u = roll_vrow_ix<dy>(H[r], H[r + 1], H[r + 2]);
                f32x2 s0 = A[r][dy].a[0], s1 = A[r][dy].a[1], sc = A[r][dy].c;
                if constexpr (SK == SK_S16) { s0 = wrap16f2(s0); s1 = wrap16f2(s1); sc = wrap16f2(sc); }      // the short accumulator (CV_8UC3 tiles never reach its ends)
                // normalizeUsingWeightMap with the shared reciprocal (k_collapse_gather: integer numerators within +-32768 over a denominator that is
                // 1e-5 - only under a zero numerator - or at least 1 / 255: quotients below 2^24, the recurrence is exact there too)
                const f32x2 den = A[r][dy].w + splat2(WEIGHT_EPS);
                const f32x2 r1 = refine_rcp(den, f32x2{__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)});
                const f32x2 n0 = div_by_refined(s0, splat2(den.x), splat2(r1.x)), n1 = div_by_refined(s1, splat2(den.y), splat2(r1.y)), nc = div_by_refined(sc, den, r1);
                if constexpr (SK == SK_S16) {
                    d0.c0 = sat_s16((int)u.a[0].x + wrap_s16((int)n0.x)); d0.c1 = sat_s16((int)u.a[0].y + wrap_s16((int)n0.y)); d0.c2 = sat_s16((int)u.c.x + wrap_s16((int)nc.x));
                    d1.c0 = sat_s16((int)u.a[1].x + wrap_s16((int)n1.x)); d1.c1 = sat_s16((int)u.a[1].y + wrap_s16((int)n1.y)); d1.c2 = sat_s16((int)u.c.y + wrap_s16((int)nc.y));
                } else {
                    // CV_8UC3 tiles (DESIGN §5): every level's Laplacian lies within +-255, so a normalised value does too (its static_cast<short> cannot
                    // wrap) and |out_k| <= 255 (L + 1) (the saturating add cannot act): static_cast<short>(q) + pyrUp as trunc(q) + u on the integer-valued
                    // floats (packed), one conversion per channel.  Same numbers.
                    const f32x2 r0 = u.a[0] + trunc2(n0), r1 = u.a[1] + trunc2(n1), rc = u.c + trunc2(nc);
                    d0.c0 = (int)r0.x; d0.c1 = (int)r0.y; d0.c2 = (int)rc.x;
                    d1.c0 = (int)r1.x; d1.c1 = (int)r1.y; d1.c2 = (int)rc.y;
                }
                d0.w = A[r][dy].w.x; d1.w = A[r][dy].w.y;
            } else {
                const UpRowPk u = roll_vrow<dy, M>(H[r], H[r + 1], H[r + 2]);
                const f32x2 den = A[r][dy].w + splat2(WEIGHT_EPS);                 // normalizeUsingWeightMap: c / (w + 1e-5f), both pixels of the row
                f32x2 n0, n1, nc;
                if constexpr (BOUNDED) {
                    const f32x2 r0 = {__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
                    const f32x2 r1 = refine_rcp(den, r0);
                    n0 = div_by_refined(A[r][dy].a[0], splat2(den.x), splat2(r1.x));
                    n1 = div_by_refined(A[r][dy].a[1], splat2(den.y), splat2(r1.y));
                    nc = div_by_refined(A[r][dy].c, den, r1);
                } else {
                    n0.x = A[r][dy].a[0].x / den.x; n0.y = A[r][dy].a[0].y / den.x; n1.x = A[r][dy].a[1].x / den.y; n1.y = A[r][dy].a[1].y / den.y;
                    nc.x = A[r][dy].c.x / den.x; nc.y = A[r][dy].c.y / den.y;
                }
                const f32x2 ra0 = u.a[0] + n0, ra1 = u.a[1] + n1, rc = u.c + nc;    // restoreImageFromLaplacePyr: pyrUp(out_k) + level
                d0.c0 = ra0.x; d0.c1 = ra0.y; d0.c2 = rc.x; d0.w = A[r][dy].w.x;
                d1.c0 = ra1.x; d1.c1 = ra1.y; d1.c2 = rc.y; d1.w = A[r][dy].w.y;
            }
            if (allin_x) {                      // the lane's two pixels as one or two vector stores + one 2-byte mask store, non-temporal
                const bool on0 = d0.w > WEIGHT_EPS, on1 = d1.w > WEIGHT_EPS;       // compare(w0, WEIGHT_EPS, CMP_GT); Blender::blend zeroes the rest
                const gp orow = roll_sgpr((gp)out.img + (size_t)((unsigned)fy * (unsigned)out.img_step));
                if (out.img_f32 == 0) {         // CV_16SC3: 12 bytes (written once, read by nobody here: -3 us against plain stores)
                    u32x3_a2 q;
                    if constexpr (!IX) {        // BOUNDED (always, for the tile types this kernel takes): |v| < 2^31, never NaN
                        const float f[6] = {on0 ? (float)d0.c0 : 0.f, on0 ? (float)d0.c1 : 0.f, on0 ? (float)d0.c2 : 0.f, on1 ? (float)d1.c0 : 0.f, on1 ? (float)d1.c1 : 0.f, on1 ? (float)d1.c2 : 0.f};
                        unsigned w3[3];
#pragma unroll
                        for (int k = 0; k < 3; ++k)
                            w3[k] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pk_i16((int)__builtin_rintf(f[2 * k]), (int)__builtin_rintf(f[2 * k + 1])));
                        q = u32x3_a2{w3[0], w3[1], w3[2]};
                    } else {
                        const int v[6] = {on0 ? (int)d0.c0 : 0, on0 ? (int)d0.c1 : 0, on0 ? (int)d0.c2 : 0, on1 ? (int)d1.c0 : 0, on1 ? (int)d1.c1 : 0, on1 ? (int)d1.c2 : 0};
                        unsigned w3[3];      // (the values are shorts already: v_cvt_pk_i16_i32 packs two per instruction, its saturation never acts)
#pragma unroll
                        for (int k = 0; k < 3; ++k) w3[k] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pk_i16(v[2 * k], v[2 * k + 1]));
                        q = u32x3_a2{w3[0], w3[1], w3[2]};
                    }
                    __builtin_nontemporal_store(q, (ROLL_GW(u32x3_a2))(orow + l_so));
                } else if (out.img_f32 == 1) {  // CV_32FC3: 24 bytes
                    const f32x3_a4 q0 = {on0 ? (float)d0.c0 : 0.f, on0 ? (float)d0.c1 : 0.f, on0 ? (float)d0.c2 : 0.f}, q1 = {on1 ? (float)d1.c0 : 0.f, on1 ? (float)d1.c1 : 0.f, on1 ? (float)d1.c2 : 0.f};
                    __builtin_nontemporal_store(q0, (ROLL_GW(f32x3_a4))(orow + 2u * l_so));
                    __builtin_nontemporal_store(q1, (ROLL_GW(f32x3_a4))(orow + 2u * l_so + 12u));
                } else {                        // CV_8UC3 (blend + convertTo(CV_8U), W:315): 6 bytes at a 2-byte aligned address = a dword and a short
                    int v[6];
                    if constexpr (!IX) {
                        v[0] = f2u8_sat<BOUNDED>(d0.c0); v[1] = f2u8_sat<BOUNDED>(d0.c1); v[2] = f2u8_sat<BOUNDED>(d0.c2);
                        v[3] = f2u8_sat<BOUNDED>(d1.c0); v[4] = f2u8_sat<BOUNDED>(d1.c1); v[5] = f2u8_sat<BOUNDED>(d1.c2);
                    } else {
                        v[0] = sat_u8((int)d0.c0); v[1] = sat_u8((int)d0.c1); v[2] = sat_u8((int)d0.c2); v[3] = sat_u8((int)d1.c0); v[4] = sat_u8((int)d1.c1); v[5] = sat_u8((int)d1.c2);
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) { if (!on0) v[k] = 0; if (!on1) v[3 + k] = 0; }
                    typedef unsigned u32_a2 __attribute__((aligned(2)));
                    __builtin_nontemporal_store((u32_a2)((unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24)), (ROLL_GW(u32_a2))(orow + (l_so >> 1)));
                    __builtin_nontemporal_store((unsigned short)((unsigned)v[4] | ((unsigned)v[5] << 8)), (ROLL_GW(unsigned short))(orow + (l_so >> 1) + 4u));
                }
                if (out.mask) {
                    ROLL_GW(unsigned short) mq = (ROLL_GW(unsigned short))(roll_sgpr((gp)out.mask + (size_t)((unsigned)fy * (unsigned)out.mask_step)) + l_sm);
                    const unsigned short mv = (unsigned short)((on0 ? 255u : 0u) | (on1 ? 0xff00u : 0u));
                    __builtin_nontemporal_store(mv, mq);
                }
            } else {
                write_final<M, BOUNDED>(out, 2 * cxl, fy, d0);
                write_final<M, BOUNDED>(out, 2 * cxl + 1, fy, d1);
            }
        };
        fine(IC<0>{});
        fine(IC<1>{});
    }
}

#ifndef ROLL_WAVES_N
#define ROLL_WAVES_N 1
#endif
#ifndef ROLL_WPE2
#define ROLL_WPE2 5
#endif
constexpr int ROLL_WAVES = ROLL_WAVES_N;      // waves per workgroup: vertically adjacent strips (they share coarse rows in the CU's L1)
#ifndef ROLL_WPE2_S16
#define ROLL_WPE2_S16 4
#endif
// waves per SIMD the register allocation aims at: 8 for one-row strips of at most two tiles, 5 for three tile slots; two-row strips 5
// (CV_16SC3 tiles carry a third window register per fine row and slot: at 5 they spilt 48 - 72 bytes and the I16 step took 77 us, at 4 it takes 62)
template <int SK, int R, int MAXT> constexpr int roll_wpe() { return MAXT >= 3 ? (R == 1 ? 5 : 4) : (R == 1 ? 8 : (SK == SK_S16 ? ROLL_WPE2_S16 : ROLL_WPE2)); }

// the strip of this wave within ONE mosaic whose tiles are [tb, te) of ts
template <int M, int SK, int R, int MAXT, class TS>
__device__ __forceinline__ void roll_wave(const TS& ts, int tb, int te, const LevelBuf& coarse_out, const OutMat& out, int cx_lo) {
    static_assert(SK == SK_U8 || SK == SK_S16, "CV_8UC3 or CV_16SC3 tiles");
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // (the wave index is uniform; say so)
    int sx, sy;
    if (out.band > 0 ? !xcd_band_block(blockIdx.x, out.grp, out.gx, out.gy, out.band, out.xmagic, sx, sy) : !xcd_block(blockIdx.x, out.grp, out.gx, out.gy, out.xmagic, sx, sy)) return;
    const int scx0 = cx_lo + sx * RL_CW, cy0 = (sy * ROLL_WAVES + wv) * R;       // first coarse column / row this wave produces (mosaic coordinates)
    if (cy0 >= coarse_out.rows) return;
    tile_range(ts, 2 * scx0, 2 * scx0 + 2 * RL_CW, tb, te);      // (a TileTab: the tiles whose columns meet the strip's; a TileSet: all of them)
    // the tiles that reach this strip, in feed order (uniform; the host launches this kernel only when no strip is reached by more than MAXT)
    int sel[MAXT], ns = 0;
#pragma unroll
    for (int s = 0; s < MAXT; ++s) sel[s] = 0;
    for (int t = tb; t < te; ++t) {
        const int tx = ts.x_tl[t], ty = ts.y_tl[t], tw = ts.w[t], th = ts.h[t];
        const bool touch = !((2 * scx0 >= tx + tw) | (2 * scx0 + 2 * RL_CW <= tx) | (2 * cy0 >= ty + th) | (2 * cy0 + 2 * R <= ty));
        if (touch) {
#pragma unroll
            for (int s = 0; s < MAXT; ++s) if (ns == s) sel[s] = t;
            ++ns;
        }
    }
    if constexpr (MAXT >= 3) {
        if (ns >= 3) { roll_strip<M, SK, R, 3, MAXT>(ts, coarse_out, out, sel, scx0, cy0, lane); return; }
    }
    if (ns >= 2) roll_strip<M, SK, R, 2, MAXT>(ts, coarse_out, out, sel, scx0, cy0, lane);
    else if (ns == 1) roll_strip<M, SK, R, 1, MAXT>(ts, coarse_out, out, sel, scx0, cy0, lane);
    else roll_strip<M, SK, R, 0, MAXT>(ts, coarse_out, out, sel, scx0, cy0, lane);
}

template <int M, int SK, int R, int MAXT>
__global__ __launch_bounds__(64 * ROLL_WAVES) __attribute__((amdgpu_waves_per_eu(roll_wpe<SK, R, MAXT>()))) void k_collapse_roll(TileSet ts, LevelBuf coarse_out, OutMat out, int cx_lo) {
    roll_wave<M, SK, R, MAXT>(ts, 0, ts.n, coarse_out, out, cx_lo);
}

// ... the tiles in a device-resident table (more than DEF_MAX of them)
template <int M, int SK, int R, int MAXT>
__global__ __launch_bounds__(64 * ROLL_WAVES) __attribute__((amdgpu_waves_per_eu(roll_wpe<SK, R, MAXT>()))) void k_collapse_roll_tab(TileTab ts, LevelBuf coarse_out, OutMat out, int cx_lo) {
    roll_wave<M, SK, R, MAXT>(ts, 0, ts.n, coarse_out, out, cx_lo);
}

// several mosaics per launch (BatchOut, blend.hip): blockIdx.z is the mosaic
template <int M, int SK, int R, int MAXT>
__global__ __launch_bounds__(64 * ROLL_WAVES) __attribute__((amdgpu_waves_per_eu(roll_wpe<SK, R, MAXT>()))) void k_collapse_roll_batch(TileSet ts, BatchOut bo, int cx_lo) {
    const int m = blockIdx.z;
    roll_wave<M, SK, R, MAXT>(ts, bo.first[m], bo.first[m + 1], bo.coarse_out[m], bo.out[m], cx_lo);
}
