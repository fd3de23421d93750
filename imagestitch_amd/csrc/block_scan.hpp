// block_scan.hpp — what the two-pass compaction "in scan order" of surf.hip and sift.hip shares: the exclusive count and the exclusive sum
// over a workgroup's work items in thread order (ballots and wave shuffles, one barrier each, no atomics), and the 3 x 3 solve both run
// inside the pass.  Device code; internal.
#pragma once
#include "isx_device.hpp"

namespace isxd {

// The exclusive count of `flag` over the block's threads in thread order, and the block's total.  `cnt` is this call's own LDS row.
template <int NT>
__device__ __forceinline__ int block_count_before(bool flag, int* cnt, int& total) {
    const int lane = (int)(threadIdx.x & (WAVE - 1)), wv = (int)(threadIdx.x / WAVE);
    const unsigned long long bal = __ballot(flag);
    if (lane == 0) cnt[wv] = __popcll(bal);
    __syncthreads();
    int before = __popcll(bal & ((1ull << lane) - 1ull));
    total = 0;
#pragma unroll
    for (int i = 0; i < NT / WAVE; ++i) { const int c = cnt[i]; before += i < wv ? c : 0; total += c; }
    return before;
}
// The exclusive sum of v over the block's threads in thread order, and the block's total (one barrier; `tot` is NT / WAVE ints of LDS).
template <int NT>
__device__ __forceinline__ int block_sum_before(int v, int* tot, int& total) {
    const int lane = (int)(threadIdx.x & (WAVE - 1)), wv = (int)(threadIdx.x / WAVE);
    int upto = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) { const int n = __shfl_up(upto, o, WAVE); upto += lane >= o ? n : 0; }
    if (lane == WAVE - 1) tot[wv] = upto;
    __syncthreads();
    int before = upto - v;
    total = 0;
#pragma unroll
    for (int i = 0; i < NT / WAVE; ++i) { const int c = tot[i]; before += i < wv ? c : 0; total += c; }
    return before;
}

// Matx_FastSolveOp<float, 3, 1>: Cramer's rule in float32 - the determinant, its reciprocal, three cofactor expansions along the first row;
// false (x untouched) where the determinant is exactly 0
__device__ __forceinline__ bool fast_solve3(float a00, float a01, float a02, float a10, float a11, float a12, float a20, float a21, float a22, float b0, float b1,
                                            float b2, float& x0, float& x1, float& x2) {
    float d = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20);
    if (d == 0.f) return false;
    d = 1.f / d;
    x0 = d * (b0 * (a11 * a22 - a12 * a21) - a01 * (b1 * a22 - a12 * b2) + a02 * (b1 * a21 - a11 * b2));
    x1 = d * (a00 * (b1 * a22 - a12 * b2) - b0 * (a10 * a22 - a12 * a20) + a02 * (a10 * b2 - b1 * a20));
    x2 = d * (a00 * (a11 * b2 - b1 * a21) - a01 * (a10 * b2 - b1 * a20) + b0 * (a10 * a21 - a11 * a20));
    return true;
}

}  // namespace isxd
