// gain_stats.hpp — what GainCompensator::feed (gain.hip) shares with BlocksGainCompensator::feed (blocks_gain.hip): the work item and
// the partial record of k_gain_feed, the one launch over a table of items, and OpenCV's hal::LU on the host.  Internal, not part of the ABI.
#pragma once
#include <vector>

#include "isx_internal.hpp"

namespace isx {

struct GainItem {
    const unsigned char* m0;   // mask i at the overlap's top-left, this item's first row
    const unsigned char* m1;   // mask j (off-diagonal only)
    const unsigned char* p0;   // image i (CV_8UC3)
    const unsigned char* p1;   // image j
    unsigned long long sm0, sm1, sp0, sp1;   // row pitches in bytes
    int rows, cols;            // the band: rows x cols pixels of the overlap
    int diag;                  // 1: count mask i only
    int pad_;
};

// partial record of one item: count, then the two limbs of image i's and of image j's sum
enum { GP_N, GP_HI0, GP_LO0, GP_HI1, GP_LO1, GP_COUNT };
struct GainPartial { unsigned long long v[GP_COUNT]; };

// What one item is sized for (gain.hip's GF_DIAG_BYTES / GF_PAIR_PIXELS): mask bytes of a diagonal item, overlap pixels of an off-diagonal one.
// A caller cuts an overlap into bands of max(1, gain_item_size(diag) / width) rows.
int gain_item_size(bool diag);

// One launch of k_gain_feed over `items` (at least one) on `st`, the partials read back into `part`: synchronises st.  The table and
// the partials live per calling thread between calls (on `device` and pinned on the host).
int gain_feed_items(const std::vector<GainItem>& items, double alg_bytes, int device, hipStream_t st, std::vector<GainPartial>& part);

// The total of the partials [first, first + count): the count, and the two exact sums scaled by 2^52
inline void gain_partial_total(const std::vector<GainPartial>& part, int first, int count, unsigned long long& cnt, unsigned __int128& s0,
                               unsigned __int128& s1) {
    cnt = 0; s0 = 0; s1 = 0;
    for (int k = first; k < first + count; ++k) {
        const GainPartial& p = part[(size_t)k];
        cnt += p.v[GP_N];
        s0 += ((unsigned __int128)p.v[GP_HI0] << 30) + p.v[GP_LO0];
        s1 += ((unsigned __int128)p.v[GP_HI1] << 30) + p.v[GP_LO1];
    }
}

// OpenCV's hal::LU (Gaussian elimination, partial pivoting by the largest |pivot|, row swaps carried into b) and its back substitution,
// in double; A is n x n row-major, b becomes the solution.  false: a pivot below 100 DBL_EPSILON (cv::solve returns false there).
bool lu_solve(std::vector<double>& A, std::vector<double>& b, int n);

}  // namespace isx
