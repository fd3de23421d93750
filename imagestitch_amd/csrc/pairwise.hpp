// pairwise.hpp — what the stages that walk pairs of overlapping tiles share on the host (DpSeamFinder, GraphCutSeamFinder, VoronoiSeamFinder,
// GainCompensator::feed): overlapRoi and the padded grid of a pair, the checks of an (images, masks) set, the staging of
// host mats and the per-thread scratch accessor.  Internal, not part of the ABI.
#pragma once
#include <algorithm>

namespace isx {

// ---- geometry (plain C++: with ISX_PAIRWISE_GEOMETRY_ONLY defined this is all of the header) --------------------------------------------
constexpr int PAIR_GAP = 10;             // the gap around the roi, as in PairwiseSeamFinder::run

// cv::detail::overlapRoi: the intersection of two tiles as (x, y, width, height); false when it is empty.  In 64 bits: corner + size may pass
// INT_MAX.
inline bool overlap_roi(const int tl1[2], int w1, int h1, const int tl2[2], int w2, int h2, int roi_xywh[4]) {
    const long long x0 = std::max(tl1[0], tl2[0]), y0 = std::max(tl1[1], tl2[1]);
    const long long x1 = std::min((long long)tl1[0] + w1, (long long)tl2[0] + w2);
    const long long y1 = std::min((long long)tl1[1] + h1, (long long)tl2[1] + h2);
    if (!(x0 < x1 && y0 < y1)) return false;
    roi_xywh[0] = (int)x0; roi_xywh[1] = (int)y0; roi_xywh[2] = (int)(x1 - x0); roi_xywh[3] = (int)(y1 - y0);
    return true;
}

// The grid of a pair: the roi (rw x rh) with PAIR_GAP cells around it (wp x hp), and each tile's coordinates of grid node (0, 0).
struct PairGrid { int rw, rh, hp, wp, oy1, ox1, oy2, ox2; };
inline bool pair_grid(const int tl1[2], int w1, int h1, const int tl2[2], int w2, int h2, PairGrid& g) {
    int roi[4];
    if (!overlap_roi(tl1, w1, h1, tl2, w2, h2, roi)) return false;
    g.rw = roi[2]; g.rh = roi[3];
    g.hp = g.rh + 2 * PAIR_GAP; g.wp = g.rw + 2 * PAIR_GAP;
    g.oy1 = (int)((long long)roi[1] - tl1[1]) - PAIR_GAP; g.ox1 = (int)((long long)roi[0] - tl1[0]) - PAIR_GAP;
    g.oy2 = (int)((long long)roi[1] - tl2[1]) - PAIR_GAP; g.ox2 = (int)((long long)roi[0] - tl2[0]) - PAIR_GAP;
    return true;
}

}  // namespace isx

#ifndef ISX_PAIRWISE_GEOMETRY_ONLY
#include <memory>
#include <vector>

#include "isx_internal.hpp"

namespace isx {

// ---- validation: the first failing check decides the code, in this order -----------------------------------------------------------------
inline int check_mask(const isx_mat& m, int i, int cols, int rows, const char* who) {
    ISX_CHECK_ARG(m.type == ISX_8UC1, ISX_ERR_TYPE, "%s: mask %d is %s (CV_8U)", who, i, type_name(m.type));
    ISX_CHECK_ARG(m.cols == cols && m.rows == rows, ISX_ERR_SIZE, "%s: mask %d is %dx%d, its image %dx%d", who, i, m.cols, m.rows, cols, rows);
    return ISX_OK;
}
// n images, all CV_8UC3 (or, with f32_too, all CV_32FC3), and their CV_8U masks of the same sizes
inline int check_tiles(int n, const isx_mat* images, const isx_mat* masks, bool f32_too, const char* who) {
    for (int i = 0; i < n; ++i) {
        ISX_TRY(check_mat(&images[i], who));
        ISX_TRY(check_mat(&masks[i], who));
        const int t = images[i].type;
        ISX_CHECK_ARG(t == images[0].type && (t == ISX_8UC3 || (f32_too && t == ISX_32FC3)), ISX_ERR_TYPE, "%s: all images must be %sCV_8UC3 (image %d is %s)",
                      who, f32_too ? "CV_32FC3 or all " : "", i, type_name(t));
        ISX_TRY(check_mask(masks[i], i, images[i].cols, images[i].rows, who));
    }
    return ISX_OK;
}
// n CV_8U masks of the given (width, height) sizes
inline int check_masks(int n, const int* sizes_wh, const isx_mat* masks, const char* who) {
    for (int i = 0; i < n; ++i) {
        const int w = sizes_wh[2 * i], h = sizes_wh[2 * i + 1];
        ISX_CHECK_ARG(w >= 0 && h >= 0, ISX_ERR_INVALID, "%s: image %d has size %d x %d", who, i, w, h);
        ISX_TRY(check_mat(&masks[i], who));
        ISX_TRY(check_mask(masks[i], i, w, h, who));
    }
    return ISX_OK;
}

// ---- staging: the host mats of a call, each through a slot of its own whose device buffer only grows ---------------------------------------
struct MatStages {
    std::vector<std::unique_ptr<MatStage>> slot;
    std::vector<MatStage*> out;          // the host mats finish() copies back: they point into the caller's arrays, so they live for one
                                         // call only - use_device() starts it empty, finish() leaves it empty
    int device = -1;
    // starts a call: the buffers live on one device, a call for another one starts afresh
    void use_device(int dev) {
        if (device != dev) clear();
        device = dev;
        out.clear();
    }
    // view = the device mat itself or, for a host mat, its copy in slot i (copied back by finish() when copy_back is set)
    int stage(size_t i, const isx_mat* m, bool copy_back, hipStream_t st, const char* who, isx_mat& view) {
        view = *m;
        if (m->device >= 0) return ISX_OK;
        if (slot.size() <= i) slot.resize(i + 1);
        if (!slot[i]) slot[i].reset(new MatStage());
        ISX_TRY(slot[i]->use_in(m, st, who));
        view = slot[i]->d;
        if (copy_back) { slot[i]->host = m; out.push_back(slot[i].get()); }
        return ISX_OK;
    }
    int finish(hipStream_t st) {
        std::vector<MatStage*> back;
        back.swap(out);
        for (MatStage* m : back) ISX_TRY(m->finish_out(st));
        return ISX_OK;
    }
    void clear() { slot.clear(); out.clear(); device = -1; }
};

// ---- the scratch a stage keeps per calling thread between calls ---------------------------------------------------------------------------
// Never destroyed at thread exit (the HIP runtime may be gone by then).  Internal linkage: one instance per T and translation unit.
template <class T> static T& per_thread() {
    static thread_local T* p = new T();
    return *p;
}

}  // namespace isx
#endif
