// imagestitch_cv_seam.hpp — the seam-finder half of the OpenCV adapter (include/imagestitch_cv.hpp has the warper and the blenders): a
// subclass of OpenCV 3.4.2's cv::detail::SeamFinder over the C-ABI library, so that the W demo's
//     seam_finder = new GraphCutSeamFinder(GraphCutSeamFinder::COST_COLOR);      // W:257
//     seam_finder->find(images_warped_f, corners, masks_warped);                  // W:264
// becomes  makePtr<isx_cv::HipGraphCutSeamFinder>()  and find runs every pair's max-flow on the MI355X (isx_graphcut_seam_find).  The cut
// is the maximal minimum cut: where the minimum cut is not unique, OpenCV's Boykov-Kolmogorov search may return another one of the same cost
// (DESIGN.md §8).  A header of its own, so that imagestitch_cv.hpp and the stub it is tested against stay as they were.
//
// Compiled inside the reference tree, where OpenCV 3.4.2 is installed; in this repository against tests/cpp/opencv_stub
// (tests/cpp/graphcut_demo.cpp, run by tests/test_gpu_graphcut_seam.py; tests/cpp/graphcut_grad_demo.cpp, run by
// tests/test_gpu_graphcut_grad.py; tests/cpp/voronoi_demo.cpp, run by tests/test_gpu_voronoi_seam.py;
// tests/cpp/seam_grad_demo.cpp, run by tests/test_gpu_seam_grad.py).
#ifndef IMAGESTITCH_CV_SEAM_HPP
#define IMAGESTITCH_CV_SEAM_HPP

#ifndef ISX_HAVE_OPENCV
#define ISX_HAVE_OPENCV
#endif
#include <opencv2/core.hpp>
#include <opencv2/stitching/detail/seam_finders.hpp>

#include <vector>

#include "imagestitch.hpp"

namespace isx_cv {

namespace detail {
// The arguments of a find as the isx finders take them.  The mapped Mat headers live as long as this object - to the end of the find that
// builds it (the unmap of an OpenCL-backed UMat happens in their destructors).  Images are mapped only where they are read.
struct SeamArgs {
    std::vector<cv::Mat> im, mk;
    std::vector<isx::Mat> ii, mm;
    std::vector<isx::Point> pts;
    SeamArgs(const std::vector<cv::UMat>& src, const std::vector<cv::Point>& corners, std::vector<cv::UMat>& masks, bool map_images = true) {
        CV_Assert(src.size() == corners.size() && masks.size() == corners.size());
        for (size_t i = 0; i < src.size(); ++i) {
            if (map_images) im.push_back(src[i].getMat(cv::ACCESS_READ));
            mk.push_back(masks[i].getMat(cv::ACCESS_RW));
        }
        for (size_t i = 0; i < src.size(); ++i) {
            if (map_images) ii.push_back(isx::Mat(im[i]));
            mm.push_back(isx::Mat(mk[i]));
            pts.push_back(isx::Point(corners[i].x, corners[i].y));
        }
    }
};
}  // namespace detail

// cv::detail::GraphCutSeamFinder(cost_type)'s find over isx::GraphCutSeamFinder, COST_COLOR or COST_COLOR_GRAD.  A CV_32FC3 value that is
// not an integer in [0, 255] throws isx::Exception(ISX_ERR_UNSUPPORTED) from find, as do CV_8UC3 tiles with COST_COLOR_GRAD.
class HipGraphCutSeamFinder : public cv::detail::SeamFinder {
public:
    explicit HipGraphCutSeamFinder(int cost_type = cv::detail::GraphCutSeamFinderBase::COST_COLOR, int device = 0) : f_(cost_type, device) {}
    void find(const std::vector<cv::UMat>& src, const std::vector<cv::Point>& corners, std::vector<cv::UMat>& masks) override {
        detail::SeamArgs a(src, corners, masks);
        f_.find(a.ii, a.pts, a.mm);
    }

private:
    isx::GraphCutSeamFinder f_;
};

// cv::detail::VoronoiSeamFinder's find over isx::VoronoiSeamFinder (S:1180, S:1192):  makePtr<isx_cv::HipVoronoiSeamFinder>().  The images are
// not mapped: only their sizes are used.
class HipVoronoiSeamFinder : public cv::detail::SeamFinder {
public:
    explicit HipVoronoiSeamFinder(int device = 0) : f_(device) {}
    void find(const std::vector<cv::UMat>& src, const std::vector<cv::Point>& corners, std::vector<cv::UMat>& masks) override {
        detail::SeamArgs a(src, corners, masks, false);
        std::vector<isx::Size> sizes;
        for (size_t i = 0; i < src.size(); ++i) sizes.push_back(isx::Size(src[i].cols, src[i].rows));
        f_.find(sizes, a.pts, a.mm);
    }

private:
    isx::VoronoiSeamFinder f_;
};

// cv::detail::DpSeamFinder(costFunc)'s find over isx::DpSeamFinder:  `new DpSeamFinder(DpSeamFinder::COLOR)` (W:253) becomes
// makePtr<isx_cv::HipDpSeamFinder>(), `new DpSeamFinder(DpSeamFinder::COLOR_GRAD)` (W:255, S:1183) makePtr<isx_cv::HipDpSeamFinder>(
// isx_cv::HipDpSeamFinder::COLOR_GRAD).  The enum is the adapter's own, with OpenCV's values (COLOR = 0, COLOR_GRAD = 1).
class HipDpSeamFinder : public cv::detail::SeamFinder {
public:
    enum CostFunction { COLOR, COLOR_GRAD };
    explicit HipDpSeamFinder(CostFunction costFunc = COLOR, int device = 0)
        : f_(costFunc == COLOR_GRAD ? isx::DpSeamFinder::COLOR_GRAD : isx::DpSeamFinder::COLOR, device) {}
    CostFunction costFunction() const { return f_.costFunction() == isx::DpSeamFinder::COLOR_GRAD ? COLOR_GRAD : COLOR; }
    void find(const std::vector<cv::UMat>& src, const std::vector<cv::Point>& corners, std::vector<cv::UMat>& masks) override {
        detail::SeamArgs a(src, corners, masks);
        f_.find(a.ii, a.pts, a.mm);
    }

private:
    isx::DpSeamFinder f_;
};

}  // namespace isx_cv

#endif
