// tests/cpp/opencv_stub — NOT OpenCV: the interface of cv::detail::SeamFinder as OpenCV 3.4.2 declares it, as far as
// include/imagestitch_cv_seam.hpp overrides it and the demos call it.
// Written from (knowledge of) OpenCV 3.4.2 modules/stitching/include/opencv2/stitching/detail/seam_finders.hpp, class CV_EXPORTS SeamFinder:
//   virtual ~SeamFinder() {}                                                                               same
//   virtual void find(const std::vector<UMat> &src, const std::vector<Point> &corners, std::vector<UMat> &masks) = 0;   same
// and of GraphCutSeamFinderBase's  enum CostType { COST_COLOR, COST_COLOR_GRAD };  (declared here as in OpenCV, nothing else of it).
// Compiled with -Werror=suggest-override -Werror=overloaded-virtual (tests/test_gpu_graphcut_seam.py): a drifted signature in the adapter
// fails the build instead of silently declaring a new virtual.
#ifndef ISX_TEST_OPENCV_STUB_SEAM_FINDERS_HPP
#define ISX_TEST_OPENCV_STUB_SEAM_FINDERS_HPP
#include <opencv2/core.hpp>
#include <vector>
namespace cv { namespace detail {
class SeamFinder {
public:
    virtual ~SeamFinder() {}
    virtual void find(const std::vector<UMat>& src, const std::vector<Point>& corners, std::vector<UMat>& masks) = 0;
};
class GraphCutSeamFinderBase {
public:
    enum CostType { COST_COLOR, COST_COLOR_GRAD };
};
}}  // namespace cv::detail
#endif
