// tests/cpp/opencv_stub_plane — NOT OpenCV.  Goes on the include path IN FRONT of tests/cpp/opencv_stub and adds the one declaration
// include/imagestitch_cv_plane.hpp needs beyond it: cv::detail::PlaneWarper, as a stock class whose warpBackward (the one member the
// adapter forwards) is not implemented here.  Everything else is the stub's own header, included next.
#ifndef ISX_TEST_OPENCV_STUB_PLANE_WARPERS_HPP
#define ISX_TEST_OPENCV_STUB_PLANE_WARPERS_HPP
#include_next <opencv2/stitching/detail/warpers.hpp>
namespace cv { namespace detail {
struct PlaneWarper : StockWarperStub { explicit PlaneWarper(float s = 1.f) : StockWarperStub(s) {} };
}}  // namespace cv::detail
#endif
