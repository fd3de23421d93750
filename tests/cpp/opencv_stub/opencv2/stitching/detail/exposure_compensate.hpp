// tests/cpp/opencv_stub — NOT OpenCV: the interface of cv::detail::ExposureCompensator as OpenCV 3.4.2 declares it, as far as
// include/imagestitch_cv_exposure.hpp overrides and the demos call it.
// Written from (knowledge of) OpenCV 3.4.2 modules/stitching/include/opencv2/stitching/detail/exposure_compensate.hpp, class CV_EXPORTS
// ExposureCompensator:
//   virtual ~ExposureCompensator() {}                                                                        same
//   enum { NO, GAIN, GAIN_BLOCKS };                                                                           same
//   static Ptr<ExposureCompensator> createDefault(int type);                                                 not declared here
//   void feed(const std::vector<Point> &corners, const std::vector<UMat> &images, const std::vector<UMat> &masks);
//        same; body = exposure_compensate.cpp: every mask paired with the value 255, then the virtual feed (W:240 calls this one)
//   virtual void feed(const std::vector<Point> &corners, const std::vector<UMat> &images,
//                     const std::vector<std::pair<UMat,uchar> > &masks) = 0;                                   same
//   virtual void apply(int index, Point corner, InputOutputArray image, InputArray mask) = 0;                 same
// Compiled with -Werror=suggest-override -Werror=overloaded-virtual (tests/test_gpu_gain_feed.py): a drifted signature in the adapter
// fails the build instead of silently declaring a new virtual.
#ifndef ISX_TEST_OPENCV_STUB_EXPOSURE_COMPENSATE_HPP
#define ISX_TEST_OPENCV_STUB_EXPOSURE_COMPENSATE_HPP
#include <opencv2/core.hpp>
#include <utility>
#include <vector>
namespace cv { namespace detail {
class ExposureCompensator {
public:
    virtual ~ExposureCompensator() {}
    enum { NO, GAIN, GAIN_BLOCKS };
    void feed(const std::vector<Point>& corners, const std::vector<UMat>& images, const std::vector<UMat>& masks) {
        std::vector<std::pair<UMat, unsigned char> > level_masks;
        for (size_t i = 0; i < masks.size(); ++i) level_masks.push_back(std::make_pair(masks[i], (unsigned char)255));
        feed(corners, images, level_masks);
    }
    virtual void feed(const std::vector<Point>& corners, const std::vector<UMat>& images,
                      const std::vector<std::pair<UMat, unsigned char> >& masks) = 0;
    virtual void apply(int index, Point corner, InputOutputArray image, InputArray mask) = 0;
};
}}  // namespace cv::detail
#endif
