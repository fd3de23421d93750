// imagestitch_cv_exposure.hpp — the exposure-compensation half of the OpenCV adapter (include/imagestitch_cv.hpp has the warper and the
// blenders): a subclass of OpenCV 3.4.2's cv::detail::ExposureCompensator over the C-ABI library, so that the demos'
//     Ptr<ExposureCompensator> compensator = ExposureCompensator::createDefault(ExposureCompensator::GAIN);   // W:238, S:1165, B:117
// becomes  makePtr<isx_cv::HipGainCompensator>()  and  feed (W:240) / apply (W:241-244) run on the MI355X.  feed estimates the gains of
// GainCompensator (isx_gain_compensator_feed: the overlap statistics on the GPU, the solve on the host); apply multiplies a tile by its
// gain (isx_gain_apply).  HipBlocksGainCompensator does the same for createDefault(ExposureCompensator::GAIN_BLOCKS), OpenCV's own default:
// one gain per 32 x 32 block, solved on the GPU, applied as a smoothed gain map (isx_blocks_gain_feed / isx_blocks_gain_apply).  A header of its own, so that imagestitch_cv.hpp and the stub it is tested against stay as they were.
//
// Compiled inside the reference tree, where OpenCV 3.4.2 is installed; in this repository against tests/cpp/opencv_stub
// (tests/cpp/gain_demo.cpp, run by tests/test_gpu_gain_feed.py; tests/cpp/blocks_gain_demo.cpp, run by tests/test_gpu_blocks_gain.py).
#ifndef IMAGESTITCH_CV_EXPOSURE_HPP
#define IMAGESTITCH_CV_EXPOSURE_HPP

#ifndef ISX_HAVE_OPENCV
#define ISX_HAVE_OPENCV
#endif
#include <opencv2/core.hpp>
#include <opencv2/stitching/detail/exposure_compensate.hpp>

#include <utility>
#include <vector>

#include "imagestitch.hpp"

namespace isx_cv {

// cv::detail::GainCompensator's behaviour over isx::GainCompensator.  Masks count where they equal 255 - the value the public
// feed(corners, images, vector<UMat> masks) pairs every mask with; another value is refused (ISX_ERR_UNSUPPORTED), not ignored.
class HipGainCompensator : public cv::detail::ExposureCompensator {
public:
    explicit HipGainCompensator(int device = 0) : c_(device) {}
    using cv::detail::ExposureCompensator::feed;
    void feed(const std::vector<cv::Point>& corners, const std::vector<cv::UMat>& images,
              const std::vector<std::pair<cv::UMat, unsigned char> >& masks) override {
        CV_Assert(images.size() == corners.size() && masks.size() == corners.size());
        // the mapped Mat headers live to the end of this call (the unmap of an OpenCL-backed UMat happens in their destructors)
        std::vector<cv::Mat> im, mk;
        std::vector<isx::Mat> ii, mm;
        std::vector<isx::Point> pts;
        for (size_t i = 0; i < images.size(); ++i) {
            if (masks[i].second != 255) throw isx::Exception(ISX_ERR_UNSUPPORTED, "HipGainCompensator::feed: mask values other than 255");
            im.push_back(images[i].getMat(cv::ACCESS_READ));
            mk.push_back(masks[i].first.getMat(cv::ACCESS_READ));
        }
        for (size_t i = 0; i < images.size(); ++i) {
            ii.push_back(isx::Mat(im[i]));
            mm.push_back(isx::Mat(mk[i]));
            pts.push_back(isx::Point(corners[i].x, corners[i].y));
        }
        c_.feed(pts, ii, mm);
    }
    // GainCompensator::apply: multiply(image, gains_(index, 0), image); corner and mask unused, as there
    void apply(int index, cv::Point corner, cv::InputOutputArray image, cv::InputArray mask) override {
        (void)mask;
        cv::Mat m = image.getMat();
        isx::Mat im(m);
        c_.apply(index, isx::Point(corner.x, corner.y), im, isx::Mat());
    }
    std::vector<double> gains() const { return c_.gains(); }

private:
    isx::GainCompensator c_;
};

// cv::detail::BlocksGainCompensator's behaviour over isx::BlocksGainCompensator (W:238-244); masks count where they equal 255, as above.
class HipBlocksGainCompensator : public cv::detail::ExposureCompensator {
public:
    explicit HipBlocksGainCompensator(int bl_width = 32, int bl_height = 32, int device = 0) : c_(bl_width, bl_height, device) {}
    using cv::detail::ExposureCompensator::feed;
    void feed(const std::vector<cv::Point>& corners, const std::vector<cv::UMat>& images,
              const std::vector<std::pair<cv::UMat, unsigned char> >& masks) override {
        CV_Assert(images.size() == corners.size() && masks.size() == corners.size());
        std::vector<cv::Mat> im, mk;
        std::vector<isx::Mat> ii, mm;
        std::vector<isx::Point> pts;
        for (size_t i = 0; i < images.size(); ++i) {
            if (masks[i].second != 255) throw isx::Exception(ISX_ERR_UNSUPPORTED, "HipBlocksGainCompensator::feed: mask values other than 255");
            im.push_back(images[i].getMat(cv::ACCESS_READ));
            mk.push_back(masks[i].first.getMat(cv::ACCESS_READ));
        }
        for (size_t i = 0; i < images.size(); ++i) {
            ii.push_back(isx::Mat(im[i]));
            mm.push_back(isx::Mat(mk[i]));
            pts.push_back(isx::Point(corners[i].x, corners[i].y));
        }
        c_.feed(pts, ii, mm);
    }
    // BlocksGainCompensator::apply: the image times its gain map resized to it; corner and mask unused, as there
    void apply(int index, cv::Point corner, cv::InputOutputArray image, cv::InputArray mask) override {
        (void)mask;
        cv::Mat m = image.getMat();
        isx::Mat im(m);
        c_.apply(index, isx::Point(corner.x, corner.y), im, isx::Mat());
    }
    std::vector<double> gains() const { return c_.gains(); }

private:
    isx::BlocksGainCompensator c_;
};

}  // namespace isx_cv

#endif
