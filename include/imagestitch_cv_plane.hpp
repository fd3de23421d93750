// imagestitch_cv_plane.hpp — the OpenCV adapter of the plane projector, beside imagestitch_cv.hpp (which it includes and leaves as it is):
//
//     // B:91   warper_creator = new cv::PlaneWarper();   ...   W:217-222   warper = warper_creator->create(scale);
//     Ptr<RotationWarper> warper = makePtr<isx_cv::HipPlaneWarper>(static_cast<float>(cameras[0].focal));
//
// isx_cv::HipPlaneWarper is a cv::detail::RotationWarper with the overloads cv::detail::PlaneWarper adds: warp / buildMaps / warpRoi /
// warpPoint with a translation T (3x1 CV_32F).  The overloads without T pass zeros, as the stock class does.  warpPoint goes through
// isx_warper_warp_point (host code, the stock arithmetic); warpBackward is forwarded to the stock class.
// Needs <opencv2/core.hpp> and <opencv2/stitching/detail/warpers.hpp> of OpenCV 3.4.x.
#pragma once
#include "imagestitch_cv.hpp"

namespace isx_cv {

class HipPlaneWarper : public cv::detail::RotationWarper {
public:
    explicit HipPlaneWarper(float scale = 1.f, int device = 0) : w_(ISX_WARP_PLANE, scale, device), stock_(scale), scale_(scale) {}
    // ---- the cv::detail::RotationWarper interface: T = 0 --------------------------------------------------------------------------
    cv::Point2f warpPoint(const cv::Point2f& pt, cv::InputArray K, cv::InputArray R) override { setT(nullptr); return point(pt, K, R); }
    cv::Rect buildMaps(cv::Size src_size, cv::InputArray K, cv::InputArray R, cv::OutputArray xmap, cv::OutputArray ymap) override {
        setT(nullptr); return maps(src_size, K, R, xmap, ymap);
    }
    cv::Point warp(cv::InputArray src, cv::InputArray K, cv::InputArray R, int interp_mode, int border_mode, cv::OutputArray dst) override {
        setT(nullptr); return warpImage(src, K, R, interp_mode, border_mode, dst);
    }
    cv::Rect warpRoi(cv::Size src_size, cv::InputArray K, cv::InputArray R) override { setT(nullptr); return roi(src_size, K, R); }
    void warpBackward(cv::InputArray src, cv::InputArray K, cv::InputArray R, int interp_mode, int border_mode, cv::Size dst_size,
                      cv::OutputArray dst) override {
        stock_.warpBackward(src, K, R, interp_mode, border_mode, dst_size, dst);
    }
    float getScale() const override { return scale_; }
    // ---- what cv::detail::PlaneWarper adds: the same four with a translation ------------------------------------------------------
    virtual cv::Point2f warpPoint(const cv::Point2f& pt, cv::InputArray K, cv::InputArray R, cv::InputArray T) { setT(&T); return point(pt, K, R); }
    virtual cv::Rect buildMaps(cv::Size src_size, cv::InputArray K, cv::InputArray R, cv::InputArray T, cv::OutputArray xmap, cv::OutputArray ymap) {
        setT(&T); return maps(src_size, K, R, xmap, ymap);
    }
    virtual cv::Point warp(cv::InputArray src, cv::InputArray K, cv::InputArray R, cv::InputArray T, int interp_mode, int border_mode,
                           cv::OutputArray dst) {
        setT(&T); return warpImage(src, K, R, interp_mode, border_mode, dst);
    }
    virtual cv::Rect warpRoi(cv::Size src_size, cv::InputArray K, cv::InputArray R, cv::InputArray T) { setT(&T); return roi(src_size, K, R); }
    isx_warper* handle() { return w_.handle(); }
private:
    void setT(const cv::_InputArray* T) {          // setCameraParams(K, R, T): T is 3x1 CV_32F
        float t[3] = {0.f, 0.f, 0.f};
        if (T) {
            cv::Mat m = T->getMat();
            CV_Assert(m.rows == 3 && m.cols == 1 && m.type() == CV_32F);
            for (int i = 0; i < 3; ++i) t[i] = m.at<float>(i, 0);
        }
        w_.setTranslation(t);
    }
    cv::Point2f point(const cv::Point2f& pt, cv::InputArray K, cv::InputArray R) {
        float k[9], r[9]; k9(K, k); k9(R, r);
        const isx::Point2f p = w_.warpPoint(isx::Point2f(pt.x, pt.y), k, r);
        return cv::Point2f(p.x, p.y);
    }
    cv::Rect roi(cv::Size src_size, cv::InputArray K, cv::InputArray R) {
        float k[9], r[9]; k9(K, k); k9(R, r);
        int q[4];
        isx::check(isx_warper_roi(w_.handle(), src_size.width, src_size.height, k, r, q, nullptr));
        return cv::Rect(q[0], q[1], q[2] - q[0] + 1, q[3] - q[1] + 1);     // Rect(tl, br + 1)
    }
    cv::Rect maps(cv::Size src_size, cv::InputArray K, cv::InputArray R, cv::OutputArray xmap, cv::OutputArray ymap) {
        float k[9], r[9]; k9(K, k); k9(R, r);
        int q[4];
        isx::check(isx_warper_roi(w_.handle(), src_size.width, src_size.height, k, r, q, nullptr));
        xmap.create(q[3] - q[1] + 1, q[2] - q[0] + 1, CV_32F);             // W:128
        ymap.create(q[3] - q[1] + 1, q[2] - q[0] + 1, CV_32F);             // W:129
        cv::Mat mx = xmap.getMat(), my = ymap.getMat();
        isx::Mat ix(mx), iy(my);
        isx::check(isx_warper_build_maps_roi(w_.handle(), k, r, q, ix.c(), iy.c()));
        return cv::Rect(q[0], q[1], q[2] - q[0], q[3] - q[1]);             // Rect(dst_tl, dst_br)  W:143
    }
    cv::Point warpImage(cv::InputArray src, cv::InputArray K, cv::InputArray R, int interp_mode, int border_mode, cv::OutputArray dst) {
        float k[9], r[9]; k9(K, k); k9(R, r);
        cv::Mat s = src.getMat();
        int q[4];
        isx::check(isx_warper_roi(w_.handle(), s.cols, s.rows, k, r, q, nullptr));
        dst.create(q[3] - q[1] + 1, q[2] - q[0] + 1, s.type());            // W:150
        cv::Mat d = dst.getMat();
        isx::Mat is(s), id(d);
        isx::check(isx_warper_warp_roi(w_.handle(), is.c(), k, r, interp_mode, border_mode, q, id.c()));   // W:157
        return cv::Point(q[0], q[1]);                                      // dst_roi.tl()  W:160
    }
    isx::RotationWarper w_;
    cv::detail::PlaneWarper stock_;
    float scale_;
};

}  // namespace isx_cv
