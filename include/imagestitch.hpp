// imagestitch.hpp — header-only C++ host-side mirror of the reference's call surface over the C-ABI.
//
// The reference is C++ on OpenCV (`cv::detail::RotationWarper`, `cv::detail::Blender`); this header gives
// the same class / method names, argument meaning and error behaviour (exceptions) on top of
// include/imagestitch_hip.h, so the pipeline code of W:217-233 / W:271-313 ports line by line:
//
//     isx::CylindricalWarper creator;                                   // W:219
//     auto warper = creator.create(focal);                              // W:222
//     isx::Point corner = warper->warp(img, K, R, isx::INTER_LINEAR, isx::BORDER_REFLECT, warped);   // W:229
//     warper->warp(mask, K, R, isx::INTER_NEAREST, isx::BORDER_CONSTANT, mask_warped);               // W:232
//     auto blender = isx::Blender::createDefault(isx::Blender::MULTI_BAND, false);                   // W:271
//     static_cast<isx::MultiBandBlender*>(blender.get())->setNumBands(4);                            // W:273
//     blender->prepare(corners, sizes);  blender->feed(img_s, mask, corner);  blender->blend(result, result_mask);
//
// With OpenCV available, define ISX_HAVE_OPENCV before including: isx::Mat then converts from / to cv::Mat
// without copying (same data / rows / cols / type() / step).
#pragma once
#include <cmath>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <cstdio>
#include <vector>

#include "imagestitch_hip.h"
#ifdef ISX_HAVE_OPENCV
#include <opencv2/core.hpp>
#endif

namespace isx {

enum { INTER_NEAREST = ISX_INTER_NEAREST, INTER_LINEAR = ISX_INTER_LINEAR };
enum { BORDER_CONSTANT = ISX_BORDER_CONSTANT, BORDER_REPLICATE = ISX_BORDER_REPLICATE, BORDER_REFLECT = ISX_BORDER_REFLECT,
       BORDER_REFLECT_101 = ISX_BORDER_REFLECT_101 };

struct Point { int x = 0, y = 0; Point() = default; Point(int x_, int y_) : x(x_), y(y_) {} };
struct Point2f { float x = 0.f, y = 0.f; Point2f() = default; Point2f(float x_, float y_) : x(x_), y(y_) {} };
struct Size { int width = 0, height = 0; Size() = default; Size(int w, int h) : width(w), height(h) {} };
struct Rect { int x = 0, y = 0, width = 0, height = 0; };

// cv::Exception analogue: thrown for every non-zero status of the C-ABI
class Exception : public std::runtime_error {
public:
    Exception(int code_, const std::string& msg) : std::runtime_error(msg), code(code_) {}
    int code;
};
inline void check(int rc) { if (rc != ISX_OK) throw Exception(rc, isx_last_error()); }

// cv::Mat-shaped matrix: owns a host buffer (create) or aliases foreign memory (host or HIP device).
class Mat {
public:
    Mat() { std::memset(&m_, 0, sizeof(m_)); m_.device = -1; }
    Mat(int rows, int cols, int type) : Mat() { create(rows, cols, type); }
    Mat(int rows, int cols, int type, void* data, size_t step, int device = -1) : Mat() {
        m_.data = data; m_.rows = rows; m_.cols = cols; m_.type = type; m_.step = step; m_.device = device;
    }
#ifdef ISX_HAVE_OPENCV
    Mat(const cv::Mat& c) : Mat(c.rows, c.cols, c.type(), c.data, c.step, -1) {}   // zero-copy view
    cv::Mat toCv() const { return cv::Mat(m_.rows, m_.cols, m_.type, m_.data, m_.step); }
#endif
    void create(int rows, int cols, int type) {   // OutputArray::create (W:128-129,150)
        // cv::Mat::create: a mat that already has this geometry keeps its buffer - whether it owns it or aliases the caller's
        // (host or device) memory
        if (m_.data != nullptr && m_.rows == rows && m_.cols == cols && m_.type == type) return;
        size_t es = elemSize(type);
        own_ = std::shared_ptr<unsigned char>(new unsigned char[(size_t)rows * cols * es], std::default_delete<unsigned char[]>());
        m_.data = own_.get(); m_.rows = rows; m_.cols = cols; m_.type = type; m_.step = (size_t)cols * es; m_.device = -1;
    }
    static size_t elemSize(int type) {
        static const int d[8] = {1, 1, 2, 2, 4, 4, 8, 2};
        return (size_t)d[type & 7] * ((type >> 3) + 1);
    }
    bool empty() const { return m_.data == nullptr; }
    int rows() const { return m_.rows; }
    int cols() const { return m_.cols; }
    int type() const { return m_.type; }
    Size size() const { return Size(m_.cols, m_.rows); }
    template <class T> T* ptr(int y) { return (T*)((unsigned char*)m_.data + (size_t)y * m_.step); }
    template <class T> const T* ptr(int y) const { return (const T*)((const unsigned char*)m_.data + (size_t)y * m_.step); }
    void setTo(unsigned char v) { for (int y = 0; y < m_.rows; ++y) std::memset(ptr<unsigned char>(y), v, (size_t)m_.cols * elemSize(m_.type)); }
    isx_mat* c() { return &m_; }
    const isx_mat* c() const { return &m_; }
private:
    isx_mat m_;
    std::shared_ptr<unsigned char> own_;
};

// cv::detail::RotationWarper (W:122-161; stock call sites B:105,109)
class RotationWarper {
public:
    RotationWarper(int kind, float scale, int device = 0) { check(isx_warper_create(kind, scale, device, &h_)); }
    virtual ~RotationWarper() { isx_warper_destroy(h_); }
    RotationWarper(const RotationWarper&) = delete;
    RotationWarper& operator=(const RotationWarper&) = delete;
    void setStream(void* hip_stream) { check(isx_warper_set_stream(h_, hip_stream)); }
    // Rect buildMaps(Size src_size, K, R, xmap, ymap)  W:122
    Rect buildMaps(Size src_size, const float K[9], const float R[9], Mat& xmap, Mat& ymap) {
        int roi[4];
        check(isx_warper_roi(h_, src_size.width, src_size.height, K, R, roi, nullptr));
        xmap.create(roi[3] - roi[1] + 1, roi[2] - roi[0] + 1, ISX_32FC1);   // W:128
        ymap.create(roi[3] - roi[1] + 1, roi[2] - roi[0] + 1, ISX_32FC1);   // W:129
        check(isx_warper_build_maps_roi(h_, K, R, roi, xmap.c(), ymap.c()));   // the fill W:133-141 over the ROI just computed: one scan per call
        Rect r; r.x = roi[0]; r.y = roi[1]; r.width = roi[2] - roi[0]; r.height = roi[3] - roi[1];   // Rect(tl, br)  W:143
        return r;
    }
    // Point warp(src, K, R, interp_mode, border_mode, dst)  W:145
    Point warp(const Mat& src, const float K[9], const float R[9], int interp_mode, int border_mode, Mat& dst) {
        int roi[4];
        check(isx_warper_roi(h_, src.cols(), src.rows(), K, R, roi, nullptr));   // buildMaps -> detectResultRoi, ONCE per call  W:126,149
        dst.create(roi[3] - roi[1] + 1, roi[2] - roi[0] + 1, src.type());   // dst.create(roi.height + 1, roi.width + 1)  W:150
        check(isx_warper_warp_roi(h_, src.c(), K, R, interp_mode, border_mode, roi, dst.c()));   // the remap with that ROI  W:157
        return Point(roi[0], roi[1]);   // dst_roi.tl()  W:160
    }
    Rect warpRoi(Size src_size, const float K[9], const float R[9]) {
        int roi[4];
        check(isx_warper_roi(h_, src_size.width, src_size.height, K, R, roi, nullptr));
        Rect r; r.x = roi[0]; r.y = roi[1]; r.width = roi[2] - roi[0] + 1; r.height = roi[3] - roi[1] + 1;
        return r;
    }
    // Not in the reference: the image and its all-255 mask in one pass (W:229 + W:232; dst_img CV_8UC3 or CV_16SC3 = + W:294), and the gain of
    // GainCompensator::apply (W:241-244) folded into that pass's store (isx_warper_set_gain; 1.0 = off)
    Point warpWithMask(const Mat& src, const float K[9], const float R[9], Mat& dst_img, Mat& dst_mask, int img_type = ISX_8UC3) {
        int roi[4];
        check(isx_warper_roi(h_, src.cols(), src.rows(), K, R, roi, nullptr));
        dst_img.create(roi[3] - roi[1] + 1, roi[2] - roi[0] + 1, img_type);
        dst_mask.create(roi[3] - roi[1] + 1, roi[2] - roi[0] + 1, ISX_8UC1);
        check(isx_warper_warp_with_mask_roi(h_, src.c(), nullptr, K, R, roi, dst_img.c(), dst_mask.c()));
        return Point(roi[0], roi[1]);
    }
    void setGain(double gain) { check(isx_warper_set_gain(h_, gain)); }
    // cv::detail::PlaneWarper's T (its warp / buildMaps / warpRoi / warpPoint overloads with a translation): sticky, zero by default; only a
    // warper made by PlaneWarper takes a non-zero one (isx_warper_set_translation)
    void setTranslation(const float T[3]) { check(isx_warper_set_translation(h_, T)); }
    // Point2f warpPoint(pt, K, R): mapForward of one source point, on the host (isx_warper_warp_point)
    Point2f warpPoint(Point2f pt, const float K[9], const float R[9]) {
        float uv[2];
        check(isx_warper_warp_point(h_, K, R, pt.x, pt.y, uv));
        return Point2f(uv[0], uv[1]);
    }
    // Not in the reference: the fused tile warps issued between the two calls (planned or _roi forms on device mats) leave as ONE launch
    // (isx_warper_begin_batch / isx_warper_end_batch); their outputs exist once endBatch() has returned and its launch has run
    void beginBatch() { check(isx_warper_begin_batch(h_)); }
    void endBatch() { check(isx_warper_end_batch(h_)); }
    isx_warper* handle() { return h_; }
private:
    isx_warper* h_ = nullptr;
};

struct WarperCreator { virtual ~WarperCreator() {} virtual std::shared_ptr<RotationWarper> create(float scale) const = 0; };
struct CylindricalWarper : WarperCreator {   // cv::CylindricalWarper  W:219
    std::shared_ptr<RotationWarper> create(float scale) const override { return std::make_shared<RotationWarper>(ISX_WARP_CYLINDRICAL, scale); }
};
struct SphericalWarper : WarperCreator {     // cv::SphericalWarper  B:93 (commented out in the reference)
    std::shared_ptr<RotationWarper> create(float scale) const override { return std::make_shared<RotationWarper>(ISX_WARP_SPHERICAL, scale); }
};
struct PlaneWarper : WarperCreator {         // cv::PlaneWarper  B:91 (commented out in the reference)
    std::shared_ptr<RotationWarper> create(float scale) const override { return std::make_shared<RotationWarper>(ISX_WARP_PLANE, scale); }
};
// The two projectors that are not separable: every pixel evaluates the restated transcendentals.  warp / warpRoi / buildMaps / warpPoint /
// setGain serve them; the planned and batched entries throw ISX_ERR_UNSUPPORTED, as does a non-zero setTranslation.
struct FisheyeWarper : WarperCreator {       // cv::FisheyeWarper  B:94 (commented out in the reference)
    std::shared_ptr<RotationWarper> create(float scale) const override { return std::make_shared<RotationWarper>(ISX_WARP_FISHEYE, scale); }
};
struct StereographicWarper : WarperCreator { // cv::StereographicWarper  B:95 (commented out in the reference)
    std::shared_ptr<RotationWarper> create(float scale) const override { return std::make_shared<RotationWarper>(ISX_WARP_STEREOGRAPHIC, scale); }
};

// cv::detail::Blender / MultiBandBlender (W:271-281,302,313)
class Blender {
public:
    enum { NO = ISX_BLEND_NO, FEATHER = ISX_BLEND_FEATHER, MULTI_BAND = ISX_BLEND_MULTI_BAND };
    virtual ~Blender() { isx_blender_destroy(h_); }
    Blender(const Blender&) = delete;              // owns the handle: a copy would destroy it twice
    Blender& operator=(const Blender&) = delete;
    static std::shared_ptr<Blender> createDefault(int type, bool try_gpu = false, int precision = ISX_PREC_I16);
    void prepare(const std::vector<Point>& corners, const std::vector<Size>& sizes) {   // W:281
        if (corners.size() != sizes.size()) throw Exception(ISX_ERR_INVALID, "prepare: corners.size() != sizes.size()");
        std::vector<int> c, s;
        for (size_t i = 0; i < corners.size(); ++i) { c.push_back(corners[i].x); c.push_back(corners[i].y); s.push_back(sizes[i].width); s.push_back(sizes[i].height); }
        check(isx_blender_prepare(h_, (int)corners.size(), c.data(), s.data()));
    }
    void prepare(Rect dst_roi) { check(isx_blender_prepare_roi(h_, dst_roi.x, dst_roi.y, dst_roi.width, dst_roi.height)); }
    void feed(const Mat& img, const Mat& mask, Point tl) { check(isx_blender_feed(h_, img.c(), mask.c(), tl.x, tl.y)); }   // W:302
    // Not in the reference: W:286-302 in one call - feed(img, dilate(seam_mask, MORPH_RECT kw x kh) & warped_mask, tl), the mask prepared
    // straight into the blender's own buffer (isx_blender_feed_dilated)
    void feedDilated(const Mat& img, const Mat& seam_mask, const Mat& warped_mask, int kw, int kh, Point tl) {
        check(isx_blender_feed_dilated(h_, img.c(), seam_mask.c(), warped_mask.c(), kw, kh, tl.x, tl.y));
    }
    void blend(Mat& dst, Mat& dst_mask) {   // W:313
        int w, h;
        check(isx_blender_result_size(h_, &w, &h));
        if (win_x1_ > win_x0_) w = win_x1_ - win_x0_;   // setWindow: the mats hold the window's columns only
        if (dst.empty() || dst.rows() != h || dst.cols() != w) dst.create(h, w, ISX_16SC3);
        dst_mask.create(h, w, ISX_8UC1);
        check(isx_blender_blend(h_, dst.c(), dst_mask.c()));
    }
    // Not in the reference: blend() of several prepared + fed blenders of one rig in ONE chain of launches (isx_blender_blend_batch);
    // dsts / dst_masks are allocated like blend()'s, every result is bit-identical to the blender's own blend().
    static void blendBatch(const std::vector<Blender*>& bs, std::vector<Mat>& dsts, std::vector<Mat>& dst_masks) {
        std::vector<isx_blender*> hs;
        std::vector<isx_mat> d, m;
        dsts.resize(bs.size()); dst_masks.resize(bs.size());
        for (size_t i = 0; i < bs.size(); ++i) {
            int w, h;
            check(isx_blender_result_size(bs[i]->h_, &w, &h));
            if (bs[i]->win_x1_ > bs[i]->win_x0_) w = bs[i]->win_x1_ - bs[i]->win_x0_;
            if (dsts[i].empty() || dsts[i].rows() != h || dsts[i].cols() != w) dsts[i].create(h, w, ISX_16SC3);
            dst_masks[i].create(h, w, ISX_8UC1);
            hs.push_back(bs[i]->h_); d.push_back(*dsts[i].c()); m.push_back(*dst_masks[i].c());
        }
        if (!bs.empty()) check(isx_blender_blend_batch(hs.data(), (int)bs.size(), d.data(), m.data()));
    }
    void setStream(void* hip_stream) { check(isx_blender_set_stream(h_, hip_stream)); }
    // Not in the reference (see imagestitch_hip.h): the deferred cycle (1: fed device mats stay valid until blend(); 2: feed() copies
    // them, OpenCV's contract) and the column window of a panorama that is cut into strips across GPUs.
    void setDeferredLevel0(int mode) { check(isx_blender_set_deferred_level0(h_, mode)); }
    void setWindow(int x0, int x1) { check(isx_blender_set_window(h_, x0, x1)); win_x0_ = x0; win_x1_ = x1; }
    isx_blender* handle() { return h_; }
protected:
    Blender() = default;
    isx_blender* h_ = nullptr;
    int win_x0_ = 0, win_x1_ = 0;
};

class MultiBandBlender : public Blender {
public:
    MultiBandBlender(int try_gpu = false, int num_bands = 5, int precision = ISX_PREC_I16, int device = 0) {
        (void)try_gpu;   // the reference passes false everywhere (W:276,278); this library IS the accelerator path
        check(isx_blender_create(ISX_BLEND_MULTI_BAND, num_bands, precision, device, &h_));
    }
    int numBands() { int n; check(isx_blender_num_bands(h_, &n)); return n; }
    void setNumBands(int val) { check(isx_blender_set_num_bands(h_, val)); }   // W:273
};

// cv::detail::FeatherBlender — the blender every reference demo actually runs (W:278-280)
class FeatherBlender : public Blender {
public:
    FeatherBlender(float sharpness = 0.02f, int device = 0) {
        check(isx_blender_create(ISX_BLEND_FEATHER, 0, ISX_PREC_I16, device, &h_));
        setSharpness(sharpness);
    }
    void setSharpness(float val) { check(isx_blender_set_sharpness(h_, val)); }   // fb->setSharpness(0.1)  W:280
};

// cv::detail::Blender itself - what Blender::createDefault(Blender::NO, false) returns (W:276): feed() copies the tile under its mask,
// blend() zeroes what no mask covered
class NoBlender : public Blender {
public:
    explicit NoBlender(int device = 0) { check(isx_blender_create(ISX_BLEND_NO, 0, ISX_PREC_I16, device, &h_)); }
};

inline std::shared_ptr<Blender> Blender::createDefault(int type, bool try_gpu, int precision) {
    if (type == NO) return std::make_shared<NoBlender>();
    if (type == FEATHER) return std::make_shared<FeatherBlender>();
    if (type != MULTI_BAND) throw Exception(ISX_ERR_INVALID, "Blender::createDefault: NO, FEATHER or MULTI_BAND");
    return std::make_shared<MultiBandBlender>(try_gpu, 5, precision);
}

// src.convertTo(dst, type) with alpha = 1, beta = 0 between the CV_8U / CV_16S / CV_32F depths (W:261, W:294, W:315's input)
inline void convertTo(const Mat& src, Mat& dst, int type, int device = 0) {
    if (dst.empty() || dst.rows() != src.rows() || dst.cols() != src.cols() || dst.type() != type) dst.create(src.rows(), src.cols(), type);
    check(isx_convert_to(src.c(), dst.c(), device, nullptr));
}

// dilate(mask, getStructuringElement(MORPH_RECT, Size(kw, kh))) [& other]  (W:286-301)
inline void dilateAnd(const Mat& mask, int kw, int kh, const Mat* other, Mat& out, int device = 0) {
    out.create(mask.rows(), mask.cols(), ISX_8UC1);
    check(isx_mask_dilate_and(mask.c(), other ? other->c() : nullptr, kw, kh, out.c(), device, nullptr));
}

// cv::resize(src, dst, dsize, fx, fy, interpolation) as OpenCV's stitching_detailed / Stitcher::composePanorama call it to bring the sources
// to seam_megapix (between W:264 and W:302 in the reference's flow): INTER_NEAREST or INTER_LINEAR on CV_8U / CV_32F, 1 or 3 channels
// (isx_resize).  An empty dsize takes (cvRound(cols * fx), cvRound(rows * fy)), ties to even.  dst must not share bytes with src (ISX_ERR_INVALID).
inline void resize(const Mat& src, Mat& dst, Size dsize, double fx = 0, double fy = 0, int interpolation = INTER_LINEAR, int device = 0) {
    if (dsize.width <= 0 || dsize.height <= 0) dsize = Size((int)std::nearbyint(src.cols() * fx), (int)std::nearbyint(src.rows() * fy));
    if (dsize.width <= 0 || dsize.height <= 0) throw Exception(ISX_ERR_SIZE, "resize: empty dsize");
    dst.create(dsize.height, dsize.width, src.type());
    check(isx_resize(src.c(), dst.c(), interpolation, device, nullptr));
}

// The compose loop's mask of one tile in one launch (isx_mask_dilate_resize_and):
//     dilate(masks_warped[i], dilated_mask, Mat());  resize(dilated_mask, seam_mask, mask_warped.size());  mask_warped = seam_mask & mask_warped;
// out = resize(dilate(seam_mask, MORPH_RECT kw x kh), warped_mask.size(), INTER_LINEAR) & warped_mask; out may be warped_mask itself (the same
// view), but must not share bytes with seam_mask, nor lie over warped_mask in any other way (ISX_ERR_INVALID)
inline void dilateResizeAnd(const Mat& seam_mask, const Mat& warped_mask, Mat& out, int kw = 3, int kh = 3, int device = 0) {
    out.create(warped_mask.rows(), warped_mask.cols(), ISX_8UC1);
    check(isx_mask_dilate_resize_and(seam_mask.c(), warped_mask.c(), kw, kh, out.c(), device, nullptr));
}
// ... without the AND: resize(dilate(seam_mask, kw x kh), size, INTER_LINEAR)
inline void dilateResizeAnd(const Mat& seam_mask, Size size, Mat& out, int kw = 3, int kh = 3, int device = 0) {
    out.create(size.height, size.width, ISX_8UC1);
    check(isx_mask_dilate_resize_and(seam_mask.c(), nullptr, kw, kh, out.c(), device, nullptr));
}

// cv::detail::DpSeamFinder as the reference restates it in-tree (S:60-1093): seam_finder->find(images_warped_f, corners, masks_seam)
// DpSeamFinder(DpSeamFinder::COLOR_GRAD) is the alternative every demo lists (W:255, S:1183): computeGradients S:549-572 and the COLOR_GRAD
// branches of computeCosts S:767-772 / S:792-797 on the GPU (isx_dp_seam_find_cost).
class DpSeamFinder {
public:
    enum CostFunction { COLOR = ISX_DP_COLOR, COLOR_GRAD = ISX_DP_COLOR_GRAD };   // S:71
    explicit DpSeamFinder(int device = 0) : cost_func_(COLOR), device_(device) {}
    explicit DpSeamFinder(CostFunction costFunc, int device = 0) : cost_func_(costFunc), device_(device) {}   // S:72
    CostFunction costFunction() const { return cost_func_; }
    void setCostFunction(CostFunction val) { cost_func_ = val; }
    void find(const std::vector<Mat>& src, const std::vector<Point>& corners, std::vector<Mat>& masks) {   // S:87, called at S:1192
        if (src.size() != corners.size() || src.size() != masks.size()) throw Exception(ISX_ERR_INVALID, "find: src, corners and masks differ in length");
        std::vector<isx_mat> im(src.size()), mk(src.size());
        std::vector<int> c;
        for (size_t i = 0; i < src.size(); ++i) { im[i] = *src[i].c(); mk[i] = *masks[i].c(); c.push_back(corners[i].x); c.push_back(corners[i].y); }
        check(isx_dp_seam_find_cost((int)src.size(), im.data(), c.data(), mk.data(), (int)cost_func_, device_, nullptr));
    }
private:
    CostFunction cost_func_;
    int device_;
};

// GraphCutSeamFinder(GraphCutSeamFinder::COST_COLOR) (W:257) and its find(images_warped_f, corners, masks_warped) (W:264): every pair's
// max-flow on the GPU, the maximal minimum cut (isx_graphcut_seam_find).  src: CV_32FC3 tiles holding integers in [0, 255] or CV_8UC3;
// masks: CV_8U, edited in place; host or device mats.  GraphCutSeamFinder(COST_COLOR_GRAD) (W:258) weighs every edge by the tiles' Sobel
// gradients as well (exact in 64-bit fixed point); it takes CV_32FC3 tiles only, as OpenCV's does.
class GraphCutSeamFinder {
public:
    enum CostType { COST_COLOR = ISX_GC_COST_COLOR, COST_COLOR_GRAD = ISX_GC_COST_COLOR_GRAD };
    explicit GraphCutSeamFinder(int cost_type = COST_COLOR, int device = 0) : cost_type_(cost_type), device_(device) {}
    void find(const std::vector<Mat>& src, const std::vector<Point>& corners, std::vector<Mat>& masks) {
        if (src.size() != corners.size() || src.size() != masks.size()) throw Exception(ISX_ERR_INVALID, "find: src, corners and masks differ in length");
        std::vector<isx_mat> im(src.size()), mk(src.size());
        std::vector<int> c;
        for (size_t i = 0; i < src.size(); ++i) { im[i] = *src[i].c(); mk[i] = *masks[i].c(); c.push_back(corners[i].x); c.push_back(corners[i].y); }
        check(isx_graphcut_seam_find((int)src.size(), im.data(), c.data(), mk.data(), cost_type_, device_, nullptr));
    }
private:
    int cost_type_, device_;
};

// VoronoiSeamFinder (S:1180) and its find(images_warped_f, corners, masks_seam) (S:1192): masks only - two city-block distance transforms
// and a compare per overlapping pair on the GPU (isx_voronoi_seam_find).  masks: CV_8U, edited in place; host or device mats.  On device
// masks nothing is synchronised: with a stream set and reserve() called first, find can be captured into a hipGraph.
class VoronoiSeamFinder {
public:
    explicit VoronoiSeamFinder(int device = 0, void* hip_stream = nullptr) : device_(device), stream_(hip_stream) {}
    void setStream(void* hip_stream) { stream_ = hip_stream; }
    void find(const std::vector<Size>& sizes, const std::vector<Point>& corners, std::vector<Mat>& masks) {
        if (sizes.size() != corners.size() || sizes.size() != masks.size()) throw Exception(ISX_ERR_INVALID, "find: sizes, corners and masks differ in length");
        std::vector<isx_mat> mk(masks.size());
        std::vector<int> c, sz;
        for (size_t i = 0; i < masks.size(); ++i) {
            mk[i] = *masks[i].c();
            c.push_back(corners[i].x); c.push_back(corners[i].y);
            sz.push_back(sizes[i].width); sz.push_back(sizes[i].height);
        }
        check(isx_voronoi_seam_find((int)masks.size(), sz.data(), c.data(), mk.data(), device_, stream_));
    }
    // the images are never read: only their sizes are used
    void find(const std::vector<Mat>& src, const std::vector<Point>& corners, std::vector<Mat>& masks) {
        std::vector<Size> sizes;
        for (size_t i = 0; i < src.size(); ++i) sizes.push_back(src[i].size());
        find(sizes, corners, masks);
    }
    void reserve(int max_roi_width, int max_roi_height) { check(isx_voronoi_seam_reserve(max_roi_width, max_roi_height, device_)); }
    static void release() { check(isx_voronoi_seam_release()); }
private:
    int device_;
    void* stream_;
};

// The features matcher of the M demo (M = the reference's 特征点匹配 demo): BestOf2NearestMatcher1 matcher(false, 0.3f, 6, 6);
// matcher(features, pairwise_matches) (M:307-308) as far as M:158 and the point gather of M:164-179 (isx_match_features): an exact 2-nearest-
// neighbour search over 32-byte descriptors on the GPU, the ratio test and the de-duplication of M:232-289.  Homography, inliers and
// confidence (M:181-229) are BestOf2NearestMatcher's, below: FeaturesMatcher leaves H and inliers_mask empty, num_inliers and confidence 0.
// CV_32FC1 descriptors of 1 .. 128 columns (the other depth CpuMatcher1::match admits, M:237) take isx_match_features_f32: an exact L2 search,
// DMatch::distance the float32 distance.  Both classes pick the entry by the mats' type; mixed types throw ISX_ERR_TYPE.
struct DMatch { int queryIdx = -1, trainIdx = -1; float distance = 0.f; };
struct ImageFeatures { int img_idx = 0; Size img_size; std::vector<Point2f> keypoints; Mat descriptors; };      // descriptors: n x 32 CV_8UC1, or n x cols CV_32FC1
struct MatchesInfo {
    int src_img_idx = -1, dst_img_idx = -1;
    std::vector<DMatch> matches;
    std::vector<Point2f> src_points, dst_points;
    std::vector<double> H;                        // empty, or the 3 x 3 homography, row-major (cv::detail::MatchesInfo::H)
    std::vector<unsigned char> inliers_mask;      // empty, or one byte per match
    int num_inliers = 0;
    double confidence = 0;
    int status = 0;                               // the ISX_HOMOGRAPHY_* bits of the pair
};

// The features finder of the F demo (F = the reference's 特征点检测 demo): OrbFeaturesFinder(grid_size, nfeatures, scaleFactor, nlevels) and
// find(image, features) (F:40-54, F:948-1017) on the GPU (isx_orb_find; tests/helpers/orb_np.py is the specification, DESIGN.md §8 "Features
// finder").  Keypoints come in canonical order (cell, level, y, x).  The sampling pattern is an input: the default is makeRandomPattern(31)
// (F:709-718); setPattern takes a CV_32SC1 512 x 2 mat of (x, y) inside the 31 x 31 patch - OpenCV's learned table, for a caller who has it.
struct KeyPoint { Point2f pt; float size = 0.f, angle = -1.f, response = 0.f; int octave = 0; };      // cv::KeyPoint as find fills it
class OrbFeaturesFinder {
public:
    explicit OrbFeaturesFinder(Size grid_size = Size(3, 1), int nfeatures = 1500, float scaleFactor = 1.3f, int nlevels = 5, int device = 0, void* hip_stream = nullptr)
        : device_(device), stream_(hip_stream) {
        check(isx_orb_default_params(&params_));
        params_.grid_width = grid_size.width; params_.grid_height = grid_size.height; params_.n_features = nfeatures; params_.scale_factor = scaleFactor;
        params_.nlevels = nlevels;
        check(isx_orb_capacity(&params_, &capacity_));
    }
    void setStream(void* hip_stream) { stream_ = hip_stream; }
    void setPattern(const Mat& pattern) { pattern_ = pattern; }
    int capacity() const { return capacity_; }
    int status() const { return status_; }        // of the last find: ISX_ORB_TRUNCATED | ISX_ORB_BAD_PATTERN
    const isx_orb_params& params() const { return params_; }
    // find(image, features) (F:948): image CV_8UC1, CV_8UC3 or CV_8UC4, host or device.  features.keypoints holds pt, features.descriptors
    // n x 32 CV_8UC1 on the host; `full`, when given, the whole cv::KeyPoint of each.
    void find(const Mat& image, ImageFeatures& features, std::vector<KeyPoint>* full = nullptr) {
        const int cap = capacity_ > 0 ? capacity_ : 1;
        Mat kp(cap, 2, ISX_32FC1), meta(cap, 4, ISX_32FC1), desc(cap, 32, ISX_8UC1), cs(1, 2, ISX_32SC1);
        check(isx_orb_find(image.c(), &params_, pattern_.empty() ? nullptr : pattern_.c(), kp.c(), meta.c(), desc.c(), cs.c(), device_, stream_));
        const int n = cs.ptr<int>(0)[0];
        status_ = cs.ptr<int>(0)[1];
        features.img_size = image.size();
        features.keypoints.clear();
        if (full) full->clear();
        features.descriptors = Mat();
        if (n > 0) features.descriptors.create(n, 32, ISX_8UC1);
        for (int r = 0; r < n; ++r) {
            const float* p = kp.ptr<float>(r);
            const float* m = meta.ptr<float>(r);
            features.keypoints.push_back(Point2f(p[0], p[1]));
            std::memcpy(features.descriptors.ptr<unsigned char>(r), desc.ptr<unsigned char>(r), 32);
            if (full) { KeyPoint k; k.pt = Point2f(p[0], p[1]); k.size = m[0]; k.angle = m[1]; k.response = m[2]; k.octave = (int)m[3]; full->push_back(k); }
        }
    }
    void operator()(const Mat& image, ImageFeatures& features) { find(image, features); }
    void reserve(Size image_size) { check(isx_orb_reserve(&params_, image_size.width, image_size.height, device_)); }
    static void release() { check(isx_orb_release()); }
private:
    isx_orb_params params_;
    Mat pattern_;
    int capacity_ = 0, status_ = 0, device_;
    void* stream_;
};

// The finder every main of the reference comments out: SurfFeaturesFinder(hess_thresh, num_octaves, num_layers, num_octaves_descr,
// num_layers_descr) of OpenCV 3.4.2's stitching module on the GPU (isx_surf_find; tests/helpers/surf_np.py is the specification, DESIGN.md §8
// "Features finder, SURF").  Keypoints come strongest first; the descriptors are n x 64 CV_32FC1, which FeaturesMatcher sends to the L2 entry.
// max_keypoints is the row count of the outputs: the strongest max_keypoints are returned and status() says ISX_SURF_TRUNCATED.
class SurfFeaturesFinder {
public:
    explicit SurfFeaturesFinder(double hess_thresh = 300., int num_octaves = 3, int num_layers = 4, int num_octaves_descr = 3, int num_layers_descr = 4,
                                int max_keypoints = 4096, int device = 0, void* hip_stream = nullptr)
        : capacity_(max_keypoints), device_(device), stream_(hip_stream) {
        check(isx_surf_default_params(&params_));
        params_.hess_thresh = hess_thresh; params_.num_octaves = num_octaves; params_.num_layers = num_layers;
        params_.num_octaves_descr = num_octaves_descr; params_.num_layers_descr = num_layers_descr;
    }
    void setStream(void* hip_stream) { stream_ = hip_stream; }
    int capacity() const { return capacity_; }
    int status() const { return status_; }        // of the last find: ISX_SURF_TRUNCATED | ISX_SURF_CANDIDATES_DROPPED
    const isx_surf_params& params() const { return params_; }
    // find(image, features): image CV_8UC1, CV_8UC3 or CV_8UC4, host or device.  features.keypoints holds pt, features.descriptors n x 64
    // CV_32FC1 on the host; `full`, when given, the whole cv::KeyPoint of each (class_id, the laplacian's sign, is not carried).
    void find(const Mat& image, ImageFeatures& features, std::vector<KeyPoint>* full = nullptr) {
        const int cap = capacity_ > 0 ? capacity_ : 1;
        Mat kp(cap, 2, ISX_32FC1), meta(cap, 5, ISX_32FC1), desc(cap, 64, ISX_32FC1), cs(1, 2, ISX_32SC1);
        check(isx_surf_find(image.c(), &params_, kp.c(), meta.c(), desc.c(), cs.c(), device_, stream_));
        const int n = cs.ptr<int>(0)[0];
        status_ = cs.ptr<int>(0)[1];
        features.img_size = image.size();
        features.keypoints.clear();
        if (full) full->clear();
        features.descriptors = Mat();
        if (n > 0) features.descriptors.create(n, 64, ISX_32FC1);
        for (int r = 0; r < n; ++r) {
            const float* p = kp.ptr<float>(r);
            const float* m = meta.ptr<float>(r);
            features.keypoints.push_back(Point2f(p[0], p[1]));
            std::memcpy(features.descriptors.ptr<float>(r), desc.ptr<float>(r), 64 * sizeof(float));
            if (full) { KeyPoint k; k.pt = Point2f(p[0], p[1]); k.size = m[0]; k.angle = m[1]; k.response = m[2]; k.octave = (int)m[3]; full->push_back(k); }
        }
    }
    void operator()(const Mat& image, ImageFeatures& features) { find(image, features); }
    void reserve(Size image_size) { check(isx_surf_reserve(&params_, image_size.width, image_size.height, capacity_ > 0 ? capacity_ : 1, device_)); }
    static void release() { check(isx_surf_release()); }
private:
    isx_surf_params params_;
    int capacity_ = 0, status_ = 0, device_;
    void* stream_;
};

// The finder cv::Stitcher and stitching_detailed --features sift offer beside the two above: SIFT::create(nfeatures, nOctaveLayers,
// contrastThreshold, edgeThreshold, sigma) of OpenCV 4.x on the GPU (isx_sift_find; tests/helpers/sift_np.py is the specification, DESIGN.md §8
// "Features finder, SIFT").  Keypoints come strongest first; the descriptors are n x 128 CV_32FC1, which FeaturesMatcher sends to the L2 entry.
// max_keypoints is the row count of the outputs: the strongest max_keypoints are returned and status() says ISX_SIFT_TRUNCATED.
class SiftFeaturesFinder {
public:
    explicit SiftFeaturesFinder(int nfeatures = 0, int n_octave_layers = 3, double contrast_threshold = 0.04, double edge_threshold = 10, double sigma = 1.6,
                                int max_keypoints = 4096, int device = 0, void* hip_stream = nullptr)
        : capacity_(max_keypoints), device_(device), stream_(hip_stream) {
        check(isx_sift_default_params(&params_));
        params_.nfeatures = nfeatures; params_.n_octave_layers = n_octave_layers; params_.contrast_threshold = contrast_threshold;
        params_.edge_threshold = edge_threshold; params_.sigma = sigma;
    }
    void setStream(void* hip_stream) { stream_ = hip_stream; }
    int capacity() const { return capacity_; }
    int status() const { return status_; }        // of the last find: ISX_SIFT_TRUNCATED | ISX_SIFT_CANDIDATES_DROPPED
    const isx_sift_params& params() const { return params_; }
    // find(image, features): image CV_8UC1, CV_8UC3 or CV_8UC4, host or device.  features.keypoints holds pt, features.descriptors n x 128
    // CV_32FC1 on the host; `full`, when given, the whole cv::KeyPoint of each: octave is packed as SIFT packs it, (octave & 255) | (layer << 8), without
    // the byte of the sub-layer offset.
    void find(const Mat& image, ImageFeatures& features, std::vector<KeyPoint>* full = nullptr) {
        const int cap = capacity_ > 0 ? capacity_ : 1;
        Mat kp(cap, 2, ISX_32FC1), meta(cap, 5, ISX_32FC1), desc(cap, 128, ISX_32FC1), cs(1, 2, ISX_32SC1);
        check(isx_sift_find(image.c(), &params_, kp.c(), meta.c(), desc.c(), cs.c(), device_, stream_));
        const int n = cs.ptr<int>(0)[0];
        status_ = cs.ptr<int>(0)[1];
        features.img_size = image.size();
        features.keypoints.clear();
        if (full) full->clear();
        features.descriptors = Mat();
        if (n > 0) features.descriptors.create(n, 128, ISX_32FC1);
        for (int r = 0; r < n; ++r) {
            const float* p = kp.ptr<float>(r);
            const float* m = meta.ptr<float>(r);
            features.keypoints.push_back(Point2f(p[0], p[1]));
            std::memcpy(features.descriptors.ptr<float>(r), desc.ptr<float>(r), 128 * sizeof(float));
            if (full) {
                KeyPoint k;
                k.pt = Point2f(p[0], p[1]); k.size = m[0]; k.angle = m[1]; k.response = m[2]; k.octave = ((int)m[3] & 255) | ((int)m[4] << 8);
                full->push_back(k);
            }
        }
    }
    void operator()(const Mat& image, ImageFeatures& features) { find(image, features); }
    void reserve(Size image_size) { check(isx_sift_reserve(&params_, image_size.width, image_size.height, capacity_ > 0 ? capacity_ : 1, device_)); }
    static void release() { check(isx_sift_release()); }
private:
    isx_sift_params params_;
    int capacity_ = 0, status_ = 0, device_;
    void* stream_;
};

class FeaturesMatcher {
public:
    explicit FeaturesMatcher(float match_conf = 0.3f, int device = 0, void* hip_stream = nullptr) : conf_(match_conf), device_(device), stream_(hip_stream) {}
    void setStream(void* hip_stream) { stream_ = hip_stream; }
    // One MatchesInfo per near pair (M:131-135: i < j, both images with features, mask(i, j) where a CV_8U n x n host mask is given), in
    // that order.  descriptors: host or device mats; keypoints and img_sizes may both be empty (then no points are gathered).
    std::vector<MatchesInfo> match(const std::vector<Mat>& descriptors, const std::vector<std::vector<Point2f> >& keypoints = std::vector<std::vector<Point2f> >(),
                                   const std::vector<Size>& img_sizes = std::vector<Size>(), const Mat& mask = Mat()) {
        const int n = (int)descriptors.size();
        const bool pts = !keypoints.empty();
        if (pts && ((int)keypoints.size() != n || (int)img_sizes.size() != n)) throw Exception(ISX_ERR_INVALID, "match: descriptors, keypoints and img_sizes differ in length");
        if (!mask.empty() && (mask.type() != ISX_8UC1 || mask.rows() != n || mask.cols() != n || mask.c()->device >= 0))
            throw Exception(ISX_ERR_INVALID, "match: the mask is not a CV_8U host mat of n x n");
        std::vector<isx_mat> d(n), kp(n);
        std::vector<int> sizes, pij;
        bool f32 = false, other = false;
        for (int i = 0; i < n; ++i) {
            d[i] = *descriptors[i].c();
            if (d[i].rows > 0 || d[i].cols > 0) (d[i].type == ISX_32FC1 ? f32 : other) = true;      // (a default Mat is an image without features)
            if (!pts) continue;
            if ((int)keypoints[i].size() != d[i].rows) throw Exception(ISX_ERR_SIZE, "match: keypoints and descriptor rows differ");
            kp[i].data = (void*)keypoints[i].data(); kp[i].rows = d[i].rows; kp[i].cols = 2; kp[i].type = ISX_32FC1; kp[i].step = sizeof(Point2f); kp[i].device = -1;
            sizes.push_back(img_sizes[i].width); sizes.push_back(img_sizes[i].height);
        }
        for (int i = 0; i < n - 1; ++i)
            for (int j = i + 1; j < n; ++j)
                if (d[i].rows > 0 && d[j].rows > 0 && (mask.empty() || mask.ptr<unsigned char>(i)[j])) { pij.push_back(i); pij.push_back(j); }
        if (f32 && other) throw Exception(ISX_ERR_TYPE, "match: descriptors of mixed types");
        const int np = (int)pij.size() / 2;
        std::vector<MatchesInfo> out(np);
        if (np == 0) return out;
        std::vector<Mat> m(np), p(np);
        std::vector<isx_mat> mm(np), pm(np);
        Mat counts(1, np, ISX_32SC1);
        for (int k = 0; k < np; ++k) {
            const int cap = d[pij[2 * k]].rows + d[pij[2 * k + 1]].rows;
            m[k].create(cap, 3, ISX_32SC1); mm[k] = *m[k].c();
            if (pts) { p[k].create(cap, 4, ISX_32FC1); pm[k] = *p[k].c(); }
        }
        if (f32)
            for (int i = 0; i < n; ++i) d[i].type = ISX_32FC1;                                    // (so that an empty default Mat passes the type check)
        check((f32 ? isx_match_features_f32 : isx_match_features)(n, d.data(), pts ? kp.data() : nullptr, pts ? sizes.data() : nullptr, np, pij.data(), conf_,
                                                                  mm.data(), pts ? pm.data() : nullptr, counts.c(), nullptr, info_, device_, stream_));
        afterMatch(pts ? &pm : nullptr, counts.c(), out);
        for (int k = 0; k < np; ++k) {
            MatchesInfo& mi = out[k];
            mi.src_img_idx = pij[2 * k]; mi.dst_img_idx = pij[2 * k + 1];
            const int cnt = counts.ptr<int>(0)[k];
            for (int r = 0; r < cnt; ++r) {
                const int* row = m[k].ptr<int>(r);
                DMatch dm; dm.queryIdx = row[0]; dm.trainIdx = row[1]; dm.distance = (float)row[2];
                if (f32) std::memcpy(&dm.distance, &row[2], sizeof(float));                       // the float entry carries the distance's bits
                mi.matches.push_back(dm);
                if (pts) { const float* q = p[k].ptr<float>(r); mi.src_points.push_back(Point2f(q[0], q[1])); mi.dst_points.push_back(Point2f(q[2], q[3])); }
            }
        }
        return out;
    }
    // matcher(features, pairwise_matches, mask) (M:123-144): pairwise_matches gets n * n entries, entry i * n + j filled for a near pair
    void operator()(const std::vector<ImageFeatures>& features, std::vector<MatchesInfo>& pairwise_matches, const Mat& mask = Mat()) {
        const size_t n = features.size();
        std::vector<Mat> d;
        std::vector<std::vector<Point2f> > kp;
        std::vector<Size> sz;
        for (size_t i = 0; i < n; ++i) { d.push_back(features[i].descriptors); kp.push_back(features[i].keypoints); sz.push_back(features[i].img_size); }
        const std::vector<MatchesInfo> near = match(d, kp, sz, mask);
        pairwise_matches.assign(n * n, MatchesInfo());                                        // M:137
        for (size_t k = 0; k < near.size(); ++k) pairwise_matches[(size_t)near[k].src_img_idx * n + near[k].dst_img_idx] = near[k];
    }
    int pairsSearched() const { return info_[0]; }
    int launches() const { return info_[1]; }     // kernel launches of the last call: at most three, however many pairs
    static void release() { check(isx_match_release()); }
    virtual ~FeaturesMatcher() {}
protected:
    // what a subclass runs on the matcher's points (NULL without keypoints) and counts mats before the records are filled
    virtual void afterMatch(std::vector<isx_mat>*, isx_mat*, std::vector<MatchesInfo>&) {}
    float conf_;
    int device_;
    void* stream_;
private:
    int info_[2] = {0, 0};
};

// BestOf2NearestMatcher1(try_use_gpu, match_conf, num_matches_thresh1, num_matches_thresh2) (R:781-782 of the 计算单应性矩阵 demo) with the whole of
// its match(), R:830-911: FeaturesMatcher's matches, then findHomography(RANSAC), the inlier mask, num_inliers, confidence and the second run
// on the inliers for every pair in one launch (isx_find_homography).  Needs keypoints.  The Levenberg-Marquardt polish of R:672 is opt-in, setRefine(true):
// isx_find_homography_lm, its OpenCV calls restated (unpinned); lmStats() then holds run()'s return value and nfJ of both passes per pair.
class BestOf2NearestMatcher : public FeaturesMatcher {
public:
    explicit BestOf2NearestMatcher(float match_conf = 0.3f, int num_matches_thresh1 = 6, int num_matches_thresh2 = 6, int device = 0, void* hip_stream = nullptr)
        : FeaturesMatcher(match_conf, device, hip_stream), thresh1_(num_matches_thresh1), thresh2_(num_matches_thresh2) {}
    void setRansac(double reproj_thresh, int max_iters, double confidence) { reproj_ = reproj_thresh; max_iters_ = max_iters; confidence_ = confidence; }
    void setRefine(bool refine, int lm_max_iters = 10) { refine_ = refine; lm_max_iters_ = lm_max_iters; }      // 10 at R:672; 1 .. 1000
    const std::vector<int>& lmStats() const { return lm_stats_; }      // after a refined match(): 4 per pair, stats columns 8 - 11; else empty
    int homographyLaunches() const { return hinfo_[1]; }      // one, however many pairs
    static void release() { FeaturesMatcher::release(); check(isx_homography_release()); }
protected:
    void afterMatch(std::vector<isx_mat>* points, isx_mat* counts, std::vector<MatchesInfo>& out) override {
        if (!points) throw Exception(ISX_ERR_INVALID, "BestOf2NearestMatcher: the homography needs keypoints and img_sizes");
        const int np = (int)out.size();
        std::vector<double> H((size_t)9 * np), conf((size_t)np);
        const int ns = refine_ ? 12 : 8;
        std::vector<int> stats((size_t)ns * np);
        std::vector<std::vector<unsigned char> > masks(np);
        std::vector<isx_mat> mm(np);
        for (int k = 0; k < np; ++k) {
            masks[k].resize((size_t)(*points)[k].rows);
            mm[k].data = masks[k].data(); mm[k].rows = (*points)[k].rows; mm[k].cols = 1; mm[k].type = ISX_8UC1; mm[k].step = 1; mm[k].device = -1;
        }
        isx_mat hm, sm, cm;
        hm.data = H.data(); hm.rows = 3 * np; hm.cols = 3; hm.type = ISX_64FC1; hm.step = 24; hm.device = -1;
        sm.data = stats.data(); sm.rows = np; sm.cols = ns; sm.type = ISX_32SC1; sm.step = 4 * (size_t)ns; sm.device = -1;
        cm.data = conf.data(); cm.rows = 1; cm.cols = np; cm.type = ISX_64FC1; cm.step = sizeof(double) * (size_t)np; cm.device = -1;
        if (refine_)
            check(isx_find_homography_lm(np, points->data(), counts, reproj_, max_iters_, confidence_, thresh1_, thresh2_, lm_max_iters_, &hm, mm.data(), &sm, &cm,
                                         hinfo_, device_, stream_));
        else
            check(isx_find_homography(np, points->data(), counts, reproj_, max_iters_, confidence_, thresh1_, thresh2_, &hm, mm.data(), &sm, &cm, hinfo_, device_, stream_));
        lm_stats_.clear();
        for (int k = 0; k < np; ++k) {
            MatchesInfo& mi = out[k];
            const int cnt = ((const int*)counts->data)[k];
            mi.status = stats[(size_t)ns * k];
            if (refine_) lm_stats_.insert(lm_stats_.end(), stats.begin() + (size_t)ns * k + 8, stats.begin() + (size_t)ns * k + 12);
            if (mi.status & ISX_HOMOGRAPHY_H) mi.H.assign(H.begin() + 9 * k, H.begin() + 9 * k + 9);
            if (cnt >= thresh1_) mi.inliers_mask.assign(masks[k].begin(), masks[k].begin() + cnt);      // R:836 returns before the mask exists
            mi.num_inliers = stats[(size_t)ns * k + 1];
            mi.confidence = conf[k];
        }
    }
private:
    int thresh1_, thresh2_;
    double reproj_ = 3.0, confidence_ = 0.995;
    int max_iters_ = 2000;
    int hinfo_[2] = {0, 0};
    bool refine_ = false;
    int lm_max_iters_ = 10;
    std::vector<int> lm_stats_;
};

// HomographyBasedEstimator1 estimator; estimator(features, pairwise_matches, cameras) (C:313-321 of the reference's 恢复相机内参数 demo;
// isx_estimate_cameras): a focal from the pairwise homographies (C:26-105), the maximum spanning tree over num_inliers (C:145-213) and the
// rotations along it (C:215-243), one rig - all images of the call - in one launch.  pairwise_matches is the matcher's n * n vector: entry
// i * n + j with i < j is read (H where status has ISX_HOMOGRAPHY_H, num_inliers), the duals are formed on the GPU.  Mat::inv(), Mat * Mat
// and Graph::walkBreadthFirst are restated, equal weights sort by i * n + j: unpinned (tests/helpers/estimator_np.py is the specification).
struct CameraParams {                             // cv::detail::CameraParams
    double focal = 1, aspect = 1, ppx = 0, ppy = 0;
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double t[3] = {0, 0, 0};
    float K32[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};   // K() and R as convertTo(CV_32F) gives them (C:329-334, C:385-386): what RotationWarper takes
    float R32[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    int parent = -2, depth = -1;                  // the camera's place in the walk from the tree's center: -1 the root, -2 not reached
    void K(double k[9]) const { k[0] = focal; k[1] = 0; k[2] = ppx; k[3] = 0; k[4] = focal * aspect; k[5] = ppy; k[6] = 0; k[7] = 0; k[8] = 1; }
};

class HomographyBasedEstimator {
public:
    explicit HomographyBasedEstimator(bool is_focals_estimated = false, int device = 0, void* hip_stream = nullptr)
        : given_(is_focals_estimated), device_(device), stream_(hip_stream) {}
    void setStream(void* hip_stream) { stream_ = hip_stream; }
    // With is_focals_estimated, focal, aspect, ppx and ppy of `cameras` come in (C:264-268); R and t are replaced either way.
    bool operator()(const std::vector<ImageFeatures>& features, const std::vector<MatchesInfo>& pairwise_matches, std::vector<CameraParams>& cameras) {
        const int n = (int)features.size();
        if ((int)pairwise_matches.size() != n * n) throw Exception(ISX_ERR_INVALID, "HomographyBasedEstimator: pairwise_matches is not n * n");
        if (given_ && (int)cameras.size() != n) throw Exception(ISX_ERR_INVALID, "HomographyBasedEstimator: is_focals_estimated needs n cameras");
        std::vector<int> sizes, pij, stats;
        std::vector<double> H, fin;
        for (int i = 0; i < n; ++i) { sizes.push_back(features[i].img_size.width); sizes.push_back(features[i].img_size.height); }
        for (int i = 0; i < n - 1; ++i)
            for (int j = i + 1; j < n; ++j) {
                const MatchesInfo& mi = pairwise_matches[(size_t)i * n + j];
                if (mi.src_img_idx < 0) continue;
                const bool has = (mi.status & ISX_HOMOGRAPHY_H) && mi.H.size() == 9;
                pij.push_back(i); pij.push_back(j);
                stats.push_back(has ? ISX_HOMOGRAPHY_H : 0); stats.push_back(mi.num_inliers);
                for (int e = 0; e < 9; ++e) H.push_back(has ? mi.H[e] : 0.0);
            }
        const int np = (int)pij.size() / 2;
        std::vector<double> conf((size_t)(np > 0 ? np : 1), 0.0), cams((size_t)16 * n);
        std::vector<float> kr((size_t)18 * n);
        std::vector<int> tree((size_t)2 * n);
        if (H.empty()) { H.resize(9); stats.resize(2); }
        if (given_)
            for (int i = 0; i < n; ++i) { fin.push_back(cameras[i].focal); fin.push_back(cameras[i].aspect); fin.push_back(cameras[i].ppx); fin.push_back(cameras[i].ppy); }
        isx_mat hm = host(H.data(), 3 * np, 3, ISX_64FC1, 24), sm = host(stats.data(), np, 2, ISX_32SC1, 8), cm = host(conf.data(), 1, np, ISX_64FC1, 8 * (size_t)(np > 0 ? np : 1));
        isx_mat fm = host(fin.data(), n, 4, ISX_64FC1, 32), om = host(cams.data(), n, 16, ISX_64FC1, 128), km = host(kr.data(), n, 18, ISX_32FC1, 72);
        isx_mat tm = host(tree.data(), n, 2, ISX_32SC1, 8), rm = host(rig_stats_, 1, 8, ISX_32SC1, 32);
        check(isx_estimate_cameras(n, sizes.data(), np, pij.data(), 1, nullptr, &hm, &sm, &cm, given_ ? &fm : nullptr, &om, &km, &tm, &rm, info_, device_, stream_));
        cameras.assign((size_t)n, CameraParams());
        for (int i = 0; i < n; ++i) {
            CameraParams& c = cameras[i];
            const double* s = &cams[(size_t)16 * i];
            c.focal = s[0]; c.aspect = s[1]; c.ppx = s[2]; c.ppy = s[3];
            std::memcpy(c.R, s + 4, sizeof(c.R)); std::memcpy(c.t, s + 13, sizeof(c.t));
            std::memcpy(c.K32, &kr[(size_t)18 * i], sizeof(c.K32)); std::memcpy(c.R32, &kr[(size_t)18 * i + 9], sizeof(c.R32));
            c.parent = tree[(size_t)2 * i]; c.depth = tree[(size_t)2 * i + 1];
        }
        return true;
    }
    const int* rigStats() const { return rig_stats_; }      // status bits (ISX_ESTIMATOR_*), candidates, the two centers, tree edges, reached, centers, min-max distance
    int launches() const { return info_[1]; }               // one
    static void release() { check(isx_estimator_release()); }
private:
    static isx_mat host(void* data, int rows, int cols, int type, size_t step) {
        isx_mat m; m.data = data; m.rows = rows; m.cols = cols; m.type = type; m.step = step; m.device = -1; return m;
    }
    bool given_;
    int device_;
    void* stream_;
    int rig_stats_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int info_[2] = {0, 0};
};

// adjuster = new detail::BundleAdjusterRay(); adjuster->setConfThresh(1); (*adjuster)(features, pairwise_matches, cameras) (W:189-194 of the
// reference's cylindrical-projection demo; isx_bundle_adjust_ray): focal and rotation of every camera refined over the inlier matches of
// every pair with confidence > conf_thresh, one rig - all images of the call - in one launch.  pairwise_matches is the matcher's n * n vector
// (entry i * n + j with i < j is read: matches, inliers_mask, confidence), features carry the keypoints, cameras are the estimator's.  The
// center is the estimator's span_tree_centers[0]: hand its rigStats() to setEstimatorStats() before the call - findMaxSpanningTree is not
// built a second time.  OpenCV's BundleAdjusterBase::estimate, CvLevMarq and cvRodrigues2 are restated; the solve is a Cholesky
// factorisation with SVBkSb's truncation rule, sin / cos / acos are restated, summation orders are fixed: unpinned
// (tests/helpers/bundle_np.py is the specification).  Returns false where estimate() would (a NaN parameter) and where the rig passes
// through (no edge, the estimator's assert): cameras are then unchanged but for K32 / R32.
// BundleAdjusterBase holds what BundleAdjusterRay and BundleAdjusterReproj share: everything but the entry point they call.
class BundleAdjusterBase {
public:
    explicit BundleAdjusterBase(int device = 0, void* hip_stream = nullptr) : device_(device), stream_(hip_stream) {}
    virtual ~BundleAdjusterBase() {}
    void setStream(void* hip_stream) { stream_ = hip_stream; }
    void setConfThresh(double conf_thresh) { conf_thresh_ = conf_thresh; }
    void setTermCriteria(int max_iter, double eps) { max_iter_ = max_iter; eps_ = eps; }      // TermCriteria(EPS + COUNT, 1000, DBL_EPSILON)
    void setEstimatorStats(const int rig_stats[8]) { std::memcpy(est_, rig_stats, sizeof(est_)); }
    bool operator()(const std::vector<ImageFeatures>& features, const std::vector<MatchesInfo>& pairwise_matches, std::vector<CameraParams>& cameras) {
        static_assert(sizeof(DMatch) == 12 && sizeof(Point2f) == 8, "DMatch is a row of queryIdx, trainIdx, distance; Point2f a row of x, y");
        const int n = (int)features.size();
        if ((int)pairwise_matches.size() != n * n) throw Exception(ISX_ERR_INVALID, std::string(name()) + ": pairwise_matches is not n * n");
        if ((int)cameras.size() != n) throw Exception(ISX_ERR_INVALID, std::string(name()) + ": needs n cameras");
        std::vector<int> sizes, pij, counts, stats;
        std::vector<double> conf;
        std::vector<isx_mat> kp(n), mt, mk;
        for (int i = 0; i < n; ++i) {
            sizes.push_back(features[i].img_size.width); sizes.push_back(features[i].img_size.height);
            kp[i] = host((void*)features[i].keypoints.data(), (int)features[i].keypoints.size(), 2, ISX_32FC1, sizeof(Point2f));
        }
        for (int i = 0; i < n - 1; ++i)
            for (int j = i + 1; j < n; ++j) {
                const MatchesInfo& mi = pairwise_matches[(size_t)i * n + j];
                if (mi.src_img_idx < 0) continue;
                pij.push_back(i); pij.push_back(j);
                counts.push_back((int)mi.matches.size());
                stats.push_back(mi.status); stats.push_back(mi.num_inliers);
                conf.push_back(mi.confidence);
                mt.push_back(host((void*)mi.matches.data(), (int)mi.matches.size(), 3, ISX_32SC1, sizeof(DMatch)));
                mk.push_back(host((void*)mi.inliers_mask.data(), (int)mi.inliers_mask.size(), 1, ISX_8UC1, 1));
            }
        const int np = (int)pij.size() / 2;
        if (np == 0) { counts.resize(1); stats.resize(2); conf.resize(1); }
        std::vector<double> cin((size_t)16 * n), cams((size_t)16 * n);
        std::vector<float> kr((size_t)18 * n);
        for (int i = 0; i < n; ++i) {
            const CameraParams& c = cameras[i];
            double* s = &cin[(size_t)16 * i];
            s[0] = c.focal; s[1] = c.aspect; s[2] = c.ppx; s[3] = c.ppy;
            std::memcpy(s + 4, c.R, sizeof(c.R)); std::memcpy(s + 13, c.t, sizeof(c.t));
        }
        isx_mat cm = host(counts.data(), 1, np, ISX_32SC1, 4 * (size_t)(np > 0 ? np : 1)), sm = host(stats.data(), np, 2, ISX_32SC1, 8);
        isx_mat fm = host(conf.data(), 1, np, ISX_64FC1, 8 * (size_t)(np > 0 ? np : 1)), em = host(est_, 1, 8, ISX_32SC1, 32);
        isx_mat im = host(cin.data(), n, 16, ISX_64FC1, 128), om = host(cams.data(), n, 16, ISX_64FC1, 128), km = host(kr.data(), n, 18, ISX_32FC1, 72);
        isx_mat rm = host(rig_stats_, 1, 8, ISX_32SC1, 32), re = host(rig_err_, 1, 2, ISX_64FC1, 16);
        check(run(n, sizes.data(), kp.data(), np, pij.data(), mt.data(), mk.data(), &cm, &sm, &fm, &em, &im, &om, &km, &rm, &re));
        for (int i = 0; i < n; ++i) {
            CameraParams& c = cameras[i];
            const double* s = &cams[(size_t)16 * i];
            c.focal = s[0]; c.aspect = s[1]; c.ppx = s[2]; c.ppy = s[3];
            std::memcpy(c.R, s + 4, sizeof(c.R)); std::memcpy(c.t, s + 13, sizeof(c.t));
            std::memcpy(c.K32, &kr[(size_t)18 * i], sizeof(c.K32)); std::memcpy(c.R32, &kr[(size_t)18 * i + 9], sizeof(c.R32));
        }
        return (rig_stats_[0] & (ISX_BUNDLE_NAN | ISX_BUNDLE_NO_EDGES | ISX_BUNDLE_EST_ASSERT)) == 0;
    }
    const int* rigStats() const { return rig_stats_; }      // status bits (ISX_BUNDLE_*), iterations, Jacobian and error evaluations, lambdaLg10, edges, matches, 0
    const double* rigErr() const { return rig_err_; }       // the first and the last |err|
    int launches() const { return info_[1]; }               // one
    static void release() { check(isx_bundle_release()); }
protected:
    virtual const char* name() const = 0;
    // the entry point on one rig of n images: isx_bundle_adjust_ray's arguments without what the members hold
    virtual int run(int n, const int* sizes, const isx_mat* kp, int np, const int* pij, const isx_mat* mt, const isx_mat* mk, const isx_mat* counts,
                    const isx_mat* stats, const isx_mat* conf, const isx_mat* est, const isx_mat* cin, isx_mat* cams, isx_mat* kr, isx_mat* rs, isx_mat* re) = 0;
    static isx_mat host(void* data, int rows, int cols, int type, size_t step) {
        isx_mat m; m.data = data; m.rows = rows; m.cols = cols; m.type = type; m.step = step; m.device = -1; return m;
    }
    int device_;
    void* stream_;
    double conf_thresh_ = 1.0, eps_ = 2.220446049250313e-16;
    int max_iter_ = 1000;
    int est_[8] = {0, 0, 0, -1, 0, 0, 1, 0};
    int rig_stats_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double rig_err_[2] = {0, 0};
    int info_[2] = {0, 0};
};
class BundleAdjusterRay : public BundleAdjusterBase {
public:
    explicit BundleAdjusterRay(int device = 0, void* hip_stream = nullptr) : BundleAdjusterBase(device, hip_stream) {}
protected:
    const char* name() const override { return "BundleAdjusterRay"; }
    int run(int n, const int* sizes, const isx_mat* kp, int np, const int* pij, const isx_mat* mt, const isx_mat* mk, const isx_mat* counts, const isx_mat* stats,
            const isx_mat* conf, const isx_mat* est, const isx_mat* cin, isx_mat* cams, isx_mat* kr, isx_mat* rs, isx_mat* re) override {
        return isx_bundle_adjust_ray(n, sizes, kp, np, pij, mt, mk, counts, stats, conf, 1, nullptr, est, cin, conf_thresh_, max_iter_, eps_, cams, kr, rs, re,
                                     info_, device_, stream_);
    }
};
// detail::BundleAdjusterReproj (commented out at W:190 of the reference; cv::Stitcher's default; isx_bundle_adjust_reproj): BundleAdjusterRay's
// call and results with focal, ppx, ppy, aspect and rotation of every camera refined over the reprojection error.  setRefinementMask takes
// OpenCV's 3 x 3 mask row by row ((0,0) focal, (0,2) ppx, (1,1) aspect, (1,2) ppy; the other entries are not read) or the flags.  A parameter
// that is not refined keeps its value and sets ISX_BUNDLE_DROPPED.  Unpinned: tests/helpers/bundle_reproj_np.py is the specification.
class BundleAdjusterReproj : public BundleAdjusterBase {
public:
    explicit BundleAdjusterReproj(int device = 0, void* hip_stream = nullptr) : BundleAdjusterBase(device, hip_stream) {}
    void setRefinementMask(const unsigned char mask[9]) {
        refine_flags_ = (mask[0] ? 1 : 0) | (mask[1] ? 2 : 0) | (mask[2] ? 4 : 0) | (mask[4] ? 8 : 0) | (mask[5] ? 16 : 0);
    }
    void setRefinementFlags(int refine_flags) { refine_flags_ = refine_flags; }
    int refinementFlags() const { return refine_flags_; }
protected:
    const char* name() const override { return "BundleAdjusterReproj"; }
    int run(int n, const int* sizes, const isx_mat* kp, int np, const int* pij, const isx_mat* mt, const isx_mat* mk, const isx_mat* counts, const isx_mat* stats,
            const isx_mat* conf, const isx_mat* est, const isx_mat* cin, isx_mat* cams, isx_mat* kr, isx_mat* rs, isx_mat* re) override {
        return isx_bundle_adjust_reproj(n, sizes, kp, np, pij, mt, mk, counts, stats, conf, 1, nullptr, est, cin, conf_thresh_, max_iter_, eps_, refine_flags_,
                                        cams, kr, rs, re, info_, device_, stream_);
    }
private:
    int refine_flags_ = 31;
};

// detail::waveCorrect(rmats, kind) (commented out at W:198, C:355-361 of the reference; cv::Stitcher's default; isx_wave_correct) on the
// cameras of one rig: R, and with it R32, of every camera replaced; focal, aspect, ppx, ppy, t and K32's values unchanged.  Returns false
// where waveCorrect returns early (one camera, a degenerate rig): the cameras are then unchanged but for K32 / R32.
enum WaveCorrectKind { WAVE_CORRECT_HORIZ = ISX_WAVE_CORRECT_HORIZ, WAVE_CORRECT_VERT = ISX_WAVE_CORRECT_VERT };
inline bool waveCorrect(std::vector<CameraParams>& cameras, WaveCorrectKind kind = WAVE_CORRECT_HORIZ, int device = 0, void* hip_stream = nullptr) {
    const int n = (int)cameras.size();
    if (n == 0) return false;
    std::vector<double> cin((size_t)16 * n), cams((size_t)16 * n);
    std::vector<float> kr((size_t)18 * n);
    int rs[2] = {0, 0};
    for (int i = 0; i < n; ++i) {
        const CameraParams& c = cameras[i];
        double* s = &cin[(size_t)16 * i];
        s[0] = c.focal; s[1] = c.aspect; s[2] = c.ppx; s[3] = c.ppy;
        std::memcpy(s + 4, c.R, sizeof(c.R)); std::memcpy(s + 13, c.t, sizeof(c.t));
    }
    isx_mat im, om, km, rm;
    im.data = cin.data(); im.rows = n; im.cols = 16; im.type = ISX_64FC1; im.step = 128; im.device = -1;
    om = im; om.data = cams.data();
    km.data = kr.data(); km.rows = n; km.cols = 18; km.type = ISX_32FC1; km.step = 72; km.device = -1;
    rm.data = rs; rm.rows = 1; rm.cols = 2; rm.type = ISX_32SC1; rm.step = 8; rm.device = -1;
    check(isx_wave_correct(n, 1, nullptr, &im, (int)kind, &om, &km, &rm, nullptr, device, hip_stream));
    for (int i = 0; i < n; ++i) {
        CameraParams& c = cameras[i];
        std::memcpy(c.R, &cams[(size_t)16 * i + 4], sizeof(c.R));
        std::memcpy(c.K32, &kr[(size_t)18 * i], sizeof(c.K32)); std::memcpy(c.R32, &kr[(size_t)18 * i + 9], sizeof(c.R32));
    }
    return rs[0] == 0;
}

// cv::imread(path) (W:166): the decoder follows the file's signature, as OpenCV's does - "BM" bitmaps and JFIF / Exif JPEGs;
// cv::imwrite(path, img) for .bmp and .jpg (W:155-156,315; "pano.jpg" S:1282)
inline Mat imread(const char* path) {
    unsigned char sig[2] = {0, 0};
    if (FILE* f = std::fopen(path, "rb")) { if (std::fread(sig, 1, 2, f) != 2) sig[0] = sig[1] = 0; std::fclose(f); }
    const bool jpeg = sig[0] == 0xFF && sig[1] == 0xD8;
    int rows = 0, cols = 0;
    check(jpeg ? isx_jpeg_size(path, &rows, &cols) : isx_bmp_size(path, &rows, &cols));
    Mat m;
    m.create(rows, cols, ISX_8UC3);
    check(jpeg ? isx_jpeg_read(path, m.c()) : isx_bmp_read(path, m.c()));
    return m;
}
// the format follows the extension, as in OpenCV: .jpg / .jpeg -> baseline JFIF at cv::IMWRITE_JPEG_QUALITY (default 95), else .bmp
inline void imwrite(const char* path, const Mat& img, int jpeg_quality = 95) {
    const char* dot = nullptr;
    for (const char* q = path; *q; ++q) if (*q == '.') dot = q;
    auto ieq = [](const char* a, const char* b) { for (; *a && *b; ++a, ++b) if ((*a | 32) != *b) return false; return *a == *b; };
    if (dot && (ieq(dot, ".jpg") || ieq(dot, ".jpeg") || ieq(dot, ".jpe"))) check(isx_jpeg_write(path, img.c(), jpeg_quality));
    else check(isx_bmp_write(path, img.c()));
}

// GainCompensator::apply: multiply(image, gain, image)  (W:241-244)
inline void gainApply(Mat& image, double gain, int device = 0) { check(isx_gain_apply(image.c(), gain, device, nullptr)); }

// cv::detail::GainCompensator, what ExposureCompensator::createDefault(ExposureCompensator::GAIN) returns (W:238-244):
// feed(corners, images_warped, masks_warped) estimates one gain per tile on the GPU (isx_gain_compensator_feed), apply(i, ...)
// multiplies tile i by its gain (isx_gain_apply).  Images CV_8UC3, masks CV_8U of the images' sizes (255 = in), host or device.
class GainCompensator {
public:
    explicit GainCompensator(int device = 0) : device_(device) {}
    void feed(const std::vector<Point>& corners, const std::vector<Mat>& images, const std::vector<Mat>& masks) {
        if (images.size() != corners.size() || images.size() != masks.size())
            throw Exception(ISX_ERR_INVALID, "feed: corners, images and masks differ in length");
        std::vector<isx_mat> im(images.size()), mk(images.size());
        std::vector<int> c;
        for (size_t i = 0; i < images.size(); ++i) { im[i] = *images[i].c(); mk[i] = *masks[i].c(); c.push_back(corners[i].x); c.push_back(corners[i].y); }
        std::vector<double> g(images.size());
        check(isx_gain_compensator_feed((int)images.size(), c.data(), im.data(), mk.data(), g.data(), nullptr, nullptr, device_, nullptr));
        gains_ = g;
    }
    // gains(): one per tile fed (GainCompensator::gains)
    std::vector<double> gains() const { return gains_; }
    void apply(int index, Point /*corner*/, Mat& image, const Mat& /*mask*/) {
        if (index < 0 || (size_t)index >= gains_.size()) throw Exception(ISX_ERR_STATE, "apply: no gain for this index (feed first)");
        check(isx_gain_apply(image.c(), gains_[(size_t)index], device_, nullptr));
    }
private:
    int device_;
    std::vector<double> gains_;
};

// cv::detail::BlocksGainCompensator(bl_width = 32, bl_height = 32), what ExposureCompensator::createDefault(ExposureCompensator::GAIN_BLOCKS)
// returns (W:238-244): feed estimates one gain per block of every tile - the statistics and the dense LU solve on the GPU
// (isx_blocks_gain_feed) - and keeps one smoothed gain map per tile on the device; apply(i, ...) multiplies tile i by its map resized to
// the tile (isx_blocks_gain_apply).  Images CV_8UC3, masks CV_8U of the images' sizes (255 = in), host or device.
class BlocksGainCompensator {
public:
    explicit BlocksGainCompensator(int bl_width = 32, int bl_height = 32, int device = 0) { check(isx_blocks_gain_create(bl_width, bl_height, device, &h_)); }
    ~BlocksGainCompensator() { isx_blocks_gain_destroy(h_); }
    BlocksGainCompensator(const BlocksGainCompensator&) = delete;
    BlocksGainCompensator& operator=(const BlocksGainCompensator&) = delete;
    void feed(const std::vector<Point>& corners, const std::vector<Mat>& images, const std::vector<Mat>& masks) {
        if (images.size() != corners.size() || images.size() != masks.size())
            throw Exception(ISX_ERR_INVALID, "feed: corners, images and masks differ in length");
        std::vector<isx_mat> im(images.size()), mk(images.size());
        std::vector<int> c;
        for (size_t i = 0; i < images.size(); ++i) { im[i] = *images[i].c(); mk[i] = *masks[i].c(); c.push_back(corners[i].x); c.push_back(corners[i].y); }
        check(isx_blocks_gain_feed(h_, (int)images.size(), c.data(), im.data(), mk.data(), nullptr));
    }
    void apply(int index, Point /*corner*/, Mat& image, const Mat& /*mask*/) { check(isx_blocks_gain_apply(h_, index, image.c(), nullptr)); }
    // the raw gains, one per block (blocks numbered image by image, rows of blocks outer)
    std::vector<double> gains() const {
        int n = 0, nb = 0;
        check(isx_blocks_gain_num_images(h_, &n, &nb));
        std::vector<double> g((size_t)nb);
        check(isx_blocks_gain_gains(h_, g.data()));
        return g;
    }
    // the smoothed gain map of tile `index`: ny x nx CV_32FC1 on the host
    Mat gainMap(int index) const {
        int n = 0, nb = 0;
        check(isx_blocks_gain_num_images(h_, &n, &nb));
        if (index < 0 || index >= n) throw Exception(ISX_ERR_INVALID, "gainMap: no such image");
        std::vector<int> cnt(2 * (size_t)n);
        check(isx_blocks_gain_block_counts(h_, cnt.data()));
        Mat m(cnt[2 * (size_t)index + 1], cnt[2 * (size_t)index], ISX_32FC1);
        check(isx_blocks_gain_map(h_, index, m.c(), nullptr));
        return m;
    }
private:
    isx_blocks_gain* h_ = nullptr;
};

}  // namespace isx
