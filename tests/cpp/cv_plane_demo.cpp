// cv_plane_demo.cpp — plane_demo.cpp's calls through the OpenCV adapter include/imagestitch_cv_plane.hpp: isx_cv::HipPlaneWarper used
// through a cv::detail::RotationWarper pointer for the interface's own members (T = 0) and directly for the overloads with a translation
// that cv::detail::PlaneWarper adds.  cv::Mat in, cv::Mat out.  Built by tests/test_gpu_cpp_plane.py against tests/cpp/opencv_stub_plane +
// tests/cpp/opencv_stub (no OpenCV in this image); same dumps as plane_demo.cpp, compared with the NumPy model.
//   usage: cv_plane_demo <w> <h> <focal> <in0.raw> <in1.raw> <out_prefix> <tx> <ty> <tz>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "imagestitch_cv_plane.hpp"

using namespace cv;
using namespace cv::detail;

static Mat rot(double yaw, double pitch, double roll) {
    double cy = cos(yaw), sy = sin(yaw), cp = cos(pitch), sp = sin(pitch), cr = cos(roll), sr = sin(roll);
    double Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy}, Rx[9] = {1, 0, 0, 0, cp, -sp, 0, sp, cp}, Rz[9] = {cr, -sr, 0, sr, cr, 0, 0, 0, 1};
    double T[9], O[9];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { T[i * 3 + j] = 0; for (int k = 0; k < 3; ++k) T[i * 3 + j] += Ry[i * 3 + k] * Rx[k * 3 + j]; }
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { O[i * 3 + j] = 0; for (int k = 0; k < 3; ++k) O[i * 3 + j] += T[i * 3 + k] * Rz[k * 3 + j]; }
    Mat R(3, 3, CV_32F);
    for (int i = 0; i < 9; ++i) R.at<float>(i / 3, i % 3) = (float)O[i];
    return R;
}

static void dump(const char* prefix, const char* name, const Mat& m) {
    char path[512];
    snprintf(path, sizeof(path), "%s_%s.raw", prefix, name);
    FILE* f = fopen(path, "wb");
    for (int y = 0; y < m.rows; ++y) fwrite(m.ptr<unsigned char>(y), 1, (size_t)m.cols * Mat::elemSize(m.type()), f);
    fclose(f);
    printf("%s %d %d %d\n", name, m.rows, m.cols, m.type());
}

int main(int argc, char** argv) {
    if (argc < 10) return 2;
    int w = atoi(argv[1]), h = atoi(argv[2]);
    float focal = (float)atof(argv[3]);
    Mat T(3, 1, CV_32F);
    for (int i = 0; i < 3; ++i) T.at<float>(i, 0) = (float)atof(argv[7 + i]);
    try {
        const int num_images = 2;
        std::vector<Mat> imgs(num_images), masks(num_images), images_warped(num_images), masks_warped(num_images);
        for (int i = 0; i < num_images; ++i) {
            imgs[i].create(h, w, CV_8UC3);
            FILE* f = fopen(argv[4 + i], "rb");
            if (!f || fread(imgs[i].data, 1, (size_t)w * h * 3, f) != (size_t)w * h * 3) return 3;
            fclose(f);
            masks[i].create(h, w, CV_8U); memset(masks[i].data, 255, (size_t)w * h);     // W:211-215
        }
        Mat K(3, 3, CV_32F);
        const float kv[9] = {focal, 0, w / 2.0f, 0, focal, h / 2.0f, 0, 0, 1};
        for (int i = 0; i < 9; ++i) K.at<float>(i / 3, i % 3) = kv[i];
        Mat R[2] = {rot(-0.2, 0.010, 0.005), rot(0.2, 0.010, 0.005)};
        isx_cv::HipPlaneWarper* plane = new isx_cv::HipPlaneWarper(focal);              // B:91 + W:222
        std::unique_ptr<RotationWarper> warper(plane);
        char name[32];
        for (int i = 0; i < num_images; ++i) {
            Point c;
            Rect q, r;
            Point2f p;
            Mat xmap, ymap;
            if (i == 0) {       // the interface's own members, through the base-class pointer (T = 0)
                c = warper->warp(imgs[i], K, R[i], 1 /* INTER_LINEAR */, 2 /* BORDER_REFLECT */, images_warped[i]);      // W:229
                warper->warp(masks[i], K, R[i], 0 /* INTER_NEAREST */, 0 /* BORDER_CONSTANT */, masks_warped[i]);      // W:232
                q = warper->warpRoi(Size(w, h), K, R[i]);
                r = warper->buildMaps(Size(w, h), K, R[i], xmap, ymap);
                p = warper->warpPoint(Point2f(w - 1.0f, 0.25f * h), K, R[i]);
            } else {            // cv::detail::PlaneWarper's overloads with T; a call without T afterwards passes zeros again (checked below)
                c = plane->warp(imgs[i], K, R[i], T, 1, 2, images_warped[i]);
                plane->warp(masks[i], K, R[i], T, 0, 0, masks_warped[i]);
                q = plane->warpRoi(Size(w, h), K, R[i], T);
                r = plane->buildMaps(Size(w, h), K, R[i], T, xmap, ymap);
                p = plane->warpPoint(Point2f(w - 1.0f, 0.25f * h), K, R[i], T);
                Rect q0 = warper->warpRoi(Size(w, h), K, R[i]);
                if (q0.x == q.x && q0.y == q.y) return 6;
            }
            if (q.x != c.x || q.y != c.y || q.width != images_warped[i].cols || q.height != images_warped[i].rows || r.x != c.x || r.y != c.y ||
                r.width != q.width - 1 || xmap.cols != q.width || ymap.rows != q.height) return 5;
            printf("corner %d %d %d\n", i, c.x, c.y);
            printf("point %d %.9g %.9g\n", i, (double)p.x, (double)p.y);
            snprintf(name, sizeof(name), "warped%d", i); dump(argv[6], name, images_warped[i]);
            snprintf(name, sizeof(name), "mask%d", i); dump(argv[6], name, masks_warped[i]);
            snprintf(name, sizeof(name), "xmap%d", i); dump(argv[6], name, xmap);
            snprintf(name, sizeof(name), "ymap%d", i); dump(argv[6], name, ymap);
        }
        // only a plane warper takes a translation
        try { float t[3] = {0.1f, 0.f, 0.f}; isx::CylindricalWarper().create(focal)->setTranslation(t); printf("no-throw\n"); return 4; }
        catch (const isx::Exception& e) { printf("throws %d\n", e.code); }
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
