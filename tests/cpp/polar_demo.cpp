// polar_demo.cpp — the reference's warp lines (W:217-233) with the last two lines of its warper list, cv::FisheyeWarper (B:94) for tile 0
// and cv::StereographicWarper (B:95) for tile 1, written against include/imagestitch.hpp: isx::FisheyeWarper, isx::StereographicWarper,
// warp / buildMaps / warpRoi / warpPoint.  Built with plain g++ and linked to libimagestitch_hip.so by tests/test_gpu_cpp_polar.py, which
// compares the files it writes with the NumPy model (tests/helpers/polar_np.py).
//   usage: polar_demo <w> <h> <focal> <in0.raw> <in1.raw> <out_prefix>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "imagestitch.hpp"

static void rot(double yaw, double pitch, double roll, float R[9]) {
    double cy = cos(yaw), sy = sin(yaw), cp = cos(pitch), sp = sin(pitch), cr = cos(roll), sr = sin(roll);
    double Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy}, Rx[9] = {1, 0, 0, 0, cp, -sp, 0, sp, cp}, Rz[9] = {cr, -sr, 0, sr, cr, 0, 0, 0, 1};
    double T[9], O[9];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { T[i * 3 + j] = 0; for (int k = 0; k < 3; ++k) T[i * 3 + j] += Ry[i * 3 + k] * Rx[k * 3 + j]; }
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { O[i * 3 + j] = 0; for (int k = 0; k < 3; ++k) O[i * 3 + j] += T[i * 3 + k] * Rz[k * 3 + j]; }
    for (int i = 0; i < 9; ++i) R[i] = (float)O[i];
}

static void dump(const char* prefix, const char* name, const isx::Mat& m) {
    char path[512];
    snprintf(path, sizeof(path), "%s_%s.raw", prefix, name);
    FILE* f = fopen(path, "wb");
    for (int y = 0; y < m.rows(); ++y) fwrite(m.ptr<unsigned char>(y), 1, (size_t)m.cols() * isx::Mat::elemSize(m.type()), f);
    fclose(f);
    printf("%s %d %d %d\n", name, m.rows(), m.cols(), m.type());
}

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    int w = atoi(argv[1]), h = atoi(argv[2]);
    float focal = (float)atof(argv[3]);
    const float T[3] = {0.125f, 0.f, 0.f};
    try {
        const int num_images = 2;
        std::vector<isx::Mat> imgs(num_images), masks(num_images), images_warped(num_images), masks_warped(num_images);
        for (int i = 0; i < num_images; ++i) {
            imgs[i].create(h, w, ISX_8UC3);
            FILE* f = fopen(argv[4 + i], "rb");
            if (!f || fread(imgs[i].ptr<unsigned char>(0), 1, (size_t)w * h * 3, f) != (size_t)w * h * 3) return 3;
            fclose(f);
            masks[i].create(h, w, ISX_8UC1); masks[i].setTo(255);                       // W:211-215
        }
        float K[9] = {focal, 0, w / 2.0f, 0, focal, h / 2.0f, 0, 0, 1};
        float R[2][9];
        rot(-0.2, 0.010, 0.005, R[0]);
        rot(0.2, 0.010, 0.005, R[1]);
        isx::FisheyeWarper fisheye_creator;                                             // B:94
        isx::StereographicWarper stereographic_creator;                                 // B:95
        char name[32];
        for (int i = 0; i < num_images; ++i) {
            const isx::WarperCreator& warper_creator = i == 0 ? (const isx::WarperCreator&)fisheye_creator : (const isx::WarperCreator&)stereographic_creator;
            auto warper = warper_creator.create(focal);                                 // W:222
            isx::Point c = warper->warp(imgs[i], K, R[i], isx::INTER_LINEAR, isx::BORDER_REFLECT, images_warped[i]);      // W:229
            warper->warp(masks[i], K, R[i], isx::INTER_NEAREST, isx::BORDER_CONSTANT, masks_warped[i]);                 // W:232
            isx::Rect q = warper->warpRoi(isx::Size(w, h), K, R[i]);
            isx::Mat xmap, ymap;
            isx::Rect r = warper->buildMaps(isx::Size(w, h), K, R[i], xmap, ymap);
            if (q.x != c.x || q.y != c.y || q.width != images_warped[i].cols() || q.height != images_warped[i].rows() || r.x != c.x || r.y != c.y ||
                r.width != q.width - 1 || xmap.cols() != q.width || ymap.rows() != q.height) return 5;
            printf("corner %d %d %d\n", i, c.x, c.y);
            isx::Point2f p = warper->warpPoint(isx::Point2f(w - 1.0f, 0.25f * h), K, R[i]);
            printf("point %d %.9g %.9g\n", i, (double)p.x, (double)p.y);
            snprintf(name, sizeof(name), "warped%d", i); dump(argv[6], name, images_warped[i]);
            snprintf(name, sizeof(name), "mask%d", i); dump(argv[6], name, masks_warped[i]);
            snprintf(name, sizeof(name), "xmap%d", i); dump(argv[6], name, xmap);
            snprintf(name, sizeof(name), "ymap%d", i); dump(argv[6], name, ymap);
        }
        // only a plane warper takes a translation
        try { isx::FisheyeWarper().create(focal)->setTranslation(T); printf("no-throw\n"); return 4; }
        catch (const isx::Exception& e) { printf("throws %d\n", e.code); }
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
