// blocks_gain_demo.cpp — block-wise exposure compensation from C++ (W:238-244), two ways: the OpenCV-free mirror isx::BlocksGainCompensator
// (include/imagestitch.hpp) on host isx::Mats, and include/imagestitch_cv_exposure.hpp's HipBlocksGainCompensator used through a
// cv::detail::ExposureCompensator pointer on the reference's vector<UMat> tiles (W:206-207), fed with the public three-argument feed
// (W:240).  Built by tests/test_gpu_blocks_gain.py against tests/cpp/opencv_stub, which compares the printed gains and the applied tiles
// with its model.
//   usage: blocks_gain_demo <dir> <n> then n times <x> <y> <w> <h>; reads <dir>/img<k>.raw (h x w x 3 u8) and <dir>/mask<k>.raw (h x w u8)
// prints  "mirror g0 g1 ..."  and  "adapter g0 g1 ..."  (one gain per block, C99 hex floats), writes what apply() made of tile k to
// <dir>/mirror<k>.raw and <dir>/adapter<k>.raw, and prints "throws 3" for an apply before any feed and "throws 7" for a mask of the wrong size.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "imagestitch_cv_exposure.hpp"

static bool read_raw(const char* dir, const char* name, int k, void* dst, size_t bytes) {
    char path[512];
    snprintf(path, sizeof(path), "%s/%s%d.raw", dir, name, k);
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const bool ok = fread(dst, 1, bytes, f) == bytes;
    fclose(f);
    return ok;
}

static bool write_raw(const char* dir, const char* name, int k, const void* src, size_t bytes) {
    char path[512];
    snprintf(path, sizeof(path), "%s/%s%d.raw", dir, name, k);
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(src, 1, bytes, f) == bytes;
    fclose(f);
    return ok;
}

static void print_gains(const char* leg, const std::vector<double>& g) {
    printf("%s", leg);
    for (double v : g) printf(" %a", v);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const char* dir = argv[1];
    const int n = atoi(argv[2]);
    if (argc < 3 + 4 * n) return 2;
    std::vector<isx::Point> corners;
    std::vector<isx::Mat> imgs, masks;
    for (int k = 0; k < n; ++k) {
        const int x = atoi(argv[3 + 4 * k]), y = atoi(argv[4 + 4 * k]), w = atoi(argv[5 + 4 * k]), h = atoi(argv[6 + 4 * k]);
        corners.push_back(isx::Point(x, y));
        imgs.push_back(isx::Mat(h, w, ISX_8UC3));
        masks.push_back(isx::Mat(h, w, ISX_8UC1));
        if (!read_raw(dir, "img", k, imgs[k].ptr<unsigned char>(0), (size_t)h * w * 3) ||
            !read_raw(dir, "mask", k, masks[k].ptr<unsigned char>(0), (size_t)h * w)) return 3;
    }

    // 1. the mirror: apply before feed, feed, gains, apply on a copy of every tile
    isx::BlocksGainCompensator mirror;
    try {
        isx::Mat t(imgs[0].rows(), imgs[0].cols(), ISX_8UC3);
        t.setTo(0);
        mirror.apply(0, corners[0], t, masks[0]);
    } catch (const isx::Exception& e) {
        printf("throws %d\n", e.code);
    }
    mirror.feed(corners, imgs, masks);
    print_gains("mirror", mirror.gains());
    for (int k = 0; k < n; ++k) {
        const size_t bytes = (size_t)imgs[k].rows() * imgs[k].cols() * 3;
        isx::Mat t(imgs[k].rows(), imgs[k].cols(), ISX_8UC3);
        std::memcpy(t.ptr<unsigned char>(0), imgs[k].ptr<unsigned char>(0), bytes);
        mirror.apply(k, corners[k], t, masks[k]);
        if (!write_raw(dir, "mirror", k, t.ptr<unsigned char>(0), bytes)) return 4;
        const isx::Mat map = mirror.gainMap(k);
        if (map.type() != ISX_32FC1 || map.empty()) return 5;
    }

    // 2. the adapter through the base class, on UMats
    std::vector<cv::Point> cc;
    std::vector<cv::UMat> ui(n), um(n);
    for (int k = 0; k < n; ++k) {
        cc.push_back(cv::Point(corners[k].x, corners[k].y));
        ui[k].create(imgs[k].rows(), imgs[k].cols(), CV_8UC3);
        um[k].create(masks[k].rows(), masks[k].cols(), 0);
        cv::Mat a = ui[k].getMat(cv::ACCESS_WRITE), b = um[k].getMat(cv::ACCESS_WRITE);
        for (int y = 0; y < a.rows; ++y) {
            std::memcpy(a.ptr<unsigned char>(y), imgs[k].ptr<unsigned char>(y), (size_t)a.cols * 3);
            std::memcpy(b.ptr<unsigned char>(y), masks[k].ptr<unsigned char>(y), (size_t)b.cols);
        }
    }
    std::shared_ptr<cv::detail::ExposureCompensator> compensator = std::make_shared<isx_cv::HipBlocksGainCompensator>();
    compensator->feed(cc, ui, um);                                                       // W:240
    print_gains("adapter", static_cast<isx_cv::HipBlocksGainCompensator*>(compensator.get())->gains());
    for (int k = 0; k < n; ++k) {                                                        // W:241-244
        cv::Mat t(imgs[k].rows(), imgs[k].cols(), CV_8UC3);
        for (int y = 0; y < t.rows; ++y) std::memcpy(t.ptr<unsigned char>(y), imgs[k].ptr<unsigned char>(y), (size_t)t.cols * 3);
        cv::Mat m = um[k].getMat(cv::ACCESS_READ);
        compensator->apply(k, cc[k], t, m);
        std::vector<unsigned char> dense((size_t)t.rows * t.cols * 3);
        for (int y = 0; y < t.rows; ++y) std::memcpy(&dense[(size_t)y * t.cols * 3], t.ptr<unsigned char>(y), (size_t)t.cols * 3);
        if (!write_raw(dir, "adapter", k, dense.data(), dense.size())) return 4;
    }

    // 3. a mask that is not its image's size
    try {
        std::vector<isx::Mat> bad = masks;
        bad[0] = isx::Mat(masks[0].rows(), masks[0].cols() - 1, ISX_8UC1);
        mirror.feed(corners, imgs, bad);
    } catch (const isx::Exception& e) {
        printf("throws %d\n", e.code);
    }
    return 0;
}
