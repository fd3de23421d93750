// graphcut_grad_demo.cpp — GraphCutSeamFinder(COST_COLOR_GRAD), the other graph cut the W demo lists (W:258, W:261, W:264), from C++, two
// ways: the OpenCV-free mirror isx::GraphCutSeamFinder
// (include/imagestitch.hpp) on host isx::Mats, and include/imagestitch_cv_seam.hpp's HipGraphCutSeamFinder used through a
// cv::detail::SeamFinder pointer on vector<UMat> tiles.  Both take the byte tiles converted to CV_32FC3 (W:261).  Built by
// tests/test_gpu_graphcut_grad.py against tests/cpp/opencv_stub, which compares the masks with its model.
//   usage: graphcut_grad_demo <dir> then n times <x> <y> <w> <h>; reads <dir>/img<k>.bin (h x w x 3 u8) and <dir>/mask<k>.bin (h x w u8)
// writes <dir>/mirror<k>.bin and <dir>/adapter<k>.bin, prints "mirror k <sum of mask bytes>" and "adapter k <sum>" per tile.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "imagestitch_cv_seam.hpp"

static bool io(const char* dir, const char* name, int k, void* p, size_t bytes, bool write) {
    char path[512];
    snprintf(path, sizeof(path), "%s/%s%d.bin", dir, name, k);
    FILE* f = fopen(path, write ? "wb" : "rb");
    if (!f) return false;
    const bool ok = (write ? fwrite(p, 1, bytes, f) : fread(p, 1, bytes, f)) == bytes;
    fclose(f);
    return ok;
}

static long long report(const char* dir, const char* leg, int k, const unsigned char* p, int rows, int cols, size_t step) {
    std::vector<unsigned char> dense((size_t)rows * cols);
    long long s = 0;
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) { dense[(size_t)y * cols + x] = p[(size_t)y * step + x]; s += p[(size_t)y * step + x]; }
    io(dir, leg, k, dense.data(), dense.size(), true);
    printf("%s %d %lld\n", leg, k, s);
    return s;
}

int main(int argc, char** argv) {
    if (argc < 2 || (argc - 2) % 4 != 0) return 2;
    const char* dir = argv[1];
    const int n = (argc - 2) / 4;
    std::vector<int> xs(n), ys(n), ws(n), hs(n);
    std::vector<std::vector<unsigned char>> img(n), msk(n);
    for (int k = 0; k < n; ++k) {
        xs[k] = atoi(argv[2 + 4 * k]); ys[k] = atoi(argv[3 + 4 * k]); ws[k] = atoi(argv[4 + 4 * k]); hs[k] = atoi(argv[5 + 4 * k]);
        img[k].resize((size_t)ws[k] * hs[k] * 3);
        msk[k].resize((size_t)ws[k] * hs[k]);
        if (!io(dir, "img", k, img[k].data(), img[k].size(), false) || !io(dir, "mask", k, msk[k].data(), msk[k].size(), false)) return 3;
    }
    try {
        // the mirror, on host isx::Mats
        std::vector<isx::Mat> src, masks;
        std::vector<isx::Point> corners;
        for (int k = 0; k < n; ++k) {
            isx::Mat f(hs[k], ws[k], ISX_32FC3), m(hs[k], ws[k], ISX_8UC1);
            for (size_t i = 0; i < img[k].size(); ++i) ((float*)f.c()->data)[i] = (float)img[k][i];
            for (int y = 0; y < hs[k]; ++y)
                for (int x = 0; x < ws[k]; ++x) ((unsigned char*)m.c()->data)[(size_t)y * m.c()->step + x] = msk[k][(size_t)y * ws[k] + x];
            src.push_back(f); masks.push_back(m); corners.push_back(isx::Point(xs[k], ys[k]));
        }
        isx::GraphCutSeamFinder(isx::GraphCutSeamFinder::COST_COLOR_GRAD).find(src, corners, masks);
        for (int k = 0; k < n; ++k) report(dir, "mirror", k, (const unsigned char*)masks[k].c()->data, hs[k], ws[k], masks[k].c()->step);

        // the adapter, through cv::detail::SeamFinder on UMats (W:257, W:264)
        std::vector<cv::UMat> images_warped_f(n), masks_warped(n);
        std::vector<cv::Point> cvc;
        for (int k = 0; k < n; ++k) {
            images_warped_f[k].create(hs[k], ws[k], CV_MAKETYPE(CV_32F, 3));
            masks_warped[k].create(hs[k], ws[k], CV_8U);
            cv::Mat f = images_warped_f[k].getMat(cv::ACCESS_WRITE), m = masks_warped[k].getMat(cv::ACCESS_WRITE);
            for (int y = 0; y < hs[k]; ++y)
                for (int x = 0; x < ws[k]; ++x) {
                    for (int c = 0; c < 3; ++c) f.ptr<float>(y)[3 * x + c] = (float)img[k][((size_t)y * ws[k] + x) * 3 + c];
                    m.ptr<unsigned char>(y)[x] = msk[k][(size_t)y * ws[k] + x];
                }
            cvc.push_back(cv::Point(xs[k], ys[k]));
        }
        cv::Ptr<cv::detail::SeamFinder> seam_finder = std::make_shared<isx_cv::HipGraphCutSeamFinder>(cv::detail::GraphCutSeamFinderBase::COST_COLOR_GRAD);
        seam_finder->find(images_warped_f, cvc, masks_warped);
        for (int k = 0; k < n; ++k) {
            cv::Mat m = masks_warped[k].getMat(cv::ACCESS_READ);
            report(dir, "adapter", k, m.data, m.rows, m.cols, m.step);
        }
    } catch (const isx::Exception& e) {
        printf("isx error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
