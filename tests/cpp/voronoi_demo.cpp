// voronoi_demo.cpp — the S demo's seam stage from C++ (S:1180, S:1192), two ways: the OpenCV-free mirror isx::VoronoiSeamFinder
// (include/imagestitch.hpp) on host isx::Mats, through both of its find() forms, and include/imagestitch_cv_seam.hpp's HipVoronoiSeamFinder
// used through a cv::detail::SeamFinder pointer on vector<UMat> tiles.  The finder never reads pixels, so the images only carry their sizes.
// Built by tests/test_gpu_voronoi_seam.py against tests/cpp/opencv_stub, which compares the masks with its model.
//   usage: voronoi_demo <dir> then n times <x> <y> <w> <h>; reads <dir>/mask<k>.bin (h x w u8)
// writes <dir>/mirror<k>.bin, <dir>/sizes<k>.bin and <dir>/adapter<k>.bin, prints "<leg> k <sum of mask bytes>" per leg and tile.
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

static void report(const char* dir, const char* leg, int k, const unsigned char* p, int rows, int cols, size_t step) {
    std::vector<unsigned char> dense((size_t)rows * cols);
    long long s = 0;
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) { dense[(size_t)y * cols + x] = p[(size_t)y * step + x]; s += p[(size_t)y * step + x]; }
    io(dir, leg, k, dense.data(), dense.size(), true);
    printf("%s %d %lld\n", leg, k, s);
}

int main(int argc, char** argv) {
    if (argc < 2 || (argc - 2) % 4 != 0) return 2;
    const char* dir = argv[1];
    const int n = (argc - 2) / 4;
    std::vector<int> xs(n), ys(n), ws(n), hs(n);
    std::vector<std::vector<unsigned char>> msk(n);
    for (int k = 0; k < n; ++k) {
        xs[k] = atoi(argv[2 + 4 * k]); ys[k] = atoi(argv[3 + 4 * k]); ws[k] = atoi(argv[4 + 4 * k]); hs[k] = atoi(argv[5 + 4 * k]);
        msk[k].resize((size_t)ws[k] * hs[k]);
        if (!io(dir, "mask", k, msk[k].data(), msk[k].size(), false)) return 3;
    }
    try {
        // the mirror on host isx::Mats: find(src, corners, masks) first, find(sizes, corners, masks) second
        for (int form = 0; form < 2; ++form) {
            std::vector<isx::Mat> src, masks;
            std::vector<isx::Size> sizes;
            std::vector<isx::Point> corners;
            for (int k = 0; k < n; ++k) {
                isx::Mat f(hs[k], ws[k], ISX_32FC3), m(hs[k], ws[k], ISX_8UC1);
                for (int y = 0; y < hs[k]; ++y)
                    for (int x = 0; x < ws[k]; ++x) m.ptr<unsigned char>(y)[x] = msk[k][(size_t)y * ws[k] + x];
                src.push_back(f); masks.push_back(m); sizes.push_back(isx::Size(ws[k], hs[k])); corners.push_back(isx::Point(xs[k], ys[k]));
            }
            isx::VoronoiSeamFinder finder;
            if (form == 0) finder.find(src, corners, masks);
            else finder.find(sizes, corners, masks);
            for (int k = 0; k < n; ++k) report(dir, form == 0 ? "mirror" : "sizes", k, masks[k].ptr<unsigned char>(0), hs[k], ws[k], masks[k].c()->step);
        }
        isx::VoronoiSeamFinder::release();

        // the adapter, through cv::detail::SeamFinder on UMats (S:1180, S:1192)
        std::vector<cv::UMat> images_warped_f(n), masks_seam(n);
        std::vector<cv::Point> cvc;
        for (int k = 0; k < n; ++k) {
            images_warped_f[k].create(hs[k], ws[k], CV_MAKETYPE(CV_32F, 3));
            masks_seam[k].create(hs[k], ws[k], CV_8U);
            cv::Mat m = masks_seam[k].getMat(cv::ACCESS_WRITE);
            for (int y = 0; y < hs[k]; ++y)
                for (int x = 0; x < ws[k]; ++x) m.ptr<unsigned char>(y)[x] = msk[k][(size_t)y * ws[k] + x];
            cvc.push_back(cv::Point(xs[k], ys[k]));
        }
        cv::Ptr<cv::detail::SeamFinder> seam_finder = std::make_shared<isx_cv::HipVoronoiSeamFinder>();
        seam_finder->find(images_warped_f, cvc, masks_seam);
        for (int k = 0; k < n; ++k) {
            cv::Mat m = masks_seam[k].getMat(cv::ACCESS_READ);
            report(dir, "adapter", k, m.data, m.rows, m.cols, m.step);
        }
    } catch (const isx::Exception& e) {
        printf("isx error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
