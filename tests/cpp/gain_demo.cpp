// gain_demo.cpp — exposure compensation from C++ (W:238-244), two ways: the OpenCV-free mirror isx::GainCompensator
// (include/imagestitch.hpp) on host isx::Mats, and include/imagestitch_cv_exposure.hpp's HipGainCompensator used through a
// cv::detail::ExposureCompensator pointer on the reference's vector<UMat> tiles (W:206-207), fed with the public three-argument feed
// (W:240).  Built by tests/test_gpu_gain_feed.py against tests/cpp/opencv_stub, which compares the printed gains with its model.
//   usage: gain_demo <dir> <n> then n times <x> <y> <w> <h>; reads <dir>/img<k>.raw (h x w x 3 u8) and <dir>/mask<k>.raw (h x w u8)
// prints  "mirror g0 g1 ..."  and  "adapter g0 g1 ..."  (C99 hex floats), "apply OK" when apply() gave saturate_cast<uchar>(cvRound(v * g))
// for every byte, and "throws 7" for a mask of the wrong size.
#include <cmath>
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

    // 1. the mirror
    isx::GainCompensator mirror;
    mirror.feed(corners, imgs, masks);
    const std::vector<double> g = mirror.gains();
    print_gains("mirror", g);

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
    std::shared_ptr<cv::detail::ExposureCompensator> compensator = std::make_shared<isx_cv::HipGainCompensator>();
    compensator->feed(cc, ui, um);                                                       // W:240
    print_gains("adapter", static_cast<isx_cv::HipGainCompensator*>(compensator.get())->gains());

    // 3. apply (W:241-244) on a copy of every tile, against the arithmetic of multiply(image, gain, image)
    bool ok = true;
    for (int k = 0; k < n; ++k) {
        cv::Mat t(imgs[k].rows(), imgs[k].cols(), CV_8UC3);
        for (int y = 0; y < t.rows; ++y) std::memcpy(t.ptr<unsigned char>(y), imgs[k].ptr<unsigned char>(y), (size_t)t.cols * 3);
        cv::Mat m = um[k].getMat(cv::ACCESS_READ);
        compensator->apply(k, cc[k], t, m);
        for (int y = 0; y < t.rows && ok; ++y)
            for (int x = 0; x < t.cols * 3; ++x) {
                const long r = std::lrint((double)imgs[k].ptr<unsigned char>(y)[x] * g[k]);   // cvRound: half to even
                const unsigned char want = (unsigned char)(r < 0 ? 0 : (r > 255 ? 255 : r));
                if (t.ptr<unsigned char>(y)[x] != want) { ok = false; break; }
            }
    }
    if (ok) printf("apply OK\n");

    // 4. a mask that is not its image's size
    try {
        std::vector<isx::Mat> bad = masks;
        bad[0] = isx::Mat(masks[0].rows(), masks[0].cols() - 1, ISX_8UC1);
        mirror.feed(corners, imgs, bad);
    } catch (const isx::Exception& e) {
        printf("throws %d\n", e.code);
    }
    return 0;
}
