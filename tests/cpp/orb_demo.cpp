// orb_demo.cpp — the first lines of every main of the reference (F = its 特征点检测 demo, F:1023-1040): OrbFeaturesFinder finder; finder(img,
// features) on two images, written against include/imagestitch.hpp, then the matcher on what it found.  Built with plain g++ and linked to
// libimagestitch_hip.so by tests/test_gpu_cpp_orb.py, which compares the files it writes with the NumPy model (tests/helpers/orb_np.py).
//   usage: orb_demo <w> <h> <channels> <image0.raw> <image1.raw> <out_prefix>
#include <cstdio>
#include <cstdlib>

#include "imagestitch.hpp"

static bool load(const char* path, isx::Mat& m) {
    FILE* f = fopen(path, "rb");
    const size_t n = (size_t)m.rows() * m.cols() * isx::Mat::elemSize(m.type());
    const bool ok = f && fread(m.ptr<unsigned char>(0), 1, n, f) == n;
    if (f) fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    try {
        const int w = atoi(argv[1]), h = atoi(argv[2]), type = atoi(argv[3]) == 3 ? ISX_8UC3 : ISX_8UC1;
        isx::OrbFeaturesFinder finder;                                  // Size(3, 1), 1500, 1.3f, 5
        std::vector<isx::ImageFeatures> features(2);
        for (int i = 0; i < 2; ++i) {
            isx::Mat img(h, w, type);
            if (!load(argv[4 + i], img)) return 3;
            std::vector<isx::KeyPoint> full;
            finder.find(img, features[i], &full);
            features[i].img_idx = i;
            char path[512];
            snprintf(path, sizeof(path), "%s_%d.raw", argv[6], i);
            FILE* f = fopen(path, "wb");
            for (size_t r = 0; r < full.size(); ++r) {
                const float row[6] = {full[r].pt.x, full[r].pt.y, full[r].size, full[r].angle, full[r].response, (float)full[r].octave};
                fwrite(row, sizeof(float), 6, f);
                fwrite(features[i].descriptors.ptr<unsigned char>((int)r), 1, 32, f);
            }
            fclose(f);
            printf("image %d keypoints %zu status %d size %d %d\n", i, full.size(), finder.status(), features[i].img_size.width, features[i].img_size.height);
        }
        isx::FeaturesMatcher matcher(0.3f);
        std::vector<isx::MatchesInfo> pairwise;
        matcher(features, pairwise);
        printf("matches %zu\n", pairwise[1].matches.size());
        isx::Mat bad(512, 2, ISX_32SC1);
        bad.setTo(0);
        bad.ptr<int>(7)[1] = -16;
        finder.setPattern(bad);
        isx::Mat img(h, w, type);
        if (!load(argv[4], img)) return 3;
        try { finder(img, features[0]); printf("no-throw\n"); return 4; }      // a point outside the patch
        catch (const isx::Exception& e) { printf("throws %d\n", e.code); }
        try { isx::OrbFeaturesFinder f(isx::Size(3, 1), 1500, 1.3f, 9); printf("no-throw\n"); return 4; }      // nlevels past ISX_ORB_MAX_LEVELS
        catch (const isx::Exception& e) { printf("throws %d\n", e.code); }
        isx::OrbFeaturesFinder::release();
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
