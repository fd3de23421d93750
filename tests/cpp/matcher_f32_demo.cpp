// matcher_f32_demo.cpp — the matching stage on CV_32F descriptors from C++ through the OpenCV-free mirror (include/imagestitch.hpp):
// isx::BestOf2NearestMatcher picks isx_match_features_f32 by the mats' type, DMatch::distance is the float32 L2 distance, and the
// homography stage runs behind it unchanged.  Built by tests/test_gpu_cpp_match_f32.py, which compares what it writes with the NumPy models
// (tests/helpers/match_f32_np.py, homography_np.py).
//   usage: matcher_f32_demo <dir> <match_conf> <cols> then n times <rows> <width> <height>; reads <dir>/desc<k>.bin (rows x cols f32) and
//          <dir>/kp<k>.bin (rows x 2 f32)
// writes per near pair <dir>/matches_<i>_<j>.bin (m x (i32, i32, f32)), <dir>/H_<i>_<j>.bin (9 f64, or empty) and prints
// "pair i j matches num_inliers status confidence-bits", then "launches L" (the matcher's), then "mixed C" - the code a call with one
// CV_8U and one CV_32F mat throws.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "imagestitch.hpp"

static bool io(const char* dir, const char* name, const char* tag, void* p, size_t bytes, bool write) {
    char path[512];
    snprintf(path, sizeof(path), "%s/%s%s.bin", dir, name, tag);
    FILE* f = fopen(path, write ? "wb" : "rb");
    if (!f) return false;
    const bool ok = bytes == 0 || (write ? fwrite(p, 1, bytes, f) : fread(p, 1, bytes, f)) == bytes;
    fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 4 || (argc - 4) % 3 != 0) return 2;
    const char* dir = argv[1];
    const float conf = (float)atof(argv[2]);
    const int cols = atoi(argv[3]), n = (argc - 4) / 3;
    try {
        std::vector<isx::ImageFeatures> features(n);
        for (int k = 0; k < n; ++k) {
            const int rows = atoi(argv[4 + 3 * k]);
            char tag[32];
            snprintf(tag, sizeof(tag), "%d", k);
            isx::ImageFeatures& f = features[k];
            f.img_idx = k;
            f.img_size = isx::Size(atoi(argv[5 + 3 * k]), atoi(argv[6 + 3 * k]));
            if (rows > 0) f.descriptors.create(rows, cols, ISX_32FC1);      // (an image without features keeps its default Mat)
            f.keypoints.resize(rows);
            if (rows > 0 && !io(dir, "desc", tag, f.descriptors.ptr<float>(0), (size_t)rows * cols * sizeof(float), false)) return 3;
            if (!io(dir, "kp", tag, f.keypoints.data(), (size_t)rows * sizeof(isx::Point2f), false)) return 3;
        }
        isx::BestOf2NearestMatcher matcher(conf, 6, 6);
        std::vector<isx::MatchesInfo> pairwise_matches;
        matcher(features, pairwise_matches);
        if ((int)pairwise_matches.size() != n * n) return 5;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                isx::MatchesInfo& mi = pairwise_matches[(size_t)i * n + j];
                if (mi.src_img_idx < 0) continue;
                char tag[64];
                snprintf(tag, sizeof(tag), "_%d_%d", i, j);
                std::vector<int> m;
                for (size_t r = 0; r < mi.matches.size(); ++r) {
                    int bits = 0;
                    memcpy(&bits, &mi.matches[r].distance, sizeof(bits));
                    m.push_back(mi.matches[r].queryIdx); m.push_back(mi.matches[r].trainIdx); m.push_back(bits);
                }
                if (!io(dir, "matches", tag, m.data(), m.size() * sizeof(int), true)) return 4;
                if (!io(dir, "H", tag, mi.H.data(), mi.H.size() * sizeof(double), true)) return 4;
                unsigned long long bits = 0;
                memcpy(&bits, &mi.confidence, sizeof(bits));
                printf("pair %d %d %d %d %d %llu\n", i, j, (int)mi.matches.size(), mi.num_inliers, mi.status, bits);
            }
        printf("launches %d\n", matcher.launches());
        int mixed = 0;
        try {
            std::vector<isx::Mat> two(2);
            two[0].create(4, 32, ISX_8UC1); two[1].create(4, cols, ISX_32FC1);
            isx::FeaturesMatcher(conf).match(two);
        } catch (const isx::Exception& e) {
            mixed = e.code;
        }
        printf("mixed %d\n", mixed);
        isx::BestOf2NearestMatcher::release();
    } catch (const isx::Exception& e) {
        printf("isx error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
