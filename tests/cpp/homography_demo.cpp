// homography_demo.cpp — BestOf2NearestMatcher1 matcher(false, conf, 6, 6); matcher(features, pairwise_matches) (R:781-782, R:830-911 of the
// reference's 计算单应性矩阵 demo) from C++ through the OpenCV-free mirror isx::BestOf2NearestMatcher (include/imagestitch.hpp).  Built by
// tests/test_gpu_cpp_homography.py, which compares what it writes with the NumPy models (tests/helpers/match_np.py, homography_np.py).
//   usage: homography_demo <dir> <match_conf> then n times <rows> <width> <height>; reads <dir>/desc<k>.bin (rows x 32 u8) and
//          <dir>/kp<k>.bin (rows x 2 f32)
// writes per near pair <dir>/H_<i>_<j>.bin (9 f64, or empty), <dir>/mask_<i>_<j>.bin (u8 per match) and prints
// "pair i j matches num_inliers status confidence-bits", then "launches L".
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
    if (argc < 3 || (argc - 3) % 3 != 0) return 2;
    const char* dir = argv[1];
    const float conf = (float)atof(argv[2]);
    const int n = (argc - 3) / 3;
    try {
        std::vector<isx::ImageFeatures> features(n);
        for (int k = 0; k < n; ++k) {
            const int rows = atoi(argv[3 + 3 * k]);
            char tag[32];
            snprintf(tag, sizeof(tag), "%d", k);
            isx::ImageFeatures& f = features[k];
            f.img_idx = k;
            f.img_size = isx::Size(atoi(argv[4 + 3 * k]), atoi(argv[5 + 3 * k]));
            f.descriptors.create(rows, 32, ISX_8UC1);
            f.keypoints.resize(rows);
            if (!io(dir, "desc", tag, f.descriptors.ptr<unsigned char>(0), (size_t)rows * 32, false)) return 3;
            if (!io(dir, "kp", tag, f.keypoints.data(), (size_t)rows * sizeof(isx::Point2f), false)) return 3;
        }
        isx::BestOf2NearestMatcher matcher(conf, 6, 6);                                       // R:781
        std::vector<isx::MatchesInfo> pairwise_matches;
        matcher(features, pairwise_matches);
        if ((int)pairwise_matches.size() != n * n) return 5;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                isx::MatchesInfo& mi = pairwise_matches[(size_t)i * n + j];
                if (mi.src_img_idx < 0) continue;
                char tag[64];
                snprintf(tag, sizeof(tag), "_%d_%d", i, j);
                if (!io(dir, "H", tag, mi.H.data(), mi.H.size() * sizeof(double), true)) return 4;
                if (!io(dir, "mask", tag, mi.inliers_mask.data(), mi.inliers_mask.size(), true)) return 4;
                unsigned long long bits = 0;
                memcpy(&bits, &mi.confidence, sizeof(bits));
                printf("pair %d %d %d %d %d %llu\n", i, j, (int)mi.matches.size(), mi.num_inliers, mi.status, bits);
            }
        printf("launches %d\n", matcher.homographyLaunches());
        isx::FeaturesMatcher plain(conf);                                                     // the base class leaves the new fields empty
        const std::vector<isx::MatchesInfo> near = plain.match(std::vector<isx::Mat>(1, features[0].descriptors));
        isx::MatchesInfo none;
        if (!near.empty() || !none.H.empty() || !none.inliers_mask.empty() || none.num_inliers != 0 || none.confidence != 0) return 6;
        isx::BestOf2NearestMatcher::release();
    } catch (const isx::Exception& e) {
        printf("isx error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
