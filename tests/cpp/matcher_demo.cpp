// matcher_demo.cpp — the M demo's matching stage from C++ (M:303-308) through the OpenCV-free mirror isx::FeaturesMatcher
// (include/imagestitch.hpp), two ways: match(descriptors, keypoints, img_sizes, mask) and matcher(features, pairwise_matches) on
// ImageFeatures.  Built by tests/test_gpu_match.py, which compares what it writes with the NumPy model (tests/helpers/match_np.py);
// tests/test_match_model.py checks that it compiles against include/ alone.
//   usage: matcher_demo <dir> <match_conf> then n times <rows> <width> <height>; reads <dir>/desc<k>.bin (rows x 32 u8) and
//          <dir>/kp<k>.bin (rows x 2 f32)
// writes <dir>/matches_<i>_<j>.bin (m x 3 i32) and <dir>/points_<i>_<j>.bin (m x 4 f32) per near pair, prints "pair i j m" per pair from
// match(), "entry i j m" per filled entry from operator(), and "launches L".
#include <cstdio>
#include <cstdlib>
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
        std::vector<isx::Mat> descriptors;
        std::vector<std::vector<isx::Point2f> > keypoints;
        std::vector<isx::Size> sizes;
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
            descriptors.push_back(f.descriptors); keypoints.push_back(f.keypoints); sizes.push_back(f.img_size);
        }
        isx::FeaturesMatcher matcher(conf);                                                  // M:307
        const std::vector<isx::MatchesInfo> near = matcher.match(descriptors, keypoints, sizes);
        for (size_t k = 0; k < near.size(); ++k) {
            const isx::MatchesInfo& mi = near[k];
            std::vector<int> m;
            std::vector<float> p;
            for (size_t r = 0; r < mi.matches.size(); ++r) {
                m.push_back(mi.matches[r].queryIdx); m.push_back(mi.matches[r].trainIdx); m.push_back((int)mi.matches[r].distance);
                p.push_back(mi.src_points[r].x); p.push_back(mi.src_points[r].y); p.push_back(mi.dst_points[r].x); p.push_back(mi.dst_points[r].y);
            }
            char tag[64];
            snprintf(tag, sizeof(tag), "_%d_%d", mi.src_img_idx, mi.dst_img_idx);
            if (!io(dir, "matches", tag, m.data(), m.size() * sizeof(int), true) || !io(dir, "points", tag, p.data(), p.size() * sizeof(float), true)) return 4;
            printf("pair %d %d %d\n", mi.src_img_idx, mi.dst_img_idx, (int)mi.matches.size());
        }
        printf("launches %d\n", matcher.launches());
        std::vector<isx::MatchesInfo> pairwise_matches;
        matcher(features, pairwise_matches);                                                  // M:308
        if ((int)pairwise_matches.size() != n * n) return 5;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j)
                if (pairwise_matches[(size_t)i * n + j].src_img_idx >= 0) printf("entry %d %d %d\n", i, j, (int)pairwise_matches[(size_t)i * n + j].matches.size());
        isx::FeaturesMatcher::release();
    } catch (const isx::Exception& e) {
        printf("isx error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
