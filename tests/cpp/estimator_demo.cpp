// estimator_demo.cpp — HomographyBasedEstimator1 estimator; estimator(features, pairwise_matches, cameras) (C:313-321 of the reference's
// 恢复相机内参数 demo) from C++ through the OpenCV-free mirror isx::HomographyBasedEstimator (include/imagestitch.hpp).  Built by
// tests/test_gpu_cpp_estimator.py, which compares what it writes with the NumPy model (tests/helpers/estimator_np.py) by bits.
//   usage: estimator_demo <dir> <given 0|1> <num_pairs> then n times <width> <height>; reads <dir>/pairs.bin (num_pairs x 4 i32: from, to,
//          status, num_inliers), <dir>/H.bin (num_pairs x 9 f64) and, with given = 1, <dir>/focals.bin (n x 4 f64)
// writes <dir>/cameras.bin (n x 16 f64: focal, aspect, ppx, ppy, R, t), <dir>/kr32.bin (n x 18 f32), <dir>/tree.bin (n x 2 i32) and prints
// "rig" and the 8 rig stats, then "launches L".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "imagestitch.hpp"

static bool io(const char* dir, const char* name, void* p, size_t bytes, bool write) {
    char path[512];
    snprintf(path, sizeof(path), "%s/%s.bin", dir, name);
    FILE* f = fopen(path, write ? "wb" : "rb");
    if (!f) return false;
    const bool ok = bytes == 0 || (write ? fwrite(p, 1, bytes, f) : fread(p, 1, bytes, f)) == bytes;
    fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 4 || (argc - 4) % 2 != 0) return 2;
    const char* dir = argv[1];
    const bool given = atoi(argv[2]) != 0;
    const int np = atoi(argv[3]), n = (argc - 4) / 2;
    try {
        std::vector<isx::ImageFeatures> features(n);
        for (int k = 0; k < n; ++k) {
            features[k].img_idx = k;
            features[k].img_size = isx::Size(atoi(argv[4 + 2 * k]), atoi(argv[5 + 2 * k]));
        }
        std::vector<int> prs((size_t)4 * np);
        std::vector<double> H((size_t)9 * np), fin((size_t)4 * n);
        if (!io(dir, "pairs", prs.data(), prs.size() * sizeof(int), false) || !io(dir, "H", H.data(), H.size() * sizeof(double), false)) return 3;
        if (given && !io(dir, "focals", fin.data(), fin.size() * sizeof(double), false)) return 3;
        std::vector<isx::MatchesInfo> pairwise_matches((size_t)n * n);
        for (int k = 0; k < np; ++k) {
            isx::MatchesInfo& mi = pairwise_matches[(size_t)prs[4 * k] * n + prs[4 * k + 1]];
            mi.src_img_idx = prs[4 * k]; mi.dst_img_idx = prs[4 * k + 1];
            mi.status = prs[4 * k + 2]; mi.num_inliers = prs[4 * k + 3];
            if (mi.status & ISX_HOMOGRAPHY_H) mi.H.assign(H.begin() + 9 * k, H.begin() + 9 * k + 9);
        }
        isx::HomographyBasedEstimator estimator(given);                                       // C:313
        std::vector<isx::CameraParams> cameras(n);                                            // C:314
        for (int k = 0; given && k < n; ++k) { cameras[k].focal = fin[4 * k]; cameras[k].aspect = fin[4 * k + 1]; cameras[k].ppx = fin[4 * k + 2]; cameras[k].ppy = fin[4 * k + 3]; }
        if (!estimator(features, pairwise_matches, cameras) || (int)cameras.size() != n) return 5;      // C:321
        std::vector<double> cams;
        std::vector<float> kr;
        std::vector<int> tree;
        for (int k = 0; k < n; ++k) {
            const isx::CameraParams& c = cameras[k];
            const double head[4] = {c.focal, c.aspect, c.ppx, c.ppy};
            cams.insert(cams.end(), head, head + 4); cams.insert(cams.end(), c.R, c.R + 9); cams.insert(cams.end(), c.t, c.t + 3);
            kr.insert(kr.end(), c.K32, c.K32 + 9); kr.insert(kr.end(), c.R32, c.R32 + 9);
            tree.push_back(c.parent); tree.push_back(c.depth);
            double k64[9];
            c.K(k64);
            for (int e = 0; e < 9; ++e)
                if ((float)k64[e] != c.K32[e]) return 6;                                      // C:386
        }
        if (!io(dir, "cameras", cams.data(), cams.size() * sizeof(double), true) || !io(dir, "kr32", kr.data(), kr.size() * sizeof(float), true) ||
            !io(dir, "tree", tree.data(), tree.size() * sizeof(int), true))
            return 4;
        printf("rig");
        for (int e = 0; e < 8; ++e) printf(" %d", estimator.rigStats()[e]);
        printf("\nlaunches %d\n", estimator.launches());
        isx::HomographyBasedEstimator::release();
    } catch (const isx::Exception& e) {
        printf("isx error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
