// bundle_reproj_demo.cpp — adjuster = new detail::BundleAdjusterReproj(); adjuster->setConfThresh(1); (*adjuster)(features,
// pairwise_matches, cameras); waveCorrect(rmats, kind) (W:190-198 of the reference's cylindrical-projection demo, commented out there) from
// C++ through the OpenCV-free mirrors isx::BundleAdjusterReproj and isx::waveCorrect (include/imagestitch.hpp).  Built by
// tests/test_gpu_cpp_bundle_reproj.py, which compares what it writes with the Python path by bits.
//   usage: bundle_reproj_demo <dir> <conf_thresh> <max_iter> <num_pairs> <refine_flags> <wave_kind> then n times <width> <height> <keypoints>; reads <dir>/keypoints.bin (all
//          images' keypoints, x y f32), <dir>/pairs.bin (num_pairs x 4 i32: from, to, status, matches), <dir>/conf.bin (num_pairs f64),
//          <dir>/matches.bin (all pairs' matches x 3 i32: queryIdx, trainIdx, distance), <dir>/masks.bin (one byte a match),
//          <dir>/cameras_in.bin (n x 16 f64) and <dir>/est.bin (8 i32: the estimator's rig stats)
// writes <dir>/cameras.bin (n x 16 f64), <dir>/kr32.bin (n x 18 f32), <dir>/err.bin (2 f64), then the wave-corrected <dir>/wave_cameras.bin
// and <dir>/wave_kr32.bin, and prints "rig" and the 8 rig stats, "ok 0|1", "launches L", "wave 0|1".
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
    if (argc < 7 || (argc - 7) % 3 != 0) return 2;
    const char* dir = argv[1];
    const double conf_thresh = atof(argv[2]);
    const int max_iter = atoi(argv[3]), np = atoi(argv[4]), refine_flags = atoi(argv[5]), wave_kind = atoi(argv[6]), n = (argc - 7) / 3;
    argv += 2;
    try {
        std::vector<isx::ImageFeatures> features(n);
        size_t total_kp = 0;
        for (int k = 0; k < n; ++k) {
            features[k].img_idx = k;
            features[k].img_size = isx::Size(atoi(argv[5 + 3 * k]), atoi(argv[6 + 3 * k]));
            features[k].keypoints.resize((size_t)atoi(argv[7 + 3 * k]));
            total_kp += features[k].keypoints.size();
        }
        std::vector<float> kp(2 * total_kp);
        std::vector<int> prs((size_t)4 * np), est(8);
        std::vector<double> conf((size_t)np), cin((size_t)16 * n);
        if (!io(dir, "keypoints", kp.data(), kp.size() * sizeof(float), false) || !io(dir, "pairs", prs.data(), prs.size() * sizeof(int), false) ||
            !io(dir, "conf", conf.data(), conf.size() * sizeof(double), false) || !io(dir, "cameras_in", cin.data(), cin.size() * sizeof(double), false) ||
            !io(dir, "est", est.data(), est.size() * sizeof(int), false))
            return 3;
        size_t at = 0, total_m = 0;
        for (int k = 0; k < n; ++k)
            for (size_t r = 0; r < features[k].keypoints.size(); ++r, ++at) features[k].keypoints[r] = isx::Point2f(kp[2 * at], kp[2 * at + 1]);
        for (int k = 0; k < np; ++k) total_m += (size_t)prs[4 * k + 3];
        std::vector<int> ms(3 * total_m);
        std::vector<unsigned char> mk(total_m);
        if (!io(dir, "matches", ms.data(), ms.size() * sizeof(int), false) || !io(dir, "masks", mk.data(), mk.size(), false)) return 3;
        std::vector<isx::MatchesInfo> pairwise_matches((size_t)n * n);
        at = 0;
        for (int k = 0; k < np; ++k) {
            isx::MatchesInfo& mi = pairwise_matches[(size_t)prs[4 * k] * n + prs[4 * k + 1]];
            mi.src_img_idx = prs[4 * k]; mi.dst_img_idx = prs[4 * k + 1];
            mi.status = prs[4 * k + 2]; mi.confidence = conf[k];
            for (int r = 0; r < prs[4 * k + 3]; ++r, ++at) {
                isx::DMatch dm; dm.queryIdx = ms[3 * at]; dm.trainIdx = ms[3 * at + 1]; dm.distance = (float)ms[3 * at + 2];
                mi.matches.push_back(dm);
                mi.inliers_mask.push_back(mk[at]);
                mi.num_inliers += mk[at] != 0;
            }
        }
        std::vector<isx::CameraParams> cameras(n);
        for (int k = 0; k < n; ++k) {
            isx::CameraParams& c = cameras[k];
            const double* s = &cin[(size_t)16 * k];
            c.focal = s[0]; c.aspect = s[1]; c.ppx = s[2]; c.ppy = s[3];
            memcpy(c.R, s + 4, sizeof(c.R)); memcpy(c.t, s + 13, sizeof(c.t));
        }
        isx::BundleAdjusterReproj adjuster;                                                   // W:190
        unsigned char mask[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};                                  // Mat_<uchar> refine_mask of stitching_detailed
        mask[0] = (refine_flags & 1) != 0; mask[1] = (refine_flags & 2) != 0; mask[2] = (refine_flags & 4) != 0;
        mask[4] = (refine_flags & 8) != 0; mask[5] = (refine_flags & 16) != 0;
        adjuster.setRefinementMask(mask);
        adjuster.setConfThresh(conf_thresh);                                                  // W:191
        adjuster.setTermCriteria(max_iter, 2.220446049250313e-16);
        adjuster.setEstimatorStats(est.data());
        const bool ok = adjuster(features, pairwise_matches, cameras);                        // W:194
        std::vector<double> cams;
        std::vector<float> kr;
        for (int k = 0; k < n; ++k) {
            const isx::CameraParams& c = cameras[k];
            const double head[4] = {c.focal, c.aspect, c.ppx, c.ppy};
            cams.insert(cams.end(), head, head + 4); cams.insert(cams.end(), c.R, c.R + 9); cams.insert(cams.end(), c.t, c.t + 3);
            kr.insert(kr.end(), c.K32, c.K32 + 9); kr.insert(kr.end(), c.R32, c.R32 + 9);
        }
        double err[2] = {adjuster.rigErr()[0], adjuster.rigErr()[1]};
        if (!io(dir, "cameras", cams.data(), cams.size() * sizeof(double), true) || !io(dir, "kr32", kr.data(), kr.size() * sizeof(float), true) ||
            !io(dir, "err", err, sizeof(err), true))
            return 4;
        printf("rig");
        for (int e = 0; e < 8; ++e) printf(" %d", adjuster.rigStats()[e]);
        printf("\nok %d\nlaunches %d\n", ok ? 1 : 0, adjuster.launches());
        const bool waved = isx::waveCorrect(cameras, wave_kind ? isx::WAVE_CORRECT_VERT : isx::WAVE_CORRECT_HORIZ);      // W:198
        cams.clear(); kr.clear();
        for (int k = 0; k < n; ++k) {
            const isx::CameraParams& c = cameras[k];
            const double head[4] = {c.focal, c.aspect, c.ppx, c.ppy};
            cams.insert(cams.end(), head, head + 4); cams.insert(cams.end(), c.R, c.R + 9); cams.insert(cams.end(), c.t, c.t + 3);
            kr.insert(kr.end(), c.K32, c.K32 + 9); kr.insert(kr.end(), c.R32, c.R32 + 9);
        }
        if (!io(dir, "wave_cameras", cams.data(), cams.size() * sizeof(double), true) || !io(dir, "wave_kr32", kr.data(), kr.size() * sizeof(float), true)) return 4;
        printf("wave %d\n", waved ? 1 : 0);
        isx::BundleAdjusterReproj::release();
    } catch (const isx::Exception& e) {
        printf("isx error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
