// resize_demo.cpp — the lines OpenCV's stitching_detailed / Stitcher::composePanorama put around the seam finder (resize the sources to
// seam_megapix; at compose time dilate the small seam mask, resize it to the warped mask's size and AND the two), written against
// include/imagestitch.hpp: isx::resize and isx::dilateResizeAnd.  Built with plain g++ and linked to libimagestitch_hip.so by
// tests/test_gpu_cpp_resize.py, which compares the files it writes with the NumPy model (tests/helpers/resize_np.py).
//   usage: resize_demo <w> <h> <image.raw> <mask_w> <mask_h> <seam_mask.raw> <warped_w> <warped_h> <warped_mask.raw> <out_prefix>
#include <cstdio>
#include <cstdlib>

#include "imagestitch.hpp"

static void dump(const char* prefix, const char* name, const isx::Mat& m) {
    char path[512];
    snprintf(path, sizeof(path), "%s_%s.raw", prefix, name);
    FILE* f = fopen(path, "wb");
    for (int y = 0; y < m.rows(); ++y) fwrite(m.ptr<unsigned char>(y), 1, (size_t)m.cols() * isx::Mat::elemSize(m.type()), f);
    fclose(f);
    printf("%s %d %d %d\n", name, m.rows(), m.cols(), m.type());
}

static bool load(const char* path, isx::Mat& m) {
    FILE* f = fopen(path, "rb");
    const size_t n = (size_t)m.rows() * m.cols() * isx::Mat::elemSize(m.type());
    const bool ok = f && fread(m.ptr<unsigned char>(0), 1, n, f) == n;
    if (f) fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 11) return 2;
    try {
        isx::Mat full_img(atoi(argv[2]), atoi(argv[1]), ISX_8UC3), seam_mask(atoi(argv[5]), atoi(argv[4]), ISX_8UC1), mask_warped(atoi(argv[8]), atoi(argv[7]), ISX_8UC1);
        if (!load(argv[3], full_img) || !load(argv[6], seam_mask) || !load(argv[9], mask_warped)) return 3;
        const char* prefix = argv[10];
        // resize(full_img, img, Size(), seam_scale, seam_scale) for the seam finder: 0.5 takes the 2 x 2 area rule, 0.4 the general path
        isx::Mat half, small, nearest, img_f, small_f;
        isx::resize(full_img, half, isx::Size(), 0.5, 0.5);
        isx::resize(full_img, small, isx::Size(), 0.4, 0.4, isx::INTER_LINEAR);
        isx::resize(full_img, nearest, isx::Size(full_img.cols() + 7, full_img.rows() - 5), 0, 0, isx::INTER_NEAREST);
        isx::convertTo(full_img, img_f, ISX_32FC3);
        isx::resize(img_f, small_f, isx::Size(small.cols(), small.rows()));
        dump(prefix, "half", half); dump(prefix, "small", small); dump(prefix, "nearest", nearest); dump(prefix, "small_f", small_f);
        // dilate(masks_warped[i], dilated_mask, Mat()); resize(dilated_mask, seam_mask, mask_warped.size()); mask_warped = seam_mask & mask_warped
        isx::Mat grey, composed;
        isx::dilateResizeAnd(seam_mask, mask_warped.size(), grey);
        isx::dilateResizeAnd(seam_mask, mask_warped, composed);
        dump(prefix, "grey", grey); dump(prefix, "composed", composed);
        isx::dilateResizeAnd(seam_mask, mask_warped, mask_warped, 20, 20);          // in place, the reference's 20 x 20 element
        dump(prefix, "inplace", mask_warped);
        try { isx::resize(full_img, half, isx::Size(8, 8), 0, 0, 2); printf("no-throw\n"); return 4; }          // INTER_CUBIC
        catch (const isx::Exception& e) { printf("throws %d\n", e.code); }
        try { isx::resize(full_img, half, isx::Size(), 0.001, 0.001); printf("no-throw\n"); return 4; }         // an empty dsize
        catch (const isx::Exception& e) { printf("throws %d\n", e.code); }
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
