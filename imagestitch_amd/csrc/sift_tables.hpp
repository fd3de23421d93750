// sift_tables.hpp — the six Gaussian kernels of SIFT at (sigma 1.6, 3 layers an octave) as float32 literals, one copy for host and device:
// kernel 0 blurs the doubled image by sig_diff = sqrt(1.6^2 - 1), kernel i = 1 .. 5 makes layer i of an octave from layer i - 1
// (sig[i] = sqrt((k^i 1.6)^2 - (k^(i-1) 1.6)^2), k = 2^(1/3)).  Each is getGaussianKernel(cvRound(8 s + 1) | 1, s): exp in double, normalised
// in double, rounded to float32 once.  tests/helpers/sift_np.py holds the same bits and regenerates them from the formula
// (tests/test_sift_model.py compares this text with it); no exp runs for the pyramid on the device, which is why other sigmas and layer
// counts are refused.  Internal.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ISX_SIFT_HD __host__ __device__
#else
#define ISX_SIFT_HD
#endif

namespace isxsi {

constexpr int SIFT_KERNELS = 6, SIFT_TAPS = 100, SIFT_MAX_HALF = 13;
// kernel k is taps sift_tap_first(k) .. sift_tap_first(k) + sift_tap_width(k) - 1
ISX_SIFT_HD inline int sift_tap_width(int k) {
    const int w[SIFT_KERNELS] = {11, 11, 13, 17, 21, 27};
    return w[k];
}
ISX_SIFT_HD inline int sift_tap_first(int k) {
    const int f[SIFT_KERNELS] = {0, 11, 22, 35, 52, 73};
    return f[k];
}
ISX_SIFT_HD inline float sift_tap(int i) {
    const float t[SIFT_TAPS] = {
        // 0: sigma 1.2489995996796799
        0x1.bbb27cp-14f, 0x1.f04b54p-10f, 0x1.2469f0p-6f, 0x1.6b036ep-4f, 0x1.dac530p-3f, 0x1.4713cep-2f, 0x1.dac530p-3f, 0x1.6b036ep-4f,
        0x1.2469f0p-6f, 0x1.f04b54p-10f, 0x1.bbb27cp-14f,
        // 1: sigma 1.2262734984654078
        0x1.4edfacp-14f, 0x1.a1407ap-10f, 0x1.0b5ddep-6f, 0x1.606d0ep-4f, 0x1.ddcdfcp-3f, 0x1.4d2364p-2f, 0x1.ddcdfcp-3f, 0x1.606d0ep-4f,
        0x1.0b5ddep-6f, 0x1.a1407ap-10f, 0x1.4edfacp-14f,
        // 2: sigma 1.5450077936447955
        0x1.1f90cap-13f, 0x1.680080p-10f, 0x1.287054p-7f, 0x1.411cd4p-5f, 0x1.c995cap-4f, 0x1.ace486p-3f, 0x1.086a76p-2f, 0x1.ace486p-3f,
        0x1.c995cap-4f, 0x1.411cd4p-5f, 0x1.287054p-7f, 0x1.680080p-10f, 0x1.1f90cap-13f,
        // 3: sigma 1.9465878414647133
        0x1.719152p-15f, 0x1.4e5a92p-12f, 0x1.d0a8dcp-10f, 0x1.eff6b8p-8f, 0x1.9695c0p-6f, 0x1.ffffbap-5f, 0x1.ef3104p-4f, 0x1.6fd80cp-3f,
        0x1.a3bafcp-3f, 0x1.6fd80cp-3f, 0x1.ef3104p-4f, 0x1.ffffbap-5f, 0x1.9695c0p-6f, 0x1.eff6b8p-8f, 0x1.d0a8dcp-10f, 0x1.4e5a92p-12f,
        0x1.719152p-15f,
        // 4: sigma 2.4525469969308156
        0x1.4ee0b6p-15f, 0x1.9634a6p-13f, 0x1.a141c6p-11f, 0x1.6af5d4p-9f, 0x1.0b5eb2p-7f, 0x1.4d9348p-6f, 0x1.606e26p-5f, 0x1.3b51b8p-4f,
        0x1.ddcf78p-4f, 0x1.3291c0p-3f, 0x1.4d246cp-3f, 0x1.3291c0p-3f, 0x1.ddcf78p-4f, 0x1.3b51b8p-4f, 0x1.606e26p-5f, 0x1.4d9348p-6f,
        0x1.0b5eb2p-7f, 0x1.6af5d4p-9f, 0x1.a141c6p-11f, 0x1.9634a6p-13f, 0x1.4ee0b6p-15f,
        // 5: sigma 3.090015587289591
        0x1.36a04cp-16f, 0x1.1f903ep-14f, 0x1.df7c20p-13f, 0x1.67ffd2p-11f, 0x1.e6d384p-10f, 0x1.286fc4p-8f, 0x1.451d18p-7f, 0x1.411c3ap-6f,
        0x1.1d9ebap-5f, 0x1.c994eep-5f, 0x1.4a176ap-4f, 0x1.ace3b6p-4f, 0x1.f5d90ep-4f, 0x1.0869f6p-3f, 0x1.f5d90ep-4f, 0x1.ace3b6p-4f,
        0x1.4a176ap-4f, 0x1.c994eep-5f, 0x1.1d9ebap-5f, 0x1.411c3ap-6f, 0x1.451d18p-7f, 0x1.286fc4p-8f, 0x1.e6d384p-10f, 0x1.67ffd2p-11f,
        0x1.df7c20p-13f, 0x1.1f903ep-14f, 0x1.36a04cp-16f};
    return t[i];
}

}  // namespace isxsi
