// surf_tables.hpp — the two Gaussian tables of SURF as float32 literals, one copy for host and device: getGaussianKernel(13, 2.5, CV_32F)
// weighs the orientation samples, getGaussianKernel(20, 3.3, CV_32F) the 20 x 20 gradients of the descriptor.  tests/helpers/surf_np.py
// holds the same bits and regenerates them from OpenCV's formula (exp in double, rounded to float, normalised by the double sum of the
// rounded values); no exp runs on the device.  Internal.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ISX_SURF_HD __host__ __device__
#else
#define ISX_SURF_HD
#endif

namespace isxsf {

ISX_SURF_HD inline float surf_g13(int i) {
    const float t[13] = {0x1.28274ap-7f, 0x1.64ff86p-6f, 0x1.6eb6e6p-5f, 0x1.40ff98p-4f, 0x1.dedf96p-4f, 0x1.306238p-3f, 0x1.49bc24p-3f,
                         0x1.306238p-3f, 0x1.dedf96p-4f, 0x1.40ff98p-4f, 0x1.6eb6e6p-5f, 0x1.64ff86p-6f, 0x1.28274ap-7f};
    return t[i];
}
ISX_SURF_HD inline float surf_g20(int i) {
    const float t[20] = {0x1.f7ed64p-10f, 0x1.1fe43ep-8f, 0x1.2c14fcp-7f, 0x1.1d5866p-6f, 0x1.ef0d7ep-6f, 0x1.87c302p-5f, 0x1.1ad252p-4f,
                         0x1.7485d8p-4f,  0x1.bf9faep-4f, 0x1.eaac98p-4f, 0x1.eaac98p-4f, 0x1.bf9faep-4f, 0x1.7485d8p-4f, 0x1.1ad252p-4f,
                         0x1.87c302p-5f,  0x1.ef0d7ep-6f, 0x1.1d5866p-6f, 0x1.2c14fcp-7f, 0x1.1fe43ep-8f, 0x1.f7ed64p-10f};
    return t[i];
}

}  // namespace isxsf
