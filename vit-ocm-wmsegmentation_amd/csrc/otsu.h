// otsu.h — the Otsu level of a 256-bin histogram, one set of statements for the host entry point ocm_otsu_threshold
// (engine.hip) and for the kernels that take the level on the device (kernels_kmeans_px.hip). Restates cv2.threshold(...,
// THRESH_OTSU)'s getThreshVal_Otsu_8u (OpenCV 4.6.0 modules/imgproc/src/thresh.cpp — an un-vendored dependency of the
// reference, opencv-python 4.6.0.66; parity unpinned: cv2 is not installable here).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// count > 0. Separate IEEE float64 operations on both sides: the device takes the host's level bit for bit.
__host__ __device__ inline int32_t ocm_otsu_level(const uint64_t *hist256, int64_t count) {
#pragma clang fp contract(off)
    const double scale = 1.0 / (double)count;
    double mu = 0;
    for (int i = 0; i < 256; ++i) mu += i * (double)hist256[i];
    mu *= scale;
    double mu1 = 0, q1 = 0, max_sigma = 0;
    int max_val = 0;
    for (int i = 0; i < 256; ++i) {
        const double p_i = (double)hist256[i] * scale;
        mu1 *= q1;
        q1 += p_i;
        const double q2 = 1.0 - q1;
        const double lo = q1 < q2 ? q1 : q2, hi = q1 < q2 ? q2 : q1;
        if (lo < 1.1920928955078125e-07 || hi > 1.0 - 1.1920928955078125e-07) continue;
        mu1 = (mu1 + i * p_i) / q1;
        const double mu2 = (mu - q1 * mu1) / q2;
        const double sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
        if (sigma > max_sigma) {
            max_sigma = sigma;
            max_val = i;
        }
    }
    return max_val;
}
