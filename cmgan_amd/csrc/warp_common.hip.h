// warp_common.hip.h - the arithmetic on rates and output counts that warp.hip (cmgan_warp) and stretch.hip (cmgan_stretch)
// share, so that the two agree on every length: one rounded float64 product per time, the valid range of a rate, and
// #{i >= 0 : fl(i r) < n}.
#pragma once
#include <math.h>

namespace {

constexpr double WP_MAX_RATE = 4.0;         // rates in [1 / WP_MAX_RATE, WP_MAX_RATE]

// one rounded float64 product, never fused with a following sum
__host__ __device__ inline double wp_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(a, b);
#else
    volatile double p = a * b;
    return p;
#endif
}

__host__ __device__ inline bool wp_rate_ok(double r) { return r >= 1.0 / WP_MAX_RATE && r <= WP_MAX_RATE; }   // a NaN: false

// #{i >= 0 : fl(i r) < n}: ceil(n / r), then single steps until fl((M - 1) r) < n <= fl(M r)
__host__ __device__ inline long long wp_count(long long n, double r) {
    if (n <= 0) return 0;
    const double nd = (double)n;
    long long M = (long long)ceil(nd / r);
    while (M > 0 && wp_mul((double)(M - 1), r) >= nd) --M;
    while (wp_mul((double)M, r) < nd) ++M;
    return M;
}

}  // namespace
