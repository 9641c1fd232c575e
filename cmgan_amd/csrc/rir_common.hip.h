// rir_common.hip.h - what the two room simulators share (rir.hip: cmgan_rir; rir_bands.hip: cmgan_rir_bands): the limits
// of a call, the block's integer prefix sum and the clamp that turns a double bound of an nz range into an int.
#pragma once
#include <math.h>
#include <stddef.h>

namespace {

constexpr int RR_TPB = 256;                 // threads of every kernel
constexpr int RR_TILE = RR_TPB;             // taps per block of the tap kernels: one per thread
constexpr int RR_CAP = 512;                 // images per LDS list chunk
constexpr int RR_UNR = 8;                   // list entries whose t0 a thread fetches at once (RR_CAP is a multiple)
constexpr int RR_MAX_K = 65536;             // longest response (the limit of cmgan_mix)
constexpr int RR_MAX_N = 255;               // largest image index per axis
constexpr int RR_MAX_TW = 64;               // largest half-width of the fractional-delay filter
constexpr int RR_PW = RR_MAX_N + 2;         // powers b^0 .. b^(N + 1) of one coefficient
constexpr double RR_PI = 3.14159265358979323846;

// exclusive prefix sum of one int per thread in thread order; `total` is the block's sum
__device__ inline int rr_scan(int v, int (*s)[RR_TPB], int& total) {
    const int t = threadIdx.x;
    int cur = 0;
    s[0][t] = v;
    __syncthreads();
    for (int off = 1; off < RR_TPB; off <<= 1) {
        int x = s[cur][t];
        if (t >= off) x += s[cur][t - off];
        s[cur ^ 1][t] = x;
        cur ^= 1;
        __syncthreads();
    }
    total = s[cur][RR_TPB - 1];
    const int incl = s[cur][t];
    __syncthreads();
    return incl - v;
}

// a double bound of an nz range as an int in [-Nz - 1, Nz + 1] (NaN included: fmax / fmin drop it)
__device__ inline int rr_bound(double v, int Nz) { return (int)fmin(fmax(v, (double)(-Nz - 1)), (double)(Nz + 1)); }

inline size_t rr_up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace
