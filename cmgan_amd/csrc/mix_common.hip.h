// mix_common.hip.h - what the two mixing translation units share (mix.hip: cmgan_mix; scene.hip: cmgan_scene): the tile
// geometry, the looping bank segment, the fixed-order block reductions and the clamps of the untrusted RIR tables.  One
// definition each, so that a scene without located sources has the bits of cmgan_mix.
#pragma once
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace {

constexpr int MX_TPB = 256;                 // threads of every kernel here
constexpr int MX_OPT = 4;                   // outputs per thread of the convolutions: outputs t, t + 256, t + 512, t + 768 of the tile
constexpr int MX_TILE = MX_TPB * MX_OPT;    // outputs per block
constexpr int MX_KC = 1024;                 // taps per LDS chunk: 8 KiB of taps + 16 KiB of signal span, both float64
constexpr int MX_MAX_K = 65536;             // longest RIR (4 s at 16 kHz)
constexpr int MX_MAX_L = 0x7fffffff - MX_TILE;   // a tile's sample indices stay in an int

// a row's bank segment: valid only if it lies inside the bank; `off` is the row's offset mod len in [0, len)
struct NoiseRow {
    const float* p;
    long long len, off;
};

__device__ inline NoiseRow mx_segment(const float* bank, long long bank_len, long long st, long long len, long long off) {
    NoiseRow r;
    r.len = len;
    const bool ok = bank && st >= 0 && r.len >= 1 && st <= bank_len && r.len <= bank_len - st;
    if (!ok) {
        r.p = nullptr;
        r.len = 1;
        r.off = 0;
        return r;
    }
    r.p = bank + st;
    const long long o = off % r.len;
    r.off = o < 0 ? o + r.len : o;
    return r;
}

__device__ inline double mix_noise(const NoiseRow& r, int i) {
    return r.p ? (double)r.p[(r.off + i) % r.len] : 0.0;
}

// v = speech + g n: one expression for the maximum and the store, so both see the same bits
__device__ inline double mix_v(double speech, double g, double n) { return fma(g, n, speech); }

__device__ inline double block_sum(double v, double* red) {          // fixed order: halves folded, every thread calls
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = MX_TPB / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__device__ inline double block_max(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = MX_TPB / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = fmax(red[t], red[t + s]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// a RIR table entry is not trusted: the index is clamped to [0, R), the length to [1, Kmax]
__device__ inline void mx_rir_row(const float* rir, int R, int Kmax, int idx, int len, const float*& h, int& K) {
    idx = idx < 0 ? 0 : (idx >= R ? R - 1 : idx);
    K = len < 1 ? 1 : (len > Kmax ? Kmax : len);
    h = rir + (size_t)idx * Kmax;
}

// the direct path: the FIRST index at which |h[0:K]| is largest (all NaN: tap 0); every thread calls, thread 0 gets it
__device__ inline int mx_direct_index(const float* h, int K, float* s_v, int* s_i) {
    const int t = threadIdx.x;
    float best = -1.f;
    int at = 0x7fffffff;
    for (int k = t; k < K; k += MX_TPB) {
        const float v = fabsf(h[k]);
        if (v > best) { best = v; at = k; }                  // ascending k: the first of equals stays
    }
    s_v[t] = best;
    s_i[t] = at;
    __syncthreads();
    for (int s = MX_TPB / 2; s > 0; s >>= 1) {
        if (t < s) {
            const float v = s_v[t + s];
            const int i = s_i[t + s];
            if (v > s_v[t] || (v == s_v[t] && i < s_i[t])) { s_v[t] = v; s_i[t] = i; }
        }
        __syncthreads();
    }
    return s_i[0] < K ? s_i[0] : 0;
}

inline size_t mx_up256(size_t v) { return (v + 255) & ~(size_t)255; }

inline int mx_tiles(int L) { return (L + MX_TILE - 1) / MX_TILE; }

}  // namespace
