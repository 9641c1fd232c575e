// lds_f64.hip.h - float64 values in LDS and the radix-2 transform over them that auxloss.hip (cmgan_aux_loss), suppress.hip
// (cmgan_suppress) and stoiloss.hip (cmgan_stoi_loss) share: the one store rule, the bit reversal, the twiddles a block
// makes itself and the decimation-in-time passes.  (metrics.hip takes bitrev from here through stoi_common.hip.h.)
#pragma once
#include <math.h>

namespace {

// A double goes into LDS as a 64-bit store that stays one, a complex value as two of them: a store of more than 64 bits
// keeps reading its data registers after it issues, and the compiler does not guard them against the next VALU write
// (tools/isa_lint.py).  volatile: the two stores are not merged; LDS by name, or the store goes flat.
typedef __attribute__((address_space(3))) volatile double lds_double;

__device__ inline void lds_put(double* p, double v) { *(lds_double*)p = v; }

__device__ inline void lds_put(double2* p, double re, double im) {
    lds_double* q = (lds_double*)p;
    q[0] = re;
    q[1] = im;
}

__device__ inline int bitrev(int i, int logn) { return (int)(__brev((unsigned)i) >> (32 - logn)); }

// tw[k] = e^{-2 pi i k / N}, k < N / 2, by a block of TPB threads: the argument 2 k / N is exact
template <int TPB>
__device__ inline void twiddles(double2* tw, int N) {
    for (int k = threadIdx.x; k < (N >> 1); k += TPB) {
        double s, c;
        sincospi((double)(2 * k) / (double)N, &s, &c);
        lds_put(tw + k, c, -s);
    }
}

// The radix-2 decimation-in-time passes over bit-reversed frames of N points in LDS, by a block of TPB threads; sign = -1
// conjugates the twiddles (the inverse, without its 1 / N).  Every product is a fused multiply-add by name, so the bits do
// not hang on the build's contraction.  Ends behind a barrier.  MANY: `count` frames, `stride` points apart; the one-frame
// form below does not divide by the frame's length.
template <int TPB, bool MANY>
__device__ __forceinline__ void fft_passes(double2* buf, const double2* tw, int N, int logN, double sign, int count, int stride) {
    const int half_n = N >> 1;
    for (int s = 1; s <= logN; ++s) {
        __syncthreads();
        const int half = 1 << (s - 1);
        for (int j = threadIdx.x; j < (MANY ? half_n * count : half_n); j += TPB) {
            const int fr = MANY ? j / half_n : 0, jj = j - fr * half_n;
            const int pos = jj & (half - 1);
            const int i0 = ((jj >> (s - 1)) << s) + pos + fr * stride, i1 = i0 + half;
            double2 w = tw[pos << (logN - s)];
            w.y *= sign;
            const double2 u = buf[i0], v = buf[i1];
            const double vr = fma(v.x, w.x, -(v.y * w.y)), vi = fma(v.x, w.y, v.y * w.x);
            lds_put(buf + i0, u.x + vr, u.y + vi);
            lds_put(buf + i1, u.x - vr, u.y - vi);
        }
    }
    __syncthreads();
}

template <int TPB>
__device__ inline void fft(double2* buf, const double2* tw, int N, int logN, double sign) {
    fft_passes<TPB, false>(buf, tw, N, logN, sign, 1, 0);
}

template <int TPB>
__device__ inline void fft(double2* buf, const double2* tw, int N, int logN, double sign, int count, int stride) {
    fft_passes<TPB, true>(buf, tw, N, logN, sign, count, stride);
}

}  // namespace
