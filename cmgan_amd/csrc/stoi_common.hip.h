// stoi_common.hip.h - the STOI front end that metrics.hip (cmgan_metrics, the scorer) and stoiloss.hip (cmgan_stoi_loss,
// the training term) share, so that the loss is the scorer's STOI formula for formula and sum for sum: the geometry and
// the tables, the resampler to 10 kHz, the silence test and its keep mask, the band envelopes and the classic band
// correlation.  Definition for definition the host module cmgan_amd/metrics.py.  The kernels stay in the two files (their
// names are the profiler's keys); they declare their LDS, find their row and call the bodies below with plain pointers.
#pragma once
#include <math.h>
#include <stddef.h>

#include "lds_f64.hip.h"

namespace {

constexpr int MT_STOI_FS = 10000, MT_STOI_N = 256, MT_STOI_HOP = 128, MT_STOI_NFFT = 512, MT_STOI_J = 15,
              MT_STOI_SEG = 30;
constexpr double MT_STOI_DYN = 40.0;

// Frame geometry of one sample rate (metrics.py: _win_hop, wss, llr, stoi / scipy resample_poly's padding rules).
struct Geom {
    int fs, win, hop, nfft, half, order;
    int up, down, half_len, fir_len, pre_remove;     // fir_len counts the zero pre-pad
};

__host__ __device__ inline bool geom_of(int fs, Geom& g) {
    if (fs != 16000 && fs != 8000) return false;
    g.fs = fs;
    g.win = fs == 16000 ? 480 : 240;                 // int(np.round(30 * fs / 1000))
    g.hop = g.win / 4;
    g.nfft = fs == 16000 ? 1024 : 512;               // 2 ** ceil(log2(2 * win))
    g.half = g.nfft / 2;
    g.order = fs < 10000 ? 10 : 16;
    g.up = 5;                                        // 10000 / gcd(10000, fs), fs / gcd(10000, fs)
    g.down = fs == 16000 ? 8 : 4;
    const int max_rate = g.up > g.down ? g.up : g.down;
    g.half_len = 10 * max_rate;
    const int pre = g.down - g.half_len % g.down;
    g.fir_len = pre + 2 * g.half_len + 1;
    g.pre_remove = (g.half_len + pre) / g.down;
    return true;
}

// samples at 10 kHz and 256-sample frames at hop 128 of a row of L samples (nS = 0: not one frame)
inline void stoi_frames(int L, const Geom& g, int* N10, int* nS) {
    const long long n10 = ((long long)L * g.up + g.down - 1) / g.down;
    *N10 = (int)n10;
    *nS = n10 > MT_STOI_N ? (int)((n10 - MT_STOI_N + MT_STOI_HOP - 1) / MT_STOI_HOP) : 0;
}

// STOI one-third-octave bands (metrics.py: _third_octave_bands(10000, 512, 15, 150)): out[0] = bands kept, then the
// [first, end) bins of all 15 bands.  stoi_band fills band k, stoi_kept the count once all bands are in.
__host__ __device__ inline void stoi_band(int k, double* out) {
    const int nbins = MT_STOI_NFFT / 2 + 1;
    const double step = (double)MT_STOI_FS / MT_STOI_NFFT;       // np.linspace(0, fs, nfft + 1)
    const double lo = 150.0 * pow(2.0, (double)(2 * k - 1) / 6.0);
    const double hi = 150.0 * pow(2.0, (double)(2 * k + 1) / 6.0);
    int a = 0, bb = 0;
    double ba = INFINITY, bh = INFINITY;
    for (int i = 0; i < nbins; ++i) {
        const double f = (double)i * step;
        const double da = (f - lo) * (f - lo), dh = (f - hi) * (f - hi);
        if (da < ba) { ba = da; a = i; }
        if (dh < bh) { bh = dh; bb = i; }
    }
    out[1 + 2 * k] = a;
    out[2 + 2 * k] = bb;
}

__host__ __device__ inline int stoi_kept(double* out) {
    int last = -1;
    for (int i = 0; i < MT_STOI_J - 1; ++i) {
        const double w0 = fmax(out[2 + 2 * i] - out[1 + 2 * i], 0.0), w1 = fmax(out[4 + 2 * i] - out[3 + 2 * i], 0.0);
        if (w1 >= w0 && w1 != 0) last = i;
    }
    out[0] = last + 2;
    return last + 2;
}

__host__ __device__ inline double hann_inner(int n, int m) {    // scipy.signal.windows.hann(n + 2)[1 : n + 1]
    const int M = n + 2;
    const double step = (M_PI - -M_PI) / (double)(M - 1);
    const double fac = (double)(m + 1) * step + -M_PI;
    return 0.5 + 0.5 * cos(fac);
}

__host__ __device__ inline double bessel_i0(double x) {         // power series; x <= 5 here
    double term = 1.0, sum = 1.0;
    const double q = 0.25 * x * x;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// firwin(2 half_len + 1, 1 / max_rate, window=('kaiser', 5.0)) without the final normalisation (tap j, 0-based)
__host__ __device__ inline double fir_raw(const Geom& g, int j) {
    const int M = 2 * g.half_len + 1;
    const double cutoff = 1.0 / (double)(g.up > g.down ? g.up : g.down);
    const double alpha = 0.5 * (M - 1);
    const double m = (double)j - alpha;
    double y = M_PI * (cutoff * m == 0.0 ? 1.0e-20 : cutoff * m);   // np.sinc
    double h = cutoff * (sin(y) / y);
    h -= 0.0 * 1.0;                                                // left band edge 0: 0 * sinc(0)
    const double wa = (M - 1) / 2.0;
    const double r = ((double)j - wa) / wa;
    const double win = bessel_i0(5.0 * sqrt(1.0 - r * r)) / bessel_i0(5.0);
    return h * win;
}

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over the block (blockDim.x a multiple of 64, <= 1024); red = 16 doubles of LDS; every thread gets the result
__device__ inline double block_sum(double v, double* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < nw; ++i) s += red[i];
    return s;
}

// in-place radix-2 DIT FFT of two length-(1 << logn) sequences in LDS, input in bit-reversed order; tw = exp(-2 pi i k /
// 1024), k < 512 (interleaved re, im)
__device__ void fft2_lds(double* ar, double* ai, double* br, double* bi, int logn, const double* tw) {
    const int n = 1 << logn;
    for (int s = 1; s <= logn; ++s) {
        const int hm = 1 << (s - 1);
        for (int t = threadIdx.x; t < n / 2; t += blockDim.x) {
            const int j = t & (hm - 1);
            const int i0 = ((t >> (s - 1)) << s) + j, i1 = i0 + hm;
            const int k = j << (10 - s);
            const double wr = tw[2 * k], wi = tw[2 * k + 1];
            double xr = ar[i1] * wr - ai[i1] * wi, xi = ar[i1] * wi + ai[i1] * wr;
            ar[i1] = ar[i0] - xr; ai[i1] = ai[i0] - xi;
            ar[i0] += xr; ai[i0] += xi;
            xr = br[i1] * wr - bi[i1] * wi; xi = br[i1] * wi + bi[i1] * wr;
            br[i1] = br[i0] - xr; bi[i1] = bi[i0] - xi;
            br[i0] += xr; bi[i0] += xi;
        }
        __syncthreads();
    }
}

__device__ inline double fmin_nan(double a, double b) {    // np.minimum: NaN propagates
    return (a != a || b != b) ? NAN : (a < b ? a : b);
}

// overlap-add sample t of the kept frames (at most two sources), in np.add.at's order
__device__ inline double ola(const double* x10, const int* src, int K, int t, const double* hann) {
    const int p = t / MT_STOI_HOP;
    double acc = 0.0;
    if (p - 1 >= 0 && p - 1 < K) {
        const int o = t - (p - 1) * MT_STOI_HOP;
        acc += x10[(size_t)src[p - 1] * MT_STOI_HOP + o] * hann[o];
    }
    if (p < K) {
        const int o = t - p * MT_STOI_HOP;
        acc += x10[(size_t)src[p] * MT_STOI_HOP + o] * hann[o];
    }
    return acc;
}

// ---- the table fill of one block, in three steps with a barrier of the kernel's between them --------------------------
// 1: every entry by its own thread - inner Hann [256], twiddles exp(-2 pi i k / 1024) [512][2], the zero-prepadded raw
// resample_poly taps [fir_len] and the band edges [1 + 2 * 15]
__device__ inline void stoi_tables_fill(const Geom& g, double* hann, double* tw, double* fir, double* edges) {
    const int t = threadIdx.x;
    const int pre = g.fir_len - (2 * g.half_len + 1);
    for (int m = t; m < MT_STOI_N; m += blockDim.x) hann[m] = hann_inner(MT_STOI_N, m);
    for (int k = t; k < 512; k += blockDim.x) {
        double sn, cs;
        sincospi((double)k / 512.0, &sn, &cs);
        tw[2 * k] = cs;
        tw[2 * k + 1] = -sn;
    }
    for (int j = t; j < g.fir_len; j += blockDim.x) fir[j] = j < pre ? 0.0 : fir_raw(g, j - pre);
    if (t < MT_STOI_J) stoi_band(t, edges);
}

// 2: thread 0 - the taps' sum (to LDS), the window's sum, the count of bands kept, each in ascending order
__device__ inline void stoi_tables_sums(const Geom& g, const double* hann, double* hsum, const double* fir, double* fir_sum,
                                        double* edges) {
    const int M = 2 * g.half_len + 1;
    const double* taps = fir + (g.fir_len - M);                    // behind the zero pre-pad
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int j = 0; j < M; ++j) sum += taps[j];
        *fir_sum = sum;
        sum = 0.0;
        for (int m = 0; m < MT_STOI_N; ++m) sum += hann[m];
        *hsum = sum;
        stoi_kept(edges);
    }
}

// 3: the taps / their sum * up
__device__ inline void stoi_tables_norm(const Geom& g, double* fir, double fir_sum) {
    const int M = 2 * g.half_len + 1;
    double* taps = fir + (g.fir_len - M);
    for (int j = threadIdx.x; j < M; j += blockDim.x) taps[j] = taps[j] / fir_sum * (double)g.up;
}

// ---- the kernels' bodies ---------------------------------------------------------------------------------------------
// scipy.signal.resample_poly(x, 10000, fs) of the rows of x (blockIdx.z = 0) and y (1), a thread per output sample:
// out[n] = sum_i x[i] h[(n + pre_remove) down - i up], i ascending.  OFFSET: x[i] + offset (the scorer's eps); without it
// the plain widening load, which keeps a -0.0
template <bool OFFSET>
__device__ inline void stoi_resample(const float* x, const float* y, double offset, int L, int N10, int fs, const double* h,
                                     double* x10, double* y10) {
    Geom g;
    geom_of(fs, g);
    const int n = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (n >= N10) return;
    const float* src = (blockIdx.z ? y : x) + (size_t)b * L;
    double* dst = (blockIdx.z ? y10 : x10) + (size_t)b * N10;
    const long long pos = (long long)(n + g.pre_remove) * g.down;
    long long i_hi = pos / g.up;
    if (i_hi > L - 1) i_hi = L - 1;
    long long i_lo = pos - (g.fir_len - 1) <= 0 ? 0 : (pos - (g.fir_len - 1) + g.up - 1) / g.up;
    double acc = 0.0;
    for (long long i = i_lo; i <= i_hi; ++i) {
        const double v = OFFSET ? (double)src[(size_t)i] + offset : (double)src[(size_t)i];
        acc += v * h[pos - i * g.up];
    }
    dst[n] = acc;
}

// silence test, a block of 256 threads per (frame blockIdx.x, row blockIdx.y): level of frame s (start s * 128), samples
// read one early with index -1 wrapping
__device__ inline void stoi_level(const double* x10, int N10, int nS, const double* hann, double* red /* LDS [16] */,
                                  double* level) {
    const int s = blockIdx.x, b = blockIdx.y, m = threadIdx.x;
    long long idx = (long long)s * MT_STOI_HOP - 1 + m;
    if (idx < 0) idx += N10;
    const double v = x10[(size_t)b * N10 + idx] * hann[m];
    const double e = block_sum(v * v, red);
    if (m == 0) level[(size_t)b * nS + s] = 20.0 * log10(sqrt(e) / 16.0);
}

// the keep mask of row b by one block: keep s iff ((level[s] - max) + 40) > 0, the kept frames' indices in ascending
// order (src, an exclusive scan), their count and, with INV, the kept position of every frame or -1.  (Here and in
// stoi_env the block's size is read once, nt: the compiler then folds the read into one scalar load.)
template <bool INV>
__device__ inline void stoi_keep(const double* level, int nS, int* src_all, int* inv_all, int* kept, int b,
                                 double* red /* LDS [16] */, int* wtot /* LDS [16] */) {
    const int t = threadIdx.x, nt = blockDim.x;
    const double* lv = level + (size_t)b * nS;
    int* src = src_all + (size_t)b * nS;
    int* inv = INV ? inv_all + (size_t)b * nS : nullptr;
    double mx = -INFINITY;
    bool nan = false;
    for (int i = t; i < nS; i += nt) {
        nan |= lv[i] != lv[i];
        mx = fmax(mx, lv[i]);
    }
    // max of the block (NaN propagates like np.max)
    const int lane = t & 63, wid = t >> 6, nw = nt >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    nan = __any(nan);
    if (lane == 0) { red[wid] = mx; wtot[wid] = nan; }
    __syncthreads();
    mx = red[0];
    for (int w = 1; w < nw; ++w) { mx = fmax(mx, red[w]); nan |= wtot[w] != 0; }
    if (nan) mx = NAN;
    __syncthreads();
    int total = 0;
    for (int i0 = 0; i0 < nS; i0 += nt) {
        const int i = i0 + t;
        const bool keep = i < nS && ((lv[i] - mx) + MT_STOI_DYN) > 0;
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wid] = __popcll(bal);
        __syncthreads();
        int off = total;
        for (int w = 0; w < wid; ++w) off += wtot[w];
        if (keep) src[off + before] = i;
        if (INV && i < nS) inv[i] = keep ? off + before : -1;
        for (int w = 0; w < nw; ++w) total += wtot[w];
        __syncthreads();
    }
    if (t == 0) kept[b] = total;
}

// band envelopes of envelope frame j < K - 1 of row b's silence-removed signals (x = reference, y = estimate) by one
// block: both frames through ONE radix-2 loop in the caller's LDS (four arrays of 512), which keeps the spectra on return;
// env is [2][B][15][nS]
__device__ inline void stoi_env(const double* x10, const double* y10, int N10, int nS, const int* src_all, int K, int j, int b,
                                const double* hann, const double* hsum, const double* tw, const double* edges, double* env,
                                int B, double* xr, double* xi, double* yr, double* yi) {
    const int t = threadIdx.x, nt = blockDim.x;
    const int* src = src_all + (size_t)b * nS;
    const double* xb = x10 + (size_t)b * N10;
    const double* yb = y10 + (size_t)b * N10;
    for (int n = t; n < MT_STOI_NFFT; n += nt) {
        double vx = 0.0, vy = 0.0;
        if (n < MT_STOI_N) {
            const int ts = j * MT_STOI_HOP + n;
            vx = ola(xb, src, K, ts, hann) * hann[n];
            vy = ola(yb, src, K, ts, hann) * hann[n];
        }
        const int r = bitrev(n, 9);
        xr[r] = vx; xi[r] = 0.0;
        yr[r] = vy; yi[r] = 0.0;
    }
    __syncthreads();
    fft2_lds(xr, xi, yr, yi, 9, tw);
    const int nb = (int)edges[0];
    if (t < 2 * nb) {
        const int sig = t / nb, band = t % nb;
        const double* re = sig ? yr : xr;
        const double* im = sig ? yi : xi;
        const double ws = *hsum;
        const int lo = (int)edges[1 + 2 * band], hi = (int)edges[2 + 2 * band];
        double e = 0.0;
        for (int k = lo; k < hi; ++k) {
            const double r = re[k] / ws, i = im[k] / ws;
            e += r * r + i * i;
        }
        env[(((size_t)sig * B + b) * MT_STOI_J + band) * nS + j] = sqrt(e);
    }
}

// the classic correlation of one band over one window: X, Y the 30 envelope values of the reference and the estimate.
// s is the band's term; the rest is what the loss's gradient goes on with
struct BandCorr {
    double s, alpha, sy2, mx, my, nx, ny;    // y' = min(Y alpha, X (1 + clipc)); means and norms of X and of y'
};

__device__ inline BandCorr stoi_band_corr(const double* X, const double* Y, double clipc) {
    double sx2 = 0.0, sy2 = 0.0, sx = 0.0;
    for (int i = 0; i < MT_STOI_SEG; ++i) { sx2 += X[i] * X[i]; sy2 += Y[i] * Y[i]; sx += X[i]; }
    const double alpha = sqrt(sx2 / sy2);
    const double mxv = sx / MT_STOI_SEG;
    double sy = 0.0;
    for (int i = 0; i < MT_STOI_SEG; ++i) sy += fmin_nan(Y[i] * alpha, X[i] * (1.0 + clipc));
    const double myv = sy / MT_STOI_SEG;
    double nx = 0.0, ny = 0.0;
    for (int i = 0; i < MT_STOI_SEG; ++i) {
        const double a = X[i] - mxv, c = fmin_nan(Y[i] * alpha, X[i] * (1.0 + clipc)) - myv;
        nx += a * a;
        ny += c * c;
    }
    nx = sqrt(nx);
    ny = sqrt(ny);
    double s = 0.0;
    for (int i = 0; i < MT_STOI_SEG; ++i) {
        const double a = X[i] - mxv, c = fmin_nan(Y[i] * alpha, X[i] * (1.0 + clipc)) - myv;
        s += (a / nx) * (c / ny);
    }
    return {s, alpha, sy2, mxv, myv, nx, ny};
}

}  // namespace
