// stoiloss.hip - negative STOI / ESTOI as a training objective on a pair of [B, L] float32 batches at 16 kHz, with its
// gradient with respect to the estimate (cmgan_stoi_loss, include/cmgan_hip.h, "Intelligibility loss").  The forward is
// cmgan_metrics' STOI (metrics.hip: metrics_resample / _stoi_level / _clip role 2 / _stoi_env / _stoi_corr / _finalize),
// formula for formula and sum for sum; its __host__ __device__ helpers are copied from there as they are.  For estimate e
// and reference r of one row:
//
//   x10 = resample_poly(x, 5, 8):  x10[n] = sum_i x[i] h[(n + 11) 8 - 5 i], i ascending, h = table 4 of cmgan_metrics_table
//   level[s] = 20 log10(sqrt(sum_m (r10[s 128 - 1 + m] hann[m])^2) / 16), index -1 wraps;  keep s iff ((level[s] - max) + 40) > 0
//   K kept frames src[0 .. K), rebuilt signal  xs[t] = sum over p in (t / 128 - 1, t / 128), 0 <= p < K, of
//                                                      x10[src[p] 128 + o] hann[o],  o = t - 128 p      (both signals)
//   envelope frame j < K - 1:  X_k = sum_n xs[128 j + n] hann[n] e^{-2 pi i k n / 512}, n < 256;
//                              env[band, j] = sqrt(sum over the band's bins k ascending of |X_k / ws|^2),  ws = sum hann
//   window w < K - 30, frames w .. w + 29, X = env of r, Y = env of e:
//     extended = 0   per band: alpha = sqrt(sum X^2 / sum Y^2),  y' = min(Y alpha, X (1 + 10^(15/20))),
//                    s_band = sum_i ((X_i - mean X) / |X - mean X|) ((y'_i - mean y') / |y' - mean y'|);  d_w = sum_band s_band / 15
//     extended = 1   both 15 x 30 matrices: every row (band) minus its mean over the 30 frames, divided by its norm; then
//                    every column (frame) minus its mean over the 15 bands, divided by its norm;  d_w = sum of the element
//                    products / 30 (per frame over the bands ascending, then over the frames ascending)
//   STOI_b = (sum_w d_w) / (K - 30);   A = sum over b ascending of (-k STOI_b) over the rows without a status
//
// Gradient (float64, one rounding to float32 per sample; r, the keep mask and everything made of r are constants; every
// stage a gather in ascending order, no atomics).  With D_w[band, i] = d d_w / d Y[band, w + i]:
//     extended = 0   u_i = (xn_i - yn_i s_band) / |y' - mean y'|,  q_i = u_i - mean u,  m_i = 1 where Y_i alpha <= X_i (1 + c)
//                    (a tie follows the estimate's branch), T = sum_i m_i q_i Y_i,
//                    D_w[band, i] = (m_i q_i alpha - (alpha / sum Y^2) Y_i T) / 15
//     extended = 1   dc = cx / 30;  per frame: u = (dc - cy (cy . dc)) / nu,  da = u - mean u (over the bands);
//                    per band: v = (da - ya (ya . da)) / n,  D_w[band, .] = v - mean v (over the frames)
//                    (cx, cy the twice-normalised matrices, ya the row-normalised estimate, n and nu its two norms)
//   1  g[band, j] = c_b sum over w = max(0, j - 29) .. min(j, K - 31) ascending of D_w[band, j - w],  c_b = -k / (K - 30)
//   2  G_k = g[band, j] Y_k / (ws^2 env[band, j]) on the band's bins (0 where env == 0), 0 on every other bin;
//      z[j, n] = hann[n] Re sum_k G_k e^{+2 pi i k n / 512}, n < 256: one 512-point transform per frame in LDS
//   3  g10[n] = sum over s in (n / 128 - 1, n / 128), 0 <= s < nS, s kept as p, of
//               hann[o] (sum over j in (t / 128 - 1, t / 128), 0 <= j < K - 1, of z[j, t - 128 j]),  o = n - 128 s,  t = 128 p + o
//   4  g16[i] = sum over n ascending of g10[n] h[(n + 11) 8 - 5 i] over the taps that exist; then the rounding
//
// Launches (a call without a gradient stops after sl_total):
//   sl_tables    inner Hann and its sum, resample_poly taps, twiddles, band edges (metrics_tables' entries, the same code)
//   sl_resample  a thread per 10 kHz sample of either signal
//   sl_level     a block per (row, frame) of the reference
//   sl_keep      a block per row: the keep mask, its scan (src), the inverse map and K
//   sl_env       a block per (row, envelope frame): the reference's frame and the estimate's through ONE radix-2 loop in
//                LDS (metrics_stoi_env's); both envelopes and the estimate's bins 0 .. 255 go to the workspace
//   sl_corr      a wave per (row, window): a lane per band (extended = 0) or per band, then per frame (extended = 1);
//                d_w, and with a gradient D_w [15][30]
//   sl_finalize  a block per row: STOI_b, kept frames, status, c_b;   sl_total  one thread: A
//   sl_env_grad  a block per (row, two envelope frames): stages 1 and 2, both frames through the one loop
//   sl_ola_grad  a thread per 10 kHz sample: stage 3;   sl_resample_grad  a thread per output sample: stage 4
// Data-dependent counts (K) are read from the workspace; grids are sized for the worst case.
#include <math.h>
#include <stdint.h>

#include <cmath>

#include "api_internal.h"

namespace {

constexpr int MT_STOI_FS = 10000, MT_STOI_N = 256, MT_STOI_HOP = 128, MT_STOI_NFFT = 512, MT_STOI_J = 15,
              MT_STOI_SEG = 30;
constexpr double MT_STOI_DYN = 40.0;
constexpr int MT_TPB = 256;
constexpr int SL_BINS = 256;           // bins 0 .. 255 of the estimate's frames are kept (the bands end below 256)

// table offsets (doubles) inside the first TB_TOTAL doubles of the workspace
constexpr int TB_EDGES = 0;            // [1 + 2 * 15]: bands kept, then (first, end) bin pairs
constexpr int TB_HANN = 64;            // [256] inner Hann window of STOI
constexpr int TB_HSUM = 320;           // [1] its sum
constexpr int TB_FIR = 384;            // [fir_len] zero-prepadded resample_poly taps
constexpr int TB_FIR_CAP = 192;
constexpr int TB_TW = 576;             // [512][2] exp(-2 pi i k / 1024)
constexpr int TB_TOTAL = 1600;
static_assert(8 + 161 <= TB_FIR_CAP && TB_FIR + TB_FIR_CAP <= TB_TW && TB_TW + 1024 <= TB_TOTAL, "table layout");

// ---- metrics.hip's helpers, as they are -----------------------------------------------------------------------------
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

__device__ inline int bitrev(int i, int logn) { return (int)(__brev((unsigned)i) >> (32 - logn)); }

// a double into LDS as a 64-bit store that stays one: a store of more than 64 bits keeps reading its data registers after
// it issues, and the compiler does not guard them against the next VALU write (tools/isa_lint.py)
typedef __attribute__((address_space(3))) volatile double lds_double;       // (volatile: not merged; LDS by name, or it goes flat)

__device__ inline void sl_put(double* p, double v) { *(lds_double*)p = v; }

// ---- the call's arguments and workspace ------------------------------------------------------------------------------
struct SlArgs {
    const float* est;
    const float* ref;
    float* g;            // [B][L] or null
    double* rows;        // [B][2]
    float* total;        // [1]
    int* status;         // [B]
    double* tb;          // tables
    double* r10;         // [B][N10]
    double* e10;         // [B][N10]
    double* level;       // [B][nS]
    int* src;            // [B][nS] kept frame indices
    int* inv;            // [B][nS] kept position of a frame, or -1
    int* kept;           // [B]
    double* env;         // [2][B][15][nS]: reference, estimate
    double* spec;        // [B][nS][SL_BINS][2] the estimate's frame spectra
    double* corr;        // [B][nS] d_w
    double* dw;          // [B][nS - 30][15][30] D_w
    double* coef;        // [B] c_b
    double* z;           // [B][nS][256] frame gradients
    double* g10;         // [B][N10]
    double k, clipc;
    int B, L, N10, nS, extended;
};

// one block: metrics_tables' STOI entries
__global__ __launch_bounds__(MT_TPB) void sl_tables(int fs, double* tb) {
    __shared__ double fir_sum;
    Geom g;
    geom_of(fs, g);
    const int t = threadIdx.x;
    const int M = 2 * g.half_len + 1, pre = g.fir_len - M;
    for (int m = t; m < MT_STOI_N; m += blockDim.x) tb[TB_HANN + m] = hann_inner(MT_STOI_N, m);
    for (int k = t; k < 512; k += blockDim.x) {
        double sn, cs;
        sincospi((double)k / 512.0, &sn, &cs);
        tb[TB_TW + 2 * k] = cs;
        tb[TB_TW + 2 * k + 1] = -sn;
    }
    for (int j = t; j < g.fir_len; j += blockDim.x) tb[TB_FIR + j] = j < pre ? 0.0 : fir_raw(g, j - pre);
    if (t < MT_STOI_J) stoi_band(t, tb + TB_EDGES);
    __syncthreads();
    if (t == 0) {
        double sum = 0.0;
        for (int j = 0; j < M; ++j) sum += tb[TB_FIR + pre + j];
        fir_sum = sum;
        sum = 0.0;
        for (int m = 0; m < MT_STOI_N; ++m) sum += tb[TB_HANN + m];
        tb[TB_HSUM] = sum;
        stoi_kept(tb + TB_EDGES);
    }
    __syncthreads();
    for (int j = t; j < M; j += blockDim.x) tb[TB_FIR + pre + j] = tb[TB_FIR + pre + j] / fir_sum * (double)g.up;
}

// scipy.signal.resample_poly(x, 10000, fs): out[n] = sum_i x[i] h[(n + pre_remove) down - i up]; z = 0 the reference
__global__ __launch_bounds__(MT_TPB) void sl_resample(SlArgs a, int fs) {
    Geom g;
    geom_of(fs, g);
    const int n = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (n >= a.N10) return;
    const float* src = (blockIdx.z ? a.est : a.ref) + (size_t)b * a.L;
    double* dst = (blockIdx.z ? a.e10 : a.r10) + (size_t)b * a.N10;
    const long long pos = (long long)(n + g.pre_remove) * g.down;
    long long i_hi = pos / g.up;
    if (i_hi > a.L - 1) i_hi = a.L - 1;
    long long i_lo = pos - (g.fir_len - 1) <= 0 ? 0 : (pos - (g.fir_len - 1) + g.up - 1) / g.up;
    const double* h = a.tb + TB_FIR;
    double acc = 0.0;
    for (long long i = i_lo; i <= i_hi; ++i) acc += (double)src[(size_t)i] * h[pos - i * g.up];
    dst[n] = acc;
}

// silence test: level of the reference's frame s (start s * 128), samples read one early with index -1 wrapping
__global__ __launch_bounds__(MT_TPB) void sl_level(SlArgs a) {
    __shared__ double red[16];
    const int s = blockIdx.x, b = blockIdx.y, m = threadIdx.x;
    long long idx = (long long)s * MT_STOI_HOP - 1 + m;
    if (idx < 0) idx += a.N10;
    const double v = a.r10[(size_t)b * a.N10 + idx] * a.tb[TB_HANN + m];
    const double e = block_sum(v * v, red);
    if (m == 0) a.level[(size_t)b * a.nS + s] = 20.0 * log10(sqrt(e) / 16.0);
}

// the keep mask and its exclusive scan (metrics_clip, role 2), and the inverse map
__global__ __launch_bounds__(MT_TPB) void sl_keep(SlArgs a) {
    __shared__ double red[16];
    __shared__ int wtot[16];
    const int b = blockIdx.x, t = threadIdx.x;
    const double* lv = a.level + (size_t)b * a.nS;
    int* src = a.src + (size_t)b * a.nS;
    int* inv = a.inv + (size_t)b * a.nS;
    double mx = -INFINITY;
    bool nan = false;
    for (int i = t; i < a.nS; i += blockDim.x) {
        nan |= lv[i] != lv[i];
        mx = fmax(mx, lv[i]);
    }
    // max of the block (NaN propagates like np.max)
    const int lane = t & 63, wid = t >> 6, nw = blockDim.x >> 6;
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
    for (int i0 = 0; i0 < a.nS; i0 += blockDim.x) {
        const int i = i0 + t;
        const bool keep = i < a.nS && ((lv[i] - mx) + MT_STOI_DYN) > 0;
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wid] = __popcll(bal);
        __syncthreads();
        int off = total;
        for (int w = 0; w < wid; ++w) off += wtot[w];
        if (keep) src[off + before] = i;
        if (i < a.nS) inv[i] = keep ? off + before : -1;
        for (int w = 0; w < nw; ++w) total += wtot[w];
        __syncthreads();
    }
    if (t == 0) a.kept[b] = total;
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

// band envelopes of envelope frame j of the silence-removed signals (x = reference, y = estimate), and the estimate's bins
__global__ __launch_bounds__(MT_TPB) void sl_env(SlArgs a) {
    __shared__ double xr[MT_STOI_NFFT], xi[MT_STOI_NFFT], yr[MT_STOI_NFFT], yi[MT_STOI_NFFT];
    const int j = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int K = a.kept[b], nS = a.nS, B = a.B;
    if (j >= K - 1) return;
    const double* tb = a.tb;
    const int* src = a.src + (size_t)b * nS;
    const double* hann = tb + TB_HANN;
    const double* xb = a.r10 + (size_t)b * a.N10;
    const double* yb = a.e10 + (size_t)b * a.N10;
    for (int n = t; n < MT_STOI_NFFT; n += blockDim.x) {
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
    fft2_lds(xr, xi, yr, yi, 9, tb + TB_TW);
    const int nb = (int)tb[TB_EDGES];
    if (t < 2 * nb) {
        const int sig = t / nb, band = t % nb;
        const double* re = sig ? yr : xr;
        const double* im = sig ? yi : xi;
        const double ws = tb[TB_HSUM];
        const int lo = (int)tb[TB_EDGES + 1 + 2 * band], hi = (int)tb[TB_EDGES + 2 + 2 * band];
        double e = 0.0;
        for (int k = lo; k < hi; ++k) {
            const double r = re[k] / ws, i = im[k] / ws;
            e += r * r + i * i;
        }
        a.env[(((size_t)sig * B + b) * MT_STOI_J + band) * nS + j] = sqrt(e);
    }
    double* sp = a.spec + ((size_t)b * nS + j) * (2 * SL_BINS);
    for (int k = t; k < SL_BINS; k += blockDim.x) {
        sp[2 * k] = yr[k];
        sp[2 * k + 1] = yi[k];
    }
}

// window w (frames w .. w + 29): d_w, and with a gradient D_w[band][i] = d d_w / d Y[band, w + i]
__global__ __launch_bounds__(64) void sl_corr(SlArgs a, int with_grad) {
    __shared__ double sc[MT_STOI_SEG];
    __shared__ double xa[MT_STOI_J][MT_STOI_SEG], ya[MT_STOI_J][MT_STOI_SEG];
    __shared__ double cx[MT_STOI_J][MT_STOI_SEG], cy[MT_STOI_J][MT_STOI_SEG];
    __shared__ double rown[MT_STOI_J], coln[MT_STOI_SEG];
    const int w = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int nS = a.nS, B = a.B;
    if (w >= a.kept[b] - MT_STOI_SEG) return;
    const double* tb = a.tb;
    const double* env = a.env;
    const double clipc = a.clipc;
    const int nb = (int)tb[TB_EDGES];
    double* D = a.dw + ((size_t)b * (nS - MT_STOI_SEG) + w) * (MT_STOI_J * MT_STOI_SEG);
    if (!a.extended) {
        if (t < nb) {
            const double* X = env + ((size_t)b * MT_STOI_J + t) * nS + w;
            const double* Y = env + (((size_t)B + b) * MT_STOI_J + t) * nS + w;
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
            sc[t] = s;
            if (with_grad) {
                // u_i = (xn_i - yn_i s) / ny;  q_i = u_i - mean u;  T = sum m_i q_i Y_i
                double su = 0.0;
                for (int i = 0; i < MT_STOI_SEG; ++i) {
                    const double xn = (X[i] - mxv) / nx, yn = (fmin_nan(Y[i] * alpha, X[i] * (1.0 + clipc)) - myv) / ny;
                    su += (xn - yn * s) / ny;
                }
                const double mu = su / MT_STOI_SEG;
                double T = 0.0;
                for (int i = 0; i < MT_STOI_SEG; ++i) {
                    const double xn = (X[i] - mxv) / nx, yn = (fmin_nan(Y[i] * alpha, X[i] * (1.0 + clipc)) - myv) / ny;
                    const double q = (xn - yn * s) / ny - mu;
                    if (Y[i] * alpha <= X[i] * (1.0 + clipc)) T += q * Y[i];
                }
                const double back = alpha / sy2 * T;
                for (int i = 0; i < MT_STOI_SEG; ++i) {
                    const double xn = (X[i] - mxv) / nx, yn = (fmin_nan(Y[i] * alpha, X[i] * (1.0 + clipc)) - myv) / ny;
                    const double q = (xn - yn * s) / ny - mu;
                    const double own = Y[i] * alpha <= X[i] * (1.0 + clipc) ? q * alpha : 0.0;
                    D[t * MT_STOI_SEG + i] = (own - back * Y[i]) / MT_STOI_J;
                }
            }
        }
        __syncthreads();
        if (t == 0) {
            double s = 0.0;
            for (int i = 0; i < nb; ++i) s += sc[i];
            a.corr[(size_t)b * nS + w] = s / MT_STOI_J;
        }
        return;
    }
    // extended: rows (bands) first, a lane per band
    if (t < nb) {
        for (int sig = 0; sig < 2; ++sig) {
            const double* V = env + (((size_t)sig * B + b) * MT_STOI_J + t) * nS + w;
            double s = 0.0;
            for (int i = 0; i < MT_STOI_SEG; ++i) s += V[i];
            const double m = s / MT_STOI_SEG;
            double q = 0.0;
            for (int i = 0; i < MT_STOI_SEG; ++i) { const double u = V[i] - m; q += u * u; }
            const double n = sqrt(q);
            double* out = sig ? ya[t] : xa[t];
            for (int i = 0; i < MT_STOI_SEG; ++i) sl_put(out + i, (V[i] - m) / n);
            if (sig) sl_put(rown + t, n);
        }
    }
    __syncthreads();
    // then columns (frames), a lane per frame
    if (t < MT_STOI_SEG) {
        for (int sig = 0; sig < 2; ++sig) {
            double (*in)[MT_STOI_SEG] = sig ? ya : xa;
            double (*out)[MT_STOI_SEG] = sig ? cy : cx;
            double s = 0.0;
            for (int q = 0; q < nb; ++q) s += in[q][t];
            const double m = s / (double)nb;
            double e = 0.0;
            for (int q = 0; q < nb; ++q) { const double u = in[q][t] - m; e += u * u; }
            const double n = sqrt(e);
            for (int q = 0; q < nb; ++q) sl_put(&out[q][t], (in[q][t] - m) / n);
            if (sig) sl_put(coln + t, n);
        }
        double p = 0.0;
        for (int q = 0; q < nb; ++q) p += cx[q][t] * cy[q][t];
        sl_put(sc + t, p);
    }
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int i = 0; i < MT_STOI_SEG; ++i) s += sc[i];
        a.corr[(size_t)b * nS + w] = s / MT_STOI_SEG;
    }
    if (!with_grad) return;
    // back through the columns: da overwrites cx (a lane touches its own column only)
    if (t < MT_STOI_SEG) {
        const double n = coln[t];
        double dot = 0.0;
        for (int q = 0; q < nb; ++q) dot += cy[q][t] * (cx[q][t] / MT_STOI_SEG);
        double su = 0.0;
        for (int q = 0; q < nb; ++q) su += (cx[q][t] / MT_STOI_SEG - cy[q][t] * dot) / n;
        const double mu = su / (double)nb;
        for (int q = 0; q < nb; ++q) sl_put(&cx[q][t], (cx[q][t] / MT_STOI_SEG - cy[q][t] * dot) / n - mu);
    }
    __syncthreads();
    // back through the rows
    if (t < nb) {
        const double n = rown[t];
        double dot = 0.0;
        for (int i = 0; i < MT_STOI_SEG; ++i) dot += ya[t][i] * cx[t][i];
        double sv = 0.0;
        for (int i = 0; i < MT_STOI_SEG; ++i) sv += (cx[t][i] - ya[t][i] * dot) / n;
        const double mv = sv / MT_STOI_SEG;
        for (int i = 0; i < MT_STOI_SEG; ++i) D[t * MT_STOI_SEG + i] = (cx[t][i] - ya[t][i] * dot) / n - mv;
    }
}

// STOI_b, kept frames, status and c_b = -k / (K - 30)
__global__ __launch_bounds__(MT_TPB) void sl_finalize(SlArgs a) {
    __shared__ double red[16];
    const int b = blockIdx.x, t = threadIdx.x;
    const int K = a.kept[b], nW = K - MT_STOI_SEG;
    double s = 0.0;
    for (int i = t; i < nW; i += blockDim.x) s += a.corr[(size_t)b * a.nS + i];
    s = block_sum(s, red);
    if (t == 0) {
        const double v = nW > 0 ? s / (double)nW : NAN;
        int st = 0;
        if (nW <= 0) st |= 1;
        else if (!(fabs(v) <= 1.79769313486231570815e308)) st |= 2;        // NaN or infinite
        a.rows[2 * (size_t)b] = st ? NAN : v;
        a.rows[2 * (size_t)b + 1] = (double)K;
        a.status[b] = st;
        a.coef[b] = st ? 0.0 : -a.k / (double)nW;
    }
}

__global__ void sl_total(SlArgs a) {
    double A = 0.0;
    for (int b = 0; b < a.B; ++b)
        if (a.status[b] == 0) A += -a.k * a.rows[2 * (size_t)b];
    a.total[0] = (float)A;
}

// stages 1 and 2 of envelope frames 2 blockIdx.x and 2 blockIdx.x + 1: conj(G) goes through the forward loop, whose real
// part is Re sum_k G_k e^{+2 pi i k n / 512}
__global__ __launch_bounds__(MT_TPB) void sl_env_grad(SlArgs a) {
    __shared__ double xr[MT_STOI_NFFT], xi[MT_STOI_NFFT], yr[MT_STOI_NFFT], yi[MT_STOI_NFFT];
    __shared__ double gb[2][MT_STOI_J];
    const int j0 = 2 * blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int K = a.kept[b], nS = a.nS, B = a.B;
    if (a.status[b] != 0 || j0 >= K - 1) return;
    const double* tb = a.tb;
    const int nb = (int)tb[TB_EDGES];
    const int nW = K - MT_STOI_SEG;
    for (int n = t; n < MT_STOI_NFFT; n += blockDim.x) { sl_put(xr + n, 0.0); sl_put(xi + n, 0.0); sl_put(yr + n, 0.0); sl_put(yi + n, 0.0); }
    if (t < 2 * nb) {
        const int f = t / nb, band = t % nb, j = j0 + f;
        double g = 0.0;
        if (j < K - 1) {
            const int w0 = j - (MT_STOI_SEG - 1) < 0 ? 0 : j - (MT_STOI_SEG - 1), w1 = j < nW - 1 ? j : nW - 1;
            const double* D = a.dw + (size_t)b * (nS - MT_STOI_SEG) * (MT_STOI_J * MT_STOI_SEG) + band * MT_STOI_SEG;
            for (int w = w0; w <= w1; ++w) g += D[(size_t)w * (MT_STOI_J * MT_STOI_SEG) + (j - w)];
            g *= a.coef[b];
        }
        sl_put(&gb[f][band], g);
    }
    __syncthreads();
    const double ws = tb[TB_HSUM];
    const int lo0 = (int)tb[TB_EDGES + 1], hi1 = (int)tb[TB_EDGES + 2 * nb];
    for (int q = t; q < 2 * SL_BINS; q += blockDim.x) {
        const int f = q / SL_BINS, k = q % SL_BINS, j = j0 + f;
        if (j >= K - 1 || k < lo0 || k >= hi1) continue;
        int band = 0;
        while (band < nb - 1 && k >= (int)tb[TB_EDGES + 2 + 2 * band]) ++band;
        if (k < (int)tb[TB_EDGES + 1 + 2 * band]) continue;
        const double e = a.env[(((size_t)B + b) * MT_STOI_J + band) * nS + j];
        if (e == 0.0) continue;
        const double* sp = a.spec + ((size_t)b * nS + j) * (2 * SL_BINS);
        const double c = gb[f][band] / (ws * ws * e);
        const int r = bitrev(k, 9);
        if (f == 0) { sl_put(xr + r, c * sp[2 * k]); sl_put(xi + r, -(c * sp[2 * k + 1])); }
        else        { sl_put(yr + r, c * sp[2 * k]); sl_put(yi + r, -(c * sp[2 * k + 1])); }
    }
    __syncthreads();
    fft2_lds(xr, xi, yr, yi, 9, tb + TB_TW);
    const double* hann = tb + TB_HANN;
    for (int q = t; q < 2 * MT_STOI_N; q += blockDim.x) {
        const int f = q / MT_STOI_N, n = q % MT_STOI_N, j = j0 + f;
        if (j < K - 1) a.z[((size_t)b * nS + j) * MT_STOI_N + n] = (f ? yr[n] : xr[n]) * hann[n];
    }
}

// stage 3: a 10 kHz sample gathers from its up to two kept frames, each from its up to two envelope frames, earlier first
__global__ __launch_bounds__(MT_TPB) void sl_ola_grad(SlArgs a) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (n >= a.N10 || a.status[b] != 0) return;
    const int K = a.kept[b], nS = a.nS;
    const int* inv = a.inv + (size_t)b * nS;
    const double* hann = a.tb + TB_HANN;
    const double* z = a.z + (size_t)b * nS * MT_STOI_N;
    const int s1 = n / MT_STOI_HOP;
    double acc = 0.0;
    for (int s = s1 - 1; s <= s1; ++s) {
        if (s < 0 || s >= nS) continue;
        const int p = inv[s];
        if (p < 0) continue;
        const int o = n - s * MT_STOI_HOP;
        const int t = p * MT_STOI_HOP + o, j1 = t / MT_STOI_HOP;
        double in = 0.0;
        for (int j = j1 - 1; j <= j1; ++j)
            if (j >= 0 && j < K - 1) in += z[(size_t)j * MT_STOI_N + (t - j * MT_STOI_HOP)];
        acc += hann[o] * in;
    }
    a.g10[(size_t)b * a.N10 + n] = acc;
}

// stage 4: the adjoint of the resampler, and the one rounding; a row with a status gets exact zeros
__global__ __launch_bounds__(MT_TPB) void sl_resample_grad(SlArgs a, int fs) {
    Geom g;
    geom_of(fs, g);
    const long long ii = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (ii >= a.L) return;
    float* out = a.g + (size_t)b * a.L + ii;
    if (a.status[b] != 0) { *out = 0.0f; return; }
    // taps 0 <= (n + pre_remove) down - up i <= fir_len - 1
    const long long base = ii * g.up;
    long long n_lo = (base + g.down - 1) / g.down - g.pre_remove;
    long long n_hi = (base + g.fir_len - 1) / g.down - g.pre_remove;
    if (n_lo < 0) n_lo = 0;
    if (n_hi > a.N10 - 1) n_hi = a.N10 - 1;
    const double* h = a.tb + TB_FIR;
    const double* g10 = a.g10 + (size_t)b * a.N10;
    double acc = 0.0;
    for (long long n = n_lo; n <= n_hi; ++n) acc += g10[n] * h[(n + g.pre_remove) * g.down - base];
    *out = (float)acc;
}

// ---- host side -------------------------------------------------------------------------------------------------------
struct SlPlan {
    int N10, nS;
    size_t tb, r10, e10, level, src, inv, kept, env, spec, corr, dw, coef, z, g10, total;   // byte offsets
};

inline size_t sl_up256(size_t v) { return (v + 255) & ~(size_t)255; }

// null: fine; else what is wrong with the shape (code in *rc)
inline const char* sl_plan(int B, int L, int fs, SlPlan& p, int* rc) {
    *rc = CMGAN_E_BADARG;
    if (B < 1 || B > 65535) return "need 1 <= B <= 65535";
    if (fs != 16000) { *rc = CMGAN_E_UNSUPPORTED; return "fs must be 16000"; }
    if (L < 1) return "L is too short for 31 frames at 10 kHz";
    Geom g;
    geom_of(fs, g);
    const long long n10 = ((long long)L * g.up + g.down - 1) / g.down;
    const long long nS = n10 > MT_STOI_N ? (n10 - MT_STOI_N + MT_STOI_HOP - 1) / MT_STOI_HOP : 0;
    if (nS < MT_STOI_SEG + 1) return "L is too short for 31 frames at 10 kHz";
    if (L > 2147483647 / g.up - 4096) return "rows are too long";
    p.N10 = (int)n10;
    p.nS = (int)nS;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = sl_up256(o + bytes); return at; };
    const size_t d = sizeof(double), Bz = (size_t)B, S = (size_t)p.nS;
    p.tb = take(TB_TOTAL * d);
    p.r10 = take(Bz * p.N10 * d);
    p.e10 = take(Bz * p.N10 * d);
    p.level = take(Bz * S * d);
    p.src = take(Bz * S * sizeof(int));
    p.inv = take(Bz * S * sizeof(int));
    p.kept = take(Bz * sizeof(int));
    p.env = take(2 * Bz * MT_STOI_J * S * d);
    p.spec = take(Bz * S * 2 * SL_BINS * d);
    p.corr = take(Bz * S * d);
    p.dw = take(Bz * (S - MT_STOI_SEG) * MT_STOI_J * MT_STOI_SEG * d);
    p.coef = take(Bz * d);
    p.z = take(Bz * S * MT_STOI_N * d);
    p.g10 = take(Bz * p.N10 * d);
    p.total = o;
    *rc = CMGAN_OK;
    return nullptr;
}

inline bool sl_overlap(const void* p, const void* q, size_t bytes) {
    const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
    return p0 < q0 + bytes && q0 < p0 + bytes;
}

}  // namespace

extern "C" size_t cmgan_stoi_loss_workspace_bytes(cmgan_handle*, int B, int L, int fs) {
    SlPlan p;
    int rc;
    return sl_plan(B, L, fs, p, &rc) ? 0 : p.total;
}

extern "C" int cmgan_stoi_loss(cmgan_handle* h, const float* est, const float* ref, int B, int L, int fs, int extended, double k,
                               double* rows, float* total, int* status, float* g_audio, void* ws, size_t ws_bytes, void* stream) {
    // every argument is judged before the handle is, so that the errors below need no GPU
    if (!est || !ref || !rows || !total || !status) return fail(h, CMGAN_E_BADARG, "cmgan_stoi_loss: null pointer");
    if (((uintptr_t)est | (uintptr_t)ref | (uintptr_t)total | (uintptr_t)status | (uintptr_t)g_audio) & 3)
        return fail(h, CMGAN_E_BADARG, "cmgan_stoi_loss: float32 and int32 buffers must be 4-byte aligned");
    if ((uintptr_t)rows & 7) return fail(h, CMGAN_E_BADARG, "cmgan_stoi_loss: rows must be 8-byte aligned");
    SlPlan p;
    int rc;
    if (const char* what = sl_plan(B, L, fs, p, &rc)) return fail(h, rc, "cmgan_stoi_loss: %s (B=%d L=%d fs=%d)", what, B, L, fs);
    if (extended != 0 && extended != 1) return fail(h, CMGAN_E_BADARG, "cmgan_stoi_loss: extended must be 0 or 1");
    if (!(k == k)) return fail(h, CMGAN_E_BADARG, "cmgan_stoi_loss: k must be a number");
    const size_t bytes = (size_t)B * (size_t)L * sizeof(float);
    if (g_audio && (sl_overlap(g_audio, est, bytes) || sl_overlap(g_audio, ref, bytes)))
        return fail(h, CMGAN_E_BADARG, "cmgan_stoi_loss: g_audio overlaps est or ref; the gradient is not formed in place");
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < p.total)
        return fail(h, CMGAN_E_BADARG, "cmgan_stoi_loss: the workspace must be 256-byte aligned and hold %zu bytes (%zu given)",
                    p.total, ws ? ws_bytes : (size_t)0);
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "cmgan_stoi_loss: null handle");
    const LaunchCtx ctx = begin(h, stream);
    hipStream_t s = ctx.stream;
    char* w = (char*)ws;
    SlArgs a;
    a.est = est;
    a.ref = ref;
    a.g = g_audio;
    a.rows = rows;
    a.total = total;
    a.status = status;
    a.tb = (double*)(w + p.tb);
    a.r10 = (double*)(w + p.r10);
    a.e10 = (double*)(w + p.e10);
    a.level = (double*)(w + p.level);
    a.src = (int*)(w + p.src);
    a.inv = (int*)(w + p.inv);
    a.kept = (int*)(w + p.kept);
    a.env = (double*)(w + p.env);
    a.spec = (double*)(w + p.spec);
    a.corr = (double*)(w + p.corr);
    a.dw = (double*)(w + p.dw);
    a.coef = (double*)(w + p.coef);
    a.z = (double*)(w + p.z);
    a.g10 = (double*)(w + p.g10);
    a.k = k;
    a.clipc = std::pow(10.0, -(-15.0) / 20.0);                     // 10 ** (-beta / 20), beta = -15
    a.B = B;
    a.L = L;
    a.N10 = p.N10;
    a.nS = p.nS;
    a.extended = extended;
    const int with_grad = g_audio ? 1 : 0;
    LAUNCH(ctx, "sl_tables", sl_tables<<<1, MT_TPB, 0, s>>>(fs, a.tb));
    LAUNCH(ctx, "sl_resample", sl_resample<<<dim3((p.N10 + MT_TPB - 1) / MT_TPB, B, 2), MT_TPB, 0, s>>>(a, fs));
    LAUNCH(ctx, "sl_level", sl_level<<<dim3(p.nS, B), MT_STOI_N, 0, s>>>(a));
    LAUNCH(ctx, "sl_keep", sl_keep<<<B, MT_TPB, 0, s>>>(a));
    LAUNCH(ctx, "sl_env", sl_env<<<dim3(p.nS, B), MT_TPB, 0, s>>>(a));
    LAUNCH(ctx, "sl_corr", sl_corr<<<dim3(p.nS - MT_STOI_SEG, B), 64, 0, s>>>(a, with_grad));
    LAUNCH(ctx, "sl_finalize", sl_finalize<<<B, MT_TPB, 0, s>>>(a));
    LAUNCH(ctx, "sl_total", sl_total<<<1, 1, 0, s>>>(a));
    if (with_grad) {
        LAUNCH(ctx, "sl_env_grad", sl_env_grad<<<dim3((p.nS + 1) / 2, B), MT_TPB, 0, s>>>(a));
        LAUNCH(ctx, "sl_ola_grad", sl_ola_grad<<<dim3((p.N10 + MT_TPB - 1) / MT_TPB, B), MT_TPB, 0, s>>>(a));
        LAUNCH(ctx, "sl_resample_grad", sl_resample_grad<<<dim3((L + MT_TPB - 1) / MT_TPB, B), MT_TPB, 0, s>>>(a, fs));
    }
    return check_launch(h, "stoi_loss");
}
