// stoiloss.hip - negative STOI / ESTOI as a training objective on a pair of [B, L] float32 batches at 16 kHz, with its
// gradient with respect to the estimate (cmgan_stoi_loss, include/cmgan_hip.h, "Intelligibility loss").  The forward is
// cmgan_metrics' STOI (metrics.hip: metrics_resample / _stoi_level / _clip role 2 / _stoi_env / _stoi_corr / _finalize),
// formula for formula and sum for sum: the two files' kernels call the same bodies in stoi_common.hip.h, and this file
// keeps what is the loss's own (the ESTOI branch, the row's value and the gradient).  For estimate e and reference r of
// one row:
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
//   sl_tables    inner Hann and its sum, resample_poly taps, twiddles, band edges (metrics_tables' entries, the same body)
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
#include "host_ranges.h"
#include "lds_f64.hip.h"
#include "stoi_common.hip.h"

namespace {

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
    stoi_tables_fill(g, tb + TB_HANN, tb + TB_TW, tb + TB_FIR, tb + TB_EDGES);
    __syncthreads();
    stoi_tables_sums(g, tb + TB_HANN, tb + TB_HSUM, tb + TB_FIR, &fir_sum, tb + TB_EDGES);
    __syncthreads();
    stoi_tables_norm(g, tb + TB_FIR, fir_sum);
}

// scipy.signal.resample_poly(x, 10000, fs): out[n] = sum_i x[i] h[(n + pre_remove) down - i up]; z = 0 the reference
__global__ __launch_bounds__(MT_TPB) void sl_resample(SlArgs a, int fs) {
    stoi_resample<false>(a.ref, a.est, 0.0, a.L, a.N10, fs, a.tb + TB_FIR, a.r10, a.e10);
}

// silence test: level of the reference's frame s (start s * 128), samples read one early with index -1 wrapping
__global__ __launch_bounds__(MT_TPB) void sl_level(SlArgs a) {
    __shared__ double red[16];
    stoi_level(a.r10, a.N10, a.nS, a.tb + TB_HANN, red, a.level);
}

// the keep mask and its exclusive scan (metrics_clip, role 2), and the inverse map
__global__ __launch_bounds__(MT_TPB) void sl_keep(SlArgs a) {
    __shared__ double red[16];
    __shared__ int wtot[16];
    const int b = blockIdx.x;
    stoi_keep<true>(a.level, a.nS, a.src, a.inv, a.kept, b, red, wtot);
}

// band envelopes of envelope frame j of the silence-removed signals (x = reference, y = estimate), and the estimate's bins
__global__ __launch_bounds__(MT_TPB) void sl_env(SlArgs a) {
    __shared__ double xr[MT_STOI_NFFT], xi[MT_STOI_NFFT], yr[MT_STOI_NFFT], yi[MT_STOI_NFFT];
    const int j = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int K = a.kept[b], nS = a.nS, B = a.B;
    if (j >= K - 1) return;
    const double* tb = a.tb;
    stoi_env(a.r10, a.e10, a.N10, nS, a.src, K, j, b, tb + TB_HANN, tb + TB_HSUM, tb + TB_TW, tb + TB_EDGES, a.env, B, xr, xi,
             yr, yi);
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
            const BandCorr c = stoi_band_corr(X, Y, clipc);
            const double s = c.s, alpha = c.alpha, sy2 = c.sy2, mxv = c.mx, myv = c.my, nx = c.nx, ny = c.ny;
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
            for (int i = 0; i < MT_STOI_SEG; ++i) lds_put(out + i, (V[i] - m) / n);
            if (sig) lds_put(rown + t, n);
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
            for (int q = 0; q < nb; ++q) lds_put(&out[q][t], (in[q][t] - m) / n);
            if (sig) lds_put(coln + t, n);
        }
        double p = 0.0;
        for (int q = 0; q < nb; ++q) p += cx[q][t] * cy[q][t];
        lds_put(sc + t, p);
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
        for (int q = 0; q < nb; ++q) lds_put(&cx[q][t], (cx[q][t] / MT_STOI_SEG - cy[q][t] * dot) / n - mu);
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
    for (int n = t; n < MT_STOI_NFFT; n += blockDim.x) { lds_put(xr + n, 0.0); lds_put(xi + n, 0.0); lds_put(yr + n, 0.0); lds_put(yi + n, 0.0); }
    if (t < 2 * nb) {
        const int f = t / nb, band = t % nb, j = j0 + f;
        double g = 0.0;
        if (j < K - 1) {
            const int w0 = j - (MT_STOI_SEG - 1) < 0 ? 0 : j - (MT_STOI_SEG - 1), w1 = j < nW - 1 ? j : nW - 1;
            const double* D = a.dw + (size_t)b * (nS - MT_STOI_SEG) * (MT_STOI_J * MT_STOI_SEG) + band * MT_STOI_SEG;
            for (int w = w0; w <= w1; ++w) g += D[(size_t)w * (MT_STOI_J * MT_STOI_SEG) + (j - w)];
            g *= a.coef[b];
        }
        lds_put(&gb[f][band], g);
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
        if (f == 0) { lds_put(xr + r, c * sp[2 * k]); lds_put(xi + r, -(c * sp[2 * k + 1])); }
        else        { lds_put(yr + r, c * sp[2 * k]); lds_put(yi + r, -(c * sp[2 * k + 1])); }
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

// null: fine; else what is wrong with the shape (code in *rc)
inline const char* sl_plan(int B, int L, int fs, SlPlan& p, int* rc) {
    *rc = CMGAN_E_BADARG;
    if (B < 1 || B > 65535) return "need 1 <= B <= 65535";
    if (fs != 16000) { *rc = CMGAN_E_UNSUPPORTED; return "fs must be 16000"; }
    if (L < 1) return "L is too short for 31 frames at 10 kHz";
    Geom g;
    geom_of(fs, g);
    stoi_frames(L, g, &p.N10, &p.nS);
    if (p.nS < MT_STOI_SEG + 1) return "L is too short for 31 frames at 10 kHz";
    if (L > 2147483647 / g.up - 4096) return "rows are too long";
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = up256(o + bytes); return at; };
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
    if (g_audio && (bytes_overlap(g_audio, bytes, est, bytes) || bytes_overlap(g_audio, bytes, ref, bytes)))
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
