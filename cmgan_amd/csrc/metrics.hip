// metrics.hip - objective speech metrics on the GPU: WSS, LLR, segmental SNR, STOI and the CSIG / CBAK / COVL
// composites (cmgan_metrics, include/cmgan_hip.h).  Definition for definition the host module cmgan_amd/metrics.py
// (itself pinned to the reference's src/tools/compute_metrics.py at 1e-9), quirks included: the off-by-one of the WSS
// nearest-peak walk, the `/ 32768` of the WSS frames, segSNR clipped to [-10, 35], STOI's silence test one sample early
// (index -1 wraps to the last sample) and STOI divided by J = 15.
//
// Arithmetic is float64 on the VALU (inputs are the library's float32 audio, widened on load, plus `offset`).  Eight
// launches per call, no host synchronisation, no atomics:
//   metrics_tables     analysis taper, sparse WSS bank, STOI band edges, inner Hann, resample_poly FIR, FFT twiddles
//   metrics_frames     (clip, frame): segSNR energies, LLR (lags, Levinson-Durbin, Toeplitz forms), WSS (1024-pt FFT)
//   metrics_resample   polyphase resample to 10 kHz (scipy.signal.resample_poly), one output sample per thread
//   metrics_stoi_level (clip, frame): energy of the 256-sample frame read one sample early
//   metrics_clip       (clip, role): radix-select trimmed means, mean segSNR, overall SNR, STOI keep mask + scan
//   metrics_stoi_env   (clip, frame): overlap-add as a gather, 512-pt FFT, one-third-octave envelopes
//   metrics_stoi_corr  (clip, window): the 30-frame correlations of every band
//   metrics_finalize   (clip): STOI mean, composites
// Data-dependent counts (kept STOI frames) are read from the workspace; grids are sized for the worst case.
// The STOI chain up to the band correlation (tables, resampler, level, keep mask, envelopes, correlation) is the set of
// bodies in stoi_common.hip.h, which stoiloss.hip (cmgan_stoi_loss) calls too: the loss is this scorer's STOI by construction.
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "api_internal.h"
#include "host_ranges.h"
#include "stoi_common.hip.h"

namespace {

constexpr int MT_NB = 25;              // WSS critical bands
constexpr int MT_BANKW = 64;           // weights kept per band (the widest band keeps 36 bins at either rate)
constexpr int MT_MAXP = 16;            // LPC order at 16 kHz
constexpr int MT_TPB = 256;
constexpr double MT_EPS = 2.220446049250313e-16;   // np.spacing(1.0)

// table offsets (doubles) inside the first TB_TOTAL doubles of the workspace
constexpr int TB_TAPER = 0;            // [win]
constexpr int TB_BANKF = 512;          // [25] first bin of each band
constexpr int TB_BANKC = 544;          // [25] bins kept
constexpr int TB_BANKW = 576;          // [25][64] weights
constexpr int TB_EDGES = 2176;         // [1 + 2 * 15]: bands kept, then (first, end) bin pairs
constexpr int TB_HANN = 2240;          // [256] inner Hann window of STOI
constexpr int TB_HSUM = 2496;          // [1] its sum
constexpr int TB_FIR = 2560;           // [fir_len] zero-prepadded resample_poly taps
constexpr int TB_FIR_CAP = 448;
constexpr int TB_TW = 3008;            // [512][2] exp(-2 pi i k / 1024)
constexpr int TB_TOTAL = 4096;
static_assert(8 + 161 <= TB_FIR_CAP && TB_FIR + TB_FIR_CAP <= TB_TW && TB_TW + 1024 <= TB_TOTAL, "table layout");

const double CB_CENTRE[MT_NB] = {50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717,
                                 904.128, 1020.38, 1148.30, 1288.72, 1442.54, 1610.70, 1794.16, 1993.93, 2211.08,
                                 2446.71, 2701.97, 2978.04, 3276.17, 3597.63};
const double CB_WIDTH[MT_NB] = {70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 77.3724, 86.0056, 95.3398, 105.411, 116.256,
                                127.914, 140.423, 153.823, 168.154, 183.457, 199.776, 217.153, 235.631, 255.255,
                                276.072, 298.126, 321.465, 346.136};
struct CriticalBands { double centre[MT_NB], width[MT_NB]; };   // passed by value to the table kernel

__host__ __device__ inline double taper_value(int win, int n) {   // 0.5 (1 - cos(2 pi n / (win + 1))), n = 1..win
    return 0.5 * (1.0 - cos(2.0 * M_PI * (double)(n + 1) / (double)(win + 1)));
}

// Gaussian critical band b at bin k, or 0 where it is cut at -30 dB   (metrics.py: wss)
__host__ __device__ inline double bank_value(const double* centre, const double* width, int fs, int half, int b, int k) {
    const double nyq = (double)fs / 2;
    const double f0 = floor(centre[b] / nyq * half);
    const double bw = width[b] / nyq * half;
    const double gain = log(width[0]) - log(width[b]);
    const double d = ((double)k - f0) / bw;
    const double v = exp(-11.0 * (d * d) + gain);
    return v > exp(-30.0 / (2.0 * 2.303)) ? v : 0.0;
}

// sparse form of band b: first bin, count (<= MT_BANKW) and weights; the kept bins of a Gaussian are contiguous
inline void bank_band(const double* centre, const double* width, int fs, int half, int b, int* first, int* count,
                      double* w) {
    int f = -1, c = 0;
    for (int k = 0; k < half; ++k) {
        const double v = bank_value(centre, width, fs, half, b, k);
        if (v > 0.0) {
            if (f < 0) f = k;
            if (c < MT_BANKW) w[c] = v;
            ++c;
        }
    }
    *first = f < 0 ? 0 : f;
    *count = c < MT_BANKW ? c : MT_BANKW;
}

inline void fir_taps(const Geom& g, double* out) {   // out[fir_len]: pre-pad zeros, taps / sum * up
    const int M = 2 * g.half_len + 1, pre = g.fir_len - M;
    double s = 0.0;
    for (int j = 0; j < M; ++j) s += fir_raw(g, j);                // the table kernel sums in the same order
    for (int j = 0; j < pre; ++j) out[j] = 0.0;
    for (int j = 0; j < M; ++j) out[pre + j] = fir_raw(g, j) / s * (double)g.up;
}

// ------------------------------------------------------------------------------------------ device helpers
__device__ inline double ld(const float* p, size_t i, double off) { return (double)p[i] + off; }

// ------------------------------------------------------------------------------------------ kernels
// one block: every table entry by its own thread where the entries are independent
__global__ __launch_bounds__(MT_TPB) void metrics_tables(int fs, CriticalBands cb, double* tb) {
    __shared__ double fir_sum;
    Geom g;
    geom_of(fs, g);
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6, nw = blockDim.x >> 6;
    for (int n = t; n < g.win; n += blockDim.x) tb[TB_TAPER + n] = taper_value(g.win, n);
    stoi_tables_fill(g, tb + TB_HANN, tb + TB_TW, tb + TB_FIR, tb + TB_EDGES);
    // WSS bank: one band per wave at a time, 64 bins per step; the kept bins are contiguous, so the first one found
    // fixes every weight's slot
    for (int b = wid; b < MT_NB; b += nw) {
        int first = -1, count = 0;
        for (int k0 = 0; k0 < g.half; k0 += 64) {
            const int k = k0 + lane;
            const double v = k < g.half ? bank_value(cb.centre, cb.width, fs, g.half, b, k) : 0.0;
            const unsigned long long bal = __ballot(v > 0.0);
            if (first < 0 && bal) first = k0 + __ffsll((long long)bal) - 1;
            count += __popcll(bal);
            if (v > 0.0 && k - first < MT_BANKW) tb[TB_BANKW + b * MT_BANKW + (k - first)] = v;
        }
        if (lane == 0) {
            tb[TB_BANKF + b] = first < 0 ? 0 : first;
            tb[TB_BANKC + b] = count < MT_BANKW ? count : MT_BANKW;
        }
    }
    __syncthreads();
    stoi_tables_sums(g, tb + TB_HANN, tb + TB_HSUM, tb + TB_FIR, &fir_sum, tb + TB_EDGES);
    __syncthreads();
    stoi_tables_norm(g, tb + TB_FIR, fir_sum);
}

struct FrameArgs {
    const float* x;
    const float* y;
    double offset;
    int L, nf, nfw, nfl;
    const double* tb;
    double* wss;      // [B][nf]
    double* llr;
    double* seg;
    double* frames;   // [B][3][nf] or null
};

// one (frame, clip) per block: segSNR energies, LLR, WSS
__global__ __launch_bounds__(MT_TPB) void metrics_frames(FrameArgs a, int fs) {
    Geom g;
    geom_of(fs, g);
    __shared__ double fx[480], fy[480];
    __shared__ double xr[1024], xi[1024], yr[1024], yi[1024];
    __shared__ double red[16];
    __shared__ double sR[2][MT_MAXP + 1], sA[2][MT_MAXP + 1], sQ[2];
    __shared__ double sE[2][MT_NB], sS[2][MT_NB], sW[MT_NB], sT[MT_NB];
    const int f = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int win = g.win, p = g.order, logn = g.nfft == 1024 ? 10 : 9;
    const size_t base = (size_t)b * a.L + (size_t)f * g.hop;
    const double* taper = a.tb + TB_TAPER;
    for (int n = t; n < g.nfft; n += blockDim.x) {
        double vx = 0.0, vy = 0.0;
        if (n < win) {
            if ((size_t)f * g.hop + n < (size_t)a.L) {
                vx = ld(a.x, base + n, a.offset) * taper[n];
                vy = ld(a.y, base + n, a.offset) * taper[n];
            }
            fx[n] = vx;
            fy[n] = vy;
        }
        const int r = bitrev(n, logn);
        xr[r] = vx / 32768.0; xi[r] = 0.0;
        yr[r] = vy / 32768.0; yi[r] = 0.0;
    }
    __syncthreads();
    // segmental SNR energies
    double ex = 0.0, en = 0.0;
    for (int n = t; n < win; n += blockDim.x) {
        const double d = fx[n] - fy[n];
        ex += fx[n] * fx[n];
        en += d * d;
    }
    ex = block_sum(ex, red);
    en = block_sum(en, red + 8);
    // LLR: autocorrelation lags 0..p of both frames, one (signal, lag) per wave at a time
    const int lane = t & 63, wid = t >> 6, nw = blockDim.x >> 6;
    for (int q = wid; q < 2 * (p + 1); q += nw) {
        const int sig = q / (p + 1), lag = q % (p + 1);
        const double* fr = sig ? fy : fx;
        double acc = 0.0;
        for (int i = lane; i < win - lag; i += 64) acc += fr[i] * fr[i + lag];
        acc = wave_sum(acc);
        if (lane == 0) sR[sig][lag] = acc;
    }
    fft2_lds(xr, xi, yr, yi, logn, a.tb + TB_TW);      // ends with a barrier: sR is visible too
    // Levinson-Durbin of both frames in two waves; a[] lives in LDS (sA[sig][1..p] holds a_1..a_p)
    if (lane == 0 && wid < 2) {
        const int sig = wid;
        const double* R = sR[sig];
        double* A = sA[sig] + 1;
        double err = R[0];
        for (int i = 0; i < p; ++i) {
            double acc = 0.0;
            for (int j = 0; j < i; ++j) acc += A[j] * R[i - j];
            const double k = (R[i + 1] - acc) / err;
            for (int j = 0; j < i / 2; ++j) {
                const double lo = A[j], hi = A[i - 1 - j];
                A[j] = lo - k * hi;
                A[i - 1 - j] = hi - k * lo;
            }
            if (i & 1) A[i / 2] = A[i / 2] - k * A[i / 2];
            A[i] = k;
            err = (1.0 - k * k) * err;
        }
        sA[sig][0] = 1.0;
        for (int j = 1; j <= p; ++j) sA[sig][j] = -sA[sig][j];
    }
    // WSS band energies of both spectra (bins 0..half-1)
    if (t < 2 * MT_NB) {
        const int sig = t / MT_NB, band = t % MT_NB;
        const double* re = sig ? yr : xr;
        const double* im = sig ? yi : xi;
        const int first = (int)a.tb[TB_BANKF + band], cnt = (int)a.tb[TB_BANKC + band];
        const double* w = a.tb + TB_BANKW + band * MT_BANKW;
        double e = 0.0;
        for (int i = 0; i < cnt; ++i) {
            const int k = first + i;
            e += (re[k] * re[k] + im[k] * im[k]) * w[i];
        }
        sE[sig][band] = 10.0 * log10(fmax(e, 1e-10));
    }
    __syncthreads();
    if (t < 2 * (MT_NB - 1)) {
        const int sig = t / (MT_NB - 1), band = t % (MT_NB - 1);
        sS[sig][band] = sE[sig][band + 1] - sE[sig][band];
    }
    // LLR quadratic forms with the clean signal's Toeplitz lags: wave 0 -> num (processed LPC), wave 1 -> den
    if (lane == 0 && wid < 2) {
        const double* A = sA[wid == 0 ? 1 : 0];
        const double* R = sR[0];
        double q = 0.0;
        for (int i = 0; i <= p; ++i) {
            double r = 0.0;
            for (int j = 0; j <= p; ++j) r += R[i > j ? i - j : j - i] * A[j];
            q += A[i] * r;
        }
        sQ[wid] = q;
    }
    __syncthreads();
    // WSS weights: nearest-peak walk per band (the reference's off-by-one kept)
    if (t < MT_NB - 1) {
        const int ns = MT_NB - 1;
        double wsum = 0.0;
        for (int sig = 0; sig < 2; ++sig) {
            const double* e = sE[sig];
            const double* s = sS[sig];
            double emax = e[0];
            for (int i = 1; i < MT_NB; ++i) emax = fmax(emax, e[i]);
            double peak;
            if (s[t] > 0) {
                int j = t;
                while (j < ns && s[j] > 0) ++j;
                peak = e[j - 1];
            } else {
                int j = t - 1;
                while (j >= 0 && !(s[j] > 0)) --j;
                peak = e[j + 1];
            }
            wsum += (20.0 / (20.0 + emax - e[t])) * (1.0 / (1.0 + peak - e[t]));
        }
        const double w = 0.5 * wsum;
        const double d = sS[0][t] - sS[1][t];
        sW[t] = w;
        sT[t] = w * (d * d);
    }
    __syncthreads();
    if (t == 0) {
        const size_t o = (size_t)b * a.nf + f;
        double wss = NAN, llr = NAN, seg = NAN;
        if (f < a.nfw) {
            double num = 0.0, den = 0.0;
            for (int i = 0; i < MT_NB - 1; ++i) { num += sT[i]; den += sW[i]; }
            wss = num / den;
            seg = 10.0 * log10(ex / (en + MT_EPS) + MT_EPS);
            if (!(seg != seg)) seg = seg < -10.0 ? -10.0 : (seg > 35.0 ? 35.0 : seg);
        }
        if (f < a.nfl) llr = log(sQ[0] / sQ[1]);
        a.wss[o] = wss;
        a.llr[o] = llr;
        a.seg[o] = seg;
        if (a.frames) {
            double* fr = a.frames + (size_t)b * 3 * a.nf + f;
            fr[0] = wss;
            fr[a.nf] = llr;
            fr[2 * (size_t)a.nf] = seg;
        }
    }
}

// scipy.signal.resample_poly(x, 10000, fs): out[n] = sum_i x[i] h[(n + pre_remove) down - i up]
__global__ __launch_bounds__(MT_TPB) void metrics_resample(const float* x, const float* y, double offset, int L, int N10,
                                                           int fs, const double* tb, double* x10, double* y10) {
    stoi_resample<true>(x, y, offset, L, N10, fs, tb + TB_FIR, x10, y10);
}

// STOI silence test: level of frame s (start s * 128), samples read one early with index -1 wrapping
__global__ __launch_bounds__(MT_TPB) void metrics_stoi_level(const double* x10, int N10, int nS, const double* tb,
                                                             double* level) {
    __shared__ double red[16];
    stoi_level(x10, N10, nS, tb + TB_HANN, red, level);
}

__device__ inline unsigned long long okey(double v) {        // order-preserving integer image; NaN sorts last
    if (v != v) return ~0ull;
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ inline double okey_value(unsigned long long k) {
    if (k == ~0ull) return NAN;
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// mean of the k smallest of v[0..n): radix select (4-bit digits, counted with wave ballots) of the k-th smallest
// integer image, then one masked sum
__device__ double trimmed_mean(const double* v, int n, int k, unsigned* cnt /* LDS [16 waves][16] */, int* sel,
                               double* red) {
    if (k <= 0) return NAN;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    unsigned long long prefix = 0, mask = 0;
    int krem = k;
    for (int shift = 60; shift >= 0; shift -= 4) {
        if (lane < 16) cnt[wid * 16 + lane] = 0;
        __syncthreads();
        for (int i0 = 0; i0 < n; i0 += blockDim.x) {
            const int i = i0 + threadIdx.x;
            bool live = false;
            int digit = 0;
            if (i < n) {
                const unsigned long long key = okey(v[i]);
                live = (key & mask) == prefix;
                digit = (int)((key >> shift) & 15);
            }
#pragma unroll
            for (int d = 0; d < 16; ++d) {
                const unsigned long long bal = __ballot(live && digit == d);
                if (lane == 0) cnt[wid * 16 + d] += (unsigned)__popcll(bal);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int d = 0;
            for (; d < 15; ++d) {
                unsigned c = 0;
                for (int w = 0; w < nw; ++w) c += cnt[w * 16 + d];
                if ((unsigned)krem <= c) break;
                krem -= (int)c;
            }
            sel[0] = d;
            sel[1] = krem;
        }
        __syncthreads();
        prefix |= (unsigned long long)sel[0] << shift;
        mask |= 15ull << shift;
        krem = sel[1];
        __syncthreads();
    }
    double s = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double x = v[i];
        if (okey(x) < prefix) { s += x; c += 1.0; }
    }
    s = block_sum(s, red);
    c = block_sum(c, red + 8);
    return (s + ((double)k - c) * okey_value(prefix)) / (double)k;
}

struct ClipArgs {
    const float* x;
    const float* y;
    double offset;
    int L, nf, nfw, nfl, kw, kl, nS;
    const double* wss;
    const double* llr;
    const double* seg;
    const double* level;
    int* src;         // [B][nS] kept frame indices
    int* kept;        // [B]
    double* clip;     // [B][4]: wss, llr, ssnr, snr
};

// role 0: trimmed WSS + mean segSNR; role 1: trimmed LLR + overall SNR; role 2: STOI keep mask and its exclusive scan
__global__ __launch_bounds__(MT_TPB) void metrics_clip(ClipArgs a) {
    __shared__ unsigned cnt[16 * 16];
    __shared__ int sel[2];
    __shared__ double red[16];
    __shared__ int wtot[16];
    const int b = blockIdx.x, role = blockIdx.y, t = threadIdx.x;
    double* out = a.clip + (size_t)b * 4;
    if (role == 0) {
        const double* seg = a.seg + (size_t)b * a.nf;
        const double wt = trimmed_mean(a.wss + (size_t)b * a.nf, a.nfw, a.kw, cnt, sel, red);
        double s = 0.0;
        for (int i = t; i < a.nfw; i += blockDim.x) s += seg[i];
        s = block_sum(s, red);
        if (t == 0) { out[0] = wt; out[2] = s / (double)a.nfw; }
    } else if (role == 1) {
        const double lt = trimmed_mean(a.llr + (size_t)b * a.nf, a.nfl, a.kl, cnt, sel, red);
        const size_t o = (size_t)b * a.L;
        double sx = 0.0, sd = 0.0;
        for (int i = t; i < a.L; i += blockDim.x) {
            const double xv = ld(a.x, o + i, a.offset), yv = ld(a.y, o + i, a.offset);
            sx += xv * xv;
            sd += (xv - yv) * (xv - yv);
        }
        sx = block_sum(sx, red);
        sd = block_sum(sd, red + 8);
        if (t == 0) { out[1] = lt; out[3] = 10.0 * log10(sx / sd); }
    } else {
        stoi_keep<false>(a.level, a.nS, a.src, nullptr, a.kept, b, red, wtot);
    }
}

// band envelopes of envelope frame j of the silence-removed signals: [2][B][15][nS]
__global__ __launch_bounds__(MT_TPB) void metrics_stoi_env(const double* x10, const double* y10, int N10, int nS,
                                                           const int* src_all, const int* kept, const double* tb,
                                                           double* env, int B) {
    __shared__ double xr[MT_STOI_NFFT], xi[MT_STOI_NFFT], yr[MT_STOI_NFFT], yi[MT_STOI_NFFT];
    const int j = blockIdx.x, b = blockIdx.y;
    const int K = kept[b];
    if (j >= K - 1) return;
    stoi_env(x10, y10, N10, nS, src_all, K, j, b, tb + TB_HANN, tb + TB_HSUM, tb + TB_TW, tb + TB_EDGES, env, B, xr, xi, yr, yi);
}

// correlation of window w (frames w .. w+29) summed over the bands / J
__global__ __launch_bounds__(64) void metrics_stoi_corr(const double* env, int nS, const int* kept, const double* tb,
                                                        double clipc, double* corr, int B) {
    __shared__ double sc[MT_STOI_J];
    const int w = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    if (w >= kept[b] - MT_STOI_SEG) return;
    const int nb = (int)tb[TB_EDGES];
    if (t < nb) {
        const double* X = env + ((size_t)b * MT_STOI_J + t) * nS + w;
        const double* Y = env + (((size_t)B + b) * MT_STOI_J + t) * nS + w;
        sc[t] = stoi_band_corr(X, Y, clipc).s;
    }
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int i = 0; i < nb; ++i) s += sc[i];
        corr[(size_t)b * nS + w] = s / MT_STOI_J;
    }
}

__device__ inline double lim(double v) { return v != v ? v : (v < 1.0 ? 1.0 : (v > 5.0 ? 5.0 : v)); }

__global__ __launch_bounds__(MT_TPB) void metrics_finalize(const double* corr, int nS, const int* kept,
                                                           const double* clip, const double* pesq, double* scores) {
    __shared__ double red[16];
    const int b = blockIdx.x, t = threadIdx.x;
    const int nW = kept[b] - MT_STOI_SEG;
    double s = 0.0;
    for (int i = t; i < nW; i += blockDim.x) s += corr[(size_t)b * nS + i];
    s = block_sum(s, red);
    if (t == 0) {
        const double* c = clip + (size_t)b * 4;
        const double wss = c[0], llr = c[1], ssnr = c[2], snr = c[3];
        const double mos = pesq ? pesq[b] : NAN;
        double* o = scores + (size_t)b * 9;
        o[0] = mos;
        o[1] = lim(3.093 - 1.029 * llr + 0.603 * mos - 0.009 * wss);
        o[2] = lim(1.634 + 0.478 * mos - 0.007 * wss + 0.063 * ssnr);
        o[3] = lim(1.594 + 0.805 * mos - 0.512 * llr - 0.007 * wss);
        o[4] = ssnr;
        o[5] = nW > 0 ? s / (double)nW : NAN;
        o[6] = wss;
        o[7] = llr;
        o[8] = snr;
    }
}

// ------------------------------------------------------------------------------------------ host side
struct Plan {
    Geom g;
    int nfw, nfl, nf, kw, kl, N10, nS;
    size_t tb, wss, llr, seg, x10, y10, level, src, kept, env, corr, clip, total;   // byte offsets
};

// 0 = ok, else a CMGAN_E_* code with `why` set
int plan_metrics(int B, int L, int fs, Plan& p, const char** why) {
    if (B <= 0 || L <= 0) { *why = "B and L must be positive"; return CMGAN_E_BADARG; }
    if (B > 65535) { *why = "at most 65535 rows per call"; return CMGAN_E_BADSHAPE; }
    if (!geom_of(fs, p.g)) { *why = "fs must be 16000 or 8000"; return CMGAN_E_UNSUPPORTED; }
    const Geom& g = p.g;
    if (L < g.win) { *why = "L is shorter than one analysis window"; return CMGAN_E_BADSHAPE; }
    // the same IEEE operations as metrics.py
    p.nfw = (int)((double)L / g.hop - (double)g.win / g.hop);
    p.nfl = (int)((double)(L - g.win) / g.hop);
    p.nf = p.nfw > p.nfl ? p.nfw : p.nfl;
    p.kw = (int)std::nearbyint((double)p.nfw * 0.95);
    p.kl = (int)std::nearbyint((double)p.nfl * 0.95);
    stoi_frames(L, g, &p.N10, &p.nS);
    if (p.nfw < 1 || p.nfl < 1 || p.nS < MT_STOI_SEG + 1) {
        *why = "L is too short for one 30-frame STOI window";
        return CMGAN_E_BADSHAPE;
    }
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = up256(o + bytes); return at; };
    const size_t d = sizeof(double);
    p.tb = take(TB_TOTAL * d);
    p.wss = take((size_t)B * p.nf * d);
    p.llr = take((size_t)B * p.nf * d);
    p.seg = take((size_t)B * p.nf * d);
    p.x10 = take((size_t)B * p.N10 * d);
    p.y10 = take((size_t)B * p.N10 * d);
    p.level = take((size_t)B * p.nS * d);
    p.src = take((size_t)B * p.nS * sizeof(int));
    p.kept = take((size_t)B * sizeof(int));
    p.env = take((size_t)2 * B * MT_STOI_J * p.nS * d);
    p.corr = take((size_t)B * p.nS * d);
    p.clip = take((size_t)B * 4 * d);
    p.total = o;
    return CMGAN_OK;
}

}  // namespace

extern "C" size_t cmgan_metrics_workspace_bytes(const cmgan_handle* h, int B, int L, int fs) {
    (void)h;
    Plan p;
    const char* why = nullptr;
    return plan_metrics(B, L, fs, p, &why) == CMGAN_OK ? p.total : 0;
}

extern "C" int cmgan_metrics(cmgan_handle* h, const float* clean, const float* enh, int B, int L, int fs,
                             const double* pesq, double offset, double* scores, double* frames, void* ws,
                             size_t ws_bytes, void* stream) {
    if (!h) return CMGAN_E_BADARG;
    if (!clean || !enh || !scores) return fail(h, CMGAN_E_BADARG, "cmgan_metrics: null pointer");
    Plan p;
    const char* why = nullptr;
    if (int rc = plan_metrics(B, L, fs, p, &why)) return fail(h, rc, "cmgan_metrics: %s (B=%d L=%d fs=%d)", why, B, L, fs);
    if (int rc = check_ws(h, ws, ws_bytes, p.total)) return rc;
    if (!std::isfinite(offset)) return fail(h, CMGAN_E_BADARG, "cmgan_metrics: offset must be finite");
    char* w = (char*)ws;
    double* tb = (double*)(w + p.tb);
    double* wss = (double*)(w + p.wss);
    double* llr = (double*)(w + p.llr);
    double* seg = (double*)(w + p.seg);
    double* x10 = (double*)(w + p.x10);
    double* y10 = (double*)(w + p.y10);
    double* level = (double*)(w + p.level);
    int* src = (int*)(w + p.src);
    int* kept = (int*)(w + p.kept);
    double* env = (double*)(w + p.env);
    double* corr = (double*)(w + p.corr);
    double* clip = (double*)(w + p.clip);
    const LaunchCtx ctx = begin(h, stream);
    hipStream_t s = ctx.stream;
    const double clipc = std::pow(10.0, -(-15.0) / 20.0);          // 10 ** (-beta / 20), beta = -15
    CriticalBands cb;
    for (int i = 0; i < MT_NB; ++i) { cb.centre[i] = CB_CENTRE[i]; cb.width[i] = CB_WIDTH[i]; }
    LAUNCH(ctx, "metrics_tables", metrics_tables<<<1, MT_TPB, 0, s>>>(fs, cb, tb));
    FrameArgs fa{clean, enh, offset, L, p.nf, p.nfw, p.nfl, tb, wss, llr, seg, frames};
    LAUNCH(ctx, "metrics_frames", metrics_frames<<<dim3(p.nf, B), MT_TPB, 0, s>>>(fa, fs));
    LAUNCH(ctx, "metrics_resample", metrics_resample<<<dim3((p.N10 + MT_TPB - 1) / MT_TPB, B, 2), MT_TPB, 0, s>>>(
                                        clean, enh, offset, L, p.N10, fs, tb, x10, y10));
    LAUNCH(ctx, "metrics_stoi_level", metrics_stoi_level<<<dim3(p.nS, B), MT_STOI_N, 0, s>>>(x10, p.N10, p.nS, tb, level));
    ClipArgs ca{clean, enh, offset, L, p.nf, p.nfw, p.nfl, p.kw, p.kl, p.nS, wss, llr, seg, level, src, kept, clip};
    LAUNCH(ctx, "metrics_clip", metrics_clip<<<dim3(B, 3), MT_TPB, 0, s>>>(ca));
    LAUNCH(ctx, "metrics_stoi_env", metrics_stoi_env<<<dim3(p.nS, B), MT_TPB, 0, s>>>(x10, y10, p.N10, p.nS, src, kept,
                                                                                      tb, env, B));
    LAUNCH(ctx, "metrics_stoi_corr", metrics_stoi_corr<<<dim3(p.nS - MT_STOI_SEG, B), 64, 0, s>>>(env, p.nS, kept, tb,
                                                                                                  clipc, corr, B));
    LAUNCH(ctx, "metrics_finalize", metrics_finalize<<<B, MT_TPB, 0, s>>>(corr, p.nS, kept, clip, pesq, scores));
    return check_launch(h, "metrics");
}

extern "C" int cmgan_metrics_table(int fs, int which, double* out, size_t cap) {
    Geom g;
    if (!geom_of(fs, g)) return fail(nullptr, CMGAN_E_UNSUPPORTED, "cmgan_metrics_table: fs must be 16000 or 8000");
    std::vector<double> v;
    switch (which) {
    case 0:
        for (int n = 0; n < g.win; ++n) v.push_back(taper_value(g.win, n));
        break;
    case 1: {
        v.assign(2 * MT_NB + MT_NB * MT_BANKW, 0.0);
        for (int b = 0; b < MT_NB; ++b) {
            int f, c;
            bank_band(CB_CENTRE, CB_WIDTH, fs, g.half, b, &f, &c, v.data() + 2 * MT_NB + b * MT_BANKW);
            v[b] = f;
            v[MT_NB + b] = c;
        }
        break;
    }
    case 2:
        v.resize(1 + 2 * MT_STOI_J);
        for (int k = 0; k < MT_STOI_J; ++k) stoi_band(k, v.data());
        v.resize(1 + 2 * stoi_kept(v.data()));
        break;
    case 3:
        for (int m = 0; m < MT_STOI_N; ++m) v.push_back(hann_inner(MT_STOI_N, m));
        break;
    case 4:
        v.resize(g.fir_len);
        fir_taps(g, v.data());
        break;
    default:
        return fail(nullptr, CMGAN_E_BADARG, "cmgan_metrics_table: which must be 0..4");
    }
    if (!out) return (int)v.size();
    if (cap < v.size()) return fail(nullptr, CMGAN_E_BADARG, "cmgan_metrics_table: cap %zu < %zu", cap, v.size());
    for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
    return (int)v.size();
}
