// rir_tail.hip - the diffuse reverberant tail behind the early part of a room impulse response (cmgan_rir_tail,
// include/cmgan_hip.h): every row of a float32 [R, K] bank such as cmgan_rir / cmgan_rir_bands make is extended in place,
// from its junction k_x = clamp(len[r], 1, K) to k_end = clamp(n_taps[r], 1, K), by noise under an exponential envelope
// that follows the caller's 60 dB decay time band by band, its level fitted to the W samples in front of the junction.
// The reference ships no impulse responses and no simulator (src/data/dataloader.py:13-50 replays pairs mixed beforehand).
// With NB' = max(NB, 1) bands (NB = 0: one band, g = {1}, D = 0), D = (NF - 1) / 2 and delta_b = 3 ln 10 / (decay[r][b] fs):
//
//   nu[q]  = (w0 + w1 + w2 + w3 - 2 (2^32 - 1)) / sqrt((2^64 - 1) / 3), (w0 .. w3) = Philox4x32-10 at counter (q, 0, 0, 0) under
//            the key seed[r]; nu[q] = 0 for q < 0.  The numerator is an integer below 2^34, the division is IEEE's
//   z_b[k] = sum_j g_b[j] h[k + D - j] on the window k_x - D - W <= k < k_x - D (j ascending, one fma per term, h = 0 outside
//            [0, k_x));  E_b = sum_k z_b[k]^2,  G_b = sum_j g_b[j]^2,  S_b = sum_k exp(-2 delta_b (k - k_x))
//   A_b    = sqrt(E_b / (G_b S_b)), 0 where E_b = 0
//   y[k]   = sum_b sum_j g_b[j] (A_b exp(-delta_b (q - k_x)) nu[q]), q = k + D - j, for k_x <= k < k_end: b ascending, then j
//            ascending, one fma per term into one accumulator from 0, the bracket rounded as (A_b exp(..)) nu
//
// Float64 on the VALU, no atomics, two launches:
//   rir_tail_fit   grid (band, row), one block each.  It judges the row (every block of a row reaches the same verdict from
//                  the same reads), stages the W + NF - 1 samples the window reaches as float32 and the band's taps in LDS;
//                  thread t computes z_b[k] for the window's samples t, t + 256, ... and adds their squares (one fma each)
//                  and the envelope terms of S_b in that ascending order, and the squares of the taps t, t + 256, ... alike;
//                  thread 0 folds the 256 partials of each of the three sums in ascending thread order and writes A_b.  The
//                  block of band 0 writes the row's status and, to the workspace, its junction (0: leave the row alone) -
//                  the second launch writes len[r], so it must not read its k_x from there.
//   rir_tail_taps  grid (tile of RT_TILE = 256 outputs, row), one output per thread.  nu is computed once for the
//                  RT_TILE + NF - 1 indices the tile's outputs reach: one Philox block per index, never one per (index,
//                  band).  Band after band the block stages e_b[q] = (A_b exp(-delta_b (q - k_x))) nu[q] for that span, one
//                  exp per element, and the band's taps; a thread then runs its NF fmas, consecutive threads reading
//                  consecutive float64 and the tap being a broadcast.  Tiles wholly below k_x do nothing, tiles wholly
//                  at or above k_end write their zeros.
// A row's bits depend on its own samples, lengths, decay times and seed alone: neither on R, nor on the other rows, nor on
// ld, nor on K beyond k_end.  Nothing read from device memory becomes an address without a clamp: k_x and k_end are clamped
// to [1, K], the window is used only where it starts at or after 0, and taps are written below K only.
#include <math.h>
#include <stdint.h>

#include "api_internal.h"
#include "host_ranges.h"
#include "philox.hip.h"

namespace {

constexpr int RT_TPB = 256;                   // threads of both kernels
constexpr int RT_TILE = RT_TPB;               // outputs per block of the taps kernel
constexpr int RT_MAX_K = 65536;               // longest response (the limit of cmgan_rir)
constexpr int RT_MAX_BANDS = 8;               // = cmgan_rir_max_bands()
constexpr int RT_MAX_FILTER = 1023;           // = cmgan_rir_max_filter()
constexpr int RT_MAX_WINDOW = 4096;           // longest fit window
constexpr int RT_FIT_SPAN = RT_MAX_WINDOW + RT_MAX_FILTER - 1;
constexpr int RT_SPAN = RT_TILE + RT_MAX_FILTER - 1;
constexpr double RT_3LN10 = CMGAN_RIR_TAIL_3LN10;
constexpr double RT_NOISE_DIV = CMGAN_RIR_TAIL_NOISE_DIV;

struct TailArgs {
    float* rir;
    int* len;                // in: the junction; out: the extended length
    const int* n_taps;
    const double* decay;     // [R][NBp]
    const long long* seed;   // [R]
    const double* filt;      // [NB][NF] or null
    int* status;             // [R]
    double* gain;            // [R][NBp]
    int* kx;                 // workspace [R]: the junction of a row that is extended, 0 for a row left alone
    long long ld;
    double fs;
    int R, K, NBp, NF, W;    // NBp = max(NB, 1); NF = 1 without a filterbank
};

__device__ inline int rt_clamp(int v, int K) { return v < 1 ? 1 : (v > K ? K : v); }

__device__ inline double rt_delta(double decay, double fs) { return RT_3LN10 / (decay * fs); }

__device__ inline double rt_noise(int q, unsigned k0, unsigned k1) {
    if (q < 0) return 0.0;
    unsigned c[4] = {(unsigned)q, 0u, 0u, 0u};
    philox4x32_10(c, k0, k1);
    const long long sum = (long long)c[0] + (long long)c[1] + (long long)c[2] + (long long)c[3] - 2LL * 4294967295LL;
    return (double)sum / RT_NOISE_DIV;
}

// ---------------------------------------------------------------- the fit kernel
__global__ __launch_bounds__(RT_TPB) void rir_tail_fit(TailArgs a) {
    __shared__ float s_h[RT_FIT_SPAN];
    __shared__ double s_g[RT_MAX_FILTER], s_e[RT_TPB], s_s[RT_TPB], s_q[RT_TPB];
    const int t = threadIdx.x, b = blockIdx.x, r = blockIdx.y;
    const int NF = a.NF, D = (NF - 1) / 2, W = a.W;
    const int kx = rt_clamp(a.len[r], a.K), kend = rt_clamp(a.n_taps[r], a.K);
    const int k_lo = kx - D - W;                                  // the window's first sample
    int status = 0;
    if (kend <= kx) status |= CMGAN_RIR_TAIL_NOTHING;
    if (k_lo < 0) status |= CMGAN_RIR_TAIL_WINDOW;
    for (int i = 0; i < a.NBp; ++i) {
        const double d = a.decay[(size_t)r * a.NBp + i];
        if (!(d > 0.0) || !(d - d == 0.0)) status |= CMGAN_RIR_TAIL_DECAY;
    }
    const float* row = a.rir + (size_t)r * a.ld;
    const int span = W + NF - 1, base = k_lo - D;                 // s_h[i] = h[base + i]; base + span = k_x
    if (k_lo >= 0) {                                              // (the whole block)
        int bad = 0;
        for (int i = t; i < span; i += RT_TPB) {
            const int q = base + i;
            const float v = q >= 0 ? row[q] : 0.f;                // q < k_x <= K
            bad |= (v - v == 0.f) ? 0 : 1;
            s_h[i] = v;
        }
        if (__syncthreads_or(bad)) status |= CMGAN_RIR_TAIL_NONFINITE;
    }
    if (status) {                                                 // (the whole block)
        if (t == 0) {
            a.gain[(size_t)r * a.NBp + b] = 0.0;
            if (b == 0) a.status[r] = status, a.kx[r] = 0;
        }
        return;
    }
    if (a.filt) {
        const double* g = a.filt + (size_t)b * NF;
        for (int i = t; i < NF; i += RT_TPB) s_g[i] = g[i];
    } else if (t == 0) {
        s_g[0] = 1.0;
    }
    __syncthreads();
    const double delta = rt_delta(a.decay[(size_t)r * a.NBp + b], a.fs);
    double e = 0.0, s = 0.0, gg = 0.0;
    for (int m = t; m < W; m += RT_TPB) {                         // k = k_lo + m: h[k + D - j] = s_h[m + 2 D - j]
        const float* hp = s_h + m + NF - 1;
        double z = 0.0;
        for (int j = 0; j < NF; ++j) z = fma(s_g[j], (double)hp[-j], z);
        e = fma(z, z, e);
        s += exp(-2.0 * delta * (double)(k_lo + m - kx));
    }
    for (int j = t; j < NF; j += RT_TPB) gg = fma(s_g[j], s_g[j], gg);
    s_e[t] = e, s_s[t] = s, s_q[t] = gg;
    __syncthreads();
    if (t != 0) return;
    double E = 0.0, S = 0.0, G = 0.0;
    for (int i = 0; i < RT_TPB; ++i) E += s_e[i], S += s_s[i], G += s_q[i];
    a.gain[(size_t)r * a.NBp + b] = E == 0.0 ? 0.0 : sqrt(E / (G * S));
    if (b == 0) a.status[r] = 0, a.kx[r] = kx;
}

// ---------------------------------------------------------------- the taps kernel
__global__ __launch_bounds__(RT_TPB) void rir_tail_taps(TailArgs a) {
    __shared__ double s_nu[RT_SPAN], s_e[RT_SPAN], s_g[RT_MAX_FILTER];
    const int t = threadIdx.x, r = blockIdx.y;
    const int k0 = blockIdx.x * RT_TILE, k = k0 + t;
    const int kx = a.kx[r];                                       // the first launch's clamp(len[r], 1, K), or 0
    if (kx < 1 || kx > a.K) return;                               // (the whole block: the row is left alone)
    const int kend = rt_clamp(a.n_taps[r], a.K);                  // > k_x: the first launch judged it
    float* out = a.rir + (size_t)r * a.ld;
    if (blockIdx.x == 0 && t == 0) a.len[r] = kend > kx ? kend : kx;
    if (k0 + RT_TILE <= kx) return;                               // (the whole block: these taps stay)
    if (k0 >= kend) {                                             // (the whole block: nothing of this tile is a tap)
        if (k < a.K) out[k] = 0.f;
        return;
    }
    const int NF = a.NF, D = (NF - 1) / 2, span = RT_TILE + NF - 1, base = k0 - D;    // s_nu[i] = nu[base + i]
    const unsigned long long key = (unsigned long long)a.seed[r];
    for (int i = t; i < span; i += RT_TPB) s_nu[i] = rt_noise(base + i, (unsigned)key, (unsigned)(key >> 32));
    const bool tap = k >= kx && k < kend;
    double acc = 0.0;
    for (int b = 0; b < a.NBp; ++b) {
        __syncthreads();                                          // s_nu is written; the last band's reads are over
        const double A = a.gain[(size_t)r * a.NBp + b];
        const double delta = rt_delta(a.decay[(size_t)r * a.NBp + b], a.fs);
        for (int i = t; i < span; i += RT_TPB) s_e[i] = (A * exp(-delta * (double)(base + i - kx))) * s_nu[i];
        if (a.filt) {
            const double* g = a.filt + (size_t)b * NF;
            for (int i = t; i < NF; i += RT_TPB) s_g[i] = g[i];
        } else if (t == 0) {
            s_g[0] = 1.0;
        }
        __syncthreads();
        if (tap) {
            const double* ep = s_e + t + NF - 1;                  // q = k + D - j: s_e[t + 2 D - j]
            for (int j = 0; j < NF; ++j) acc = fma(s_g[j], ep[-j], acc);
        }
    }
    if (k >= kx && k < a.K) out[k] = tap ? (float)acc : 0.f;
}

// ---------------------------------------------------------------- the host side
inline bool rt_shape_ok(int R, int K, int NB, int NF) {
    return R >= 1 && R <= 65535 && K >= 1 && K <= RT_MAX_K && NB >= 0 && NB <= RT_MAX_BANDS && NF >= 1 && NF <= RT_MAX_FILTER
        && (NF & 1);
}

}  // namespace

extern "C" int cmgan_rir_tail_tile(void) { return RT_TILE; }
extern "C" int cmgan_rir_tail_max_window(void) { return RT_MAX_WINDOW; }

extern "C" size_t cmgan_rir_tail_workspace_bytes(const cmgan_handle*, int R, int K, int NB, int NF) {
    return rt_shape_ok(R, K, NB, NF) ? up256((size_t)R * sizeof(int)) : 0;
}

extern "C" int cmgan_rir_tail(cmgan_handle* h, float* rir, int R, int K, long long ld, int* len, const int* n_taps,
                              const double* decay, const long long* seed, const double* filt, int NB, int NF, int window,
                              int fs, int* status, double* gain, void* ws, size_t ws_bytes, void* stream) {
    // every argument is judged before the handle is, so that the errors below need no GPU (the message of a call
    // without a handle is read with cmgan_last_error(NULL))
    if (!rir || !len || !n_taps || !decay || !seed || !status || !gain)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_tail: null pointer");
    if (((uintptr_t)rir | (uintptr_t)len | (uintptr_t)n_taps | (uintptr_t)status) & 3)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_tail: float32 / int32 buffers must be 4-byte aligned");
    if (((uintptr_t)decay | (uintptr_t)seed | (uintptr_t)filt | (uintptr_t)gain) & 7)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_tail: float64 / int64 buffers must be 8-byte aligned");
    if (R < 1 || R > 65535 || K < 1 || ld < K)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_tail: need 1 <= R <= 65535, K >= 1, ld >= K (R=%d K=%d ld=%lld)", R, K, ld);
    if (NB < 0 || NB > RT_MAX_BANDS)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_tail: need 0 <= NB <= %d bands (NB=%d)", RT_MAX_BANDS, NB);
    if ((NB == 0) != (filt == nullptr))
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_tail: the filter table must be null with NB = 0 and only then (NB=%d)", NB);
    if (NF < 1 || !(NF & 1))
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_tail: the filter length must be odd and >= 1 (NF=%d)", NF);
    if (window < 1 || window > RT_MAX_WINDOW)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_tail: the window must have 1 .. %d samples (window=%d)", RT_MAX_WINDOW, window);
    if (fs < 1) return fail(h, CMGAN_E_BADARG, "cmgan_rir_tail: fs must be positive (fs=%d)", fs);
    if (K > RT_MAX_K)
        return fail(h, CMGAN_E_UNSUPPORTED, "cmgan_rir_tail: responses of up to %d taps are supported (K=%d)", RT_MAX_K, K);
    if (NF > RT_MAX_FILTER)
        return fail(h, CMGAN_E_UNSUPPORTED, "cmgan_rir_tail: filters of up to %d taps are supported (NF=%d)", RT_MAX_FILTER, NF);
    const size_t need = up256((size_t)R * sizeof(int));
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < need)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_tail: the workspace must be 256-byte aligned and hold %zu bytes (%zu given)",
                    need, ws ? ws_bytes : (size_t)0);
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "cmgan_rir_tail: null handle");
    const LaunchCtx ctx = begin(h, stream);
    hipStream_t s = ctx.stream;
    TailArgs a;
    a.rir = rir;
    a.len = len;
    a.n_taps = n_taps;
    a.decay = decay;
    a.seed = seed;
    a.filt = filt;
    a.status = status;
    a.gain = gain;
    a.kx = (int*)ws;
    a.ld = ld;
    a.fs = (double)fs;
    a.R = R, a.K = K, a.NBp = NB > 0 ? NB : 1, a.NF = filt ? NF : 1, a.W = window;
    LAUNCH(ctx, "rir_tail_fit", rir_tail_fit<<<dim3(a.NBp, R), RT_TPB, 0, s>>>(a));
    LAUNCH(ctx, "rir_tail_taps", rir_tail_taps<<<dim3((K + RT_TILE - 1) / RT_TILE, R), RT_TPB, 0, s>>>(a));
    return check_launch(h, "rir_tail");
}
