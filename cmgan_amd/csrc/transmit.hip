// transmit.hip - what a telephone or VoIP link does to a [B, L] float32 batch on the device (cmgan_transmit,
// include/cmgan_hip.h, "Transmission"): a codec per row (16-bit PCM, G.711 mu-law or A-law), frames that are lost, and a
// receiver that covers the holes by repeating the last pitch period (after G.711 Appendix I, simplified so that every
// step is stated) or leaves them as gaps.  The reference has no counterpart: its data path replays fixed pairs
// (src/data/dataloader.py).  For row b with n = lengths[b] (L without lengths), F = frame, K = ceil(n / F):
//
//   z[i] = codec(x[i])                 0: x bit for bit; 1 .. 3 from q = sat16(rint(x 32768)) (half to even, NaN -> 0):
//                                      q / 32768, ulaw2lin(lin2ulaw(q)) / 32768, alaw2lin(lin2alaw(q)) / 32768
//   y = z; every maximal run of lost frames k0 .. k1 - 1 (s = k0 F, e = min(k1 F, n)) in ascending order, with h(i) = y[i]
//   as it stands (earlier concealment included) and 0 for i < 0:
//     plc 0:  y[s .. e) = 0
//     plc 1:  P    = the lag in pmin .. pmax with the largest 2 C - E, C = sum_{i<W} h(s-W+i) h(s-W-P+i), E = sum_{i<W}
//                    h(s-W-P+i)^2: float64 sums in ascending i; NaN counts as -inf; the smallest P among equal maxima
//             v[i] = h(s-P+i) for i < P - Q, Q = floor(P / 4); fl(1-t) h(s-P+i) + t h(s-2P+i), t = (i-(P-Q)+1) / (Q+1), from there
//             g(j) = min(1, max(0, (6A - j) / (5A)))
//             y[s+j] = f32(g(j) v[j mod P]) for j < e - s;  and if e < n, with R = min(Q, F, n-e), M = e - s, t = (i+1) / (R+1):
//             y[e+i] = f32(fl(1-t) g(M+i) v[(M+i) mod P] + t z[e+i]) for i < R
//
// Two launches, no workspace, no atomics.  transmit_codec is elementwise over the batch and byte-bound (8 bytes per
// sample); it also writes the zeros of an INVALID row and of the samples from n on.  The concealment is a serial chain
// along a row - a later loss conceals from a history that may itself be concealed - so in transmit_conceal ONE block
// owns a row and walks its runs, as stretch_rows walks its frames: a batch of 32 rows keeps 32 compute units busy and
// no more.  It works on y alone (z[e+i] of the fade back is y[e+i] as the codec launch left it: frame k1 is good, and
// no earlier run reaches it), so in place and out of place are one path.  A run stages the W + pmax history samples in
// LDS as float64 (16 KB at most; v takes 8 KB more); every lag has a thread of its own that runs both sums in one
// ascending chain of fused multiply-adds (a product of two float32 values is exact in float64, so the sums are those
// of the unfused definition, bit for bit, and P can be compared for equality with a host model); neighbouring threads
// read consecutive LDS words for h(s-W-P+i), and h(s-W+i) is a broadcast.  The best (score, P) of the block is found by
// wave shuffles and one LDS step; the order on that key is total, so the winner does not depend on the order of the
// reduction.  The block's own earlier writes to y are read back after __syncthreads().  Samples from n on and table
// columns from K on are never read.  A row's bits depend on its own samples, tables and length alone.
#include <math.h>
#include <stdint.h>

#include "api_internal.h"

namespace {

constexpr int TX_TPB = 256;                 // threads of transmit_conceal: pmax - pmin + 1 = 161 lags at the defaults in one pass
constexpr int TX_WAVES = TX_TPB / 64;
constexpr int TX_EW_TPB = 256, TX_EW_RUN = 4;      // transmit_codec: a block converts TX_EW_TPB x TX_EW_RUN samples of one row
constexpr int TX_MIN_FRAME = 16, TX_MAX_FRAME = 4096;
constexpr int TX_MIN_LAG = 16, TX_MAX_LAG = 1024;
constexpr int TX_MIN_WINDOW = 16, TX_MAX_WINDOW = 1024;
constexpr int TX_NO_LAG = 0x7fffffff;       // the lag of "no candidate yet": behind every real one
static_assert(TX_MAX_LAG / 4 <= TX_TPB, "the fade back (R <= pmax / 4 samples) is one sample per thread");

struct TransmitArgs {
    const float* x;
    float* y;
    const int* lengths;          // null: every row has L samples
    const unsigned char* lost;   // [B, ldl]
    const int* codec;            // [B]
    const int* plc;              // [B]
    int* status;                 // [B] or null
    int* lag;                    // [B, ldl] or null
    long long ldx, ldy, ldl;
    int B, L, F, pmin, pmax, W, A;
};

__device__ inline bool tx_row_ok(int n, int L, int codec, int plc) {
    return n >= 0 && n <= L && codec >= 0 && codec <= 3 && plc >= 0 && plc <= 1;
}

// q = sat16(rint(x 32768)): the product is exact (or an infinity), rintf rounds half to even, NaN gives 0
__device__ inline int tx_quantise(float x) {
    float s = x * 32768.0f;
    if (!(s == s)) return 0;
    s = fminf(fmaxf(s, -32768.0f), 32767.0f);
    return (int)rintf(s);
}

// G.711 mu-law at 16 bits, there and back (audioop's lin2ulaw / ulaw2lin at width 2): the 14-bit magnitude, clipped and
// biased, has its segment in its bit length
__device__ inline int tx_ulaw(int q) {
    const int v = q >> 2;
    const bool neg = v < 0;
    const int m = min(neg ? -v : v, 8159) + 33;
    const int seg = 26 - __clz(m);                                      // bit length - 6; m >= 33
    const int code = seg >= 8 ? 0x7F : ((seg << 4) | ((m >> (seg + 1)) & 0xF));     // (before the complement, sign apart)
    const int t = (((code & 0xF) << 3) + 0x84) << (code >> 4);
    return neg ? 0x84 - t : t - 0x84;
}

// G.711 A-law at 16 bits, there and back (audioop's lin2alaw / alaw2lin at width 2), on the 13-bit value
__device__ inline int tx_alaw(int q) {
    const int v = q >> 3;
    const bool neg = v < 0;
    const int m = neg ? -v - 1 : v;
    const int seg = max(27 - __clz(m | 1), 0);                          // bit length - 5, 0 for m < 32
    const int mant = (m >> (seg < 2 ? 1 : seg)) & 0xF;
    int t = mant << 4;
    t = seg == 0 ? t + 8 : (seg == 1 ? t + 0x108 : (t + 0x108) << (seg - 1));
    return neg ? -t : t;
}

__device__ inline float tx_codec(float x, int codec) {
    if (codec == 0) return x;
    int q = tx_quantise(x);
    if (codec == 2) q = tx_ulaw(q);
    else if (codec == 3) q = tx_alaw(q);
    return (float)q * (1.0f / 32768.0f);                                // |q| < 2^16: exact
}

__global__ __launch_bounds__(TX_EW_TPB) void transmit_codec(TransmitArgs a) {
    const int b = blockIdx.y;
    const int n = a.lengths ? a.lengths[b] : a.L;
    const int codec = a.codec[b];
    const bool valid = tx_row_ok(n, a.L, codec, a.plc[b]);
    const float* row = a.x + (size_t)b * a.ldx;
    float* out = a.y + (size_t)b * a.ldy;
    const long long i0 = (long long)blockIdx.x * (TX_EW_TPB * TX_EW_RUN) + threadIdx.x;
#pragma unroll
    for (int r = 0; r < TX_EW_RUN; ++r) {
        const long long i = i0 + (long long)r * TX_EW_TPB;
        if (i >= a.L) break;
        out[i] = (valid && i < n) ? tx_codec(row[i], codec) : 0.0f;     // samples from n on are never read
    }
}

// (score a, lag pa) is better than (b, pb): the larger score, and among equal scores the smaller lag
__device__ inline bool tx_better(double a, int pa, double b, int pb) { return a > b || (a == b && pa < pb); }

// g(j): the numerator is an exact integer, one IEEE division
__device__ inline double tx_gain(long long j, double six_a, double five_a) {
    const double g = (six_a - (double)j) / five_a;
    return fmin(1.0, fmax(0.0, g));
}

__global__ __launch_bounds__(TX_TPB) void transmit_conceal(TransmitArgs a) {
    __shared__ double s_h[TX_MAX_WINDOW + TX_MAX_LAG];                  // h(s - W - pmax .. s)
    __shared__ double s_v[TX_MAX_LAG];                                  // the pitch period that is repeated
    __shared__ unsigned long long s_lost[TX_WAVES];                     // the table columns of the chunk being walked, a bit each
    __shared__ double s_score[TX_WAVES];
    __shared__ int s_lag[TX_WAVES];
    const int t = threadIdx.x, b = blockIdx.x, F = a.F, W = a.W, pmin = a.pmin, pmax = a.pmax;
    float* row = a.y + (size_t)b * a.ldy;
    const unsigned char* lost = a.lost + (size_t)b * a.ldl;
    int* lag = a.lag ? a.lag + (size_t)b * a.ldl : nullptr;
    const int n = a.lengths ? a.lengths[b] : a.L;
    const int plc = a.plc[b];
    const bool valid = tx_row_ok(n, a.L, a.codec[b], plc);
    if (t == 0 && a.status) a.status[b] = valid ? 0 : 1;
    const long long K = valid ? ((long long)n + F - 1) / F : 0;
    // every lag starts as 0 (-1 from K on); the thread that wrote lag[k0] is the one that overwrites it with P
    if (lag)
        for (long long k = t; k < a.ldl; k += TX_TPB) lag[k] = k < K ? 0 : -1;
    const double six_a = 6.0 * (double)a.A, five_a = 5.0 * (double)a.A;

    long long k0 = -1;                                                  // the first frame of the run being collected, or -1
    for (long long c0 = 0; c0 <= K; c0 += TX_TPB) {                     // (c0 == K: one more round closes a run that ends at K)
        __syncthreads();                                                // the previous chunk has been walked
        const bool flag = c0 + t < K && lost[c0 + t] != 0;
        const unsigned long long wave_bits = __ballot(flag);
        if ((t & 63) == 0) s_lost[t >> 6] = wave_bits;
        __syncthreads();
        for (int w = 0; w < TX_WAVES && c0 + 64 * w <= K; ++w) {
            const unsigned long long bits = s_lost[w];                  // bit j: frame base + j is lost; frames from K on read as good
            const long long base = c0 + 64 * w;
            int at = 0;
            while (at < 64) {
                const unsigned long long rest = (k0 < 0 ? bits : ~bits) >> at;     // the next lost frame, or the next good one
                if (!rest) break;
                at += __builtin_ctzll(rest);
                if (k0 < 0) {
                    k0 = base + at;
                    continue;
                }
                // ---- the run k0 .. k - 1 (frame k is good, or k == K)
                const long long k = base + at, kr = k0, s = kr * F, e = min(k * (long long)F, (long long)n);
                const long long M = e - s;
                k0 = -1;
                if (plc == 0) {
                    for (long long i = s + t; i < e; i += TX_TPB) row[i] = 0.0f;
                    continue;
                }
                __syncthreads();                                        // earlier runs' samples are in y; s_h and s_v are free
                const long long h0 = s - W - pmax;
                for (int i = t; i < W + pmax; i += TX_TPB) {
                    const long long src = h0 + i;
                    s_h[i] = src >= 0 ? (double)row[src] : 0.0;
                }
                // z[e + t] of the fade back, asked for now and used last: R <= pmax / 4 <= TX_TPB, one sample per thread
                const float zf = (t < (pmax >> 2) && t < F && e + t < n) ? row[e + t] : 0.0f;
                __syncthreads();
                double best = -INFINITY;
                int best_lag = TX_NO_LAG;
                const double* pa = s_h + pmax;                          // h(s - W + i)
                for (int P = pmin + t; P <= pmax; P += TX_TPB) {
                    const double* pb = s_h + (pmax - P);                // h(s - W - P + i)
                    double C = 0.0, E = 0.0;
#pragma unroll 4
                    for (int i = 0; i < W; ++i) {                       // one ascending chain per sum
                        const double u = pb[i];
                        C = fma(pa[i], u, C);
                        E = fma(u, u, E);
                    }
                    double sc = 2.0 * C - E;
                    if (!(sc == sc)) sc = -INFINITY;
                    if (tx_better(sc, P, best, best_lag)) {
                        best = sc;
                        best_lag = P;
                    }
                }
                for (int m = 32; m >= 1; m >>= 1) {
                    const double os = __shfl_xor(best, m);
                    const int ol = __shfl_xor(best_lag, m);
                    if (tx_better(os, ol, best, best_lag)) {
                        best = os;
                        best_lag = ol;
                    }
                }
                if ((t & 63) == 0) {
                    s_score[t >> 6] = best;
                    s_lag[t >> 6] = best_lag;
                }
                __syncthreads();
                best = s_score[0];
                best_lag = s_lag[0];
                for (int v = 1; v < TX_WAVES; ++v)
                    if (tx_better(s_score[v], s_lag[v], best, best_lag)) {
                        best = s_score[v];
                        best_lag = s_lag[v];
                    }
                const int P = best_lag;                                 // pmin is always a candidate, so a lag was found
                const int Q = P >> 2;
                if (lag && t == (int)(kr % TX_TPB)) lag[kr] = P;
                // ---- the period: the last P samples, their last quarter cross-faded into the period before
                const int hp = W + pmax - P;                            // s_h[hp + i] = h(s - P + i)
                for (int i = t; i < P; i += TX_TPB) {
                    double v = s_h[hp + i];
                    if (i >= P - Q) {
                        const double f = (double)(i - (P - Q) + 1) / (double)(Q + 1);
                        const int j = hp - P + i;                       // h(s - 2 P + i): staged, unless W < P + Q - i
                        const long long src = s - 2LL * P + i;
                        const double u = j >= 0 ? s_h[j] : (src >= 0 ? (double)row[src] : 0.0);
                        v = fma(f, u, (1.0 - f) * v);                    // fused by name: the bits do not hang on the build's contraction
                    }
                    s_v[i] = v;
                }
                __syncthreads();
                // ---- fill, then fade back into the good frame behind the run
                const int Mi = (int)M;                                  // M <= n < 2^31
                for (int jj = t; jj < Mi; jj += TX_TPB) row[s + jj] = (float)(tx_gain(jj, six_a, five_a) * s_v[jj % P]);
                const int R = e < n ? (int)min((long long)min(Q, F), (long long)n - e) : 0;
                if (t < R) {
                    const double f = (double)(t + 1) / (double)(R + 1);
                    const double c = tx_gain(M + t, six_a, five_a) * s_v[(int)((M + t) % P)];
                    row[e + t] = (float)fma(f, (double)zf, (1.0 - f) * c);
                }
            }
        }
    }
}

}  // namespace

extern "C" int cmgan_transmit_max_lag(void) { return TX_MAX_LAG; }

extern "C" int cmgan_transmit_max_window(void) { return TX_MAX_WINDOW; }

extern "C" int cmgan_transmit(cmgan_handle* h, const float* x, int B, int L, long long ldx, const int* lengths,
                              const unsigned char* lost, long long ldl, const int* codec, const int* plc, int frame, int pmin,
                              int pmax, int window, int fade, float* y, long long ldy, int* status, int* lag, void* stream) {
    // every argument is judged before the handle is, so that the errors below need no GPU (the message of a call
    // without a handle is read with cmgan_last_error(NULL))
    if (!x || !lost || !codec || !plc || !y) return fail(h, CMGAN_E_BADARG, "cmgan_transmit: null pointer");
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)lengths | (uintptr_t)codec | (uintptr_t)plc | (uintptr_t)status |
         (uintptr_t)lag) & 3)
        return fail(h, CMGAN_E_BADARG, "cmgan_transmit: float32 / int32 buffers must be 4-byte aligned");
    if (B < 1 || B > 65535 || L < 1 || ldx < L || ldy < L)
        return fail(h, CMGAN_E_BADARG, "cmgan_transmit: need 1 <= B <= 65535, L >= 1, ldx >= L, ldy >= L (B=%d L=%d ldx=%lld "
                    "ldy=%lld)", B, L, ldx, ldy);
    if (frame < TX_MIN_FRAME || frame > TX_MAX_FRAME)
        return fail(h, CMGAN_E_BADARG, "cmgan_transmit: frame must lie in [%d, %d] (frame=%d)", TX_MIN_FRAME, TX_MAX_FRAME, frame);
    if (pmin < TX_MIN_LAG || pmin > pmax || pmax > TX_MAX_LAG)
        return fail(h, CMGAN_E_BADARG, "cmgan_transmit: need %d <= pmin <= pmax <= %d (pmin=%d pmax=%d)", TX_MIN_LAG, TX_MAX_LAG,
                    pmin, pmax);
    if (window < TX_MIN_WINDOW || window > TX_MAX_WINDOW)
        return fail(h, CMGAN_E_BADARG, "cmgan_transmit: window must lie in [%d, %d] (window=%d)", TX_MIN_WINDOW, TX_MAX_WINDOW,
                    window);
    if (fade < 1) return fail(h, CMGAN_E_BADARG, "cmgan_transmit: fade must be >= 1 (fade=%d)", fade);
    if (ldl < ((long long)L + frame - 1) / frame)
        return fail(h, CMGAN_E_BADARG, "cmgan_transmit: ldl must be at least ceil(L / frame) = %lld (ldl=%lld)",
                    ((long long)L + frame - 1) / frame, ldl);
    if (!((const float*)y == x && ldy == ldx)) {                       // in place is the one overlap there may be
        const uintptr_t x0 = (uintptr_t)x, x1 = x0 + ((size_t)(B - 1) * (size_t)ldx + (size_t)L) * sizeof(float);
        const uintptr_t y0 = (uintptr_t)y, y1 = y0 + ((size_t)(B - 1) * (size_t)ldy + (size_t)L) * sizeof(float);
        if (x0 < y1 && y0 < x1)
            return fail(h, CMGAN_E_BADARG, "cmgan_transmit: x and y overlap; only y == x with ldy == ldx (in place) is allowed");
    }
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "cmgan_transmit: null handle");
    const LaunchCtx ctx = begin(h, stream);
    TransmitArgs a;
    a.x = x;
    a.y = y;
    a.lengths = lengths;
    a.lost = lost;
    a.codec = codec;
    a.plc = plc;
    a.status = status;
    a.lag = lag;
    a.ldx = ldx;
    a.ldy = ldy;
    a.ldl = ldl;
    a.B = B;
    a.L = L;
    a.F = frame;
    a.pmin = pmin;
    a.pmax = pmax;
    a.W = window;
    a.A = fade;
    const unsigned tiles = (unsigned)(((long long)L + TX_EW_TPB * TX_EW_RUN - 1) / (TX_EW_TPB * TX_EW_RUN));
    LAUNCH(ctx, "transmit_codec", transmit_codec<<<dim3(tiles, B), TX_EW_TPB, 0, ctx.stream>>>(a));
    LAUNCH(ctx, "transmit_conceal", transmit_conceal<<<dim3(B), TX_TPB, 0, ctx.stream>>>(a));
    return check_launch(h, "transmit");
}
