// rir_stats.hip - what a room impulse response measures as, on the device (cmgan_rir_stats, include/cmgan_hip.h): the
// Schroeder decay curve and the room-acoustic parameters of ISO 3382-1 as its published description gives them - EDT, T20,
// T30, DRR, C50, C80, D50, Ts - broad-band and in the bands of a caller-supplied FIR filterbank, for every row of a
// float32 [R, K] bank such as cmgan_rir / cmgan_rir_bands make.  The reference ships no impulse responses and no meter
// (src/data/dataloader.py:13-50 replays pairs mixed beforehand).  For row r with n = clamp(len[r], 1, K) and slice s
// (0: broad-band, 1 + b: band b):
//
//   y_s[k] = sum_j g_b[j] h[k + D - j] (j ascending, one fma per term, h = 0 outside [0, n));  y_0 = h;  e[k] = y_s[k]^2
//   EDC[k] = sum_{j >= k} e[j],  E = EDC[0],  ka(x) = the smallest k < n with EDC[k] <= 10^(-x/10) E
//   k0 = the smallest k that maximises |h[k]|;  the regressions and ratios of the header on the ranges these give
//
// Float64 on the VALU, no atomics, two launches:
//   rir_stats_energy  grid (tile, slice, row).  A block owns RS_TILE = 1024 consecutive samples, a thread RS_RUN = 4
//                     consecutive ones.  It stages the span its outputs reach (RS_TILE + NFp - 1 samples, NFp = NF rounded
//                     up to 4, zeros outside [0, n)) and the band's taps (zeros from NF on) in LDS.  The span is stored in
//                     four quarters, sample i at quarter i & 3, place i >> 2: the threads of a wave, whose samples lie 4
//                     apart, then read consecutive float64.  Four taps at a time a thread fetches four new samples and
//                     keeps three of the seven it holds, so a fused multiply-add costs half an LDS read where the join of
//                     cmgan_rir_bands pays two; every output's chain still runs in ascending j.  Slice 0 is the filter
//                     {1}: fma(1, h, 0) = h.  It writes e[k] (zeros from n to the tile's end) and the tile's total from a
//                     fixed tree: a thread's four in order, then halves folded.  Tiles that begin at or after n do nothing.
//   rir_stats_scan    grid (slice, row), one block each.  k0 and the non-finite test from a pass over the row (a max-
//                     reduction under the total order larger |h|, then smaller index); the tiles' totals folded in
//                     descending tile order into entry sums; then tile after tile a suffix scan from the tile's entry sum
//                     (in a thread, then across the threads through LDS), the smallest index under each of the four
//                     thresholds as an integer minimum, the ratio sums per thread in ascending k, the curve to the
//                     workspace (and to edc_dev).  A second pass over the curve adds the three regressions' sums, whose
//                     ranges are then known.  Every per-thread sum is folded by the same fixed tree.
// Every float64 reduction runs in an order that depends on n and the tile grid alone, so a row's bits depend neither on R
// nor on the other rows, nor on ld, nor on K beyond n; slice 0 does not depend on NB.  Nothing read from device memory
// becomes an address, except k0, which the kernel computed itself as an index below n.
#include <math.h>
#include <stdint.h>

#include "api_internal.h"
#include "host_ranges.h"

namespace {

constexpr int RS_TPB = 256;                   // threads of both kernels
constexpr int RS_RUN = 4;                     // consecutive samples per thread
constexpr int RS_TILE = RS_TPB * RS_RUN;      // samples per block of the energy kernel, per step of the scan
constexpr int RS_MAX_K = 65536;               // longest response (the limit of cmgan_rir)
constexpr int RS_MAX_TILES = RS_MAX_K / RS_TILE;
constexpr int RS_MAX_BANDS = 8;               // = cmgan_rir_max_bands()
constexpr int RS_MAX_FILTER = 1023;           // = cmgan_rir_max_filter()
constexpr int RS_NFP = (RS_MAX_FILTER + 3) / 4 * 4;
constexpr int RS_QS = (RS_TILE + RS_NFP) / 4; // places per quarter of the staged span (RS_TILE + NFp - 1 samples)
constexpr int RS_P = 10;                      // output columns
static_assert(RS_TPB == 256, "the scans and trees take eight steps");
static_assert(RS_MAX_TILES <= RS_TPB, "a thread stages one tile total");

struct StatsArgs {
    const float* rir;
    const int* len;          // null: every row has K samples
    const double* filt;      // [NB][NF] or null
    double* stats;           // [R][NB + 1][RS_P]
    int* status;             // [R][NB + 1] or null
    double* edc_out;         // [R][NB + 1][K] or null
    double* e;               // workspace [R][NB + 1][Kp]: the energies, Kp = nt RS_TILE
    double* edc;             // workspace [R][NB + 1][Kp]: the decay curve
    double* tsum;            // workspace [R][NB + 1][nt]: a tile's total
    long long ld;
    double fs;
    int R, K, NB, NF, nt, Kp;
    int w, o50, o80;         // the direct window's half-width, round(0.05 fs), round(0.08 fs), each <= RS_MAX_K
};

__device__ inline int rs_rows_n(const StatsArgs& a, int r) {
    if (!a.len) return a.K;
    const int n = a.len[r];
    return n < 1 ? 1 : (n > a.K ? a.K : n);
}

__device__ inline double rs_block_sum(double v, double* red) {       // fixed order: halves folded, every thread calls
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = RS_TPB / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__device__ inline int rs_block_min(int v, int* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = RS_TPB / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = red[t + s] < red[t] ? red[t + s] : red[t];
        __syncthreads();
    }
    const int r = red[0];
    __syncthreads();
    return r;
}

// ---------------------------------------------------------------- the energy kernel
__global__ __launch_bounds__(RS_TPB) void rir_stats_energy(StatsArgs a) {
    __shared__ double s_h[4 * RS_QS], s_g[RS_NFP], s_red[RS_TPB];
    const int t = threadIdx.x, s = blockIdx.y, r = blockIdx.z;
    const int n = rs_rows_n(a, r);
    const int k0 = blockIdx.x * RS_TILE;
    if (k0 >= n) return;                                          // (the whole block: the scan never visits this tile)
    const int NF = s ? a.NF : 1, D = (NF - 1) / 2, C = (NF + 3) / 4, NFp = 4 * C;
    const float* row = a.rir + (size_t)r * a.ld;
    // s_h: sample i of the span is h[base + i], i = (k - k0) + (NFp - 1) - j for output k and tap j
    const int base = k0 + D - (NFp - 1), span = RS_TILE + NFp - 1;
    for (int i = t; i < span; i += RS_TPB) {
        const int q = base + i;
        s_h[(i & 3) * RS_QS + (i >> 2)] = (q >= 0 && q < n) ? (double)row[q] : 0.0;
    }
    if (s) {
        const double* g = a.filt + (size_t)(s - 1) * NF;
        for (int i = t; i < NFp; i += RS_TPB) s_g[i] = i < NF ? g[i] : 0.0;
    } else if (t < 4) {
        s_g[t] = t == 0 ? 1.0 : 0.0;
    }
    __syncthreads();
    // outputs k0 + 4 t + u, u = 0 .. 3.  Taps j = 4 c + a' use the samples 4 (t + C - 1 - c) + v, v = u + 3 - a' in 0 .. 6:
    // w[0 .. 3] are fetched, w[4 .. 6] are the last chunk's w[0 .. 2]
    double acc[RS_RUN] = {0.0, 0.0, 0.0, 0.0};
    double w[7];
    const double* sp = s_h + t + (C - 1);
    w[4] = sp[1], w[5] = sp[RS_QS + 1], w[6] = sp[2 * RS_QS + 1];
    for (int c = 0; c < C; ++c, --sp) {
        w[0] = sp[0], w[1] = sp[RS_QS], w[2] = sp[2 * RS_QS], w[3] = sp[3 * RS_QS];
        const double g[4] = {s_g[4 * c], s_g[4 * c + 1], s_g[4 * c + 2], s_g[4 * c + 3]};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int u = 0; u < RS_RUN; ++u) acc[u] = fma(g[j], w[u + 3 - j], acc[u]);
        w[4] = w[0], w[5] = w[1], w[6] = w[2];
    }
    const int k = k0 + RS_RUN * t;
    double e[RS_RUN];
#pragma unroll
    for (int u = 0; u < RS_RUN; ++u) e[u] = k + u < n ? acc[u] * acc[u] : 0.0;
    const size_t slice = (size_t)r * (a.NB + 1) + s;
    double* out = a.e + slice * a.Kp + k;
#pragma unroll
    for (int u = 0; u < RS_RUN; ++u) out[u] = e[u];
    const double total = rs_block_sum(((e[0] + e[1]) + e[2]) + e[3], s_red);
    if (t == 0) a.tsum[slice * a.nt + blockIdx.x] = total;
}

// ---------------------------------------------------------------- the scan kernel
__device__ inline double rs_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ inline double rs_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// 10 log10(num / den) of two sums of energies; an empty denominator gives +inf
__device__ inline double rs_ratio_db(double num, double den) { return den == 0.0 ? rs_inf() : 10.0 * log10(num / den); }

__global__ __launch_bounds__(RS_TPB) void rir_stats_scan(StatsArgs a) {
    __shared__ double s_a[RS_TPB], s_b[RS_TPB], s_in[RS_MAX_TILES], s_late[2], s_E;
    __shared__ float s_bv[RS_TPB];
    __shared__ int s_bi[RS_TPB];
    const int t = threadIdx.x, s = blockIdx.x, r = blockIdx.y;
    const int n = rs_rows_n(a, r);
    const float* row = a.rir + (size_t)r * a.ld;
    const size_t slice = (size_t)r * (a.NB + 1) + s;
    double* stats = a.stats + slice * RS_P;
    double* edc_out = a.edc_out ? a.edc_out + slice * a.K : nullptr;

    // k0 and the non-finite test: thread t looks at k = t, t + 256, ..., so its own best is its first
    float bv = -1.f;
    int bi = 0, bad = 0;
    for (int k = t; k < n; k += RS_TPB) {
        const float v = row[k], av = fabsf(v);
        bad |= (v - v == 0.f) ? 0 : 1;
        if (av > bv) bv = av, bi = k;
    }
    bad = __syncthreads_or(bad);
    if (bad) {                                                    // (the whole block)
        if (t < RS_P) stats[t] = rs_nan();
        if (t == 0 && a.status) a.status[slice] = CMGAN_RIR_STATS_NONFINITE | CMGAN_RIR_STATS_NO_EDT | CMGAN_RIR_STATS_NO_T20
                                                  | CMGAN_RIR_STATS_NO_T30;
        if (edc_out)
            for (int k = t; k < a.K; k += RS_TPB) edc_out[k] = k < n ? rs_nan() : 0.0;
        return;
    }
    s_bv[t] = bv;
    s_bi[t] = bi;
    __syncthreads();
    for (int h = RS_TPB / 2; h > 0; h >>= 1) {
        if (t < h) {
            const float ov = s_bv[t + h];
            const int oi = s_bi[t + h];
            if (ov > s_bv[t] || (ov == s_bv[t] && oi < s_bi[t])) s_bv[t] = ov, s_bi[t] = oi;
        }
        __syncthreads();
    }
    const int k0 = s_bi[0];                                       // < n: every row has a sample, and none is a NaN
    const int lo = k0 - a.w > 0 ? k0 - a.w : 0, hi = k0 + a.w < n - 1 ? k0 + a.w : n - 1;
    const int k50 = k0 + a.o50 < n ? k0 + a.o50 : n, k80 = k0 + a.o80 < n ? k0 + a.o80 : n;

    // entry sums: the tiles' totals in descending tile order
    const int ntn = (n + RS_TILE - 1) / RS_TILE;
    if (t < ntn) s_a[t] = a.tsum[slice * a.nt + t];
    if (t < 2) s_late[t] = 0.0;
    __syncthreads();
    if (t == 0) {
        double acc = 0.0;
        for (int ti = ntn - 1; ti >= 0; --ti) {
            s_in[ti] = acc;
            acc += s_a[ti];
        }
        s_E = acc;
    }
    __syncthreads();
    const double E = s_E;
    const double thr[4] = {CMGAN_RIR_STATS_DOWN_5 * E, CMGAN_RIR_STATS_DOWN_10 * E, CMGAN_RIR_STATS_DOWN_25 * E,
                           CMGAN_RIR_STATS_DOWN_35 * E};

    // the curve, the threshold indices and the ratio sums
    const double* e_ws = a.e + slice * a.Kp;
    double* edc_ws = a.edc + slice * a.Kp;
    int ka[4] = {n, n, n, n};
    double pre = 0.0, mid = 0.0, post = 0.0, early50 = 0.0, early80 = 0.0, ts = 0.0;
    for (int ti = 0; ti < ntn; ++ti) {
        const int kb = ti * RS_TILE + RS_RUN * t;
        double e[RS_RUN], suf[RS_RUN];
#pragma unroll
        for (int u = 0; u < RS_RUN; ++u) e[u] = e_ws[kb + u];
        suf[3] = e[3];
        suf[2] = e[2] + suf[3];
        suf[1] = e[1] + suf[2];
        suf[0] = e[0] + suf[1];
        // inclusive suffix scan of the threads' totals
        double* src = s_a;
        double* dst = s_b;
        src[t] = suf[0];
        __syncthreads();
        for (int off = 1; off < RS_TPB; off <<= 1) {
            double x = src[t];
            if (t + off < RS_TPB) x += src[t + off];
            dst[t] = x;
            double* sw = src;
            src = dst;
            dst = sw;
            __syncthreads();
        }
        const double after = s_in[ti] + (t + 1 < RS_TPB ? src[t + 1] : 0.0);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < RS_RUN; ++u) {
            const int k = kb + u;
            if (k >= n) continue;
            const double c = k == 0 ? E : after + suf[u];
#pragma unroll
            for (int x = 0; x < 4; ++x)
                if (c <= thr[x] && k < ka[x]) ka[x] = k;
            if (k == k50) s_late[0] = c;
            if (k == k80) s_late[1] = c;
            if (k < lo) pre += e[u];
            else if (k <= hi) mid += e[u];
            else post += e[u];
            if (k < k50) early50 += e[u];
            if (k < k80) early80 += e[u];
            if (k > k0) ts = fma((double)(k - k0), e[u], ts);
            edc_ws[k] = c;
            if (edc_out) edc_out[k] = c;
        }
    }
    if (edc_out)
        for (int k = n + t; k < a.K; k += RS_TPB) edc_out[k] = 0.0;
    pre = rs_block_sum(pre, s_a);
    mid = rs_block_sum(mid, s_a);
    post = rs_block_sum(post, s_a);
    early50 = rs_block_sum(early50, s_a);
    early80 = rs_block_sum(early80, s_a);
    ts = rs_block_sum(ts, s_a);
#pragma unroll
    for (int x = 0; x < 4; ++x) ka[x] = rs_block_min(ka[x], s_bi);

    // the regressions: EDT on [0, ka(10)), T20 on [ka(5), ka(25)), T30 on [ka(5), ka(35))
    const int beg[3] = {0, ka[0], ka[0]}, end[3] = {ka[1], ka[2], ka[3]};
    bool fit[3];
    double kbar[3], sum[3] = {0.0, 0.0, 0.0};
    int kend = 0;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        fit[x] = end[x] < n && end[x] - beg[x] >= 2;
        kbar[x] = 0.5 * (double)(beg[x] + end[x] - 1);
        if (fit[x] && end[x] > kend) kend = end[x];
    }
    for (int k = t; k < kend; k += RS_TPB) {                      // (the curve this block wrote, behind the barriers above)
        const double L = 10.0 * log10(edc_ws[k] / E);
#pragma unroll
        for (int x = 0; x < 3; ++x)
            if (fit[x] && k >= beg[x] && k < end[x]) sum[x] = fma((double)k - kbar[x], L, sum[x]);
    }
#pragma unroll
    for (int x = 0; x < 3; ++x) sum[x] = rs_block_sum(sum[x], s_a);
    if (t != 0) return;

    int status = 0;
    double time[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const double m = (double)(end[x] - beg[x]);
        const double slope = a.fs * sum[x] / (m * (m * m - 1.0) / 12.0);
        const bool ok = fit[x] && slope < 0.0;
        time[x] = ok ? -60.0 / slope : rs_nan();
        if (!ok) status |= CMGAN_RIR_STATS_NO_EDT << x;
    }
    if (E == 0.0) {
        status |= CMGAN_RIR_STATS_ZERO;
        stats[0] = 0.0;
        for (int c = 1; c < RS_P; ++c) stats[c] = rs_nan();
    } else {
        stats[0] = E;
        stats[1] = (double)k0;
        stats[2] = rs_ratio_db(mid, pre + post);
        stats[3] = rs_ratio_db(early50, s_late[0]);
        stats[4] = rs_ratio_db(early80, s_late[1]);
        stats[5] = early50 / E;
        stats[6] = ts / (a.fs * E);
        stats[7] = time[0];
        stats[8] = time[1];
        stats[9] = time[2];
    }
    if (a.status) a.status[slice] = status;
}

// ---------------------------------------------------------------- the host side
inline int rs_tiles(int K) { return (K + RS_TILE - 1) / RS_TILE; }

inline bool rs_shape_ok(int R, int K, int NB, int NF) {
    return R >= 1 && R <= 65535 && K >= 1 && K <= RS_MAX_K && NB >= 0 && NB <= RS_MAX_BANDS && NF >= 1 && NF <= RS_MAX_FILTER
        && (NF & 1);
}

struct StatsLayout {
    size_t e, edc, tsum, total;          // byte offsets
};

inline StatsLayout rs_layout(int R, int K, int NB) {
    const size_t slices = (size_t)R * (NB + 1), curve = up256(slices * rs_tiles(K) * RS_TILE * sizeof(double));
    StatsLayout l;
    l.e = 0;
    l.edc = curve;
    l.tsum = 2 * curve;
    l.total = l.tsum + up256(slices * rs_tiles(K) * sizeof(double));
    return l;
}

}  // namespace

extern "C" int cmgan_rir_stats_tile(void) { return RS_TILE; }
extern "C" int cmgan_rir_stats_columns(void) { return RS_P; }

extern "C" size_t cmgan_rir_stats_workspace_bytes(const cmgan_handle*, int R, int K, int NB, int NF) {
    return rs_shape_ok(R, K, NB, NF) ? rs_layout(R, K, NB).total : 0;
}

extern "C" int cmgan_rir_stats(cmgan_handle* h, const float* rir, int R, int K, long long ld, const int* len,
                               const double* filt, int NB, int NF, int fs, double direct_ms, double* stats, int* status,
                               double* edc, void* ws, size_t ws_bytes, void* stream) {
    // every argument is judged before the handle is, so that the errors below need no GPU (the message of a call
    // without a handle is read with cmgan_last_error(NULL))
    if (!rir || !stats) return fail(h, CMGAN_E_BADARG, "cmgan_rir_stats: null pointer");
    if (((uintptr_t)rir | (uintptr_t)len | (uintptr_t)status) & 3)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_stats: float32 / int32 buffers must be 4-byte aligned");
    if (((uintptr_t)filt | (uintptr_t)stats | (uintptr_t)edc) & 7)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_stats: float64 buffers must be 8-byte aligned");
    if (R < 1 || R > 65535 || K < 1 || ld < K)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_stats: need 1 <= R <= 65535, K >= 1, ld >= K (R=%d K=%d ld=%lld)", R, K, ld);
    if (NB < 0 || NB > RS_MAX_BANDS)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_stats: need 0 <= NB <= %d bands (NB=%d)", RS_MAX_BANDS, NB);
    if ((NB == 0) != (filt == nullptr))
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_stats: the filter table must be null with NB = 0 and only then (NB=%d)", NB);
    if (NF < 1 || !(NF & 1))
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_stats: the filter length must be odd and >= 1 (NF=%d)", NF);
    if (fs < 1) return fail(h, CMGAN_E_BADARG, "cmgan_rir_stats: fs must be positive (fs=%d)", fs);
    if (!(direct_ms >= 0.0) || !(direct_ms <= 1.0e300))
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_stats: direct_ms must be finite and >= 0 (%g)", direct_ms);
    if (K > RS_MAX_K)
        return fail(h, CMGAN_E_UNSUPPORTED, "cmgan_rir_stats: responses of up to %d taps are supported (K=%d)", RS_MAX_K, K);
    if (NF > RS_MAX_FILTER)
        return fail(h, CMGAN_E_UNSUPPORTED, "cmgan_rir_stats: filters of up to %d taps are supported (NF=%d)", RS_MAX_FILTER, NF);
    const StatsLayout l = rs_layout(R, K, NB);
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < l.total)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_stats: the workspace must be 256-byte aligned and hold %zu bytes (%zu given)",
                    l.total, ws ? ws_bytes : (size_t)0);
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "cmgan_rir_stats: null handle");
    const LaunchCtx ctx = begin(h, stream);
    hipStream_t s = ctx.stream;
    char* w = (char*)ws;
    StatsArgs a;
    a.rir = rir;
    a.len = len;
    a.filt = filt;
    a.stats = stats;
    a.status = status;
    a.edc_out = edc;
    a.e = (double*)(w + l.e);
    a.edc = (double*)(w + l.edc);
    a.tsum = (double*)(w + l.tsum);
    a.ld = ld;
    a.fs = (double)fs;
    a.R = R, a.K = K, a.NB = NB, a.NF = NF;
    a.nt = rs_tiles(K);
    a.Kp = a.nt * RS_TILE;
    // round() is to nearest, halves up; every offset is clipped to n by the kernel, so RS_MAX_K stands for anything larger
    const double wd = floor(direct_ms * (double)fs / 1000.0 + 0.5);
    const long long o50 = ((long long)fs + 10) / 20, o80 = (4LL * fs + 25) / 50;
    a.w = wd < (double)RS_MAX_K ? (int)wd : RS_MAX_K;
    a.o50 = o50 < RS_MAX_K ? (int)o50 : RS_MAX_K;
    a.o80 = o80 < RS_MAX_K ? (int)o80 : RS_MAX_K;
    LAUNCH(ctx, "rir_stats_energy", rir_stats_energy<<<dim3(a.nt, NB + 1, R), RS_TPB, 0, s>>>(a));
    LAUNCH(ctx, "rir_stats_scan", rir_stats_scan<<<dim3(NB + 1, R), RS_TPB, 0, s>>>(a));
    return check_launch(h, "rir_stats");
}
