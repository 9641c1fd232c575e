// level.hip - the active speech level of a [B, L] float32 batch on the device (cmgan_speech_level, include/cmgan_hip.h):
// the level meter of ITU-T P.56, method B, as its published description gives it.  The reference has no level handling at
// all (src/data/dataloader.py:13-50 replays pairs mixed beforehand).  For row b with n = clamp(lengths[b], 0, L):
//
//   g   = exp(-1 / (0.03 fs))              I = ceil(0.2 fs)              c_j = 2^(j-15), j = 0..14
//   p_i = g p_{i-1} + (1-g) |x_i|,  q_i = g q_{i-1} + (1-g) p_i,          p_{-1} = q_{-1} = 0
//   a_j = #{ i < n : q_i' >= c_j for some i' in [i-I, i] }                (activity with hangover)
//   sq  = sum x_i^2,  ms = sq / n,  A_j = 10 log10(sq / a_j),  D_j = A_j - 20 log10(c_j),  M = 15.9
//   A*  = A_0 if D_0 <= M; else A_{j-1} + t (A_j - A_{j-1}), t = (D_{j-1} - M) / (D_{j-1} - D_j), at the first j < J with
//         D_j <= M; else A_{J-1}                                           (J = #{ j : a_j > 0 })
//   active_ms = 10^(A* / 10),  activity = ms / active_ms
//
// The envelope is a linear recurrence, so a segment of m samples run from zero state, ending in (P, Q), acts on an incoming
// state as   p' = g^m p + P,   q' = g^m q + m (1-g) g^m p + Q,   and two adjacent segments compose to a third.  Four
// launches, float64 on the VALU, no atomics, no host synchronisation:
//   level_scan    a block owns a tile of LV_TILE samples of one row, a thread LV_RUN consecutive ones.  Each thread runs its
//                 samples from zero state, the 256 segments are combined by an inclusive scan through LDS, and the block
//                 writes the tile's (P, Q) and its sum of x^2.  Samples at i >= n are never read; they count as zeros, so a
//                 row's bits do not depend on how far L reaches past n.
//   level_fold    one block per row: the same scan over the tiles' segments, 256 tiles at a time in ascending order, gives
//                 every tile its incoming state; the partial sums of x^2 are added in ascending slot order.
//   level_cross   per tile: every thread's entry state from the tile's incoming state and the in-tile scan, then its samples
//                 in sequence.  The thresholds are nested, so a sample has a level l_i = #{ j : q_i >= c_j }; wave ballots
//                 find, per threshold, the first and the last sample of the tile with l_i > j.
//   level_select  one block per row.  LV_TILE <= I + 1 for every fs >= 8000, so every valid sample of a tile after its first
//                 crossing is active: a tile adds valid - first_j, and the hangover that reaches it from the last crossing
//                 before it adds clamp(last_in_j + I + 1 - tile_start, 0, first_j).  That crossing lies at most
//                 ceil(I / LV_TILE) tiles back, so every (tile, threshold) pair is a thread's work of its own and the sums
//                 are integer sums, exact in any order.  Then the selection.
// Every float64 reduction runs in an order that depends on the tile grid alone, so a row's bits depend neither on B nor
// on the other rows, nor on L beyond n.
#include <math.h>
#include <stdint.h>

#include "api_internal.h"
#include "host_ranges.h"

namespace {

constexpr int LV_TPB = 256;                 // threads of every kernel here
constexpr int LV_RUN = 4;                   // consecutive samples per thread
constexpr int LV_TILE = LV_TPB * LV_RUN;    // samples per block
constexpr int LV_NTH = 15;                  // thresholds c_j = 2^(j-15)
constexpr int LV_FS_MIN = 8000, LV_FS_MAX = 192000;
constexpr int LV_MAX_L = 0x7fffffff - LV_TILE;   // a tile's sample indices stay in an int
constexpr double LV_MARGIN = 15.9;          // dB between the active level and its threshold
// level_select counts every valid sample after a tile's first crossing as active: the hangover must span the tile
static_assert(LV_TPB == 256, "the scans take eight steps");
static_assert(LV_TILE <= LV_FS_MIN / 5 + 1, "a tile must be no longer than the shortest hangover + 1");
static_assert(LV_TILE < (1 << 15), "first / last crossing are packed in 16 bits each");
constexpr int LV_BACK_MAX = (LV_FS_MAX / 5 + LV_TILE - 1) / LV_TILE;   // tiles the longest hangover reaches back over
static_assert(LV_BACK_MAX < LV_TPB, "level_select stages the tiles before a chunk with it");

struct LevelArgs {
    const float* x;
    const int* lengths;      // null: every row has L samples
    double* level;           // [B][3]
    long long* counts;       // [B][16] or null
    double* seg_p;           // workspace [B][nt]: a tile's (P, Q) from zero state ...
    double* seg_q;
    double* in_p;            // ... and the state before its first sample
    double* in_q;
    double* part_sq;         // [B][nt]
    double* sq;              // [B]
    int* cross;              // [B][nt][16]: first | (last + 1) << 16 per threshold, first = LV_TILE when there is none
    long long ld;
    double tau;              // 0.03 fs: g^m = exp(-m / tau)
    double gp_run[8];        // g^(LV_RUN 2^k) and g^(LV_TILE 2^k), k = 0..7: the steps of the two scans (made by the host,
    double gp_tile[8];       // so that the same bits reach every block)
    int B, L, nt, hang;      // hang = I
};

__device__ inline int lv_rows_n(const LevelArgs& a, int b) {
    if (!a.lengths) return a.L;
    const int n = a.lengths[b];
    return n < 0 ? 0 : (n > a.L ? a.L : n);
}

__device__ inline double lv_gpow(const LevelArgs& a, double m) { return exp(-m / a.tau); }

// Inclusive scan of 256 segments of `unit` samples each, thread t holding segment t as (P, Q).  Before the step with
// offset s, the segments of threads t >= s cover s units, so the step composes with g^(unit s) for all of them.
__device__ inline void lv_scan(const double (&gp)[8], double unit, double omg, double& P, double& Q, double* s_p, double* s_q) {
    const int t = threadIdx.x;
    int k = 0;
#pragma unroll
    for (int s = 1; s < LV_TPB; s <<= 1, ++k) {
        s_p[t] = P;
        s_q[t] = Q;
        __syncthreads();
        if (t >= s) {
            const double m = unit * (double)s, gm = gp[k];
            const double Pa = s_p[t - s], Qa = s_q[t - s];
            Q = fma(gm, Qa, fma(m * omg * gm, Pa, Q));
            P = fma(gm, Pa, P);
        }
        __syncthreads();
    }
}

// the thread's LV_RUN samples of the tile (zeros from the row's end on) and the segment they make from zero state
__device__ inline void lv_run(const LevelArgs& a, int b, int n, double g, double omg, double (&ax)[LV_RUN], double& P, double& Q) {
    const int i0 = blockIdx.x * LV_TILE + threadIdx.x * LV_RUN;
    const float* row = a.x + (size_t)b * a.ld;
    P = Q = 0.0;
#pragma unroll
    for (int r = 0; r < LV_RUN; ++r) {
        ax[r] = i0 + r < n ? (double)row[i0 + r] : 0.0;
        P = fma(g, P, omg * fabs(ax[r]));
        Q = fma(g, Q, omg * P);
    }
}

__device__ inline double lv_block_sum(double v, double* red) {       // fixed order: halves folded, every thread calls
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = LV_TPB / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// ------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(LV_TPB) void level_scan(LevelArgs a) {
    __shared__ double s_p[LV_TPB], s_q[LV_TPB];
    const int t = threadIdx.x, b = blockIdx.y;
    const int n = lv_rows_n(a, b);
    const double g = lv_gpow(a, 1.0), omg = 1.0 - g;
    double ax[LV_RUN], P, Q;
    lv_run(a, b, n, g, omg, ax, P, Q);
    double sq = 0.0;
#pragma unroll
    for (int r = 0; r < LV_RUN; ++r) sq = fma(ax[r], ax[r], sq);
    lv_scan(a.gp_run, (double)LV_RUN, omg, P, Q, s_p, s_q);
    sq = lv_block_sum(sq, s_p);
    const size_t e = (size_t)b * a.nt + blockIdx.x;
    if (t == LV_TPB - 1) {
        a.seg_p[e] = P;
        a.seg_q[e] = Q;
    }
    if (t == 0) a.part_sq[e] = sq;
}

__global__ __launch_bounds__(LV_TPB) void level_fold(LevelArgs a) {
    __shared__ double s_p[LV_TPB], s_q[LV_TPB];
    const int t = threadIdx.x, b = blockIdx.x;
    const double omg = 1.0 - lv_gpow(a, 1.0);
    const size_t e0 = (size_t)b * a.nt;
    double cp = 0.0, cq = 0.0;                                   // the state before the chunk's first tile
    for (int k0 = 0; k0 < a.nt; k0 += LV_TPB) {
        const int k = k0 + t;
        double P = k < a.nt ? a.seg_p[e0 + k] : 0.0, Q = k < a.nt ? a.seg_q[e0 + k] : 0.0;
        lv_scan(a.gp_tile, (double)LV_TILE, omg, P, Q, s_p, s_q);
        // the state after tile k: the chunk's incoming state through the t + 1 tiles up to it
        const double m = (double)LV_TILE * (double)(t + 1), gm = lv_gpow(a, m);
        const double ep = fma(gm, cp, P), eq = fma(gm, cq, fma(m * omg * gm, cp, Q));
        s_p[t] = ep;
        s_q[t] = eq;
        __syncthreads();
        if (k < a.nt) {
            a.in_p[e0 + k] = t ? s_p[t - 1] : cp;
            a.in_q[e0 + k] = t ? s_q[t - 1] : cq;
        }
        cp = s_p[LV_TPB - 1];
        cq = s_q[LV_TPB - 1];
        __syncthreads();
    }
    double sq = 0.0;
    for (int k = t; k < a.nt; k += LV_TPB) sq += a.part_sq[e0 + k];
    sq = lv_block_sum(sq, s_p);
    if (t == 0) a.sq[b] = sq;
}

__global__ __launch_bounds__(LV_TPB) void level_cross(LevelArgs a) {
    __shared__ double s_p[LV_TPB], s_q[LV_TPB];
    __shared__ int s_first[LV_TPB / 64][LV_NTH + 1], s_last[LV_TPB / 64][LV_NTH + 1];
    const int t = threadIdx.x, b = blockIdx.y;
    const int n = lv_rows_n(a, b);
    const double g = lv_gpow(a, 1.0), omg = 1.0 - g;
    double ax[LV_RUN], P, Q;
    lv_run(a, b, n, g, omg, ax, P, Q);
    lv_scan(a.gp_run, (double)LV_RUN, omg, P, Q, s_p, s_q);
    s_p[t] = P;
    s_q[t] = Q;
    __syncthreads();
    const size_t e = (size_t)b * a.nt + blockIdx.x;
    const double ip = a.in_p[e], iq = a.in_q[e];
    // entry state: the tile's incoming state through the t runs before this one, plus what those runs made from zero
    const double m = (double)(LV_RUN * t), gm = lv_gpow(a, m);
    double p = fma(gm, ip, t ? s_p[t - 1] : 0.0);
    double q = fma(gm, iq, fma(m * omg * gm, ip, t ? s_q[t - 1] : 0.0));
    const int i0 = blockIdx.x * LV_TILE + t * LV_RUN;
    int lvl[LV_RUN];
#pragma unroll
    for (int r = 0; r < LV_RUN; ++r) {
        p = fma(g, p, omg * fabs(ax[r]));
        q = fma(g, q, omg * p);
        int l = 0;
        double c = 1.0 / 32768.0;
#pragma unroll
        for (int j = 0; j < LV_NTH; ++j, c *= 2.0) l += q >= c ? 1 : 0;          // nested thresholds: a NaN is below all
        lvl[r] = i0 + r < n ? l : 0;
    }
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int j = 0; j < LV_NTH; ++j) {
        int first = LV_TILE, last = -1;
#pragma unroll
        for (int r = 0; r < LV_RUN; ++r) {
            const unsigned long long mask = __ballot(lvl[r] > j);
            if (mask) {
                const int lo = (wave * 64 + (__ffsll((long long)mask) - 1)) * LV_RUN + r;
                const int hi = (wave * 64 + (63 - __clzll((long long)mask))) * LV_RUN + r;
                first = lo < first ? lo : first;
                last = hi > last ? hi : last;
            }
        }
        if (lane == 0) {
            s_first[wave][j] = first;
            s_last[wave][j] = last;
        }
    }
    __syncthreads();
    if (t <= LV_NTH) {
        int first = LV_TILE, last = -1;
        if (t < LV_NTH) {
            for (int w = 0; w < LV_TPB / 64; ++w) {
                first = s_first[w][t] < first ? s_first[w][t] : first;
                last = s_last[w][t] > last ? s_last[w][t] : last;
            }
        }
        a.cross[e * 16 + t] = first | ((last + 1) << 16);
    }
}

__global__ __launch_bounds__(LV_TPB) void level_select(LevelArgs a) {
    __shared__ int s_c[(LV_TPB + LV_BACK_MAX) * 16];
    __shared__ long long s_part[LV_TPB];
    __shared__ long long s_a[LV_NTH];
    const int t = threadIdx.x, b = blockIdx.x;
    const int n = lv_rows_n(a, b);
    const int* cross = a.cross + (size_t)b * a.nt * 16;
    const int back = (a.hang + LV_TILE - 1) / LV_TILE;           // the tiles a hangover can reach back over (<= LV_BACK_MAX)
    const int j = t & 15, sub = t >> 4;                          // a thread keeps one threshold: 16 tiles per pass
    long long cnt = 0;
    for (int k0 = 0; k0 < a.nt; k0 += LV_TPB) {
        const int nk = a.nt - k0 < LV_TPB ? a.nt - k0 : LV_TPB;
        const int h = k0 < back ? k0 : back;                     // tiles before the chunk that are staged with it
        for (int q = t; q < (nk + h) * 16; q += LV_TPB) s_c[q] = cross[(size_t)(k0 - h) * 16 + q];
        __syncthreads();
        for (int k = sub; k < nk && j < LV_NTH; k += LV_TPB / 16) {
            long long valid = (long long)n - (long long)(k0 + k) * LV_TILE;
            valid = valid < 0 ? 0 : (valid > LV_TILE ? LV_TILE : valid);
            const int first = s_c[(h + k) * 16 + j] & 0xffff;
            const long long lim = first < LV_TILE ? first : valid;          // the samples before the tile's first crossing
            if (first < LV_TILE) cnt += valid - first;
            // the hangover of the last crossing before the tile: d tiles back, at sample `last` of that tile
            for (int d = 1; lim > 0 && d <= back && d <= h + k; ++d) {
                const int last = (s_c[(h + k - d) * 16 + j] >> 16) - 1;
                if (last < 0) continue;
                const long long reach = (long long)last + a.hang + 1 - (long long)d * LV_TILE;
                cnt += reach < 0 ? 0 : (reach > lim ? lim : reach);
                break;
            }
        }
        __syncthreads();
    }
    s_part[t] = cnt;
    __syncthreads();
    if (t < LV_NTH) {
        long long sum = 0;
        for (int k = 0; k < LV_TPB / 16; ++k) sum += s_part[t + 16 * k];
        s_a[t] = sum;
    }
    __syncthreads();
    if (t < 16 && a.counts) a.counts[(size_t)b * 16 + t] = t < LV_NTH ? s_a[t] : (long long)n;
    if (t != 0) return;
    const double sq = a.sq[b];
    double ms = 0.0, act = 0.0, frac = 0.0;
    int J = 0;
    while (J < LV_NTH && s_a[J] > 0) ++J;
    if (n > 0 && !(fabs(sq) <= 1.79769313486231570815e308)) {
        ms = act = frac = nan("");
    } else if (n > 0 && sq != 0.0 && J > 0) {
        const double c20 = 20.0 * log10(2.0);
        double A_prev = 10.0 * log10(sq / (double)s_a[0]);
        double D_prev = A_prev - (double)(0 - 15) * c20;
        double As = A_prev;
        if (D_prev > LV_MARGIN) {
            for (int j = 1; j < J; ++j) {
                const double A = 10.0 * log10(sq / (double)s_a[j]);
                const double D = A - (double)(j - 15) * c20;
                if (D <= LV_MARGIN) {
                    const double tt = (D_prev - LV_MARGIN) / (D_prev - D);
                    As = A_prev + tt * (A - A_prev);
                    break;
                }
                A_prev = A;
                D_prev = D;
                As = A;                                            // no threshold qualifies: A_{J-1}
            }
        }
        ms = sq / (double)n;
        act = pow(10.0, As / 10.0);
        frac = ms / act;
    }
    a.level[(size_t)b * 3 + 0] = ms;
    a.level[(size_t)b * 3 + 1] = act;
    a.level[(size_t)b * 3 + 2] = frac;
}

inline int lv_tiles(int L) { return (L + LV_TILE - 1) / LV_TILE; }

struct LevelLayout {
    size_t tiles, sq, cross, total;    // byte offsets: 5 float64 [B][nt] planes from `tiles` | sq [B] | cross int32 [B][nt][16]
    size_t tile_stride;
};

inline LevelLayout lv_layout(int B, int L) {
    LevelLayout l;
    l.tiles = 0;
    l.tile_stride = up256((size_t)B * lv_tiles(L) * sizeof(double));
    l.sq = 5 * l.tile_stride;
    l.cross = l.sq + up256((size_t)B * sizeof(double));
    l.total = l.cross + up256((size_t)B * lv_tiles(L) * 16 * sizeof(int));
    return l;
}

inline bool lv_shape_ok(int B, int L) { return B >= 1 && B <= 65535 && L >= 1 && L <= LV_MAX_L; }

}  // namespace

extern "C" int cmgan_speech_level_tile(void) { return LV_TILE; }

extern "C" size_t cmgan_speech_level_workspace_bytes(int B, int L) { return lv_shape_ok(B, L) ? lv_layout(B, L).total : 0; }

extern "C" int cmgan_speech_level(cmgan_handle* h, const float* x, int B, int L, long long ld, const int* lengths, int fs,
                                  double* level, long long* counts, void* ws, size_t ws_bytes, void* stream) {
    // every argument is judged before the handle is, so that the errors below need no GPU (the message of a call
    // without a handle is read with cmgan_last_error(NULL))
    if (!x || !level) return fail(h, CMGAN_E_BADARG, "cmgan_speech_level: null pointer");
    if (((uintptr_t)x | (uintptr_t)lengths) & 3)
        return fail(h, CMGAN_E_BADARG, "cmgan_speech_level: float32 / int32 buffers must be 4-byte aligned");
    if (((uintptr_t)level | (uintptr_t)counts) & 7)
        return fail(h, CMGAN_E_BADARG, "cmgan_speech_level: float64 / int64 buffers must be 8-byte aligned");
    if (B < 1 || B > 65535 || L < 1 || ld < L)
        return fail(h, CMGAN_E_BADARG, "cmgan_speech_level: need 1 <= B <= 65535, L >= 1, ld >= L (B=%d L=%d ld=%lld)", B, L, ld);
    if (L > LV_MAX_L)
        return fail(h, CMGAN_E_BADARG, "cmgan_speech_level: rows of up to %d samples are supported (L=%d)", LV_MAX_L, L);
    if (fs < LV_FS_MIN || fs > LV_FS_MAX)
        return fail(h, CMGAN_E_BADARG, "cmgan_speech_level: fs must lie in [%d, %d] (fs=%d)", LV_FS_MIN, LV_FS_MAX, fs);
    const LevelLayout l = lv_layout(B, L);
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < l.total)
        return fail(h, CMGAN_E_BADARG, "cmgan_speech_level: the workspace must be 256-byte aligned and hold %zu bytes (%zu given)",
                    l.total, ws ? ws_bytes : (size_t)0);
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "cmgan_speech_level: null handle");
    const LaunchCtx ctx = begin(h, stream);
    hipStream_t s = ctx.stream;
    char* w = (char*)ws;
    LevelArgs a;
    a.x = x;
    a.lengths = lengths;
    a.level = level;
    a.counts = counts;
    a.seg_p = (double*)(w + l.tiles);
    a.seg_q = (double*)(w + l.tiles + l.tile_stride);
    a.in_p = (double*)(w + l.tiles + 2 * l.tile_stride);
    a.in_q = (double*)(w + l.tiles + 3 * l.tile_stride);
    a.part_sq = (double*)(w + l.tiles + 4 * l.tile_stride);
    a.sq = (double*)(w + l.sq);
    a.cross = (int*)(w + l.cross);
    a.ld = ld;
    a.tau = 0.03 * (double)fs;
    for (int k = 0; k < 8; ++k) {
        a.gp_run[k] = exp(-(double)(LV_RUN << k) / a.tau);
        a.gp_tile[k] = exp(-(double)(LV_TILE << k) / a.tau);
    }
    a.B = B;
    a.L = L;
    a.nt = lv_tiles(L);
    a.hang = (fs + 4) / 5;                 // I = ceil(0.2 fs)
    const dim3 grid(a.nt, B);
    LAUNCH(ctx, "level_scan", level_scan<<<grid, LV_TPB, 0, s>>>(a));
    LAUNCH(ctx, "level_fold", level_fold<<<B, LV_TPB, 0, s>>>(a));
    LAUNCH(ctx, "level_cross", level_cross<<<grid, LV_TPB, 0, s>>>(a));
    LAUNCH(ctx, "level_select", level_select<<<B, LV_TPB, 0, s>>>(a));
    return check_launch(h, "speech_level");
}
