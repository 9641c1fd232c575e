// stretch.hip - tempo perturbation of a [B, L] float32 batch on the device (cmgan_stretch, include/cmgan_hip.h): every row is
// time-stretched by its OWN rate, any float64 in [1/4, 4] read from device memory, with the pitch kept: WSOLA
// (waveform-similarity overlap-add, Verhelst & Roelands 1993).  The reference has no counterpart: its data path replays
// fixed pairs (src/data/dataloader.py).  For row b with n = lengths[b] (L without lengths; x reads as 0 outside [0, n)),
// r = rate[b] input time per output time, H = hop and D = search:
//
//   M    = min(N, #{i >= 0 : fl(i r) < n})              out_len[b], cmgan_warp's count; K = ceil(M / H) frames
//   p_k  = floor(fl((k H) r))                           the nominal position of frame k: one rounded float64 product
//   q_0  = c_0 = 0;  c_k = q_{k-1} + H                  the natural continuation of the previous segment
//   q_k  = c_k                                          if |c_k - p_k| <= D and 0 <= c_k < n: no search, the frame is a copy
//        = p_k + argmax_d s(d), |d| <= D, 0 <= p_k + d < n    otherwise, with
//   s(d) = 2 C - E,  C = sum_i x[q + i] x[c_k + i],  E = sum_i x[q + i]^2,  q = p_k + d,  float64 sums over i = 0 .. H-1
//          ascending; a NaN score counts as -inf; among equal maxima the earliest of d = 0, -1, +1, -2, +2, ... wins
//   f[i] = 0.5 - 0.5 cospi(i / H),  g[i] = fl(1 - f[i])
//   y[b, k H + i] = f32( f[i] x[q_k + i] + g[i] x[c_k + i] )      for 0 <= i < H and k H + i < M;  zeros from M on
//
// A row whose rate is not a finite number in [1/4, 4], or whose length lies outside [0, L], is INVALID: N zeros, status
// 1, out_len 0.  One launch, no workspace, no atomics.  The frames of a row form a serial chain (q_k needs q_{k-1}), so
// ONE block owns a row and walks its frames; a batch of 32 rows keeps 32 compute units busy and no more.  A frame that is
// searched stages the candidate span x[p - D .. p + D + H) and the continuation x[c .. c + H) in LDS; every candidate
// has a thread of its own that runs both sums in one ascending chain of fused multiply-adds (a product of two float32
// values is exact in float64, so the sums are those of the unfused definition, bit for bit, and q_k can be compared for
// equality with a host model); neighbouring threads read consecutive LDS words for x[q + i], and x[c + i] is a broadcast.
// The best (score, visiting rank) of the block is found by wave shuffles and one LDS step; the order on that key is
// total, so the winner does not depend on the order of the reduction.  Samples from n on are never read.  A row's bits
// depend on its own samples, rate and length alone.
#include <math.h>
#include <stdint.h>

#include "api_internal.h"
#include "warp_common.hip.h"

namespace {

constexpr int ST_TPB = 512;                 // threads of stretch_rows: 2 D + 1 = 321 candidates at the defaults in one pass
constexpr int ST_WAVES = ST_TPB / 64;
constexpr int ST_MIN_HOP = 16, ST_MAX_HOP = 1024;
constexpr int ST_MAX_SEARCH = 1024;
constexpr int ST_NO_RANK = 0x7fffffff;      // the rank of "no candidate yet": behind every real one

struct StretchArgs {
    const float* x;
    float* y;
    const int* lengths;      // null: every row has L samples
    const double* rate;      // [B]
    int* out_len;            // [B] or null
    int* status;             // [B] or null
    int* pos;                // [B, KP] or null
    int* searched;           // [B] or null
    long long ldx, ldy;
    int B, L, N, H, D, KP;   // KP = ceil(N / H): the frames a row can have
};

// (score a, rank ra) is better than (b, rb): the larger score, and among equal scores the earlier visit
__device__ inline bool st_better(double a, int ra, double b, int rb) { return a > b || (a == b && ra < rb); }

__global__ __launch_bounds__(ST_TPB) void stretch_rows(StretchArgs a) {
    __shared__ double s_f[ST_MAX_HOP];                                  // the fade-in weights
    // both spans are kept as float64 (40 KB with the weights): the conversion is then paid once per staged sample, not
    // once per product, and the inner loop is two LDS reads and two multiply-adds
    __shared__ double s_a[2 * ST_MAX_SEARCH + ST_MAX_HOP];              // x[p - D .. p + D + H)
    __shared__ double s_b[ST_MAX_HOP];                                  // x[c .. c + H)
    __shared__ double s_score[ST_WAVES];
    __shared__ int s_rank[ST_WAVES];
    const int t = threadIdx.x, b = blockIdx.x, H = a.H, D = a.D;
    const float* row = a.x + (size_t)b * a.ldx;
    float* out = a.y + (size_t)b * a.ldy;
    int* pos = a.pos ? a.pos + (size_t)b * a.KP : nullptr;
    const double r = a.rate[b];
    const int n = a.lengths ? a.lengths[b] : a.L;
    const bool valid = wp_rate_ok(r) && n >= 0 && n <= a.L;
    long long M = valid ? wp_count(n, r) : 0;
    if (M > a.N) M = a.N;
    const int K = (int)((M + H - 1) / H);
    for (int i = t; i < H; i += ST_TPB) s_f[i] = 0.5 - 0.5 * cospi((double)i / (double)H);
    __syncthreads();

    long long q = 0;
    int n_searched = 0;
    for (int k = 0; k < K; ++k) {
        const long long o0 = (long long)k * H;
        long long c = 0;
        if (k > 0) {
            const long long p = (long long)floor(wp_mul((double)o0, r));          // 0 <= p < n, because o0 < M
            c = q + H;
            const long long off = c - p;
            if (off >= -D && off <= D && c < n) {
                q = c;
            } else {
                ++n_searched;
                const long long a0 = p - D;
                for (int j = t; j < 2 * D + H; j += ST_TPB) {
                    const long long s = a0 + j;
                    s_a[j] = (s >= 0 && s < n) ? (double)row[s] : 0.0;
                }
                for (int i = t; i < H; i += ST_TPB) s_b[i] = (c + i < n) ? (double)row[c + i] : 0.0;
                __syncthreads();
                double best = -INFINITY;
                int best_rank = ST_NO_RANK;
                for (int j = t; j <= 2 * D; j += ST_TPB) {
                    const long long qc = a0 + j;
                    if (qc < 0 || qc >= n) continue;
                    const double* pa = s_a + j;
                    double C = 0.0, E = 0.0;
#pragma unroll 4
                    for (int i = 0; i < H; ++i) {                                  // one ascending chain per sum
                        const double u = pa[i];
                        C = fma(u, s_b[i], C);
                        E = fma(u, u, E);
                    }
                    double s = 2.0 * C - E;
                    if (!(s == s)) s = -INFINITY;
                    const int d = j - D;
                    const int rank = d == 0 ? 0 : (d < 0 ? -2 * d - 1 : 2 * d);
                    if (st_better(s, rank, best, best_rank)) {
                        best = s;
                        best_rank = rank;
                    }
                }
                for (int m = 32; m >= 1; m >>= 1) {
                    const double os = __shfl_xor(best, m);
                    const int orank = __shfl_xor(best_rank, m);
                    if (st_better(os, orank, best, best_rank)) {
                        best = os;
                        best_rank = orank;
                    }
                }
                if ((t & 63) == 0) {
                    s_score[t >> 6] = best;
                    s_rank[t >> 6] = best_rank;
                }
                __syncthreads();
                best = s_score[0];
                best_rank = s_rank[0];
                for (int w = 1; w < ST_WAVES; ++w)
                    if (st_better(s_score[w], s_rank[w], best, best_rank)) {
                        best = s_score[w];
                        best_rank = s_rank[w];
                    }
                // d = 0 is always a candidate, so a rank was found: 0 -> 0, 2 m - 1 -> -m, 2 m -> +m
                const int d = (best_rank & 1) ? -((best_rank + 1) >> 1) : (best_rank >> 1);
                q = p + d;
            }
        }
        if (t == 0 && pos) pos[k] = (int)q;
        for (int i = t; i < H; i += ST_TPB) {
            const long long o = o0 + i;
            if (o >= M) break;
            const long long ia = q + i, ib = c + i;
            const double u = (ia >= 0 && ia < n) ? (double)row[ia] : 0.0;      // (q >= 0 always: d = 0 is a candidate)
            const double v = ib == ia ? u : (ib < n ? (double)row[ib] : 0.0);
            const double f = s_f[i], g = 1.0 - f;
            out[o] = (float)(f * u + g * v);
        }
    }
    for (long long o = M + t; o < a.N; o += ST_TPB) out[o] = 0.0f;
    if (pos)
        for (int k = K + t; k < a.KP; k += ST_TPB) pos[k] = -1;
    if (t == 0) {
        if (a.status) a.status[b] = valid ? 0 : 1;
        if (a.out_len) a.out_len[b] = (int)M;
        if (a.searched) a.searched[b] = n_searched;
    }
}

}  // namespace

extern "C" int cmgan_stretch_max_hop(void) { return ST_MAX_HOP; }

extern "C" int cmgan_stretch_max_search(void) { return ST_MAX_SEARCH; }

extern "C" int cmgan_stretch(cmgan_handle* h, const float* x, int B, int L, long long ldx, const int* lengths, const double* rate,
                             int hop, int search, float* y, int N, long long ldy, int* out_len, int* status, int* pos,
                             int* searched, void* stream) {
    // every argument is judged before the handle is, so that the errors below need no GPU (the message of a call
    // without a handle is read with cmgan_last_error(NULL))
    if (!x || !rate || !y) return fail(h, CMGAN_E_BADARG, "cmgan_stretch: null pointer");
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)lengths | (uintptr_t)out_len | (uintptr_t)status | (uintptr_t)pos |
         (uintptr_t)searched) & 3)
        return fail(h, CMGAN_E_BADARG, "cmgan_stretch: float32 / int32 buffers must be 4-byte aligned");
    if ((uintptr_t)rate & 7) return fail(h, CMGAN_E_BADARG, "cmgan_stretch: the float64 rates must be 8-byte aligned");
    if (B < 1 || B > 65535 || L < 1 || N < 1 || ldx < L || ldy < N)
        return fail(h, CMGAN_E_BADARG, "cmgan_stretch: need 1 <= B <= 65535, L >= 1, N >= 1, ldx >= L, ldy >= N (B=%d L=%d "
                    "N=%d ldx=%lld ldy=%lld)", B, L, N, ldx, ldy);
    if (hop < ST_MIN_HOP || hop > ST_MAX_HOP)
        return fail(h, CMGAN_E_BADARG, "cmgan_stretch: hop must lie in [%d, %d] (hop=%d)", ST_MIN_HOP, ST_MAX_HOP, hop);
    if (search < 0 || search > ST_MAX_SEARCH)
        return fail(h, CMGAN_E_BADARG, "cmgan_stretch: search must lie in [0, %d] (search=%d)", ST_MAX_SEARCH, search);
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + ((size_t)(B - 1) * (size_t)ldx + (size_t)L) * sizeof(float);
    const uintptr_t y0 = (uintptr_t)y, y1 = y0 + ((size_t)(B - 1) * (size_t)ldy + (size_t)N) * sizeof(float);
    if (x0 < y1 && y0 < x1) return fail(h, CMGAN_E_BADARG, "cmgan_stretch: x and y overlap");
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "cmgan_stretch: null handle");
    const LaunchCtx ctx = begin(h, stream);
    StretchArgs a;
    a.x = x;
    a.y = y;
    a.lengths = lengths;
    a.rate = rate;
    a.out_len = out_len;
    a.status = status;
    a.pos = pos;
    a.searched = searched;
    a.ldx = ldx;
    a.ldy = ldy;
    a.B = B;
    a.L = L;
    a.N = N;
    a.H = hop;
    a.D = search;
    a.KP = (int)(((long long)N + hop - 1) / hop);
    LAUNCH(ctx, "stretch_rows", stretch_rows<<<dim3(B), ST_TPB, 0, ctx.stream>>>(a));
    return check_launch(h, "stretch");
}
