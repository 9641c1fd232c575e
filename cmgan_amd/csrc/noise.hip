// noise.hip - synthetic noise on the device (cmgan_noise, include/cmgan_hip.h): every row of a float32 [N, K] array is a
// fresh noise of its own colour, modulation, hum and clicks, made from a seed and a few small per-row tables.  The
// reference ships no noise and no generator (src/data/dataloader.py:13-50 replays pairs mixed beforehand).  Row r is, for
// 0 <= k < len[r] with the absolute sample index n = start[r] + k:
//
//   nu[q]  = (w0 + w1 + w2 + w3 - 2 (2^32 - 1)) / sqrt((2^64 - 1) / 3), (w0 .. w3) = Philox4x32-10 at counter (q mod 2^32,
//            q div 2^32, 0, 0) under the key seed[r]: the noise of rir_tail.hip, which stops at q < 2^32.  The numerator is an
//            integer below 2^34, the division is IEEE's
//   imp[q] = imp_amp ((double)((int64)v1 - 2^31) / 2^31) if v0 < imp_thr, else 0, (v0, v1, ..) = Philox at counter (q mod
//            2^32, q div 2^32, 1, 0); imp_thr = 0: no clicks and no second Philox block
//   e[q]   = nu[q] + imp[q], 0 for q < 0
//   s[n]   = sum_j fir[r][j] e[n - j], j ascending, one fma per term into one accumulator from 0
//   g[n]   = fma(env[r][p1] - env[r][p0], (double)(n - p0 H) / (double)H, env[r][p0]), p0 = min(n div H, P - 1), p1 = min(p0 + 1,
//            P - 1); 1 without an envelope
//   t[n]   = sum_m amp_m sinpi(2 frac(fma(nu_m, (double)n, phi_m))), m ascending, one fma per term from 0, frac(x) = x - floor(x)
//   y[k]   = (float) fma(g[n], s[n], t[n]); 0 for len[r] <= k < K
//
// Every sample is a pure function of (the row's tables, n): a row made whole and the same row made in chunks with `start`
// advanced have the same bits.  Float64 on the VALU, no atomics, two launches:
//   noise_judge  one block per row.  It reads every table entry the row uses and writes the verdict - the row's length, or
//                -1 for an invalid row - to the workspace, and the status.
//   noise_rows   grid (tile of NZ_TILE = 256 outputs, row), one output per thread.  e is computed once for the NZ_TILE + NF - 1
//                indices the tile's outputs reach - one Philox block per index, a second only where the row has clicks - and
//                staged in LDS as float64 (10.2 KB at NF = 1023); a thread then runs its NF fmas, consecutive threads
//                reading consecutive float64 (a half wave covers the 64 banks of an 8-byte read once).  The tap is the
//                same for the whole block: it comes from the row's table through scalar loads, eight taps at a time, and
//                is an SGPR operand of the fma - staged in LDS too, every fma would cost a second LDS read, and the LDS is
//                what bounds this loop (tools/probes/noise_taps_lds.patch: 1.5 times as long from 255 taps on).  Envelope
//                and tones follow, and one store.  Tiles at or beyond the row's length write their zeros.
// A row's bits depend on its own table entries alone: neither on N, nor on the other rows, nor on ld, nor on K beyond len.
// Nothing read from device memory becomes an address without a clamp: the length is clamped to [0, K], the tone count to
// [0, M], the envelope index to [0, P - 1]; a start only enters counters and arithmetic.
#include <math.h>
#include <stdint.h>

#include "api_internal.h"
#include "host_ranges.h"
#include "philox.hip.h"

namespace {

constexpr int NZ_TPB = 256;                   // threads of both kernels
constexpr int NZ_TILE = NZ_TPB;               // outputs per block of noise_rows
constexpr int NZ_MAX_FILTER = 1023;           // = cmgan_noise_max_filter()
constexpr int NZ_MAX_TONES = 8;               // = cmgan_noise_max_tones()
constexpr int NZ_MAX_POINTS = 4096;           // = cmgan_noise_max_points()
constexpr int NZ_SPAN = NZ_TILE + NZ_MAX_FILTER - 1;
constexpr int NZ_MAX_K = 2147483647 - NZ_TILE;
constexpr long long NZ_MAX_INDEX = 1LL << 40; // start + K may not exceed it
constexpr double NZ_NOISE_DIV = CMGAN_RIR_TAIL_NOISE_DIV;
constexpr double NZ_2P31 = 2147483648.0, NZ_2P32 = 4294967296.0;

struct NoiseArgs {
    float* out;
    const long long* seed;   // [N]
    const long long* start;  // [N] or null
    const int* len;          // [N] or null
    const double* fir;       // [N][NF]
    const double* env;       // [N][P] or null
    const double* tones;     // [N][M][3] or null
    const int* n_tones;      // [N] or null (M for every row)
    const double* imp;       // [N][2] or null
    int* status;             // [N]
    int* verdict;            // workspace [N]: the row's length in [0, K], or -1 for an invalid row
    long long ld;
    int N, K, NF, P, H, M;
};

__device__ inline bool nz_finite(double v) { return v - v == 0.0; }

// e[q] of the row with the key (k0, k1): nu[q], plus a click where the second block's first word is below thr
__device__ inline double nz_excite(long long q, unsigned k0, unsigned k1, unsigned thr, double amp) {
#pragma clang fp contract(off)
    if (q < 0) return 0.0;
    const unsigned lo = (unsigned)((unsigned long long)q & 0xffffffffull), hi = (unsigned)((unsigned long long)q >> 32);
    unsigned c[4] = {lo, hi, 0u, 0u};
    philox4x32_10(c, k0, k1);
    const long long sum = (long long)c[0] + (long long)c[1] + (long long)c[2] + (long long)c[3] - 2LL * 4294967295LL;
    const double nu = (double)sum / NZ_NOISE_DIV;
    if (thr == 0u) return nu;
    unsigned v[4] = {lo, hi, 1u, 0u};
    philox4x32_10(v, k0, k1);
    const double imp = v[0] < thr ? amp * ((double)((long long)v[1] - 2147483648LL) / NZ_2P31) : 0.0;
    return nu + imp;
}

// ---------------------------------------------------------------- the judge
__global__ __launch_bounds__(NZ_TPB) void noise_judge(NoiseArgs a) {
    const int t = threadIdx.x, r = blockIdx.x;
    int bad = 0;
    const int len = a.len ? a.len[r] : a.K;
    if (len < 0 || len > a.K) bad = 1;
    const long long start = a.start ? a.start[r] : 0;
    if (start < 0 || start > NZ_MAX_INDEX - (long long)a.K) bad = 1;
    int nt = a.tones ? (a.n_tones ? a.n_tones[r] : a.M) : 0;
    if (nt < 0 || nt > a.M) bad = 1, nt = 0;                      // the row's tones are then not read
    const double* fir = a.fir + (size_t)r * a.NF;
    for (int i = t; i < a.NF; i += NZ_TPB) bad |= nz_finite(fir[i]) ? 0 : 1;
    if (a.env) {
        const double* env = a.env + (size_t)r * a.P;
        for (int i = t; i < a.P; i += NZ_TPB) bad |= nz_finite(env[i]) ? 0 : 1;
    }
    if (t < nt) {
        const double* tn = a.tones + ((size_t)r * a.M + t) * 3;
        if (!(tn[0] >= 0.0 && tn[0] <= 0.5) || !nz_finite(tn[1]) || !nz_finite(tn[2])) bad = 1;     // a NaN compares false
    }
    if (a.imp && t == 0) {
        const double thr = a.imp[(size_t)r * 2], amp = a.imp[(size_t)r * 2 + 1];
        if (!(thr >= 0.0 && thr < NZ_2P32) || thr != floor(thr) || !nz_finite(amp)) bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (t == 0) a.verdict[r] = bad ? -1 : len, a.status[r] = bad ? 1 : 0;
}

// ---------------------------------------------------------------- the rows
__global__ __launch_bounds__(NZ_TPB) void noise_rows(NoiseArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_e[NZ_SPAN];
    const int t = threadIdx.x, r = blockIdx.y;
    const int k0 = blockIdx.x * NZ_TILE, k = k0 + t;
    const int verdict = a.verdict[r];
    const int len = verdict < 0 ? 0 : (verdict > a.K ? a.K : verdict);
    float* out = a.out + (size_t)r * a.ld;
    if (k0 >= len) {                                              // (the whole block: nothing of this tile is a sample)
        if (k < a.K) out[k] = 0.f;
        return;
    }
    const int NF = a.NF, span = NZ_TILE + NF - 1;
    const long long start = a.start ? a.start[r] : 0;
    const long long base = start + (long long)k0 - (long long)(NF - 1);      // s_e[i] = e[base + i]
    const unsigned long long key = (unsigned long long)a.seed[r];
    unsigned thr = 0u;
    double amp = 0.0;
    if (a.imp) thr = (unsigned)a.imp[(size_t)r * 2], amp = a.imp[(size_t)r * 2 + 1];    // (judged: a whole number below 2^32)
    for (int i = t; i < span; i += NZ_TPB) s_e[i] = nz_excite(base + i, (unsigned)key, (unsigned)(key >> 32), thr, amp);
    const double* __restrict__ fir = a.fir + (size_t)r * NF;
    __syncthreads();
    if (k >= len) {
        if (k < a.K) out[k] = 0.f;
        return;
    }
    const double* ep = s_e + t + NF - 1;                          // e[n - j] = s_e[t + NF - 1 - j]
    double s = 0.0;
    for (int j = 0; j < NF; ++j) s = fma(fir[j], ep[-j], s);        // fir[j]: one address for the block, a scalar load
    const long long n = start + (long long)k;
    double g = 1.0;
    if (a.env) {
        const double* env = a.env + (size_t)r * a.P;
        const long long d = n / (long long)a.H;
        const int p0 = d < (long long)(a.P - 1) ? (int)d : a.P - 1;
        const int p1 = p0 + 1 < a.P ? p0 + 1 : a.P - 1;
        const double e0 = env[p0], frac = (double)(n - (long long)p0 * (long long)a.H) / (double)a.H;
        g = fma(env[p1] - e0, frac, e0);
    }
    double tone = 0.0;
    if (a.tones) {
        int nt = a.n_tones ? a.n_tones[r] : a.M;
        nt = nt < 0 ? 0 : (nt > a.M ? a.M : nt);
        const double* tn = a.tones + (size_t)r * a.M * 3;
        for (int m = 0; m < nt; ++m) {
            const double x = fma(tn[3 * m], (double)n, tn[3 * m + 2]);
            tone = fma(tn[3 * m + 1], sinpi(2.0 * (x - floor(x))), tone);
        }
    }
    out[k] = (float)fma(g, s, tone);
}

// ---------------------------------------------------------------- the host side
}  // namespace

extern "C" int cmgan_noise_tile(void) { return NZ_TILE; }
extern "C" int cmgan_noise_max_filter(void) { return NZ_MAX_FILTER; }
extern "C" int cmgan_noise_max_tones(void) { return NZ_MAX_TONES; }
extern "C" int cmgan_noise_max_points(void) { return NZ_MAX_POINTS; }

extern "C" size_t cmgan_noise_workspace_bytes(int N) { return N >= 1 && N <= 65535 ? up256((size_t)N * sizeof(int)) : 0; }

extern "C" int cmgan_noise(cmgan_handle* h, float* out, int N, int K, long long ld, const long long* seed, const long long* start,
                           const int* len, const double* fir, int NF, const double* env, int P, int H, const double* tones,
                           const int* n_tones, int M, const double* imp, int* status, void* ws, size_t ws_bytes, void* stream) {
    // every argument is judged before the handle is, so that the errors below need no GPU (the message of a call
    // without a handle is read with cmgan_last_error(NULL))
    if ((!out && K > 0) || !seed || !fir || !status) return fail(h, CMGAN_E_BADARG, "cmgan_noise: null pointer");
    if (((uintptr_t)out | (uintptr_t)len | (uintptr_t)n_tones | (uintptr_t)status) & 3)
        return fail(h, CMGAN_E_BADARG, "cmgan_noise: float32 / int32 buffers must be 4-byte aligned");
    if (((uintptr_t)seed | (uintptr_t)start | (uintptr_t)fir | (uintptr_t)env | (uintptr_t)tones | (uintptr_t)imp) & 7)
        return fail(h, CMGAN_E_BADARG, "cmgan_noise: float64 / int64 buffers must be 8-byte aligned");
    if (N < 1 || N > 65535 || K < 0 || K > NZ_MAX_K || ld < K)
        return fail(h, CMGAN_E_BADARG, "cmgan_noise: need 1 <= N <= 65535, 0 <= K <= 2^31 - 1 - %d, ld >= K (N=%d K=%d ld=%lld)",
                    NZ_TILE, N, K, ld);
    if (NF < 1 || NF > NZ_MAX_FILTER)
        return fail(h, CMGAN_E_BADARG, "cmgan_noise: need 1 <= NF <= %d filter taps (NF=%d)", NZ_MAX_FILTER, NF);
    if (env ? (P < 1 || P > NZ_MAX_POINTS || H < 1) : (P != 0 || H != 0))
        return fail(h, CMGAN_E_BADARG, "cmgan_noise: an envelope needs 1 <= P <= %d points and a hop H >= 1, none needs P = H = 0 "
                    "(P=%d H=%d)", NZ_MAX_POINTS, P, H);
    if (M < 0 || M > NZ_MAX_TONES || (M == 0) != (tones == nullptr) || (n_tones && !tones))
        return fail(h, CMGAN_E_BADARG, "cmgan_noise: need 0 <= M <= %d tones, the tone table null with M = 0 and only then, and "
                    "no tone counts without it (M=%d)", NZ_MAX_TONES, M);
    const size_t need = up256((size_t)N * sizeof(int));
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < need)
        return fail(h, CMGAN_E_BADARG, "cmgan_noise: the workspace must be 256-byte aligned and hold %zu bytes (%zu given)",
                    need, ws ? ws_bytes : (size_t)0);
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "cmgan_noise: null handle");
    const LaunchCtx ctx = begin(h, stream);
    hipStream_t s = ctx.stream;
    NoiseArgs a;
    a.out = out;
    a.seed = seed;
    a.start = start;
    a.len = len;
    a.fir = fir;
    a.env = env;
    a.tones = tones;
    a.n_tones = n_tones;
    a.imp = imp;
    a.status = status;
    a.verdict = (int*)ws;
    a.ld = ld;
    a.N = N, a.K = K, a.NF = NF, a.P = P, a.H = H, a.M = M;
    LAUNCH(ctx, "noise_judge", noise_judge<<<N, NZ_TPB, 0, s>>>(a));
    if (K > 0) LAUNCH(ctx, "noise_rows", noise_rows<<<dim3((K + NZ_TILE - 1) / NZ_TILE, N), NZ_TPB, 0, s>>>(a));
    return check_launch(h, "noise");
}
