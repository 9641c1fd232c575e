// warp.hip - speed perturbation of a [B, L] float32 batch on the device (cmgan_warp, include/cmgan_hip.h): every row is
// resampled by its OWN rate, any float64 in [1/4, 4], read from device memory.  The reference has no counterpart: its
// data path replays fixed pairs (src/data/dataloader.py).  For row b with n = lengths[b] (L without lengths) and
// r = rate[b] input samples per output sample, everything in float64:
//
//   t_i  = fl(i r)                                      the time of output i, one rounded product
//   M    = min(N, #{i >= 0 : t_i < n})                  out_len[b]; outputs from M on are zeros
//   fc   = rolloff (r > 1 ? 1 / r : 1),   W = zeros / fc
//   h(d) = fc sinc(fc d) (0.5 + 0.5 cospi(d / W))  for |d| < W,   sinc(z) = sinpi(z) / (pi z), sinc(0) = 1
//   y[b, i] = f32( sum_k x[b, k] h(t_i - k) )           over the integers k with |t_i - k| < W and 0 <= k < n, ascending
//
// A row whose rate is not a finite number in [1/4, 4], or whose length lies outside [0, L], is INVALID: N zeros,
// status 1, out_len 0.  One launch, no workspace, no atomics: a block owns WP_TILE consecutive outputs of one row, a
// thread one of them.  The input span the tile reaches (at most 4 WP_TILE + 2 x 512 + a few samples) is staged in LDS
// with 16-byte loads; samples from n on are never read.
// The per-tap cost would be a sine and a cosine.  Both angles fall by a constant from one tap to the next (pi fc for
// the sinc, pi / W for the window), so a thread evaluates sinpi / cospi at its first tap and then turns the two
// (sin, cos) pairs by the angle-addition identities with cospi / sinpi of the step.  Two things are kept direct:
//   - the taps with |d| < 1 (at most two per output) take sinpi(fc d) and cospi(d / W) themselves: there the quotient
//     sin / (pi fc d) would magnify the turned pair's absolute error, and h(0) is exactly fc;
//   - with fc = 1 the step is (cospi(1), sinpi(1)) = (-1, 0) exactly, so a pair that starts at an integer d keeps an
//     exact zero sine: r = 1 with rolloff = 1 copies the row bit for bit.
// A thread's sum depends on its own row's samples, rate and length alone, in ascending k: the same bits from run to run,
// whatever B, the neighbours, the padding behind ldx / ldy or L beyond n are.
#include <math.h>
#include <stdint.h>

#include "api_internal.h"
#include "warp_common.hip.h"

namespace {

constexpr int WP_TPB = 256;                 // threads of warp_rows
constexpr int WP_TILE = WP_TPB;             // outputs per block, one per thread
constexpr int WP_MIN_ZEROS = 4, WP_MAX_ZEROS = 64;
constexpr double WP_MIN_ROLLOFF = 0.5;
constexpr int WP_MAX_W = 512;               // zeros / fc <= 64 x 4 / 0.5
constexpr int WP_SPAN = 4 * WP_TILE + 2 * WP_MAX_W + 64;   // floats of LDS: the span of a tile, its alignment, slack
constexpr long long WP_MAX_N = 1LL << 50;   // cmgan_warp_out_len: lengths whose products stay exact integers
constexpr double WP_PI = 3.14159265358979323846;

// (wp_mul, wp_rate_ok and wp_count: warp_common.hip.h, shared with stretch.hip)

// the integers k with |t - k| < W, judged on the float64 difference: [k0, k1] before the clamp to the row
__device__ inline void wp_support(double t, double W, long long& k0, long long& k1) {
    long long a = (long long)floor(t - W);
    while (!(t - (double)a < W)) ++a;
    while (t - (double)(a - 1) < W) --a;
    long long b = (long long)ceil(t + W);
    while (!(t - (double)b > -W)) --b;
    while (t - (double)(b + 1) > -W) ++b;
    k0 = a;
    k1 = b;
}

struct WarpArgs {
    const float* x;
    float* y;
    const int* lengths;      // null: every row has L samples
    const double* rate;      // [B]
    int* out_len;            // [B] or null
    int* status;             // [B] or null
    double rolloff;
    long long ldx, ldy;
    int B, L, N, zeros;
};

__global__ __launch_bounds__(WP_TPB) void warp_rows(WarpArgs a) {
    __shared__ __attribute__((aligned(16))) float s_x[WP_SPAN];
    const int t = threadIdx.x, b = blockIdx.y;
    const long long o0 = (long long)blockIdx.x * WP_TILE, o = o0 + t;
    float* out = a.y + (size_t)b * a.ldy;
    const double r = a.rate[b];
    const int n = a.lengths ? a.lengths[b] : a.L;
    const bool valid = wp_rate_ok(r) && n >= 0 && n <= a.L;
    long long M = valid ? wp_count(n, r) : 0;
    if (M > a.N) M = a.N;
    if (blockIdx.x == 0 && t == 0) {
        if (a.status) a.status[b] = valid ? 0 : 1;
        if (a.out_len) a.out_len[b] = (int)M;
    }
    if (o0 >= M) {                                                      // the whole tile: an invalid row, or past the row's end
        if (o < a.N) out[o] = 0.0f;
        return;
    }
    const double fc = a.rolloff * (r > 1.0 ? 1.0 / r : 1.0);
    const double W = (double)a.zeros / fc;
    const int cnt = M - o0 < WP_TILE ? (int)(M - o0) : WP_TILE;
    // the span of the tile: the times rise with the output index, and so do both ends of the support
    long long ka, kb, k0, k1;
    wp_support(wp_mul((double)o0, r), W, ka, k1);
    wp_support(wp_mul((double)(o0 + cnt - 1), r), W, k0, kb);
    if (ka < 0) ka = 0;
    if (kb > n - 1) kb = n - 1;
    const float* row = a.x + (size_t)b * a.ldx;
    // `front` samples are loaded in front of the span so that every float4 is 16-byte aligned in memory
    const int front = (int)((((unsigned long long)(uintptr_t)row >> 2) + (unsigned long long)ka) & 3ull);
    const long long qa = ka - front;
    int nvec = ((int)(kb - ka) + 1 + front + 3) >> 2;
    if (nvec > WP_SPAN / 4) nvec = WP_SPAN / 4;                         // (never: WP_SPAN covers the widest tile)
    for (int v = t; v < nvec; v += WP_TPB) {
        const long long q = qa + 4 * (long long)v;
        float4 f;
        if (q >= 0 && q + 3 < n) {
            f = *reinterpret_cast<const float4*>(row + q);
        } else {
            f.x = (q >= 0 && q < n) ? row[q] : 0.f;
            f.y = (q + 1 >= 0 && q + 1 < n) ? row[q + 1] : 0.f;
            f.z = (q + 2 >= 0 && q + 2 < n) ? row[q + 2] : 0.f;
            f.w = (q + 3 >= 0 && q + 3 < n) ? row[q + 3] : 0.f;
        }
        *reinterpret_cast<float4*>(s_x + 4 * v) = f;
    }
    __syncthreads();
    if (t >= cnt) {
        if (o < a.N) out[o] = 0.0f;
        return;
    }
    const double tn = wp_mul((double)o, r);
    wp_support(tn, W, k0, k1);
    if (k0 < ka) k0 = ka;                                              // the clamp to [0, n): the span has it already
    if (k1 > kb) k1 = kb;
    if (k1 - qa >= 4LL * nvec) k1 = qa + 4LL * nvec - 1;               // (never)
    const int taps = (int)(k1 - k0) + 1;
    const float* xs = s_x + (int)(k0 - qa);
    // the step of both angles, and the pairs at the first tap
    const double cd = cospi(fc), sd = sinpi(fc), cwd = cospi(1.0 / W), swd = sinpi(1.0 / W);
    const double d0 = tn - (double)k0;
    double s = sinpi(fc * d0), c = cospi(fc * d0), ws = sinpi(d0 / W), wc = cospi(d0 / W);
    double acc = 0.0;
    for (int j = 0; j < taps; ++j) {
        const double d = tn - (double)(k0 + j);
        double sj = s, wj = wc;
#ifdef WARP_DIRECT_TRIG                                                 // the A/B build: sinpi / cospi at every tap
        {
#else
        if (fabs(d) < 1.0) {
#endif
            sj = sinpi(fc * d);
            wj = cospi(d / W);
        }
        const double sinc = d == 0.0 ? 1.0 : sj / (WP_PI * (fc * d));
        const double h = fc * sinc * (0.5 + 0.5 * wj);
        acc = fma((double)xs[j], h, acc);
        const double s2 = s * cd - c * sd, c2 = c * cd + s * sd;       // d falls by 1: both angles by their step
        const double ws2 = ws * cwd - wc * swd, wc2 = wc * cwd + ws * swd;
        s = s2;
        c = c2;
        ws = ws2;
        wc = wc2;
    }
    out[o] = (float)acc;
}

}  // namespace

extern "C" int cmgan_warp_tile(void) { return WP_TILE; }

extern "C" double cmgan_warp_max_rate(void) { return WP_MAX_RATE; }

extern "C" int cmgan_warp_max_zeros(void) { return WP_MAX_ZEROS; }

extern "C" long long cmgan_warp_out_len(long long n, double rate) {
    if (n < 0 || n > WP_MAX_N || !wp_rate_ok(rate)) return -1;
    return wp_count(n, rate);
}

extern "C" int cmgan_warp(cmgan_handle* h, const float* x, int B, int L, long long ldx, const int* lengths, const double* rate,
                          int zeros, double rolloff, float* y, int N, long long ldy, int* out_len, int* status, void* stream) {
    // every argument is judged before the handle is, so that the errors below need no GPU (the message of a call
    // without a handle is read with cmgan_last_error(NULL))
    if (!x || !rate || !y) return fail(h, CMGAN_E_BADARG, "cmgan_warp: null pointer");
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)lengths | (uintptr_t)out_len | (uintptr_t)status) & 3)
        return fail(h, CMGAN_E_BADARG, "cmgan_warp: float32 / int32 buffers must be 4-byte aligned");
    if ((uintptr_t)rate & 7) return fail(h, CMGAN_E_BADARG, "cmgan_warp: the float64 rates must be 8-byte aligned");
    if (B < 1 || B > 65535 || L < 1 || N < 1 || ldx < L || ldy < N)
        return fail(h, CMGAN_E_BADARG, "cmgan_warp: need 1 <= B <= 65535, L >= 1, N >= 1, ldx >= L, ldy >= N (B=%d L=%d N=%d "
                    "ldx=%lld ldy=%lld)", B, L, N, ldx, ldy);
    if (zeros < WP_MIN_ZEROS || zeros > WP_MAX_ZEROS)
        return fail(h, CMGAN_E_BADARG, "cmgan_warp: zeros must lie in [%d, %d] (zeros=%d)", WP_MIN_ZEROS, WP_MAX_ZEROS, zeros);
    if (!(rolloff >= WP_MIN_ROLLOFF && rolloff <= 1.0))                // a NaN fails
        return fail(h, CMGAN_E_BADARG, "cmgan_warp: rolloff must lie in [%g, 1] (rolloff=%g)", WP_MIN_ROLLOFF, rolloff);
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + ((size_t)(B - 1) * (size_t)ldx + (size_t)L) * sizeof(float);
    const uintptr_t y0 = (uintptr_t)y, y1 = y0 + ((size_t)(B - 1) * (size_t)ldy + (size_t)N) * sizeof(float);
    if (x0 < y1 && y0 < x1) return fail(h, CMGAN_E_BADARG, "cmgan_warp: x and y overlap");
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "cmgan_warp: null handle");
    const LaunchCtx ctx = begin(h, stream);
    WarpArgs a;
    a.x = x;
    a.y = y;
    a.lengths = lengths;
    a.rate = rate;
    a.out_len = out_len;
    a.status = status;
    a.rolloff = rolloff;
    a.ldx = ldx;
    a.ldy = ldy;
    a.B = B;
    a.L = L;
    a.N = N;
    a.zeros = zeros;
    const dim3 grid((unsigned)(((long long)N + WP_TILE - 1) / WP_TILE), B);
    LAUNCH(ctx, "warp_rows", warp_rows<<<grid, WP_TPB, 0, ctx.stream>>>(a));
    return check_launch(h, "warp");
}
