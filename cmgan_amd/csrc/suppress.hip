// suppress.hip - the recording device's own single-channel noise suppressor on a [B, L] float32 batch (cmgan_suppress,
// include/cmgan_hip.h, "Suppression"): a short-time spectral gain from a minimum-tracking noise estimate and the
// decision-directed a-priori SNR, by the Wiener rule, power spectral subtraction or Ephraim and Malah's log-MMSE rule.
// The reference has no counterpart: its data path replays fixed pairs (src/data/dataloader.py).  For row b with n =
// lengths[b] (L without lengths), n_fft = N, h = N / 2, F = N / 2 + 1, T_b = ceil(n / h) + 1, w[k] = sin(pi k / N) and the
// table row (rule, a_dd, a_n, D, bias, g_min, xi_min):
//
//   Y_t[f] = sum_k x~[(t-1) h + k] w[k] e^{-2 pi i f k / N};  K_t the same from the key (x without one);  A_t = |K_t|^2
//   P_t    = a_n P_{t-1} + (1 - a_n) A_t, P_{-1} = A_0;   lam_t = max(bias min_{t-D < u <= t} P_u, 2^-60);   gam_t = min(A_t / lam_t, 40)
//   xi_t   = max(a_dd G_{t-1}^2 gam_{t-1} + (1 - a_dd) max(gam_t - 1, 0), xi_min)  (t = 0: without the first term);   q = xi_t / (1 + xi_t)
//   G_t    = max(g_min, q | sqrt(q) | min(q exp(E1(max(q gam_t, 2^-30)) / 2), 1))  for rule 1 | 2 | 3
//   z_t    = irfft(G_t Y_t);   y[t h + r] = f32(z_t[r + h] w[r + h] + z_{t+1}[r] w[r])
//
// Three launches, no atomics, float64 throughout with one rounding to float32.
//   suppress_analyse  a block per (row, frame): the windowed frame goes to LDS as complex float64 in bit-reversed order
//                     (16 KB at N = 1024), a radix-2 transform runs there with twiddles the block makes itself (sincospi of
//                     an exact argument, 8 KB), and bins 0 .. N / 2 go to the workspace as complex128 [B, T, F]; A goes to a
//                     float64 [B, T, F] plane.  With a key the SAME loop body runs a second time on the key's frame, so a
//                     key that is x gives the bits of no key.
//   suppress_gain     a thread per (row, bin), a wave per 64 consecutive bins, walks t: the loads along f coalesce, the next
//                     frame's A is asked for before this frame's step.  The minimum over the last D values is exact,
//                     whatever keeps it: time is cut into blocks of D frames, a ring of D values per thread in LDS ([D][64],
//                     64 KB at D = 128) holds the running block, at every block's end one backward pass turns it into
//                     suffix minima, and the window's minimum is min(suffix of the block before, prefix of this one): two
//                     LDS reads and two writes per step however long the window is.  G overwrites A in place.
//   suppress_synth    a block per (row, h outputs) rebuilds the two frames the span needs: G Y and its mirror image go to
//                     LDS, the inverse transform runs on both at once, and the earlier frame's second half and the later
//                     frame's first are windowed, added and rounded.  It reads the workspace alone, so in place and out of
//                     place are one path.  Rows of rule 0 are copied, invalid rows and samples from n on are zeros.
// E1 by two fixed formulas (the header states them): a Horner series of SP_E1_TERMS fused multiply-adds below 2, with the
// coefficients riding in the kernel arguments (scalar registers), and from 2 on a continued fraction of depth
// SP_E1_DEPTH run backwards as a ratio (n, d), two products and a difference per level and ONE division at the end.
// The LDS store rule, the twiddles and the radix-2 passes are lds_f64.hip.h's, shared with auxloss.hip and stoiloss.hip.
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "api_internal.h"
#include "host_ranges.h"
#include "lds_f64.hip.h"

namespace {

constexpr int SP_TPB = 256;                 // threads of the two transform kernels
constexpr int SP_MAX_N = 1024;
constexpr int SP_MAX_WINDOW = 128;          // D
constexpr int SP_LANES = 64;                // bins per block of suppress_gain: one wave
constexpr int SP_E1_TERMS = 26, SP_E1_DEPTH = 40;
constexpr double SP_E1_SPLIT = 2.0;
constexpr double SP_EULER = 0.57721566490153286060651209008240243;
constexpr double SP_GAMMA_MAX = 40.0, SP_LAM_MIN = 0x1p-60, SP_V_MIN = 0x1p-30;
constexpr int SP_MAX_L = 2147483647 - 2 * SP_MAX_N;

struct SuppressArgs {
    const float* x;
    const float* key;            // null: x is its own key
    float* y;                    // may be x (in place)
    const int* lengths;          // null: every row has L samples
    const double* table;         // [B][7]
    int* status;                 // [B] or null
    double* gain;                // [B][T][F] or null
    double2* Y;                  // workspace [B][T][F]
    double* AG;                  // workspace [B][T][F]: A, then G
    long long ldx, ldk, ldy;
    int B, L, N, logN, T;        // T = ceil(L / h) + 1
    double e1c[SP_E1_TERMS];     // c_k = (-1)^(k+1) / (k k!), k = 1 .. SP_E1_TERMS
};

struct SpRow {
    double a_dd, a_n, bias, g_min, xi_min;
    int rule, D, n, Tb;          // n = Tb = 0 for an invalid row
    bool ok;
};

__device__ inline SpRow sp_row(const SuppressArgs& a, int b) {
    const double* p = a.table + (size_t)b * 7;
    const double rule = p[0], D = p[3];
    SpRow r;
    r.a_dd = p[1], r.a_n = p[2], r.bias = p[4], r.g_min = p[5], r.xi_min = p[6];
    r.n = a.lengths ? a.lengths[b] : a.L;
    r.ok = (rule == 0.0 || rule == 1.0 || rule == 2.0 || rule == 3.0) && r.a_dd >= 0.0 && r.a_dd < 1.0 && r.a_n >= 0.0 &&
           r.a_n < 1.0 && D >= 1.0 && D <= (double)SP_MAX_WINDOW && D == floor(D) && r.bias > 0.0 && r.bias <= 16.0 &&
           r.g_min > 0.0 && r.g_min <= 1.0 && r.xi_min >= 0.0 && r.xi_min <= 1.0 && r.n >= 0 && r.n <= a.L;   // a NaN compares false
    r.rule = r.ok ? (int)rule : 0;
    r.D = r.ok ? (int)D : 1;
    if (!r.ok) r.n = 0;
    const int h = a.N >> 1;
    r.Tb = r.n > 0 ? (r.n + h - 1) / h + 1 : 0;
    return r;
}

__global__ __launch_bounds__(SP_TPB) void suppress_analyse(SuppressArgs a) {
    __shared__ double2 s_buf[SP_MAX_N];
    __shared__ double2 s_tw[SP_MAX_N / 2];
    const int t = blockIdx.x, b = blockIdx.y, N = a.N, h = N >> 1, F = h + 1;
    const SpRow r = sp_row(a, b);
    if (r.rule == 0 || t >= r.Tb) return;                               // block-uniform
    twiddles<SP_TPB>(s_tw, N);
    const size_t at = ((size_t)b * a.T + t) * F;
    const int passes = a.key ? 2 : 1;
    for (int pass = 0; pass < passes; ++pass) {                         // ONE body for the signal and the key
        const float* src = pass == 0 ? a.x + (size_t)b * a.ldx : a.key + (size_t)b * a.ldk;
        __syncthreads();                                                // the pass before has read s_buf
        for (int k = threadIdx.x; k < N; k += SP_TPB) {
            const long long i = (long long)(t - 1) * h + k;
            const double v = (i >= 0 && i < r.n) ? (double)src[i] : 0.0;
            lds_put(s_buf + bitrev(k, a.logN), v * sinpi((double)k / (double)N), 0.0);
        }
        fft<SP_TPB>(s_buf, s_tw, N, a.logN, 1.0, 1, SP_MAX_N);          // (one frame through the many-frames form, as ever)
        for (int f = threadIdx.x; f < F; f += SP_TPB) {
            const double2 v = s_buf[f];
            if (pass == 0) a.Y[at + f] = v;
            if (pass == passes - 1) a.AG[at + f] = fma(v.x, v.x, v.y * v.y);
        }
    }
}

// E1(x) for x > 0 by the header's two formulas
__device__ inline double sp_e1(const SuppressArgs& a, double x) {
#pragma clang fp contract(off)
    if (x < SP_E1_SPLIT) {
        double s = a.e1c[SP_E1_TERMS - 1];
#pragma unroll
        for (int k = SP_E1_TERMS - 2; k >= 0; --k) s = fma(s, x, a.e1c[k]);
        return (-SP_EULER - log(x)) + s * x;
    }
    double n = x + (double)(2 * SP_E1_DEPTH + 1), d = 1.0;
#pragma unroll 8
    for (int k = SP_E1_DEPTH; k >= 1; --k) {
        const double nn = (x + (double)(2 * k - 1)) * n - (double)(k * k) * d;
        d = n;
        n = nn;
    }
    return exp(-x) * (d / n);
}

__global__ __launch_bounds__(SP_LANES) void suppress_gain(SuppressArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_ring[SP_MAX_WINDOW * SP_LANES];
    const int lane = threadIdx.x, b = blockIdx.y, F = (a.N >> 1) + 1, T = a.T;
    const int f = blockIdx.x * SP_LANES + lane;
    const SpRow r = sp_row(a, b);
    if (blockIdx.x == 0 && lane == 0 && a.status) a.status[b] = r.ok ? 0 : 1;
    if (f >= F) return;                                                 // (no barrier below: a thread's ring is its own)
    const size_t at = (size_t)b * T * F + f;
    double* gout = a.gain ? a.gain + at : nullptr;
    if (r.rule == 0) {                                                  // rule 0, or an invalid row (Tb = 0)
        if (gout)
            for (int t = 0; t < T; ++t) gout[(size_t)t * F] = t < r.Tb ? 1.0 : 0.0;
        return;
    }
    double* ag = a.AG + at;
    lds_double* ring = (lds_double*)(s_ring + lane);                     // (64-bit stores that stay 64-bit: lds_f64.hip.h)
    const double oma_n = 1.0 - r.a_n, oma_dd = 1.0 - r.a_dd;
    const int D = r.D;
    double A = r.Tb > 0 ? ag[0] : 0.0;
    double P = A, pre = INFINITY, Gp = 0.0, gp = 0.0;
    int slot = 0;
    for (int t = 0; t < r.Tb; ++t) {
        const double A_next = t + 1 < r.Tb ? ag[(size_t)(t + 1) * F] : 0.0;     // asked for now, used in the next step
        if (slot == D) {                                                // a block of D frames ends: its suffix minima
            slot = 0;
            double m = INFINITY;
            for (int j = D - 1; j >= 0; --j) {
                m = fmin(m, ring[j * SP_LANES]);
                ring[j * SP_LANES] = m;
            }
            pre = INFINITY;
        }
        P = r.a_n * P + oma_n * A;
        pre = fmin(pre, P);
        const double suf = (t >= D && slot + 1 < D) ? ring[(slot + 1) * SP_LANES] : INFINITY;
        ring[slot * SP_LANES] = P;
        ++slot;
        const double lam = fmax(r.bias * fmin(pre, suf), SP_LAM_MIN);
        const double gam = fmin(A / lam, SP_GAMMA_MAX);
        double xi = oma_dd * fmax(gam - 1.0, 0.0);
        if (t > 0) xi = r.a_dd * (Gp * Gp) * gp + xi;
        xi = fmax(xi, r.xi_min);
        const double q = xi / (1.0 + xi);
        double G;
        if (r.rule == 1) G = q;
        else if (r.rule == 2) G = sqrt(q);
        else G = fmin(q * exp(sp_e1(a, fmax(q * gam, SP_V_MIN)) / 2.0), 1.0);
        G = fmax(G, r.g_min);
        ag[(size_t)t * F] = G;
        if (gout) gout[(size_t)t * F] = G;
        Gp = G;
        gp = gam;
        A = A_next;
    }
    if (gout)
        for (int t = r.Tb; t < T; ++t) gout[(size_t)t * F] = 0.0;
}

__global__ __launch_bounds__(SP_TPB) void suppress_synth(SuppressArgs a) {
    __shared__ double2 s_buf[2 * SP_MAX_N];
    __shared__ double2 s_tw[SP_MAX_N / 2];
    const int j = blockIdx.x, b = blockIdx.y, N = a.N, h = N >> 1, F = h + 1;
    const SpRow r = sp_row(a, b);
    const long long i0 = (long long)j * h;                              // < L
    float* out = a.y + (size_t)b * a.ldy;
    if (i0 >= r.n || r.rule == 0) {                                     // block-uniform: zeros, or the copy of rule 0
        const float* row = a.x + (size_t)b * a.ldx;
        for (int k = threadIdx.x; k < h; k += SP_TPB) {
            const long long i = i0 + k;
            if (i < a.L) out[i] = i < r.n ? row[i] : 0.0f;              // (i < n only at rule 0: samples from n on are never read)
        }
        return;
    }
    twiddles<SP_TPB>(s_tw, N);
    // frames j and j + 1 (both below T_b, because i0 < n): G Y on bins 0 .. N / 2, its conjugate on the mirrored bins
    for (int k = threadIdx.x; k < 2 * F; k += SP_TPB) {
        const int fr = k / F, f = k - fr * F;
        const size_t at = ((size_t)b * a.T + j + fr) * F + f;
        const double g = a.AG[at];
        const double2 v = a.Y[at];
        const bool edge = f == 0 || f == h;                             // their imaginary parts do not reach a real output
        const double re = g * v.x, im = edge ? 0.0 : g * v.y;
        lds_put(s_buf + fr * SP_MAX_N + bitrev(f, a.logN), re, im);
        if (!edge) lds_put(s_buf + fr * SP_MAX_N + bitrev(N - f, a.logN), re, -im);
    }
    fft<SP_TPB>(s_buf, s_tw, N, a.logN, -1.0, 2, SP_MAX_N);
    const double inv = 1.0 / (double)N;                                 // a power of two: exact
    for (int k = threadIdx.x; k < h; k += SP_TPB) {
#pragma clang fp contract(off)
        const long long i = i0 + k;
        if (i < r.n) {
            const double early = (s_buf[k + h].x * inv) * sinpi((double)(k + h) / (double)N);
            const double late = (s_buf[SP_MAX_N + k].x * inv) * sinpi((double)k / (double)N);
            out[i] = (float)(early + late);
        } else if (i < a.L) {
            out[i] = 0.0f;
        }
    }
}

inline bool sp_shape_ok(int B, int L, int N) {
    return B >= 1 && B <= 65535 && L >= 1 && L <= SP_MAX_L && (N == 256 || N == 512 || N == 1024);
}

struct SpLayout {
    size_t Y, AG, total;        // byte offsets: complex128 [B][T][F] | float64 [B][T][F]
    int T, F;
};

inline SpLayout sp_layout(int B, int L, int N) {
    SpLayout l;
    const int h = N / 2;
    l.T = (int)(((long long)L + h - 1) / h) + 1;
    l.F = h + 1;
    const size_t cells = (size_t)B * (size_t)l.T * (size_t)l.F;
    l.Y = 0;
    l.AG = up256(cells * 2 * sizeof(double));
    l.total = l.AG + up256(cells * sizeof(double));
    return l;
}

}  // namespace

extern "C" int cmgan_suppress_max_window(void) { return SP_MAX_WINDOW; }

extern "C" size_t cmgan_suppress_workspace_bytes(int B, int L, int n_fft) {
    return sp_shape_ok(B, L, n_fft) ? sp_layout(B, L, n_fft).total : 0;
}

extern "C" int cmgan_suppress(cmgan_handle* h, const float* x, int B, int L, long long ldx, const float* key, long long ldk,
                              const int* lengths, const double* table, int n_fft, float* y, long long ldy, int* status,
                              double* gain, void* ws, size_t ws_bytes, void* stream) {
    // every argument is judged before the handle is, so that the errors below need no GPU (the message of a call
    // without a handle is read with cmgan_last_error(NULL))
    if (!x || !table || !y) return fail(h, CMGAN_E_BADARG, "cmgan_suppress: null pointer");
    if (((uintptr_t)x | (uintptr_t)key | (uintptr_t)y | (uintptr_t)lengths | (uintptr_t)status) & 3)
        return fail(h, CMGAN_E_BADARG, "cmgan_suppress: float32 / int32 buffers must be 4-byte aligned");
    if (((uintptr_t)table | (uintptr_t)gain) & 7)
        return fail(h, CMGAN_E_BADARG, "cmgan_suppress: float64 buffers must be 8-byte aligned");
    if (n_fft != 256 && n_fft != 512 && n_fft != 1024)
        return fail(h, CMGAN_E_BADARG, "cmgan_suppress: n_fft must be 256, 512 or 1024 (n_fft=%d)", n_fft);
    if (B < 1 || B > 65535 || L < 1 || ldx < L || ldy < L || (key && ldk < L))
        return fail(h, CMGAN_E_BADARG,
                    "cmgan_suppress: need 1 <= B <= 65535, L >= 1, ldx >= L, ldy >= L, ldk >= L with a key (B=%d L=%d ldx=%lld "
                    "ldy=%lld ldk=%lld)", B, L, ldx, ldy, ldk);
    if (L > SP_MAX_L)
        return fail(h, CMGAN_E_BADARG, "cmgan_suppress: rows of up to %d samples are supported (L=%d)", SP_MAX_L, L);
    if (!((const float*)y == x && ldy == ldx) && rows_overlap(x, ldx, y, ldy, B, L))   // in place is the one overlap there may be
        return fail(h, CMGAN_E_BADARG, "cmgan_suppress: x and y overlap; only y == x with ldy == ldx (in place) is allowed");
    if (key && !((const float*)y == key && ldy == ldk) && rows_overlap(key, ldk, y, ldy, B, L))
        return fail(h, CMGAN_E_BADARG, "cmgan_suppress: key and y overlap; only y == key with ldy == ldk is allowed");
    const SpLayout l = sp_layout(B, L, n_fft);
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < l.total)
        return fail(h, CMGAN_E_BADARG, "cmgan_suppress: the workspace must be 256-byte aligned and hold %zu bytes (%zu given)",
                    l.total, ws ? ws_bytes : (size_t)0);
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "cmgan_suppress: null handle");
    const LaunchCtx ctx = begin(h, stream);
    hipStream_t s = ctx.stream;
    char* w = (char*)ws;
    SuppressArgs a;
    a.x = x;
    a.key = key;
    a.y = y;
    a.lengths = lengths;
    a.table = table;
    a.status = status;
    a.gain = gain;
    a.Y = (double2*)(w + l.Y);
    a.AG = (double*)(w + l.AG);
    a.ldx = ldx;
    a.ldk = key ? ldk : 0;
    a.ldy = ldy;
    a.B = B;
    a.L = L;
    a.N = n_fft;
    a.logN = n_fft == 256 ? 8 : (n_fft == 512 ? 9 : 10);
    a.T = l.T;
    double fact = 1.0;
    for (int k = 1; k <= SP_E1_TERMS; ++k) {                           // c_k = (-1)^(k+1) / (k k!), k! a running float64 product
        fact = fact * (double)k;
        a.e1c[k - 1] = ((k & 1) ? 1.0 : -1.0) / ((double)k * fact);
    }
    LAUNCH(ctx, "suppress_analyse", suppress_analyse<<<dim3(l.T, B), SP_TPB, 0, s>>>(a));
    LAUNCH(ctx, "suppress_gain", suppress_gain<<<dim3((l.F + SP_LANES - 1) / SP_LANES, B), SP_LANES, 0, s>>>(a));
    LAUNCH(ctx, "suppress_synth", suppress_synth<<<dim3(l.T - 1, B), SP_TPB, 0, s>>>(a));
    return check_launch(h, "suppress");
}
