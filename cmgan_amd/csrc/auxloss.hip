// auxloss.hip - two auxiliary training objectives on a pair of [B, L] float32 batches, with their gradient (cmgan_aux_loss,
// include/cmgan_hip.h, "Auxiliary losses"): the multi-resolution STFT loss (spectral convergence + log-magnitude L1 at up
// to four window lengths) and negative SI-SDR.  The reference has no counterpart: its generator loss sees one resolution
// (src/train.py:124-151).  For estimate e, reference r, resolution n (hop h = n / 4, F = n / 2 + 1, T = 1 + L / h, periodic
// Hann window w, frames centred with reflect padding of n / 2):
//
//   X_x[t, f] = sum_k w[k] x~[t h + k] e^{-2 pi i f k / n};   m_x = sqrt(max(|X_x|^2, 1e-7))            x in {e, r}
//   N = sum (m_r - m_e)^2,  D = sum m_r^2,  sc = sqrt(N) / sqrt(D) (0 where N == 0),  lm = mean |ln m_r - ln m_e|
//   MR_b = mean_n (sc + lm);   SISDR_b = 10 log10((<s, s> + 1e-8) / (<q, q> + 1e-8)),  s = a r',  q = e' - s,
//   a = <e', r'> / (<r', r'> + 1e-8),  x' = x - mean x;   A = sum_b (k_mr MR_b - k_si SISDR_b),  g = dA / de
//
// float64 throughout with one rounding to float32, fixed-order reductions, no atomics.  Launches:
//   aux_spectra  (per resolution) a block per (row, frame): the windowed frame of r, then of e, goes through ONE loop body
//                - complex float64 in LDS in bit-reversed order, a radix-2 transform with twiddles the block makes itself
//                (48 KB at n = 2048) - so a row with e == r bit for bit has m_e == m_r bit for bit.  m_r and X_e go to the
//                workspace ([B, T, F] float64 and complex128), the frame's three sums to a partials plane.
//   aux_si_part  a block per (row, tile of AX_SI_TILE samples): the five sums of SI-SDR.
//   aux_fold     a block per row: a thread per resolution adds the frames' partials in ascending order, another the
//                tiles'; writes the row's values, (N, D) and the two SI-SDR gradient coefficients and two means.
//   aux_total    one thread: A and its two parts over b ascending (a term whose weight is 0 is left out).
//   aux_grad     (per resolution, with a gradient and k_mr != 0) a block per (row, frame): the spectral gradient
//                c X_e per cell from the folded (N, D), bins above n / 2 zero, the conjugate transform, the window; the
//                frame's n float64 samples overwrite the frame's own X_e slot (8 n of its 8 n + 16 bytes: the block has
//                read all of it before).
//   aux_join     a thread per output sample gathers, per resolution in the caller's order, the up to four frames over
//                the sample's own padded position, then over its mirror in the left margin, then in the right one; then
//                the SI-SDR term; one rounding.  Gather form: nothing is added to memory.
// Storing X_e and m_r (24 bytes a cell) instead of transforming twice: the backward then runs one transform a frame.
// The LDS store rule, the twiddles and the radix-2 passes are lds_f64.hip.h's, shared with suppress.hip and stoiloss.hip.
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "api_internal.h"
#include "host_ranges.h"
#include "lds_f64.hip.h"

namespace {

constexpr int AX_TPB = 256;
constexpr int AX_MAX_RES = 4;
constexpr int AX_MAX_N = 2048;
constexpr int AX_SI_TILE = 4096;
constexpr int AX_FOLD_TPB = 64;
constexpr double AX_CLAMP = 1e-7, AX_EPS = 1e-8;
constexpr double AX_DB = 4.3429448190325182765112891891661;    // 10 / ln 10
constexpr int AX_MAX_L = 2147483647 - 2 * AX_MAX_N;

struct AuxRes {
    size_t X, M, P;              // byte offsets: complex128 [B][T][F] | float64 [B][T][F] | float64 [B][T][3]
    int N, logN, T, F;
};

struct AuxArgs {
    const float* est;
    const float* ref;
    float* g;                    // [B][L] or null
    double* rows;                // [B][2 R + 1]
    float* total;                // [3]
    char* ws;
    AuxRes res[AX_MAX_RES];
    size_t SI, ND, CO;           // byte offsets: float64 [B][tiles][5] | [B][AX_MAX_RES][2] | [B][4]
    double k_mr, k_si;
    int B, L, R, tiles;
};

__device__ inline double ax_hann(int k, int N) {
#pragma clang fp contract(off)
    return 0.5 - 0.5 * cospi((double)(2 * k) / (double)N);
}

// red[v][0] = sum over the block's threads of vals[v], by halving: the order is the block's shape alone
template <int NV>
__device__ inline void ax_block_sum(double* red, const double (&vals)[NV]) {
    for (int v = 0; v < NV; ++v) red[v * AX_TPB + threadIdx.x] = vals[v];
    __syncthreads();
    for (int s = AX_TPB >> 1; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int v = 0; v < NV; ++v) red[v * AX_TPB + threadIdx.x] += red[v * AX_TPB + threadIdx.x + s];
        __syncthreads();
    }
}

__global__ __launch_bounds__(AX_TPB) void aux_spectra(AuxArgs a, int ri) {
#pragma clang fp contract(off)
    extern __shared__ double2 ax_lds[];                                 // [N] frame | [N / 2] twiddles
    __shared__ double s_red[3 * AX_TPB];
    const AuxRes r = a.res[ri];
    const int t = blockIdx.x, b = blockIdx.y, N = r.N, h = N >> 2, F = r.F;
    double2* buf = ax_lds;
    double2* tw = ax_lds + N;
    twiddles<AX_TPB>(tw, N);
    const size_t at = ((size_t)b * r.T + t) * F;
    double2* X = (double2*)(a.ws + r.X) + at;
    double* M = (double*)(a.ws + r.M) + at;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int pass = 0; pass < 2; ++pass) {                              // ONE body for the reference and the estimate
        const float* src = (pass == 0 ? a.ref : a.est) + (size_t)b * a.L;
        __syncthreads();                                                // the pass before has read buf
        for (int k = threadIdx.x; k < N; k += AX_TPB) {
            long long i = (long long)t * h + k - (N >> 1);              // reflect padding: L > N / 2, one fold is enough
            if (i < 0) i = -i;
            if (i >= a.L) i = 2LL * (a.L - 1) - i;
            lds_put(buf + bitrev(k, r.logN), (double)src[i] * ax_hann(k, N), 0.0);
        }
        fft<AX_TPB>(buf, tw, N, r.logN, 1.0);
        for (int f = threadIdx.x; f < F; f += AX_TPB) {
            const double2 v = buf[f];
            const double P = fma(v.x, v.x, v.y * v.y);
            const double m = sqrt(P < AX_CLAMP ? AX_CLAMP : P);         // (a NaN stays one)
            if (pass == 0) {
                M[f] = m;                                               // read back below by this same thread
            } else {
                X[f] = v;
                const double mr = M[f], d = mr - m;
                acc[0] = fma(d, d, acc[0]);
                acc[1] = fma(mr, mr, acc[1]);
                acc[2] += fabs(log(mr) - log(m));
            }
        }
    }
    ax_block_sum<3>(s_red, acc);
    if (threadIdx.x < 3) ((double*)(a.ws + r.P))[((size_t)b * r.T + t) * 3 + threadIdx.x] = s_red[threadIdx.x * AX_TPB];
}

__global__ __launch_bounds__(AX_TPB) void aux_si_part(AuxArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_red[5 * AX_TPB];
    const int tile = blockIdx.x, b = blockIdx.y;
    const float* e = a.est + (size_t)b * a.L;
    const float* r = a.ref + (size_t)b * a.L;
    const long long i0 = (long long)tile * AX_SI_TILE;
    const long long i1 = i0 + AX_SI_TILE < a.L ? i0 + AX_SI_TILE : a.L;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                          // sum e, sum r, sum e e, sum r r, sum e r
    for (long long i = i0 + threadIdx.x; i < i1; i += AX_TPB) {
        const double x = (double)e[i], y = (double)r[i];
        acc[0] += x;
        acc[1] += y;
        acc[2] = fma(x, x, acc[2]);
        acc[3] = fma(y, y, acc[3]);
        acc[4] = fma(x, y, acc[4]);
    }
    ax_block_sum<5>(s_red, acc);
    if (threadIdx.x < 5) ((double*)(a.ws + a.SI))[((size_t)b * a.tiles + tile) * 5 + threadIdx.x] = s_red[threadIdx.x * AX_TPB];
}

__global__ __launch_bounds__(AX_FOLD_TPB) void aux_fold(AuxArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.x, tid = threadIdx.x, R = a.R;
    double* row = a.rows + (size_t)b * (2 * R + 1);
    if (tid < R) {
        const AuxRes r = a.res[tid];
        const double* p = (const double*)(a.ws + r.P) + (size_t)b * r.T * 3;
        double N = 0.0, D = 0.0, Lg = 0.0;
        for (int t = 0; t < r.T; ++t) {
            N += p[3 * t];
            D += p[3 * t + 1];
            Lg += p[3 * t + 2];
        }
        double* nd = (double*)(a.ws + a.ND) + ((size_t)b * AX_MAX_RES + tid) * 2;
        nd[0] = N;
        nd[1] = D;
        row[2 * tid] = N == 0.0 ? 0.0 : sqrt(N) / sqrt(D);              // (a NaN stays one)
        row[2 * tid + 1] = Lg / ((double)r.T * (double)r.F);
    } else if (tid == AX_FOLD_TPB - 1) {
        const double* p = (const double*)(a.ws + a.SI) + (size_t)b * a.tiles * 5;
        double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < a.tiles; ++j)
            for (int v = 0; v < 5; ++v) s[v] += p[5 * j + v];
        const double n = (double)a.L, me = s[0] / n, mr = s[1] / n;
        double Ee = s[2] - s[0] * me, Rr = s[3] - s[1] * mr;
        const double Er = s[4] - s[0] * mr;
        Ee = Ee < 0.0 ? 0.0 : Ee;
        Rr = Rr < 0.0 ? 0.0 : Rr;
        const double al = Er / (Rr + AX_EPS);
        double qq = (Ee - 2.0 * al * Er) + al * al * Rr;
        qq = qq < 0.0 ? 0.0 : qq;
        const double S = al * al * Rr + AX_EPS, Q = qq + AX_EPS;
        row[2 * R] = AX_DB * (log(S) - log(Q));
        // dSISDR / de = AX_DB (ce e' + cr r'): the header derives the two
        const double ce = -2.0 / Q;
        const double cr = 2.0 * al * Rr / ((Rr + AX_EPS) * S) + (2.0 * al / Q) * (1.0 + AX_EPS / (Rr + AX_EPS));
        double* co = (double*)(a.ws + a.CO) + (size_t)b * 4;
        co[0] = -a.k_si * AX_DB * ce;
        co[1] = -a.k_si * AX_DB * cr;
        co[2] = me;
        co[3] = mr;
    }
}

__global__ void aux_total(AuxArgs a) {
#pragma clang fp contract(off)
    const int R = a.R;
    double A = 0.0, Amr = 0.0, Asi = 0.0;
    for (int b = 0; b < a.B; ++b) {
        const double* row = a.rows + (size_t)b * (2 * R + 1);
        double mr = 0.0;
        for (int i = 0; i < R; ++i) mr += row[2 * i] + row[2 * i + 1];
        const double pm = a.k_mr != 0.0 ? a.k_mr * (mr / (double)R) : 0.0;      // a term of weight 0 is left out
        const double ps = a.k_si != 0.0 ? a.k_si * row[2 * R] : 0.0;
        A += pm - ps;
        Amr += pm;
        Asi -= ps;
    }
    a.total[0] = (float)A;
    a.total[1] = (float)Amr;
    a.total[2] = (float)Asi;
}

__global__ __launch_bounds__(AX_TPB) void aux_grad(AuxArgs a, int ri) {
#pragma clang fp contract(off)
    extern __shared__ double2 ax_lds[];
    const AuxRes r = a.res[ri];
    const int t = blockIdx.x, b = blockIdx.y, N = r.N, F = r.F;
    double2* buf = ax_lds;
    double2* tw = ax_lds + N;
    twiddles<AX_TPB>(tw, N);
    const size_t at = ((size_t)b * r.T + t) * F;
    double2* X = (double2*)(a.ws + r.X) + at;
    const double* M = (const double*)(a.ws + r.M) + at;
    const double* nd = (const double*)(a.ws + a.ND) + ((size_t)b * AX_MAX_RES + ri) * 2;
    const double Nn = nd[0], Dd = nd[1];
    const double inv_sc = Nn == 0.0 ? 0.0 : 1.0 / (sqrt(Nn) * sqrt(Dd));
    const double inv_tf = 1.0 / ((double)r.T * (double)r.F), kr = a.k_mr / (double)a.R;
    for (int f = threadIdx.x; f < N; f += AX_TPB) {
        double re = 0.0, im = 0.0;
        if (f < F) {
            const double2 v = X[f];
            const double mr = M[f];
            const double P = fma(v.x, v.x, v.y * v.y);
            const double m = sqrt(P < AX_CLAMP ? AX_CLAMP : P);
            double c = 0.0;
            if (!(P < AX_CLAMP)) {                                      // below the clamp the derivative is 0
                const double dl = log(m) - log(mr);
                const double sg = dl > 0.0 ? 1.0 : (dl < 0.0 ? -1.0 : 0.0);
                c = kr * ((m - mr) * inv_sc + sg * inv_tf / m) / m;
            }
            re = c * v.x;
            im = (f == 0 || f == F - 1) ? 0.0 : c * v.y;                 // their imaginary parts reach no real output
        }
        lds_put(buf + bitrev(f, r.logN), re, im);
    }
    fft<AX_TPB>(buf, tw, N, r.logN, -1.0);                                   // (its first barrier: every X[f] has been read)
    double* z = (double*)X;                                             // the frame gradient over the frame's own spectrum
    for (int k = threadIdx.x; k < N; k += AX_TPB) z[k] = buf[k].x * ax_hann(k, N);
}

// the frames of one padded position j, ascending
__device__ inline double ax_gather(const double* zrow, int j, int N, int h, int T, int F) {
#pragma clang fp contract(off)
    int t0 = j - N + h;
    t0 = t0 < 0 ? 0 : t0 / h;
    int t1 = j / h;
    t1 = t1 > T - 1 ? T - 1 : t1;
    double s = 0.0;
    for (int t = t0; t <= t1; ++t) s += zrow[(size_t)t * (2 * F) + (j - t * h)];
    return s;
}

__global__ __launch_bounds__(AX_TPB) void aux_join(AuxArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.y, L = a.L;
    const long long ii = (long long)blockIdx.x * AX_TPB + threadIdx.x;
    if (ii >= L) return;
    const int i = (int)ii;
    double g = 0.0;
    if (a.k_mr != 0.0) {
        for (int ri = 0; ri < a.R; ++ri) {
            const AuxRes r = a.res[ri];
            const int N = r.N, h = N >> 2, half = N >> 1;
            const double* zrow = (const double*)(a.ws + r.X) + (size_t)b * r.T * (2 * r.F);
            double s = ax_gather(zrow, i + half, N, h, r.T, r.F);
            if (i >= 1 && i <= half) s += ax_gather(zrow, half - i, N, h, r.T, r.F);
            if (i <= L - 2 && i >= L - 1 - half) s += ax_gather(zrow, (L - 1) + (L - 1 - i) + half, N, h, r.T, r.F);
            g += s;
        }
    }
    if (a.k_si != 0.0) {
        const double* co = (const double*)(a.ws + a.CO) + (size_t)b * 4;
        const double e = (double)a.est[(size_t)b * L + i] - co[2], y = (double)a.ref[(size_t)b * L + i] - co[3];
        g += co[0] * e + co[1] * y;
    }
    a.g[(size_t)b * L + i] = (float)g;
}

// null: fine; else what is wrong with the shape
inline const char* ax_shape_error(int B, int L, int n_res, const int* n_fft) {
    if (B < 1 || B > 65535) return "need 1 <= B <= 65535";
    if (n_res < 1 || n_res > AX_MAX_RES || !n_fft) return "need 1 to 4 resolutions";
    int top = 0;
    for (int i = 0; i < n_res; ++i) {
        const int n = n_fft[i];
        if (n != 256 && n != 512 && n != 1024 && n != 2048) return "a resolution must be 256, 512, 1024 or 2048";
        for (int j = 0; j < i; ++j)
            if (n_fft[j] == n) return "the resolutions must be distinct";
        top = n > top ? n : top;
    }
    if (L <= top / 2) return "L must exceed half the longest window (reflect padding)";
    if (L > AX_MAX_L) return "rows are too long";
    return nullptr;
}

inline size_t ax_layout(AuxArgs& a, int B, int L, int n_res, const int* n_fft) {
    size_t off = 0;
    for (int i = 0; i < n_res; ++i) {
        AuxRes& r = a.res[i];
        r.N = n_fft[i];
        r.logN = r.N == 256 ? 8 : (r.N == 512 ? 9 : (r.N == 1024 ? 10 : 11));
        r.T = 1 + L / (r.N / 4);
        r.F = r.N / 2 + 1;
        const size_t cells = (size_t)B * (size_t)r.T * (size_t)r.F;
        r.X = off;
        off += up256(cells * 2 * sizeof(double));
        r.M = off;
        off += up256(cells * sizeof(double));
        r.P = off;
        off += up256((size_t)B * (size_t)r.T * 3 * sizeof(double));
    }
    a.B = B;
    a.L = L;
    a.R = n_res;
    a.tiles = (L + AX_SI_TILE - 1) / AX_SI_TILE;
    a.SI = off;
    off += up256((size_t)B * (size_t)a.tiles * 5 * sizeof(double));
    a.ND = off;
    off += up256((size_t)B * AX_MAX_RES * 2 * sizeof(double));
    a.CO = off;
    off += up256((size_t)B * 4 * sizeof(double));
    return off;
}

}  // namespace

extern "C" int cmgan_aux_loss_max_resolutions(void) { return AX_MAX_RES; }

extern "C" size_t cmgan_aux_loss_workspace_bytes(cmgan_handle*, int B, int L, int n_res, const int* n_fft_host) {
    if (ax_shape_error(B, L, n_res, n_fft_host)) return 0;
    AuxArgs a;
    return ax_layout(a, B, L, n_res, n_fft_host);
}

extern "C" int cmgan_aux_loss(cmgan_handle* h, const float* est, const float* ref, int B, int L, int n_res, const int* n_fft_host,
                              double k_mr, double k_si, double* rows, float* total, float* g_audio, void* ws, size_t ws_bytes,
                              void* stream) {
    // every argument is judged before the handle is, so that the errors below need no GPU
    if (!est || !ref || !rows || !total) return fail(h, CMGAN_E_BADARG, "cmgan_aux_loss: null pointer");
    if (((uintptr_t)est | (uintptr_t)ref | (uintptr_t)total | (uintptr_t)g_audio) & 3)
        return fail(h, CMGAN_E_BADARG, "cmgan_aux_loss: float32 buffers must be 4-byte aligned");
    if ((uintptr_t)rows & 7) return fail(h, CMGAN_E_BADARG, "cmgan_aux_loss: rows must be 8-byte aligned");
    if (const char* what = ax_shape_error(B, L, n_res, n_fft_host))
        return fail(h, CMGAN_E_BADARG, "cmgan_aux_loss: %s (B=%d L=%d n_res=%d)", what, B, L, n_res);
    if (!(k_mr == k_mr) || !(k_si == k_si)) return fail(h, CMGAN_E_BADARG, "cmgan_aux_loss: k_mr and k_si must be numbers");
    const size_t bytes = (size_t)B * (size_t)L * sizeof(float);
    if (g_audio && (bytes_overlap(g_audio, bytes, est, bytes) || bytes_overlap(g_audio, bytes, ref, bytes)))
        return fail(h, CMGAN_E_BADARG, "cmgan_aux_loss: g_audio overlaps est or ref; the gradient is not formed in place");
    AuxArgs a;
    const size_t need = ax_layout(a, B, L, n_res, n_fft_host);
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < need)
        return fail(h, CMGAN_E_BADARG, "cmgan_aux_loss: the workspace must be 256-byte aligned and hold %zu bytes (%zu given)",
                    need, ws ? ws_bytes : (size_t)0);
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "cmgan_aux_loss: null handle");
    const LaunchCtx ctx = begin(h, stream);
    hipStream_t s = ctx.stream;
    a.est = est;
    a.ref = ref;
    a.g = g_audio;
    a.rows = rows;
    a.total = total;
    a.ws = (char*)ws;
    a.k_mr = k_mr;
    a.k_si = k_si;
    for (int i = 0; i < n_res; ++i) {
        const size_t lds = (size_t)a.res[i].N * 3 / 2 * sizeof(double2);
        LAUNCH(ctx, "aux_spectra", aux_spectra<<<dim3(a.res[i].T, B), AX_TPB, lds, s>>>(a, i));
    }
    LAUNCH(ctx, "aux_si_part", aux_si_part<<<dim3(a.tiles, B), AX_TPB, 0, s>>>(a));
    LAUNCH(ctx, "aux_fold", aux_fold<<<B, AX_FOLD_TPB, 0, s>>>(a));
    LAUNCH(ctx, "aux_total", aux_total<<<1, 1, 0, s>>>(a));
    if (g_audio) {
        if (k_mr != 0.0)
            for (int i = 0; i < n_res; ++i) {
                const size_t lds = (size_t)a.res[i].N * 3 / 2 * sizeof(double2);
                LAUNCH(ctx, "aux_grad", aux_grad<<<dim3(a.res[i].T, B), AX_TPB, lds, s>>>(a, i));
            }
        LAUNCH(ctx, "aux_join", aux_join<<<dim3((L + AX_TPB - 1) / AX_TPB, B), AX_TPB, 0, s>>>(a));
    }
    return check_launch(h, "aux_loss");
}
