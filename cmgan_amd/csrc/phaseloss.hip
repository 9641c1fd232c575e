// phaseloss.hip - the three anti-wrapping phase terms of MP-SENet (Lu, Ai, Ling 2023) on the spectrum the generator emits,
// with their gradient (cmgan_phase_loss, include/cmgan_hip.h, "Phase loss"): instantaneous phase, group delay and
// instantaneous angular frequency of est_real + i est_imag against clean_spec.  The reference has no counterpart: its loss
// sees phase only through the RI term and the waveform L1 (src/train.py:124-151).  Per cell (t, f) of row b:
//
//   p = atan2(est_imag, est_real),  q = atan2(clean_im, clean_re);   r(x) = remainder(x, TWO_PI) (IEEE, exact),  AW(x) = |r(x)|
//   void: |est|^2 or |clean|^2 is 0 or below floor^2 (float64, exact squares, one rounding in their sum), or an input is not finite
//   ip_b  = mean over the non-void cells of AW(p - q)
//   gd_b  = mean over the pairs (t, f), f >= 1, both cells non-void, of AW((p[t,f] - p[t,f-1]) - (q[t,f] - q[t,f-1]))
//   iaf_b = mean over the pairs (t, f), t >= 1, both cells non-void, of AW((p[t,f] - p[t-1,f]) - (q[t,f] - q[t-1,f]))
//   A = sum_b (k_ip ip_b + k_gd gd_b + k_iaf iaf_b);   g = dA / d(est_real, est_imag) through dp = (-im, re) / |z|^2
//
// MP-SENet's matrix form of the group delay also carries a boundary column for f = 0 (the phase of bin 0 itself); it is
// left out here: the terms are the differences of neighbours alone.  float64 throughout, one rounding to float32 per
// gradient sample, fixed-order reductions, no atomics.  A block owns PL_TT consecutive frames of one row and all F bins:
// the call moves 16 bytes in and 8 out per cell, and the angles cost two float64 atan2 a cell, so the neighbours' angles
// are not recomputed per term - a frame's (p, q) go to LDS once (p = NaN marks a void cell) and the frame before the tile
// (and, for the gradient, behind it) is read again as a halo: (PL_TT + 1) / PL_TT and (PL_TT + 2) / PL_TT of the cells.
// Launches:
//   pl_terms  a block per (row, tile of PL_TT frames): the three sums and the three counts of the tile's own terms (a
//             pair belongs to the tile of its LATER cell), a thread's terms in ascending (t, f), the threads by halving;
//             six float64 to the workspace.
//   pl_fold   a block per row: thread i < 3 adds term i's tile partials in ascending order; rows, counts, status.
//   pl_total  one thread: A and its three parts over b ascending (a term whose k is 0 is left out).
//   pl_grad   (with a gradient) a block per (row, tile): the same angles with a halo on both sides, the counts read from
//             counts_dev; every cell GATHERS its at most five terms in the order ip, gd, iaf.
#include <math.h>
#include <stdint.h>

#include "api_internal.h"
#include "host_ranges.h"

namespace {

constexpr int PL_TPB = 256;
constexpr int PL_TT = 8;                     // frames of a tile
constexpr int PL_FOLD_TPB = 64;
constexpr int PL_MAX_F = 1024;               // three frames of (p, q) in LDS: 48 F bytes
constexpr int PL_MAX_T = 1000000;            // T F fits an int32 count
constexpr double PL_TWO_PI = 6.283185307179586476925286766559;      // the double nearest 2 pi

struct PhaseArgs {
    const float* er;             // [B][T][F]
    const float* ei;
    const float* clean;          // [B][2][T][F]
    double* rows;                // [B][3]
    int* counts;                 // [B][3]
    float* total;                // [4]
    int* status;                 // [B]
    float* g_real;               // [B][T][F] or null
    float* g_imag;
    double* part;                // workspace: [B][tiles][6] = three sums, three counts
    double k[3];
    double floor2;
    int B, T, F, tiles;
};

// (p, q) of one cell; p = NaN where the cell is void
__device__ inline double2 pl_angles(const PhaseArgs& a, int b, int t, int f) {
#pragma clang fp contract(off)
    const size_t plane = (size_t)a.T * a.F, at = (size_t)t * a.F + f;
    const double re = (double)a.er[(size_t)b * plane + at], im = (double)a.ei[(size_t)b * plane + at];
    const double cr = (double)a.clean[(size_t)b * 2 * plane + at], ci = (double)a.clean[((size_t)b * 2 + 1) * plane + at];
    const double me = re * re + im * im, mc = cr * cr + ci * ci;        // exact squares, one rounding each sum
    const bool ok = isfinite(re) && isfinite(im) && isfinite(cr) && isfinite(ci) && me > 0.0 && mc > 0.0 &&
                    !(me < a.floor2) && !(mc < a.floor2);
    double2 v;
    v.x = ok ? atan2(im, re) : (double)NAN;
    v.y = ok ? atan2(ci, cr) : 0.0;
    return v;
}

__device__ inline void pl_fill(const PhaseArgs& a, double2* row, int b, int t) {
    for (int f = threadIdx.x; f < a.F; f += PL_TPB) row[f] = pl_angles(a, b, t, f);
}

__device__ inline bool pl_void(const double2& v) { return v.x != v.x; }

// r((c.p - n.p) - (c.q - n.q)): c the later cell of the pair
__device__ inline double pl_pair(const double2& c, const double2& n) {
#pragma clang fp contract(off)
    return remainder((c.x - n.x) - (c.y - n.y), PL_TWO_PI);
}

__device__ inline double pl_sign(double r) { return r > 0.0 ? 1.0 : (r < 0.0 ? -1.0 : 0.0); }

__global__ __launch_bounds__(PL_TPB) void pl_terms(PhaseArgs a) {
#pragma clang fp contract(off)
    extern __shared__ double2 pl_lds[];                                 // [2][F]
    __shared__ double s_red[6 * PL_TPB];
    const int b = blockIdx.y, F = a.F;
    const int t0 = blockIdx.x * PL_TT, t1 = t0 + PL_TT < a.T ? t0 + PL_TT : a.T;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = t0 > 0 ? t0 - 1 : t0; t < t1; ++t) {
        double2* cur = pl_lds + (size_t)(t & 1) * F;
        const double2* prev = pl_lds + (size_t)((t & 1) ^ 1) * F;
        pl_fill(a, cur, b, t);
        __syncthreads();
        if (t >= t0) {
            for (int f = threadIdx.x; f < F; f += PL_TPB) {
                const double2 c = cur[f];
                if (pl_void(c)) continue;
                acc[0] += fabs(remainder(c.x - c.y, PL_TWO_PI));
                acc[3] += 1.0;
                if (f >= 1) {
                    const double2 n = cur[f - 1];
                    if (!pl_void(n)) {
                        acc[1] += fabs(pl_pair(c, n));
                        acc[4] += 1.0;
                    }
                }
                if (t >= 1) {
                    const double2 n = prev[f];
                    if (!pl_void(n)) {
                        acc[2] += fabs(pl_pair(c, n));
                        acc[5] += 1.0;
                    }
                }
            }
        }
        __syncthreads();                                                // the next frame overwrites prev
    }
    for (int v = 0; v < 6; ++v) s_red[v * PL_TPB + threadIdx.x] = acc[v];
    __syncthreads();
    for (int s = PL_TPB >> 1; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int v = 0; v < 6; ++v) s_red[v * PL_TPB + threadIdx.x] += s_red[v * PL_TPB + threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 6) a.part[((size_t)b * a.tiles + blockIdx.x) * 6 + threadIdx.x] = s_red[threadIdx.x * PL_TPB];
}

__global__ __launch_bounds__(PL_FOLD_TPB) void pl_fold(PhaseArgs a) {
#pragma clang fp contract(off)
    __shared__ int s_bit[3];
    const int b = blockIdx.x, i = threadIdx.x;
    if (i < 3) {
        const double* p = a.part + (size_t)b * a.tiles * 6;
        double S = 0.0, N = 0.0;
        for (int j = 0; j < a.tiles; ++j) {
            S += p[6 * j + i];
            N += p[6 * j + 3 + i];                                      // whole numbers below 2^31: exact
        }
        a.rows[(size_t)b * 3 + i] = N > 0.0 ? S / N : 0.0;
        a.counts[(size_t)b * 3 + i] = (int)N;
        s_bit[i] = N > 0.0 ? 0 : (1 << i);
    }
    __syncthreads();
    if (i == 0) a.status[b] = s_bit[0] | s_bit[1] | s_bit[2];
}

__global__ void pl_total(PhaseArgs a) {
#pragma clang fp contract(off)
    double A = 0.0, part[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < a.B; ++b) {
        double x[3];
        for (int i = 0; i < 3; ++i) {
            x[i] = a.k[i] != 0.0 ? a.k[i] * a.rows[(size_t)b * 3 + i] : 0.0;    // a term of weight 0 is left out
            part[i] += x[i];
        }
        A += (x[0] + x[1]) + x[2];
    }
    a.total[0] = (float)A;
    for (int i = 0; i < 3; ++i) a.total[1 + i] = (float)part[i];
}

__global__ __launch_bounds__(PL_TPB) void pl_grad(PhaseArgs a) {
#pragma clang fp contract(off)
    extern __shared__ double2 pl_lds[];                                 // [3][F]: frame t lives in slot t % 3
    const int b = blockIdx.y, F = a.F, T = a.T;
    const int t0 = blockIdx.x * PL_TT, t1 = t0 + PL_TT < T ? t0 + PL_TT : T;
    double c3[3];                                                       // k_i / N_i, 0 where the term has no gradient
    for (int i = 0; i < 3; ++i) {
        const int N = a.counts[(size_t)b * 3 + i];
        c3[i] = (a.k[i] != 0.0 && N > 0) ? a.k[i] / (double)N : 0.0;
    }
    const size_t plane = (size_t)T * F;
    if (t0 > 0) pl_fill(a, pl_lds + (size_t)((t0 - 1) % 3) * F, b, t0 - 1);
    pl_fill(a, pl_lds + (size_t)(t0 % 3) * F, b, t0);
    for (int t = t0; t < t1; ++t) {
        if (t + 1 < T) pl_fill(a, pl_lds + (size_t)((t + 1) % 3) * F, b, t + 1);
        __syncthreads();
        const double2* cur = pl_lds + (size_t)(t % 3) * F;
        const double2* up = pl_lds + (size_t)((t + 2) % 3) * F;         // frame t - 1
        const double2* down = pl_lds + (size_t)((t + 1) % 3) * F;
        for (int f = threadIdx.x; f < F; f += PL_TPB) {
            const size_t at = (size_t)b * plane + (size_t)t * F + f;
            const double2 c = cur[f];
            float gr = 0.f, gi = 0.f;
            if (!pl_void(c)) {
                double s_gd = 0.0, s_iaf = 0.0;
                if (f >= 1 && !pl_void(cur[f - 1])) s_gd += pl_sign(pl_pair(c, cur[f - 1]));
                if (f + 1 < F && !pl_void(cur[f + 1])) s_gd -= pl_sign(pl_pair(cur[f + 1], c));
                if (t >= 1 && !pl_void(up[f])) s_iaf += pl_sign(pl_pair(c, up[f]));
                if (t + 1 < T && !pl_void(down[f])) s_iaf -= pl_sign(pl_pair(down[f], c));
                double d = c3[0] * pl_sign(remainder(c.x - c.y, PL_TWO_PI));
                d += c3[1] * s_gd;
                d += c3[2] * s_iaf;
                if (d != 0.0) {
                    const double re = (double)a.er[at], im = (double)a.ei[at];
                    const double m2 = re * re + im * im;
                    gr = (float)(d * (-im / m2));
                    gi = (float)(d * (re / m2));
                }
            }
            a.g_real[at] = gr;
            a.g_imag[at] = gi;
        }
        __syncthreads();                                                // the next fill overwrites frame t - 1
    }
}

inline bool pl_shape_ok(int B, int T) { return B >= 1 && B <= 65535 && T >= 1 && T <= PL_MAX_T; }

inline int pl_tiles(int T) { return (T + PL_TT - 1) / PL_TT; }

}  // namespace

extern "C" int cmgan_phase_loss_tile_frames(void) { return PL_TT; }

extern "C" size_t cmgan_phase_loss_workspace_bytes(cmgan_handle*, int B, int T) {
    if (!pl_shape_ok(B, T)) return 0;
    return up256((size_t)B * (size_t)pl_tiles(T) * 6 * sizeof(double));
}

extern "C" int cmgan_phase_loss(cmgan_handle* h, const float* est_real, const float* est_imag, const float* clean_spec, int B,
                                int T, double k_ip, double k_gd, double k_iaf, double floor, double* rows, int* counts,
                                float* total, int* status, float* g_real, float* g_imag, void* ws, size_t ws_bytes,
                                void* stream) {
    // every argument that can be judged without the handle's F is judged before the handle is
    if (!est_real || !est_imag || !clean_spec || !rows || !counts || !total || !status)
        return fail(h, CMGAN_E_BADARG, "cmgan_phase_loss: null pointer");
    if (((uintptr_t)est_real | (uintptr_t)est_imag | (uintptr_t)clean_spec | (uintptr_t)counts | (uintptr_t)total |
         (uintptr_t)status | (uintptr_t)g_real | (uintptr_t)g_imag) & 3)
        return fail(h, CMGAN_E_BADARG, "cmgan_phase_loss: float32 and int32 buffers must be 4-byte aligned");
    if ((uintptr_t)rows & 7) return fail(h, CMGAN_E_BADARG, "cmgan_phase_loss: rows must be 8-byte aligned");
    if (B < 1 || B > 65535) return fail(h, CMGAN_E_BADARG, "cmgan_phase_loss: need 1 <= B <= 65535 (B=%d)", B);
    if (T < 1 || T > PL_MAX_T) return fail(h, CMGAN_E_BADARG, "cmgan_phase_loss: need 1 <= T <= %d (T=%d)", PL_MAX_T, T);
    if (!(k_ip == k_ip) || !(k_gd == k_gd) || !(k_iaf == k_iaf))
        return fail(h, CMGAN_E_BADARG, "cmgan_phase_loss: k_ip, k_gd and k_iaf must be numbers");
    if (!(floor >= 0.0)) return fail(h, CMGAN_E_BADARG, "cmgan_phase_loss: floor must be a number >= 0");
    if ((g_real == nullptr) != (g_imag == nullptr))
        return fail(h, CMGAN_E_BADARG, "cmgan_phase_loss: the gradient needs both g_real and g_imag, the values alone neither");
    const size_t need = cmgan_phase_loss_workspace_bytes(nullptr, B, T);
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < need)
        return fail(h, CMGAN_E_BADARG, "cmgan_phase_loss: the workspace must be 256-byte aligned and hold %zu bytes (%zu given)",
                    need, ws ? ws_bytes : (size_t)0);
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "cmgan_phase_loss: null handle");
    const int F = h->cfg.num_features;
    if (F < 1 || F > PL_MAX_F)
        return fail(h, CMGAN_E_BADARG, "cmgan_phase_loss: the handle's F = %d is outside 1 .. %d", F, PL_MAX_F);
    const size_t bytes = (size_t)B * (size_t)T * (size_t)F * sizeof(float);
    if (g_real) {
        float* const g[2] = {g_real, g_imag};
        for (int i = 0; i < 2; ++i)
            if (bytes_overlap(g[i], bytes, est_real, bytes) || bytes_overlap(g[i], bytes, est_imag, bytes) ||
                bytes_overlap(g[i], bytes, clean_spec, 2 * bytes))
                return fail(h, CMGAN_E_BADARG, "cmgan_phase_loss: a gradient buffer overlaps an input; the gradient is not formed in place");
        if (bytes_overlap(g_real, bytes, g_imag, bytes))
            return fail(h, CMGAN_E_BADARG, "cmgan_phase_loss: g_real overlaps g_imag");
    }
    PhaseArgs a;
    a.er = est_real;
    a.ei = est_imag;
    a.clean = clean_spec;
    a.rows = rows;
    a.counts = counts;
    a.total = total;
    a.status = status;
    a.g_real = g_real;
    a.g_imag = g_imag;
    a.part = (double*)ws;
    a.k[0] = k_ip;
    a.k[1] = k_gd;
    a.k[2] = k_iaf;
    a.floor2 = floor * floor;
    a.B = B;
    a.T = T;
    a.F = F;
    a.tiles = pl_tiles(T);
    const LaunchCtx ctx = begin(h, stream);
    hipStream_t s = ctx.stream;
    const size_t row_bytes = (size_t)F * sizeof(double2);
    LAUNCH(ctx, "pl_terms", pl_terms<<<dim3(a.tiles, B), PL_TPB, 2 * row_bytes, s>>>(a));
    LAUNCH(ctx, "pl_fold", pl_fold<<<B, PL_FOLD_TPB, 0, s>>>(a));
    LAUNCH(ctx, "pl_total", pl_total<<<1, 1, 0, s>>>(a));
    if (g_real) LAUNCH(ctx, "pl_grad", pl_grad<<<dim3(a.tiles, B), PL_TPB, 3 * row_bytes, s>>>(a));
    return check_launch(h, "phase_loss");
}
