// resample.hip - rational-rate polyphase FIR resampling of a [B, L] float32 batch (cmgan_resample, include/cmgan_hip.h):
// the arithmetic of scipy.signal.resample_poly(x, up, down) with its default window ('kaiser', 5.0) and
// padtype='constant'.  The reference asserts sr == 16000 (src/evaluation.py:19) and leaves resampling to the user.
//
//   g = gcd(fs_in, fs_out), up = fs_out / g, down = fs_in / g, m = max(up, down), half_len = 10 m
//   h = firwin(2 half_len + 1, 1 / m, window=('kaiser', 5.0)) * up, pre = down - half_len % down zeros in front
//   pre_remove = (half_len + pre) / down,   N = ceil(L up / down)
//   y[n] = sum_i x[i] h[(n + pre_remove) down - i up],  tap index in [0, len(h)),  x = 0 outside [0, L)
//
// Float32 samples in and out; products and sums in float64 on the VALU, the taps of one output added in ascending tap
// index, one rounding to float32 at the store.  Two launches per call, no host synchronisation, no atomics:
//   resample_table   the taps, PHASE-major: tab[p][j] = h[p + j up], T = ceil(len(h) / up) (rounded up to even) entries
//                    per phase, zero beyond len(h).  Output n uses phase p = pos % up, pos = (n + pre_remove) down, and
//                    input i_hi - j with tap j, i_hi = pos / up: one contiguous row of the table, walked with 16-byte loads,
//                    where the tap-major order would make every tap read a gather with stride `down` across the lanes.
//   resample_poly    a block computes a tile of <= 256 consecutive outputs of one row, one per thread.  The input span
//                    the tile reaches is staged in LDS with 16-byte loads (zero where the buffer has no sample); with
//                    up == 1 every output uses the same taps, which then sit in LDS too.
// Every thread runs all T taps of its phase: a tap that falls outside the signal or past len(h) adds 0 * h or x * 0,
// which leaves a float64 sum unchanged.  That is what makes a chunked call (outputs [n0, n0 + n_out) from a buffer that
// holds samples [pos_in, pos_in + n_buf)) give the same bits as the whole-signal call.
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "api_internal.h"
#include "host_ranges.h"

namespace {

constexpr int RS_TPB = 256;            // threads of resample_poly = most outputs per tile
constexpr int RS_SPAN_CAP = 8192;      // floats of LDS for a tile's input span (32 KiB)
constexpr int RS_TAPS_LDS = 2048;      // doubles of LDS for the taps when up == 1 (16 KiB)
constexpr int RS_TB_TPB = 1024;        // threads of resample_table (one block)
constexpr int RS_MAX_RATE = 640;       // largest reduced up / down

struct RsGeom {
    int up, down, half_len, pre, n_taps, pre_remove;   // n_taps counts the zero pre-pad
    int T;                                             // taps per phase (even)
};

inline long long gcd_ll(long long a, long long b) {
    while (b) { const long long t = a % b; a = b; b = t; }
    return a;
}

// false: a rate is not positive or the reduced ratio is beyond RS_MAX_RATE.  fs_in == fs_out gives up = down = 1 (a copy).
inline bool rs_geom(int fs_in, int fs_out, RsGeom& g) {
    if (fs_in <= 0 || fs_out <= 0) return false;
    const long long d = gcd_ll(fs_in, fs_out);
    const long long up = fs_out / d, down = fs_in / d;
    if (up > RS_MAX_RATE || down > RS_MAX_RATE) return false;
    g.up = (int)up;
    g.down = (int)down;
    g.half_len = 10 * (g.up > g.down ? g.up : g.down);
    g.pre = g.down - g.half_len % g.down;
    g.n_taps = g.pre + 2 * g.half_len + 1;
    g.pre_remove = (g.half_len + g.pre) / g.down;
    g.T = ((g.n_taps + g.up - 1) / g.up + 1) & ~1;
    return true;
}

__host__ __device__ inline double rs_bessel_i0(double x) {      // power series; x <= 5 here
    double term = 1.0, sum = 1.0;
    const double q = 0.25 * x * x;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// firwin(2 half_len + 1, 1 / m, window=('kaiser', 5.0)) before its normalisation by the sum: tap j (0-based)
__host__ __device__ inline double rs_fir_raw(const RsGeom& g, int j) {
    const int M = 2 * g.half_len + 1;
    const double cutoff = 1.0 / (double)(g.up > g.down ? g.up : g.down);
    const double alpha = 0.5 * (M - 1);
    const double m = (double)j - alpha;
    const double y = M_PI * (cutoff * m == 0.0 ? 1.0e-20 : cutoff * m);     // np.sinc
    const double h = cutoff * (sin(y) / y);
    const double r = ((double)j - alpha) / alpha;
    const double win = rs_bessel_i0(5.0 * sqrt(1.0 - r * r)) / rs_bessel_i0(5.0);
    return h * win;
}

// Sum of the raw taps in the table kernel's order: slot t of RS_TB_TPB adds taps t, t + RS_TB_TPB, ... (index incl. the
// pre-pad), ascending; the slots are then folded in halves.
inline void rs_taps_host(const RsGeom& g, double* out) {          // out[n_taps]: pre-pad zeros, taps / sum * up
    std::vector<double> part(RS_TB_TPB, 0.0);
    for (int k = g.pre; k < g.n_taps; ++k) part[k % RS_TB_TPB] += (out[k] = rs_fir_raw(g, k - g.pre));
    for (int s = RS_TB_TPB / 2; s > 0; s >>= 1)
        for (int t = 0; t < s; ++t) part[t] += part[t + s];
    for (int k = 0; k < g.n_taps; ++k) out[k] = k < g.pre ? 0.0 : out[k] / part[0] * (double)g.up;
}

// ------------------------------------------------------------------------------------------ kernels
// one block: tab[p * T + j] = h[p + j up].  A thread evaluates each of its taps once: raw into the table, summed as it
// goes, scaled in place once the sum is known (the same thread wrote the entry).
__global__ __launch_bounds__(RS_TB_TPB) void resample_table(RsGeom g, double* tab) {
    __shared__ double part[RS_TB_TPB];
    const int t = threadIdx.x;
    const int total = g.up * g.T;
    double acc = 0.0;
    for (int k = t; k < total; k += RS_TB_TPB) {
        double r = 0.0;
        if (k >= g.pre && k < g.n_taps) {
            r = rs_fir_raw(g, k - g.pre);
            acc += r;
        }
        tab[(size_t)(k % g.up) * g.T + k / g.up] = r;
    }
    part[t] = acc;
    __syncthreads();
    for (int s = RS_TB_TPB / 2; s > 0; s >>= 1) {
        if (t < s) part[t] += part[t + s];
        __syncthreads();
    }
    const double sum = part[0];
    for (int k = t; k < total; k += RS_TB_TPB) {
        const size_t e = (size_t)(k % g.up) * g.T + k / g.up;
        tab[e] = tab[e] / sum * (double)g.up;
    }
}

struct RsArgs {
    const float* x;
    float* y;
    const double* tab;
    long long ld_in, ld_out, pos_in, n0;
    int n_buf, n_out, up, down, T, pre_remove, tile;
};

// TAPS_LDS: up == 1 and T <= RS_TAPS_LDS.  STAGED: the span of a.tile outputs fits RS_SPAN_CAP (the host picks a.tile so
// that it does; only a decimator whose one phase is longer than the cap runs un-staged, straight from global memory).
template <bool TAPS_LDS, bool STAGED>
__global__ __launch_bounds__(RS_TPB) void resample_poly(RsArgs a) {
    __shared__ __attribute__((aligned(16))) float s_x[STAGED ? RS_SPAN_CAP : 4];
    __shared__ __attribute__((aligned(16))) double s_h[TAPS_LDS ? RS_TAPS_LDS : 2];
    const int t = threadIdx.x;
    const int o_first = blockIdx.x * a.tile;                      // first output of the tile, counted from n0
    const int cnt = a.n_out - o_first < a.tile ? a.n_out - o_first : a.tile;
    const float* row = a.x + (size_t)blockIdx.y * a.ld_in;
    const long long n_first = a.n0 + o_first;
    const long long i_first = ((n_first + a.pre_remove) * a.down) / a.up;   // newest input of the first output
    const long long s_start = i_first - (a.T - 1);               // oldest input the tile reaches (signal index)
    int front = 0;
    if (STAGED) {
        const long long i_last = ((n_first + cnt - 1 + a.pre_remove) * a.down) / a.up;
        const long long q0 = s_start - a.pos_in;                  // the same sample as a buffer index (may be < 0)
        // `front` samples are loaded in front of the span so that every float4 is 16-byte aligned in memory
        front = (int)((((unsigned long long)(uintptr_t)row >> 2) + (unsigned long long)q0) & 3ull);
        const long long qa = q0 - front;
        const int len = (int)(i_last - s_start) + 1 + front;
        int nvec = (len + 3) >> 2;
        if (nvec > RS_SPAN_CAP / 4) nvec = RS_SPAN_CAP / 4;       // (never: the host sized a.tile for it)
        for (int v = t; v < nvec; v += RS_TPB) {
            const long long q = qa + 4 * (long long)v;
            float4 f;
            if (q >= 0 && q + 3 < a.n_buf) {
                f = *reinterpret_cast<const float4*>(row + q);
            } else {
                f.x = (q >= 0 && q < a.n_buf) ? row[q] : 0.f;
                f.y = (q + 1 >= 0 && q + 1 < a.n_buf) ? row[q + 1] : 0.f;
                f.z = (q + 2 >= 0 && q + 2 < a.n_buf) ? row[q + 2] : 0.f;
                f.w = (q + 3 >= 0 && q + 3 < a.n_buf) ? row[q + 3] : 0.f;
            }
            *reinterpret_cast<float4*>(s_x + 4 * v) = f;
        }
    }
    if (TAPS_LDS)
        for (int j = t; j < a.T; j += RS_TPB) s_h[j] = a.tab[j];
    if (STAGED || TAPS_LDS) __syncthreads();
    if (t >= cnt) return;
    const long long pos = (n_first + t + a.pre_remove) * a.down;
    const long long i_hi = pos / a.up;
    const int p = (int)(pos - i_hi * a.up);
    const double* h = TAPS_LDS ? s_h : a.tab + (size_t)p * a.T;
    double acc = 0.0;
    if (STAGED) {
        const float* xs = s_x + (int)(i_hi - s_start) + front;    // xs[-j] = x[i_hi - j]
        for (int j = 0; j < a.T; j += 2) {
            const double2 hh = *reinterpret_cast<const double2*>(h + j);
            acc = fma((double)xs[-j], hh.x, acc);
            acc = fma((double)xs[-j - 1], hh.y, acc);
        }
    } else {
        for (int j = 0; j < a.T; ++j) {
            const long long q = i_hi - j - a.pos_in;
            const float v = (q >= 0 && q < a.n_buf) ? row[q] : 0.f;
            acc = fma((double)v, h[j], acc);
        }
    }
    a.y[(size_t)blockIdx.y * a.ld_out + o_first + t] = (float)acc;
}

// fs_in == fs_out: y[n] = x[n]
__global__ __launch_bounds__(RS_TPB) void resample_copy(RsArgs a) {
    const int o = blockIdx.x * RS_TPB + threadIdx.x;
    if (o >= a.n_out) return;
    const long long q = a.n0 + o - a.pos_in;
    a.y[(size_t)blockIdx.y * a.ld_out + o] = (q >= 0 && q < a.n_buf) ? a.x[(size_t)blockIdx.y * a.ld_in + q] : 0.f;
}

// Outputs per block: the most (<= RS_TPB) whose span, floor((n - 1) down / up) + 1 + T samples plus 3 of alignment in
// front, rounded up to whole float4s, fits RS_SPAN_CAP.  0: not even one does.
inline int rs_tile(const RsGeom& g) {
    const long long room = (long long)RS_SPAN_CAP - g.T - 7;      // floor((n - 1) down / up) <= room
    if (room < 0) return 0;
    const long long n = ((room + 1) * g.up - 1) / g.down + 1;
    return n > RS_TPB ? RS_TPB : (int)n;
}

inline size_t rs_ws_bytes(const RsGeom& g) { return up256((size_t)g.up * g.T * sizeof(double)); }

}  // namespace

extern "C" int cmgan_resample_geometry(int fs_in, int fs_out, int* up, int* down, int* n_taps, int* pre_remove) {
    RsGeom g;
    if (!rs_geom(fs_in, fs_out, g))
        return fail(nullptr, CMGAN_E_UNSUPPORTED, "cmgan_resample: %d -> %d Hz needs positive rates whose reduced ratio "
                    "stays within %d", fs_in, fs_out, RS_MAX_RATE);
    if (up) *up = g.up;
    if (down) *down = g.down;
    if (n_taps) *n_taps = g.n_taps;
    if (pre_remove) *pre_remove = g.pre_remove;
    return CMGAN_OK;
}

extern "C" long long cmgan_resample_out_len(int fs_in, int fs_out, long long n_in) {
    RsGeom g;
    if (!rs_geom(fs_in, fs_out, g)) return CMGAN_E_UNSUPPORTED;
    if (n_in < 0) return CMGAN_E_BADARG;
    return (n_in * g.up + g.down - 1) / g.down;
}

extern "C" int cmgan_resample_table(int fs_in, int fs_out, double* out, size_t cap) {
    RsGeom g;
    if (int rc = cmgan_resample_geometry(fs_in, fs_out, nullptr, nullptr, nullptr, nullptr)) return rc;
    rs_geom(fs_in, fs_out, g);
    if (!out) return g.n_taps;
    if (cap < (size_t)g.n_taps) return fail(nullptr, CMGAN_E_BADARG, "cmgan_resample_table: cap %zu < %d", cap, g.n_taps);
    rs_taps_host(g, out);
    return g.n_taps;
}

extern "C" size_t cmgan_resample_workspace_bytes(const cmgan_handle* h, int fs_in, int fs_out) {
    (void)h;
    RsGeom g;
    return rs_geom(fs_in, fs_out, g) ? rs_ws_bytes(g) : 0;
}

extern "C" int cmgan_resample(cmgan_handle* h, const float* x, int B, int n_buf, long long ld_in, long long pos_in,
                              int fs_in, int fs_out, long long n0, int n_out, float* y, long long ld_out, void* ws,
                              size_t ws_bytes, void* stream) {
    if (!h) return CMGAN_E_BADARG;
    if (!x || !y) return fail(h, CMGAN_E_BADARG, "cmgan_resample: null pointer");
    if (((uintptr_t)x & 3) || ((uintptr_t)y & 3)) return fail(h, CMGAN_E_BADARG, "cmgan_resample: buffers must be 4-byte aligned");
    if (B <= 0 || B > 65535 || n_buf < 0 || n_out < 0 || ld_in < n_buf || ld_out < n_out || pos_in < 0 || n0 < 0)
        return fail(h, CMGAN_E_BADARG, "cmgan_resample: need 0 < B <= 65535, 0 <= n_buf <= ld_in, 0 <= n_out <= ld_out, "
                    "pos_in >= 0, n0_out >= 0 (B=%d n_buf=%d ld_in=%lld pos_in=%lld n0_out=%lld n_out=%d ld_out=%lld)",
                    B, n_buf, ld_in, pos_in, n0, n_out, ld_out);
    RsGeom g;
    if (!rs_geom(fs_in, fs_out, g))
        return fail(h, CMGAN_E_UNSUPPORTED, "cmgan_resample: %d -> %d Hz needs positive rates whose reduced ratio stays "
                    "within %d", fs_in, fs_out, RS_MAX_RATE);
    if (int rc = check_ws(h, ws, ws_bytes, rs_ws_bytes(g))) return rc;
    if (n_out == 0) return CMGAN_OK;
    const LaunchCtx ctx = begin(h, stream);
    hipStream_t s = ctx.stream;
    RsArgs a{x, y, (const double*)ws, ld_in, ld_out, pos_in, n0, n_buf, n_out, g.up, g.down, g.T, g.pre_remove, RS_TPB};
    if (g.up == 1 && g.down == 1) {
        LAUNCH(ctx, "resample_copy", resample_copy<<<dim3((n_out + RS_TPB - 1) / RS_TPB, B), RS_TPB, 0, s>>>(a));
        return check_launch(h, "resample");
    }
    LAUNCH(ctx, "resample_table", resample_table<<<1, RS_TB_TPB, 0, s>>>(g, (double*)ws));
    const int tile = rs_tile(g);
    a.tile = tile > 0 ? tile : RS_TPB;
    const dim3 grid((n_out + a.tile - 1) / a.tile, B);
    if (tile == 0)
        LAUNCH(ctx, "resample_poly", resample_poly<false, false><<<grid, RS_TPB, 0, s>>>(a));
    else if (g.up == 1 && g.T <= RS_TAPS_LDS)
        LAUNCH(ctx, "resample_poly", resample_poly<true, true><<<grid, RS_TPB, 0, s>>>(a));
    else
        LAUNCH(ctx, "resample_poly", resample_poly<false, true><<<grid, RS_TPB, 0, s>>>(a));
    return check_launch(h, "resample");
}
