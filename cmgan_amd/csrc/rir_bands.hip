// rir_bands.hip - room impulse responses with frequency-dependent walls and air absorption (cmgan_rir_bands,
// include/cmgan_hip.h): the image-source method of rir.hip simulated in NB frequency bands at once and joined by a
// caller-supplied FIR filterbank.  The reference ships no impulse responses and no simulator (its data path replays pairs
// mixed beforehand, src/data/dataloader.py:13-50).
//
//   row r: room L, source s, receiver m (columns 0 - 8 of cmgan_rir's table), per band b the six reflection coefficients
//          and the air attenuation m_b in nepers per metre;  k_r = clamp(n_taps[r], 1, K), D = (NF - 1) / 2
//   image (n, p) as in cmgan_rir:  a_b = prod_axis b_{b,axis0}^|n - p| b_{b,axis1}^|n| exp(-m_b d) / (4 pi max(d, CMGAN_RIR_DMIN))
//   h_b[q] = sum_images a_b w(q - tau) sinc(q - tau), 0 <= q < k_r + D
//   h[k]   = sum_b sum_j g_b[j] h_b[k + D - j]   (b, then j ascending, one fma per term)
//   rir[r, k] = f32(h[k]) for k < k_r, 0 for k_r <= k < K;  len[r] = k_r
//
// An image's position, delay, window and sinc are the same in every band; only its amplitude differs.  So the image list
// of rir_taps is built ONCE and a thread carries one accumulator per band.  Float64 throughout, one rounding to float32
// at the store, no atomics.  Three launches per call:
//   rir_bands_prep   one block per row: judges the row (a non-finite entry in columns 0 - 8 or in its band table, a size
//                    <= 0, a coefficient outside [0, 1] or a negative m_b makes it invalid: zeros, len 1), writes len, and
//                    leaves in the workspace the row's record: its 9 numbers, k_r (0 = invalid), the m_b and the powers
//                    b^e, e = 0 .. 256, of its 6 NB coefficients (pow(), so 0^0 = 1).  Eight bands of powers (96 KiB) do
//                    not fit beside the list in LDS: they stay in the workspace and are read, through the caches, while
//                    the list is built - four per (column, band) and two per (image, band), never per tap.
//   rir_bands_taps   rir_taps over K + D taps with NB accumulators: the same range solve, count, prefix sum and
//                    order-preserving compaction, once per image.  A list entry holds t0 = k0 - tau, sin(pi t0) / pi,
//                    cos(pi t0 / tw) / 2, sin(pi t0 / tw) / 2 and the image's NB amplitudes; a thread forms
//                    v = w(t) sinc(t) once per entry inside its window and adds a_b v to accumulator b.  The sums go to the
//                    workspace as float64 [R, NB, K + D]; only q < k_r + D is written, and only that is read.
//   rir_bands_join   one block per (tile of RR_TILE outputs, row): band after band it stages the span its outputs reach,
//                    RR_TILE + NF - 1 samples (zeros outside [0, k_r + D)), and the band's NF filter taps in LDS, and every
//                    thread runs its double sum in the stated order into ONE accumulator; it rounds once and writes the
//                    zeros beyond k_r.  Consecutive threads read consecutive float64 (no bank conflict), the filter tap is
//                    a broadcast.
// Per (tap, band) the images are added in the enumeration order of rir_taps whatever R, the other rows and the launch are.
// Nothing read from a table becomes an address: list places come from counts, the nz bounds are clamped as doubles, the
// filter values are only ever multiplied.
#include <math.h>
#include <stdint.h>

#include "api_internal.h"
#include "rir_common.hip.h"

namespace {

constexpr int RB_MAX_BANDS = 8;
constexpr int RB_MAX_FILTER = 1023;
constexpr int RB_HEAD = 24;                       // record: 9 room numbers, (unused), k_r at 15, m_b at 16 .. 23
constexpr int RB_SPAN = RR_TILE + RB_MAX_FILTER - 1;

// Between the 8-byte LDS stores of a list entry: merged into one 16-byte store (ds_write2_b64), the later data dwords are
// still being read by the LDS path when the next VALU instruction overwrites them (tools/isa_lint.py).
#define RB_KEEP_APART() asm volatile("" ::: "memory")

__host__ __device__ inline size_t rb_rec(int NB) { return (size_t)RB_HEAD + (size_t)6 * NB * RR_PW; }      // float64 words of a row's record

struct BandArgs {
    const double* rooms;
    const double* bands;     // [R][NB][7]
    const double* filt;      // [NB][NF]
    const int* n_taps;
    float* rir;
    int* len;
    double* rec;             // workspace: [R][rb_rec(NB)]
    double* hb;              // workspace: [R][NB][K + D]
    long long ld;
    double fs, c;
    int R, K, NB, NF, tw, Nx, Ny, Nz;
};

__global__ __launch_bounds__(RR_TPB) void rir_bands_prep(BandArgs a) {
    const int t = threadIdx.x, r = blockIdx.x;
    const double* room = a.rooms + (size_t)r * 15;
    const double* band = a.bands + (size_t)r * a.NB * 7;
    double* rec = a.rec + (size_t)r * rb_rec(a.NB);
    bool ok = true;
    for (int i = 0; i < 9; ++i) {
        const double v = room[i];
        ok = ok && (v - v == 0.0);                               // finite
        if (i < 3) ok = ok && v > 0.0;
    }
    for (int i = 0; i < a.NB * 7; ++i) {
        const double v = band[i];
        ok = ok && (v - v == 0.0) && v >= 0.0;
        if (i % 7 < 6) ok = ok && v <= 1.0;
    }
    int kr = a.n_taps[r];
    kr = kr < 1 ? 1 : (kr > a.K ? a.K : kr);
    if (!ok) kr = 1;
    if (t < 9) rec[t] = room[t];
    if (t >= 9 && t < 15) rec[t] = 0.0;
    if (t == 15) rec[15] = ok ? (double)kr : 0.0;
    if (t >= 16 && t < RB_HEAD) rec[t] = (ok && t - 16 < a.NB) ? band[(t - 16) * 7 + 6] : 0.0;
    if (t == 0) a.len[r] = kr;
    for (int i = t; i < 6 * a.NB * RR_PW; i += RR_TPB) {
        const int w = i / RR_PW, e = i - w * RR_PW;              // w = 6 b + wall
        const int b = w / 6;
        rec[RB_HEAD + i] = ok ? pow(band[b * 7 + (w - 6 * b)], (double)e) : 0.0;
    }
}

template <int NB>
__global__ __launch_bounds__(RR_TPB) void rir_bands_taps(BandArgs a) {
    __shared__ double s_t0[RR_CAP + RR_UNR], s_sp[RR_CAP], s_hc[RR_CAP], s_hs[RR_CAP];
    __shared__ double s_amp[NB][RR_CAP];
    __shared__ int s_scan[2][RR_TPB];
    const int t = threadIdx.x, r = blockIdx.y;
    const int k0 = blockIdx.x * RR_TILE, k = k0 + t;
    const int D = (a.NF - 1) / 2, KD = a.K + D;
    const double* rec = a.rec + (size_t)r * rb_rec(NB);
    const double* pw = rec + RB_HEAD;                            // [NB][6][RR_PW]
    const int kr = (int)rec[15];                                 // 0: an invalid row
    const int kq = kr > 0 ? kr + D : 0;                          // the band responses hold taps [0, kq)
    if (k0 >= kq) return;                                        // (the whole block; nothing from kq on is ever read)
    const double Lx = rec[0], Ly = rec[1], Lz = rec[2];
    const double sx = rec[3], sy = rec[4], sz = rec[5];
    const double mx = rec[6], my = rec[7], mz = rec[8];
    double air[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) air[b] = rec[16 + b];
    const int k_last = (k0 + RR_TILE < kq ? k0 + RR_TILE : kq) - 1;
    const double twd = (double)a.tw;
    const double t_lo = (double)(k0 - a.tw), t_hi = (double)(k_last + a.tw);     // an image reaches the tile iff t_lo < tau < t_hi
    // the same shell in metres, a little wider than exact, for the nz range solve only
    const double d_hi = t_hi * a.c / a.fs * (1.0 + 1e-12);
    const double d_lo = t_lo > 0.0 ? t_lo * a.c / a.fs * (1.0 - 1e-12) : 0.0;
    const double d_hi2 = d_hi * d_hi, d_lo2 = d_lo * d_lo;
    const double spm = a.fs / a.c;                               // samples per metre: tau = d * spm everywhere below
    const double inv_2lz = 0.5 / Lz;                             // (range solve only)
    const int wy = 2 * a.Ny + 1;
    const int ncols = (2 * a.Nx + 1) * wy * 8;
    // this thread's tap: j = t
    const double jd = (double)t;
    const double cj = cospi(jd / twd), sj = sinpi(jd / twd);
    const double sgn = (t & 1) ? -1.0 : 1.0;
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;

    for (int c0 = 0; c0 < ncols; c0 += RR_TPB) {
        const int col = c0 + t;
        // ---- this thread's column: the nz candidates [lo1, hi1] then [lo2, hi2] (ascending, disjoint)
        int lo1 = 0, hi1 = -1, lo2 = 0, hi2 = -1;
        double q = 0.0, zo = 0.0;
        int pz = 0, ax = 0, bx = 0, ay = 0, by = 0;              // the exponents of the column's four x / y coefficients
        if (col < ncols) {
            const int p = col & 7, xy = col >> 3;
            const int ix = xy / wy, iy = xy - ix * wy;
            const int nx = ix - a.Nx, ny = iy - a.Ny;
            const int px = p >> 2, py = (p >> 1) & 1;
            pz = p & 1;
            const double dx = fma((double)(2 * nx), Lx, (px ? -sx : sx) - mx);
            const double dy = fma((double)(2 * ny), Ly, (py ? -sy : sy) - my);
            q = fma(dy, dy, dx * dx);
            zo = (pz ? -sz : sz) - mz;
            const int ex = nx - px, ey = ny - py;
            ax = ex < 0 ? -ex : ex;
            bx = nx < 0 ? -nx : nx;
            ay = ey < 0 ? -ey : ey;
            by = ny < 0 ? -ny : ny;
            const double B = d_hi2 - q;
            if (B > 0.0) {
                const double z_hi = sqrt(B), A = d_lo2 - q;
                const double z_lo = A > 0.0 ? sqrt(A) : 0.0;
                // dz = zo + 2 nz Lz in [-z_hi, -z_lo] or [z_lo, z_hi], one index of margin on each side
                int nl = rr_bound(ceil((-z_hi - zo) * inv_2lz), a.Nz) - 1, nh = rr_bound(floor((-z_lo - zo) * inv_2lz), a.Nz) + 1;
                int pl = rr_bound(ceil((z_lo - zo) * inv_2lz), a.Nz) - 1, ph = rr_bound(floor((z_hi - zo) * inv_2lz), a.Nz) + 1;
                nl = nl < -a.Nz ? -a.Nz : nl;
                pl = pl < -a.Nz ? -a.Nz : pl;
                nh = nh > a.Nz ? a.Nz : nh;
                ph = ph > a.Nz ? a.Nz : ph;
                if (nh >= pl - 1) {                               // the two ranges meet: one range
                    lo1 = nl < pl ? nl : pl;
                    hi1 = ph > nh ? ph : nh;
                } else {
                    lo1 = nl; hi1 = nh; lo2 = pl; hi2 = ph;
                }
            }
        }
        const int n1 = hi1 >= lo1 ? hi1 - lo1 + 1 : 0;
        const int ncand = n1 + (hi2 >= lo2 ? hi2 - lo2 + 1 : 0);
        // ---- count the candidates that reach the tile, with the delay the entries are made from
        int cnt = 0;
        for (int i = 0; i < ncand; ++i) {
            const int nz = i < n1 ? lo1 + i : lo2 + (i - n1);
            const double dz = fma((double)(2 * nz), Lz, zo);
            const double tau = sqrt(fma(dz, dz, q)) * spm;
            cnt += (tau > t_lo && tau < t_hi) ? 1 : 0;
        }
        int total;
        const int base = rr_scan(cnt, s_scan, total);
        // the column's x / y factor per band (exponents <= N + 1 < RR_PW: indices, not table values)
        double cxy[NB];
        if (cnt > 0) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const double* pb = pw + (size_t)b * 6 * RR_PW;
                cxy[b] = pb[0 * RR_PW + ax] * pb[1 * RR_PW + bx] * pb[2 * RR_PW + ay] * pb[3 * RR_PW + by];
            }
        } else {
#pragma unroll
            for (int b = 0; b < NB; ++b) cxy[b] = 0.0;
        }
        // ---- the round's list, RR_CAP entries at a time
        int cursor = 0, pos = base;
        for (int cs = 0; cs < total; cs += RR_CAP) {
            const int end = cs + RR_CAP;
            while (cursor < ncand && pos < end && pos < base + cnt) {
                const int nz = cursor < n1 ? lo1 + cursor : lo2 + (cursor - n1);
                ++cursor;
                const double dz = fma((double)(2 * nz), Lz, zo);
                const double d = sqrt(fma(dz, dz, q));
                const double tau = d * spm;
                if (!(tau > t_lo && tau < t_hi)) continue;
                const int e = pos - cs;                           // >= 0: a chunk is filled before the next begins
                ++pos;
                const int ez = nz - pz;
                const int az = ez < 0 ? -ez : ez, bz = nz < 0 ? -nz : nz;
                const double spread = 4.0 * RR_PI * fmax(d, CMGAN_RIR_DMIN);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const double* pb = pw + (size_t)b * 6 * RR_PW;
                    const double att = air[b] == 0.0 ? 1.0 : exp(-air[b] * d);
                    s_amp[b][e] = cxy[b] * pb[4 * RR_PW + az] * pb[5 * RR_PW + bz] * att / spread;
                    RB_KEEP_APART();
                }
                const double t0 = (double)k0 - tau, ang = t0 / twd;
                s_t0[e] = t0;
                RB_KEEP_APART();
                s_sp[e] = sinpi(t0) / RR_PI;
                RB_KEEP_APART();
                s_hc[e] = 0.5 * cospi(ang);
                RB_KEEP_APART();
                s_hs[e] = 0.5 * sinpi(ang);
                RB_KEEP_APART();
            }
            const int n = total - cs < RR_CAP ? total - cs : RR_CAP;
            if (t < RR_UNR) s_t0[n + t] = 1.0e300;                // the tail of the last group of RR_UNR: in no window
            __syncthreads();
            if (k < kq) {
                for (int i = 0; i < n; i += RR_UNR) {
                    double tt[RR_UNR];
#pragma unroll
                    for (int u = 0; u < RR_UNR; ++u) tt[u] = jd + s_t0[i + u];     // one LDS latency for the group
#pragma unroll
                    for (int u = 0; u < RR_UNR; ++u)
                        if (fabs(tt[u]) < twd) {
                            const double w = 0.5 + (cj * s_hc[i + u] - sj * s_hs[i + u]);
                            const double sc = tt[u] == 0.0 ? 1.0 : sgn * s_sp[i + u] / tt[u];
                            const double v = w * sc;
#pragma unroll
                            for (int b = 0; b < NB; ++b) acc[b] = fma(s_amp[b][i + u], v, acc[b]);
                        }
                }
            }
            __syncthreads();
        }
    }
    if (k < kq) {
        double* hb = a.hb + (size_t)r * NB * KD;
#pragma unroll
        for (int b = 0; b < NB; ++b) hb[(size_t)b * KD + k] = acc[b];
    }
}

__global__ __launch_bounds__(RR_TPB) void rir_bands_join(BandArgs a) {
    __shared__ double s_h[RB_SPAN], s_g[RB_MAX_FILTER];
    const int t = threadIdx.x, r = blockIdx.y;
    const int k0 = blockIdx.x * RR_TILE, k = k0 + t;
    const int NF = a.NF, D = (NF - 1) / 2, KD = a.K + D;
    const int kr = (int)a.rec[(size_t)r * rb_rec(a.NB) + 15];     // 0: an invalid row
    float* out = a.rir + (size_t)r * a.ld;
    if (k0 >= kr) {                                              // (the whole block: nothing of this tile is a tap)
        if (k < a.K) out[k] = 0.f;
        return;
    }
    const int kq = kr + D, span = RR_TILE + NF - 1;
    double acc = 0.0;
    for (int b = 0; b < a.NB; ++b) {
        const double* hb = a.hb + ((size_t)r * a.NB + b) * KD;
        const double* g = a.filt + (size_t)b * NF;
        for (int i = t; i < span; i += RR_TPB) {                  // s_h[i] = h_b[k0 - D + i]
            const int q = k0 - D + i;
            s_h[i] = (q >= 0 && q < kq) ? hb[q] : 0.0;
        }
        for (int i = t; i < NF; i += RR_TPB) s_g[i] = g[i];
        __syncthreads();
        if (k < kr) {
            const double* hp = s_h + t + NF - 1;                  // h_b[k + D - j] = s_h[t + 2 D - j]
            for (int j = 0; j < NF; ++j) acc = fma(s_g[j], hp[-j], acc);
        }
        __syncthreads();
    }
    if (k < a.K) out[k] = k < kr ? (float)acc : 0.f;
}

inline bool rb_shape_ok(int R, int K, int tw, int NB, int NF) {
    return R >= 1 && R <= 65535 && K >= 1 && K <= RR_MAX_K && tw >= 1 && tw <= RR_MAX_TW && NB >= 1 && NB <= RB_MAX_BANDS &&
           NF >= 1 && NF <= RB_MAX_FILTER && (NF & 1);
}

inline size_t rb_rec_bytes(int R, int NB) { return rr_up256((size_t)R * rb_rec(NB) * sizeof(double)); }

template <int NB>
void rb_launch_taps(const LaunchCtx& ctx, hipStream_t s, const dim3& grid, const BandArgs& a) {
    LAUNCH(ctx, "rir_bands_taps", rir_bands_taps<NB><<<grid, RR_TPB, 0, s>>>(a));
}

}  // namespace

extern "C" int cmgan_rir_max_bands(void) { return RB_MAX_BANDS; }

extern "C" int cmgan_rir_max_filter(void) { return RB_MAX_FILTER; }

extern "C" size_t cmgan_rir_bands_workspace_bytes(const cmgan_handle* h, int R, int K, int tw, int NB, int NF) {
    (void)h;
    if (!rb_shape_ok(R, K, tw, NB, NF)) return 0;
    return rb_rec_bytes(R, NB) + rr_up256((size_t)R * NB * (size_t)(K + (NF - 1) / 2) * sizeof(double));
}

extern "C" int cmgan_rir_bands(cmgan_handle* h, const double* rooms, const double* bands, const int* n_taps, int R, int K,
                               int NB, const double* filt, int NF, int fs, double c, int tw, int Nx, int Ny, int Nz,
                               float* rir, long long ld, int* len, void* ws, size_t ws_bytes, void* stream) {
    // every argument is judged before the handle is, so that the errors below need no GPU (the message of a call
    // without a handle is read with cmgan_last_error(NULL))
    if (!rooms || !bands || !filt || !n_taps || !rir || !len) return fail(h, CMGAN_E_BADARG, "cmgan_rir_bands: null pointer");
    if (((uintptr_t)rooms | (uintptr_t)bands | (uintptr_t)filt) & 7)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_bands: the float64 room, band and filter tables must be 8-byte aligned");
    if (((uintptr_t)n_taps | (uintptr_t)rir | (uintptr_t)len) & 3)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_bands: float32 / int32 buffers must be 4-byte aligned");
    if (R < 1 || R > 65535 || K < 1 || ld < K)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_bands: need 1 <= R <= 65535, K >= 1, ld >= K (R=%d K=%d ld=%lld)", R, K, ld);
    if (NB < 1 || NB > RB_MAX_BANDS)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_bands: need 1 <= NB <= %d bands (NB=%d)", RB_MAX_BANDS, NB);
    if (NF < 1 || !(NF & 1))
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_bands: the filter length must be odd and >= 1 (NF=%d)", NF);
    if (fs < 1) return fail(h, CMGAN_E_BADARG, "cmgan_rir_bands: fs must be positive (fs=%d)", fs);
    if (!(c > 0.0) || !(c <= 1.0e300))
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_bands: the speed of sound c must be positive and finite (%g)", c);
    if (tw < 1) return fail(h, CMGAN_E_BADARG, "cmgan_rir_bands: tw must be >= 1 (tw=%d)", tw);
    if (Nx < 0 || Ny < 0 || Nz < 0)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir_bands: image ranges must be >= 0 (Nx=%d Ny=%d Nz=%d)", Nx, Ny, Nz);
    if (K > RR_MAX_K)
        return fail(h, CMGAN_E_UNSUPPORTED, "cmgan_rir_bands: responses of up to %d taps are supported (K=%d)", RR_MAX_K, K);
    if (NF > RB_MAX_FILTER)
        return fail(h, CMGAN_E_UNSUPPORTED, "cmgan_rir_bands: filters of up to %d taps are supported (NF=%d)", RB_MAX_FILTER, NF);
    if (tw > RR_MAX_TW)
        return fail(h, CMGAN_E_UNSUPPORTED, "cmgan_rir_bands: a filter half-width of up to %d samples is supported (tw=%d)",
                    RR_MAX_TW, tw);
    if (Nx > RR_MAX_N || Ny > RR_MAX_N || Nz > RR_MAX_N)
        return fail(h, CMGAN_E_UNSUPPORTED, "cmgan_rir_bands: image ranges of up to %d are supported (Nx=%d Ny=%d Nz=%d)",
                    RR_MAX_N, Nx, Ny, Nz);
    if (8LL * (2 * Nx + 1) * (2 * Ny + 1) * (2 * Nz + 1) >= (1LL << 31))
        return fail(h, CMGAN_E_UNSUPPORTED,
                    "cmgan_rir_bands: 8 (2Nx+1)(2Ny+1)(2Nz+1) must stay below 2^31 (Nx=%d Ny=%d Nz=%d)", Nx, Ny, Nz);
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "cmgan_rir_bands: null handle");
    if (int rc = check_ws(h, ws, ws_bytes, cmgan_rir_bands_workspace_bytes(h, R, K, tw, NB, NF))) return rc;
    const LaunchCtx ctx = begin(h, stream);
    hipStream_t s = ctx.stream;
    const int D = (NF - 1) / 2;
    BandArgs a;
    a.rooms = rooms;
    a.bands = bands;
    a.filt = filt;
    a.n_taps = n_taps;
    a.rir = rir;
    a.len = len;
    a.rec = (double*)ws;
    a.hb = (double*)((char*)ws + rb_rec_bytes(R, NB));
    a.ld = ld;
    a.fs = (double)fs;
    a.c = c;
    a.R = R;
    a.K = K;
    a.NB = NB;
    a.NF = NF;
    a.tw = tw;
    a.Nx = Nx;
    a.Ny = Ny;
    a.Nz = Nz;
    const dim3 grid_taps((K + D + RR_TILE - 1) / RR_TILE, R), grid_join((K + RR_TILE - 1) / RR_TILE, R);
    LAUNCH(ctx, "rir_bands_prep", rir_bands_prep<<<R, RR_TPB, 0, s>>>(a));
    switch (NB) {
        case 1: rb_launch_taps<1>(ctx, s, grid_taps, a); break;
        case 2: rb_launch_taps<2>(ctx, s, grid_taps, a); break;
        case 3: rb_launch_taps<3>(ctx, s, grid_taps, a); break;
        case 4: rb_launch_taps<4>(ctx, s, grid_taps, a); break;
        case 5: rb_launch_taps<5>(ctx, s, grid_taps, a); break;
        case 6: rb_launch_taps<6>(ctx, s, grid_taps, a); break;
        case 7: rb_launch_taps<7>(ctx, s, grid_taps, a); break;
        default: rb_launch_taps<8>(ctx, s, grid_taps, a); break;
    }
    LAUNCH(ctx, "rir_bands_join", rir_bands_join<<<grid_join, RR_TPB, 0, s>>>(a));
    return check_launch(h, "rir_bands");
}
