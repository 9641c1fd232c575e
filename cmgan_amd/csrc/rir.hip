// rir.hip - room impulse responses of shoe-box rooms by the image-source method on the device (cmgan_rir,
// include/cmgan_hip.h): Allen & Berkley 1979 with Peterson's Hann-windowed sinc for the fractional delays.  The
// reference ships no impulse responses and no simulator (its data path replays pairs mixed beforehand,
// src/data/dataloader.py:13-50); this file makes the [R, Kmax] float32 bank + int32 lengths that cmgan_mix consumes.
//
//   row r: room L, source s, receiver m, reflection coefficients b (wall at 0, wall at L per axis), k_r = clamp(n_taps[r], 1, K)
//   image (n, p), |n_axis| <= N_axis, p in {0,1}^3:  offset_axis = (1 - 2 p) s + 2 n L - m, d = |offset|, tau = d fs / c
//   a = prod_axis b_axis0^|n - p| b_axis1^|n| / (4 pi max(d, CMGAN_RIR_DMIN))
//   h[k] = sum_images a w(k - tau) sinc(k - tau), w(t) = (1 + cos(pi t / tw)) / 2 for |t| < tw, else 0
//   rir[r, k] = f32(h[k]) for k < k_r, 0 for k_r <= k < K;  len[r] = k_r
//
// Float64 throughout, one rounding to float32 at the store, no atomics.  Two launches per call:
//   rir_prep   one block per row: judges the row (a non-finite entry, a size <= 0 or a coefficient outside [0, 1] makes the
//              row invalid: zeros, len 1), writes len, and leaves in the workspace a record of the row: its 15 numbers, k_r
//              (0 = invalid) and the powers b^e, e = 0 .. 256, of its six coefficients (pow(), so 0^0 = 1)
//   rir_taps   one block per (tile of RR_TILE taps, row), one thread per tap holding the tap's accumulator.  The images are
//              visited in ONE fixed order - columns (nx, ny, p) ascending, nz ascending inside a column - in rounds of 256
//              columns, one per thread.  A thread solves the nz range whose delay can reach the tile's time shell
//              tau in (k0 - tw, k_last + tw) (a superset: one index of margin on each side), counts the images that do reach
//              it with the delay every later step uses, and an integer prefix sum over the block gives each image its
//              place in the round's list: order-preserving compaction.  The list lives in LDS, RR_CAP entries at a time
//              (a round with more is consumed in chunks), an entry being what depends on the image alone:
//                  t0 = k0 - tau, sin(pi t0) / pi, a / 2, (a / 2) cos(pi t0 / tw), (a / 2) sin(pi t0 / tw)
//              Every thread then adds the list in list order.  For tap k0 + j: t = j + t0, sin(pi t) = (-1)^j sin(pi t0)
//              (one sin per image) and a w(t) = a / 2 + cos(pi j / tw) (a / 2) cos(pi t0 / tw) - sin(pi j / tw) (a / 2)
//              sin(pi t0 / tw): the angle-addition identity with the thread's own two constants, no trigonometry per
//              (image, tap); what is left is one division.  Entries outside |t| < tw are skipped, so an image that a
//              larger N than needed adds changes no bit.  A thread fetches the t0 of RR_UNR entries at once, one LDS
//              latency per group instead of one per entry (measured: a fifth to a quarter off the call).
// A tap's sum is therefore in enumeration order whatever R, the other rows and the launch are: the same bits from run to
// run, row r independent of R.  Nothing read from the tables becomes an address: the list index comes from counts, the
// nz bounds are clamped as doubles before they become ints, and taps are written below K only.
#include <math.h>
#include <stdint.h>

#include "api_internal.h"
#include "rir_common.hip.h"

namespace {

constexpr int RR_HEAD = 16;                 // record: 15 room numbers, k_r
constexpr int RR_REC = RR_HEAD + 6 * RR_PW; // float64 words of a row's record in the workspace

struct RirArgs {
    const double* rooms;
    const int* n_taps;
    float* rir;
    int* len;
    double* rec;             // workspace: [R][RR_REC]
    long long ld;
    double fs, c;
    int R, K, tw, Nx, Ny, Nz;
};

__global__ __launch_bounds__(RR_TPB) void rir_prep(RirArgs a) {
    const int t = threadIdx.x, r = blockIdx.x;
    const double* room = a.rooms + (size_t)r * 15;
    double* rec = a.rec + (size_t)r * RR_REC;
    bool ok = true;
    for (int i = 0; i < 15; ++i) {
        const double v = room[i];
        ok = ok && (v - v == 0.0);                               // finite
        if (i < 3) ok = ok && v > 0.0;
        if (i >= 9) ok = ok && v >= 0.0 && v <= 1.0;
    }
    int kr = a.n_taps[r];
    kr = kr < 1 ? 1 : (kr > a.K ? a.K : kr);
    if (!ok) kr = 1;
    if (t < 15) rec[t] = room[t];
    if (t == 15) rec[15] = ok ? (double)kr : 0.0;
    if (t == 0) a.len[r] = kr;
    for (int i = t; i < 6 * RR_PW; i += RR_TPB) {
        const int w = i / RR_PW, e = i - w * RR_PW;
        rec[RR_HEAD + i] = ok ? pow(room[9 + w], (double)e) : 0.0;
    }
}

// one list entry for the tap at t = tt (its window test included); `sgn` = (-1)^j, cj / sj = cos / sin(pi j / tw)
__device__ inline double rr_tap(double acc, double tt, double twd, double sgn, double cj, double sj, double sp, double ha,
                                double hc, double hs) {
    const double wa = ha + (cj * hc - sj * hs);
    const double sc = tt == 0.0 ? 1.0 : sgn * sp / tt;
    return fma(wa, sc, acc);
}

__global__ __launch_bounds__(RR_TPB) void rir_taps(RirArgs a) {
    __shared__ double s_pw[6 * RR_PW];
    __shared__ double s_t0[RR_CAP + RR_UNR], s_sp[RR_CAP], s_ha[RR_CAP], s_hc[RR_CAP], s_hs[RR_CAP];
    __shared__ int s_scan[2][RR_TPB];
    const int t = threadIdx.x, r = blockIdx.y;
    const int k0 = blockIdx.x * RR_TILE, k = k0 + t;
    const double* rec = a.rec + (size_t)r * RR_REC;
    float* out = a.rir + (size_t)r * a.ld;
    const int kr = (int)rec[15];                                 // 0: an invalid row
    if (k0 >= kr) {                                              // (the whole block: nothing of this tile is a tap)
        if (k < a.K) out[k] = 0.f;
        return;
    }
    for (int i = t; i < 6 * RR_PW; i += RR_TPB) s_pw[i] = rec[RR_HEAD + i];
    const double Lx = rec[0], Ly = rec[1], Lz = rec[2];
    const double sx = rec[3], sy = rec[4], sz = rec[5];
    const double mx = rec[6], my = rec[7], mz = rec[8];
    __syncthreads();
    const int k_last = (k0 + RR_TILE < kr ? k0 + RR_TILE : kr) - 1;
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
    double acc = 0.0;

    for (int c0 = 0; c0 < ncols; c0 += RR_TPB) {
        const int col = c0 + t;
        // ---- this thread's column: the nz candidates [lo1, hi1] then [lo2, hi2] (ascending, disjoint)
        int lo1 = 0, hi1 = -1, lo2 = 0, hi2 = -1;
        double q = 0.0, zo = 0.0, cxy = 0.0;
        int pz = 0;
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
            cxy = s_pw[0 * RR_PW + (ex < 0 ? -ex : ex)] * s_pw[1 * RR_PW + (nx < 0 ? -nx : nx)]
                * s_pw[2 * RR_PW + (ey < 0 ? -ey : ey)] * s_pw[3 * RR_PW + (ny < 0 ? -ny : ny)];
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
                const double amp = cxy * s_pw[4 * RR_PW + (ez < 0 ? -ez : ez)] * s_pw[5 * RR_PW + (nz < 0 ? -nz : nz)]
                                 / (4.0 * RR_PI * fmax(d, CMGAN_RIR_DMIN));
                const double t0 = (double)k0 - tau, ha = 0.5 * amp, ang = t0 / twd;
                s_t0[e] = t0;
                s_sp[e] = sinpi(t0) / RR_PI;
                s_ha[e] = ha;
                s_hc[e] = ha * cospi(ang);
                s_hs[e] = ha * sinpi(ang);
            }
            const int n = total - cs < RR_CAP ? total - cs : RR_CAP;
            if (t < RR_UNR) s_t0[n + t] = 1.0e300;                // the tail of the last group of RR_UNR: in no window
            __syncthreads();
            if (k < kr) {
                for (int i = 0; i < n; i += RR_UNR) {
                    double tt[RR_UNR];
#pragma unroll
                    for (int u = 0; u < RR_UNR; ++u) tt[u] = jd + s_t0[i + u];     // one LDS latency for the group
#pragma unroll
                    for (int u = 0; u < RR_UNR; ++u)
                        if (fabs(tt[u]) < twd)
                            acc = rr_tap(acc, tt[u], twd, sgn, cj, sj, s_sp[i + u], s_ha[i + u], s_hc[i + u], s_hs[i + u]);
                }
            }
            __syncthreads();
        }
    }
    if (k < a.K) out[k] = k < kr ? (float)acc : 0.f;
}

inline bool rr_shape_ok(int R, int K, int tw) {
    return R >= 1 && R <= 65535 && K >= 1 && K <= RR_MAX_K && tw >= 1 && tw <= RR_MAX_TW;
}

}  // namespace

extern "C" int cmgan_rir_tile(void) { return RR_TILE; }

extern "C" int cmgan_rir_list_capacity(void) { return RR_CAP; }

extern "C" size_t cmgan_rir_workspace_bytes(const cmgan_handle* h, int R, int K, int tw) {
    (void)h;
    return rr_shape_ok(R, K, tw) ? rr_up256((size_t)R * RR_REC * sizeof(double)) : 0;
}

extern "C" int cmgan_rir(cmgan_handle* h, const double* rooms, const int* n_taps, int R, int K, int fs, double c, int tw,
                         int Nx, int Ny, int Nz, float* rir, long long ld, int* len, void* ws, size_t ws_bytes,
                         void* stream) {
    // every argument is judged before the handle is, so that the errors below need no GPU (the message of a call
    // without a handle is read with cmgan_last_error(NULL))
    if (!rooms || !n_taps || !rir || !len) return fail(h, CMGAN_E_BADARG, "cmgan_rir: null pointer");
    if ((uintptr_t)rooms & 7) return fail(h, CMGAN_E_BADARG, "cmgan_rir: the float64 room table must be 8-byte aligned");
    if (((uintptr_t)n_taps | (uintptr_t)rir | (uintptr_t)len) & 3)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir: float32 / int32 buffers must be 4-byte aligned");
    if (R < 1 || R > 65535 || K < 1 || ld < K)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir: need 1 <= R <= 65535, K >= 1, ld >= K (R=%d K=%d ld=%lld)", R, K, ld);
    if (fs < 1) return fail(h, CMGAN_E_BADARG, "cmgan_rir: fs must be positive (fs=%d)", fs);
    if (!(c > 0.0) || !(c <= 1.0e300))
        return fail(h, CMGAN_E_BADARG, "cmgan_rir: the speed of sound c must be positive and finite (%g)", c);
    if (tw < 1) return fail(h, CMGAN_E_BADARG, "cmgan_rir: tw must be >= 1 (tw=%d)", tw);
    if (Nx < 0 || Ny < 0 || Nz < 0)
        return fail(h, CMGAN_E_BADARG, "cmgan_rir: image ranges must be >= 0 (Nx=%d Ny=%d Nz=%d)", Nx, Ny, Nz);
    if (K > RR_MAX_K)
        return fail(h, CMGAN_E_UNSUPPORTED, "cmgan_rir: responses of up to %d taps are supported (K=%d)", RR_MAX_K, K);
    if (tw > RR_MAX_TW)
        return fail(h, CMGAN_E_UNSUPPORTED, "cmgan_rir: a filter half-width of up to %d samples is supported (tw=%d)",
                    RR_MAX_TW, tw);
    if (Nx > RR_MAX_N || Ny > RR_MAX_N || Nz > RR_MAX_N)
        return fail(h, CMGAN_E_UNSUPPORTED, "cmgan_rir: image ranges of up to %d are supported (Nx=%d Ny=%d Nz=%d)",
                    RR_MAX_N, Nx, Ny, Nz);
    if (8LL * (2 * Nx + 1) * (2 * Ny + 1) * (2 * Nz + 1) >= (1LL << 31))
        return fail(h, CMGAN_E_UNSUPPORTED, "cmgan_rir: 8 (2Nx+1)(2Ny+1)(2Nz+1) must stay below 2^31 (Nx=%d Ny=%d Nz=%d)",
                    Nx, Ny, Nz);
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "cmgan_rir: null handle");
    if (int rc = check_ws(h, ws, ws_bytes, cmgan_rir_workspace_bytes(h, R, K, tw))) return rc;
    const LaunchCtx ctx = begin(h, stream);
    hipStream_t s = ctx.stream;
    RirArgs a;
    a.rooms = rooms;
    a.n_taps = n_taps;
    a.rir = rir;
    a.len = len;
    a.rec = (double*)ws;
    a.ld = ld;
    a.fs = (double)fs;
    a.c = c;
    a.R = R;
    a.K = K;
    a.tw = tw;
    a.Nx = Nx;
    a.Ny = Ny;
    a.Nz = Nz;
    const dim3 grid((K + RR_TILE - 1) / RR_TILE, R);
    LAUNCH(ctx, "rir_prep", rir_prep<<<R, RR_TPB, 0, s>>>(a));
    LAUNCH(ctx, "rir_taps", rir_taps<<<grid, RR_TPB, 0, s>>>(a));
    return check_launch(h, "rir");
}
