// rir.hip - room impulse responses of shoe-box rooms by the image-source method on the device (include/cmgan_hip.h):
// Allen & Berkley 1979 with Peterson's Hann-windowed sinc for the fractional delays, as cmgan_rir with one set of wall
// coefficients and as cmgan_rir_bands in NB frequency bands joined by a caller-supplied FIR filterbank.  The reference
// ships no impulse responses and no simulator (its data path replays pairs mixed beforehand, src/data/dataloader.py:13-50);
// this file makes the [R, Kmax] float32 bank + int32 lengths that cmgan_mix consumes.
//
//   row r: room L, source s, receiver m, k_r = clamp(n_taps[r], 1, K);  cmgan_rir: reflection coefficients b (wall at 0,
//          wall at L per axis);  cmgan_rir_bands: per band b six coefficients and the air attenuation m_b in Np/m, D = (NF - 1) / 2
//   image (n, p), |n_axis| <= N_axis, p in {0,1}^3:  offset_axis = (1 - 2 p) s + 2 n L - m, d = |offset|, tau = d fs / c
//   a = prod_axis b_axis0^|n - p| b_axis1^|n| / (4 pi max(d, CMGAN_RIR_DMIN)),  a_b the same with band b's walls times exp(-m_b d)
//   w(t) = (1 + cos(pi t / tw)) / 2 for |t| < tw, else 0
//   cmgan_rir:        h[k] = sum_images a w(k - tau) sinc(k - tau)
//   cmgan_rir_bands:  h_b[q] = sum_images a_b w(q - tau) sinc(q - tau), 0 <= q < k_r + D
//                     h[k] = sum_b sum_j g_b[j] h_b[k + D - j]   (b, then j ascending, one fma per term)
//   rir[r, k] = f32(h[k]) for k < k_r, 0 for k_r <= k < K;  len[r] = k_r
//
// Float64 throughout, one rounding to float32 at the store, no atomics.  A prep kernel (rir_prep, rir_bands_prep), one
// block per row, judges the row (a non-finite entry, a size <= 0, a coefficient outside [0, 1] or a negative m_b makes it
// invalid: zeros, len 1), writes len, and leaves in the workspace the row's record: its numbers, k_r (0 = invalid) and
// the powers b^e, e = 0 .. 256, of its coefficients (pow(), so 0^0 = 1).  A tap kernel then sums the images.
//
// THE ENUMERATION, once for both tap kernels (rr_tile, rr_column, rr_count, rr_scan, rr_list, rr_consume).  One block per
// (tile of RR_TILE taps, row), one thread per tap.  The images are visited in ONE fixed order - columns (nx, ny, p)
// ascending, nz ascending inside a column - in rounds of 256 columns, one per thread.  A thread solves the nz range whose
// delay can reach the tile's time shell tau in (k0 - tw, k_last + tw) (a superset: one index of margin on each side),
// counts the images that do reach it with the delay every later step uses, and an integer prefix sum over the block
// gives each image its place in the round's list: order-preserving compaction.  The list lives in LDS, RR_CAP entries at
// a time (a round with more is consumed in chunks); an entry is what depends on the image alone, t0 = k0 - tau first.
// Every thread then adds the list in list order; for tap k0 + j, t = j + t0, and entries outside |t| < tw are skipped, so
// an image that a larger N than needed adds changes no bit.  A thread fetches the t0 of RR_UNR entries at once, one LDS
// latency per group instead of one per entry (measured: a fifth to a quarter off the call).  A tap's sum
// is therefore in enumeration order whatever R, the other rows and the launch are: the same bits from run to run, row r
// independent of R.  Nothing read from a table becomes an address: list places come from counts, the nz bounds are
// clamped as doubles before they become ints, taps are written below K only, filter values are only ever multiplied.
//
// THE TWO ENTRY FORMS.  sin(pi t) = (-1)^j sin(pi t0) (one sin per image), and cos(pi (j + t0) / tw) by angle addition
// with the thread's own cos / sin(pi j / tw): no trigonometry per (image, tap); what is left is one division.
//   rir_taps            powers in LDS; entry t0, sin(pi t0) / pi, a / 2, (a / 2) cos(pi t0 / tw), (a / 2) sin(pi t0 / tw);
//                       a w(t) = a / 2 + cos(pi j / tw) (a / 2) cos(pi t0 / tw) - sin(pi j / tw) (a / 2) sin(pi t0 / tw)
//   rir_bands_taps<NB>  K + D taps, NB accumulators.  Eight bands of powers (96 KiB) do not fit beside the list in LDS:
//                       they stay in the workspace and are read, through the caches, while the list is built - four per
//                       (column, band), two per (image, band), never per tap.  Entry t0, sin(pi t0) / pi, cos(pi t0 / tw) / 2,
//                       sin(pi t0 / tw) / 2 and the NB amplitudes; v = w(t) sinc(t) once per entry, then a_b v to accumulator
//                       b.  The sums go to the workspace as float64 [R, NB, K + D]; only q < k_r + D is written or read.
//   rir_bands_join      one block per (tile of RR_TILE outputs, row): band after band it stages the span its outputs reach,
//                       RR_TILE + NF - 1 samples (zeros outside [0, k_r + D)), and the band's NF filter taps in LDS; every
//                       thread runs its double sum in the stated order into ONE accumulator, rounds once and writes the
//                       zeros beyond k_r.  Consecutive threads read consecutive float64, the filter tap is a broadcast.
//
// DIRECTIVITY (cmgan_rir_dir, cmgan_rir_bands_dir): first-order patterns at both ends, per band.  The gain of an image,
//   g_b = fma(1 - alpha_s,b, cos_s, alpha_s,b) fma(1 - alpha_m,b, cos_m, alpha_m,b),  cos_m = (o . v) / d,  cos_s = -(o . u_p) / d,
// with u_p the source's unit facing vector mirrored with the image ((1 - 2 p) u per axis) and v the receiver's, depends
// on the image and not on the tap: it is one more factor of the amplitude an entry already stores.  The tap kernels are
// templates on DIR; the DIR forms read the unit vectors and the alphas from a longer record (the prep kernels of the
// DIR calls judge and normalise the two tables), and their entry lambdas multiply g_b in.  The list layout, rr_consume
// and the DIR = false instantiations are what they were.  A pattern of all ones gives g_b = fma(0, cos, 1)^2 = 1.0
// exactly, so such a row has the bits of the plain call.
#include <math.h>
#include <stdint.h>

#include "api_internal.h"
#include "host_ranges.h"

namespace {

constexpr int RR_TPB = 256;                 // threads of every kernel
constexpr int RR_TILE = RR_TPB;             // taps per block of the tap kernels: one per thread
constexpr int RR_CAP = 512;                 // images per LDS list chunk
constexpr int RR_UNR = 8;                   // list entries whose t0 a thread fetches at once (RR_CAP is a multiple)
constexpr int RR_MAX_K = 65536;             // longest response (the limit of cmgan_mix)
constexpr int RR_MAX_N = 255;               // largest image index per axis
constexpr int RR_MAX_TW = 64;               // largest half-width of the fractional-delay filter
constexpr int RR_PW = RR_MAX_N + 2;         // powers b^0 .. b^(N + 1) of one coefficient
constexpr double RR_PI = 3.14159265358979323846;
constexpr int RB_MAX_BANDS = 8;
constexpr int RB_MAX_FILTER = 1023;
constexpr int RB_SPAN = RR_TILE + RB_MAX_FILTER - 1;
// a row's record in the workspace, float64 words: the room's numbers, k_r at RR_KR, then the powers
constexpr int RR_KR = 15;
constexpr int RR_HEAD = 16;                 // cmgan_rir: 15 room numbers, k_r
constexpr int RB_AIR = 16;
constexpr int RB_HEAD = 24;                 // cmgan_rir_bands: 9 room numbers, (unused), k_r, m_b at RB_AIR .. 23
constexpr int RR_REC = RR_HEAD + 6 * RR_PW;
__host__ __device__ inline size_t rb_rec(int NB) { return (size_t)RB_HEAD + (size_t)6 * NB * RR_PW; }
// the records of the directional calls are longer: behind the powers the unit vectors u, v and (alpha_s, alpha_m) per band
constexpr int RD_ALPHA = 6;
constexpr double RD_MAX_COMPONENT = 1.0e100;   // of a facing vector: its square stays finite
__host__ __device__ inline size_t rd_words(int NB) { return (size_t)RD_ALPHA + (size_t)2 * NB; }
template <bool DIR>
__host__ __device__ inline size_t rr_rec_words() { return (size_t)RR_REC + (DIR ? rd_words(1) : 0); }
template <bool DIR>
__host__ __device__ inline size_t rb_rec_words(int NB) { return rb_rec(NB) + (DIR ? rd_words(NB) : 0); }

// Between the 8-byte LDS stores of a list entry: merged into one 16-byte store (ds_write2_b64), the later data dwords are
// still being read by the LDS path when the next VALU instruction overwrites them (tools/isa_lint.py).
#define RB_KEEP_APART() asm volatile("" ::: "memory")

struct RirArgs {
    const double* rooms;
    const int* n_taps;
    float* rir;
    int* len;
    double* rec;             // workspace: [R][RR_REC] or [R][rb_rec(NB)]
    long long ld;
    double fs, c;
    int R, K, tw, Nx, Ny, Nz;
};

struct BandArgs : RirArgs {
    const double* bands;     // [R][NB][7]
    const double* filt;      // [NB][NF]
    double* hb;              // workspace: [R][NB][K + D]
    int NB, NF;
};

struct DirArgs {             // the prep kernels of the directional calls only: the tap kernels read the record
    const double* orient;    // [R][6]
    const double* pattern;   // [R][NB][2]
};

// ---------------------------------------------------------------- the prep kernels
__device__ inline bool rr_finite(double v) { return v - v == 0.0; }
__device__ inline int rr_clamp_taps(int n_taps, int K, bool ok) { return !ok || n_taps < 1 ? 1 : (n_taps > K ? K : n_taps); }

// columns 0 - 8 of a room: all finite, the sizes positive
__device__ inline bool rr_geometry_ok(const double* room) {
    bool ok = true;
    for (int i = 0; i < 9; ++i) ok = ok && rr_finite(room[i]) && (i >= 3 || room[i] > 0.0);
    return ok;
}

// pw[w][e] = coef(w)^e for e = 0 .. RR_PW - 1 (zeros for an invalid row), the block's threads over all (w, e)
template <class Coef>
__device__ inline void rr_powers(double* pw, int ncoef, bool ok, Coef coef) {
    for (int i = threadIdx.x; i < ncoef * RR_PW; i += RR_TPB) {
        const int w = i / RR_PW, e = i - w * RR_PW;
        pw[i] = ok ? pow(coef(w), (double)e) : 0.0;
    }
}

// Row r of the two tables of a directional call, judged (a non-finite entry, an alpha outside [0, 1], a component beyond
// RD_MAX_COMPONENT, a zero vector at an end that has some alpha < 1); `out` gets the unit vectors u, v (zeros for a zero
// vector: every alpha of that end is then 1 and the cosine is multiplied by 0) and the nb (alpha_s, alpha_m) pairs.
__device__ inline bool rd_prep(const DirArgs& d, int r, int nb, double* out) {
    const int t = threadIdx.x;
    const double* o = d.orient + (size_t)r * 6;
    const double* p = d.pattern + (size_t)r * nb * 2;
    bool ok = true, aimed_s = false, aimed_m = false;
    for (int i = 0; i < 6; ++i) ok = ok && rr_finite(o[i]) && fabs(o[i]) <= RD_MAX_COMPONENT;
    for (int i = 0; i < 2 * nb; ++i) {
        ok = ok && p[i] >= 0.0 && p[i] <= 1.0;                    // (a NaN fails both)
        if (i & 1) aimed_m = aimed_m || p[i] < 1.0;
        else aimed_s = aimed_s || p[i] < 1.0;
    }
    const double nu = sqrt(fma(o[2], o[2], fma(o[1], o[1], o[0] * o[0])));
    const double nv = sqrt(fma(o[5], o[5], fma(o[4], o[4], o[3] * o[3])));
    ok = ok && (!aimed_s || nu > 0.0) && (!aimed_m || nv > 0.0);
    if (t < RD_ALPHA) {
        const double n = t < 3 ? nu : nv;
        out[t] = (ok && n > 0.0) ? o[t] / n : 0.0;
    } else if (t < RD_ALPHA + 2 * nb) {
        out[t] = ok ? p[t - RD_ALPHA] : 1.0;
    }
    return ok;
}

// `ok`: what the caller has judged of the row already; `rec` the row's record
__device__ inline void rir_prep_row(const RirArgs& a, double* rec, bool ok) {
    const int t = threadIdx.x, r = blockIdx.x;
    const double* room = a.rooms + (size_t)r * 15;
    ok = ok && rr_geometry_ok(room);
    for (int i = 9; i < 15; ++i) ok = ok && rr_finite(room[i]) && room[i] >= 0.0 && room[i] <= 1.0;
    const int kr = rr_clamp_taps(a.n_taps[r], a.K, ok);
    if (t < 15) rec[t] = room[t];
    if (t == RR_KR) rec[RR_KR] = ok ? (double)kr : 0.0;
    if (t == 0) a.len[r] = kr;
    rr_powers(rec + RR_HEAD, 6, ok, [&](int w) { return room[9 + w]; });
}

__global__ __launch_bounds__(RR_TPB) void rir_prep(RirArgs a) {
    const int r = blockIdx.x;
    rir_prep_row(a, a.rec + (size_t)r * rr_rec_words<false>(), true);
}

__global__ __launch_bounds__(RR_TPB) void rir_dir_prep(RirArgs a, DirArgs d) {
    const int r = blockIdx.x;
    double* rec = a.rec + (size_t)r * rr_rec_words<true>();
    rir_prep_row(a, rec, rd_prep(d, r, 1, rec + RR_REC));
}

__device__ inline void rir_bands_prep_row(const BandArgs& a, double* rec, bool ok) {
    const int t = threadIdx.x, r = blockIdx.x;
    const double* room = a.rooms + (size_t)r * 15;
    const double* band = a.bands + (size_t)r * a.NB * 7;
    ok = ok && rr_geometry_ok(room);
    for (int i = 0; i < a.NB * 7; ++i) ok = ok && rr_finite(band[i]) && band[i] >= 0.0 && (i % 7 == 6 || band[i] <= 1.0);
    const int kr = rr_clamp_taps(a.n_taps[r], a.K, ok);
    if (t < 9) rec[t] = room[t];
    if (t >= 9 && t < RR_KR) rec[t] = 0.0;
    if (t == RR_KR) rec[RR_KR] = ok ? (double)kr : 0.0;
    if (t >= RB_AIR && t < RB_HEAD) rec[t] = (ok && t - RB_AIR < a.NB) ? band[(t - RB_AIR) * 7 + 6] : 0.0;
    if (t == 0) a.len[r] = kr;
    rr_powers(rec + RB_HEAD, 6 * a.NB, ok, [&](int w) { return band[w / 6 * 7 + w % 6]; });      // w = 6 b + wall
}

__global__ __launch_bounds__(RR_TPB) void rir_bands_prep(BandArgs a) {
    const int r = blockIdx.x;
    rir_bands_prep_row(a, a.rec + (size_t)r * rb_rec_words<false>(a.NB), true);
}

__global__ __launch_bounds__(RR_TPB) void rir_bands_dir_prep(BandArgs a, DirArgs d) {
    const int r = blockIdx.x;
    double* rec = a.rec + (size_t)r * rb_rec_words<true>(a.NB);
    rir_bands_prep_row(a, rec, rd_prep(d, r, a.NB, rec + rb_rec(a.NB)));
}

// ---------------------------------------------------------------- the enumeration
// the tile's shell and the room's geometry
struct RrTile {
    double Lx, Ly, Lz, sx, sy, sz, mx, my, mz;
    double t_lo, t_hi;       // an image reaches the tile iff t_lo < tau < t_hi
    double d_lo2, d_hi2;     // the same shell in metres squared, a little wider than exact, for the nz range solve only
    double spm;              // samples per metre: tau = d * spm everywhere
    double inv_2lz;          // (range solve only)
    int Nx, Ny, Nz, wy, ncols;
};

// `rec` is the row's record, [k0, k_last] the tile's taps
__device__ inline RrTile rr_tile(const RirArgs& a, const double* rec, int k0, int k_last) {
    RrTile g;
    g.Lx = rec[0], g.Ly = rec[1], g.Lz = rec[2], g.sx = rec[3], g.sy = rec[4], g.sz = rec[5], g.mx = rec[6], g.my = rec[7], g.mz = rec[8];
    g.t_lo = (double)(k0 - a.tw), g.t_hi = (double)(k_last + a.tw);
    const double d_hi = g.t_hi * a.c / a.fs * (1.0 + 1e-12);
    const double d_lo = g.t_lo > 0.0 ? g.t_lo * a.c / a.fs * (1.0 - 1e-12) : 0.0;
    g.d_hi2 = d_hi * d_hi, g.d_lo2 = d_lo * d_lo;
    g.spm = a.fs / a.c, g.inv_2lz = 0.5 / g.Lz;
    g.Nx = a.Nx, g.Ny = a.Ny, g.Nz = a.Nz;
    g.wy = 2 * a.Ny + 1, g.ncols = (2 * a.Nx + 1) * g.wy * 8;
    return g;
}

// a double bound of an nz range as an int in [-Nz - 1, Nz + 1] (NaN included: fmax / fmin drop it)
__device__ inline int rr_bound(double v, int Nz) { return (int)fmin(fmax(v, (double)(-Nz - 1)), (double)(Nz + 1)); }

// a column (nx, ny, p): its nz candidates [lo1, hi1] then [lo2, hi2] (ascending, disjoint; n1 in the first, ncand in
// all), dx^2 + dy^2, the z offset of nz = 0, and the places w RR_PW + exponent of its four x / y powers in a [6][RR_PW]
// table (exponents <= N + 1 < RR_PW: indices, not table values).  A column past the last has no candidates and places 0.
// A directional column (RrColumn<true>) also carries px, py, dx and dy - the mirror signs and the offset; the plain one
// is the struct it was.
template <bool DIR>
struct RrAim {};
template <>
struct RrAim<true> {
    int px, py;
    double dx, dy;
};
template <bool DIR>
struct RrColumn : RrAim<DIR> {
    int lo1, lo2, n1, ncand, pz, ax, bx, ay, by;
    double q, zo;
};

template <bool DIR>
__device__ inline RrColumn<DIR> rr_column(const RrTile& g, int col) {
    RrColumn<DIR> c = {};
    int hi1 = -1, hi2 = -1;
    if (col < g.ncols) {
        const int p = col & 7, xy = col >> 3;
        const int ix = xy / g.wy, iy = xy - ix * g.wy;
        const int nx = ix - g.Nx, ny = iy - g.Ny;
        const int px = p >> 2, py = (p >> 1) & 1;
        c.pz = p & 1;
        const double dx = fma((double)(2 * nx), g.Lx, (px ? -g.sx : g.sx) - g.mx);
        const double dy = fma((double)(2 * ny), g.Ly, (py ? -g.sy : g.sy) - g.my);
        if constexpr (DIR) c.px = px, c.py = py, c.dx = dx, c.dy = dy;
        c.q = fma(dy, dy, dx * dx);
        c.zo = (c.pz ? -g.sz : g.sz) - g.mz;
        c.ax = 0 * RR_PW + abs(nx - px), c.bx = 1 * RR_PW + abs(nx), c.ay = 2 * RR_PW + abs(ny - py), c.by = 3 * RR_PW + abs(ny);
        const double B = g.d_hi2 - c.q;
        if (B > 0.0) {
            const double z_hi = sqrt(B), A = g.d_lo2 - c.q;
            const double z_lo = A > 0.0 ? sqrt(A) : 0.0;
            // dz = zo + 2 nz Lz in [-z_hi, -z_lo] or [z_lo, z_hi], one index of margin on each side
            int nl = rr_bound(ceil((-z_hi - c.zo) * g.inv_2lz), g.Nz) - 1, nh = rr_bound(floor((-z_lo - c.zo) * g.inv_2lz), g.Nz) + 1;
            int pl = rr_bound(ceil((z_lo - c.zo) * g.inv_2lz), g.Nz) - 1, ph = rr_bound(floor((z_hi - c.zo) * g.inv_2lz), g.Nz) + 1;
            nl = max(nl, -g.Nz), pl = max(pl, -g.Nz);
            nh = min(nh, g.Nz), ph = min(ph, g.Nz);
            if (nh >= pl - 1) {                                   // the two ranges meet: one range
                c.lo1 = min(nl, pl);
                hi1 = max(ph, nh);
            } else {
                c.lo1 = nl; hi1 = nh; c.lo2 = pl; hi2 = ph;
            }
        }
    }
    c.n1 = hi1 >= c.lo1 ? hi1 - c.lo1 + 1 : 0;
    c.ncand = c.n1 + (hi2 >= c.lo2 ? hi2 - c.lo2 + 1 : 0);
    return c;
}

// candidate i of a column: its nz, its distance, and whether its delay reaches the tile
template <class Column>
__device__ inline int rr_nz(const Column& c, int i) { return i < c.n1 ? c.lo1 + i : c.lo2 + (i - c.n1); }
__device__ inline bool rr_reaches(const RrTile& g, double tau) { return tau > g.t_lo && tau < g.t_hi; }
template <class Column>
__device__ inline double rr_distance(const RrTile& g, const Column& c, int nz) {
    const double dz = fma((double)(2 * nz), g.Lz, c.zo);
    return sqrt(fma(dz, dz, c.q));
}

// the candidates that reach the tile, with the delay the entries are made from
template <class Column>
__device__ inline int rr_count(const RrTile& g, const Column& c) {
    int cnt = 0;
    for (int i = 0; i < c.ncand; ++i) cnt += rr_reaches(g, rr_distance(g, c, rr_nz(c, i)) * g.spm) ? 1 : 0;
    return cnt;
}

// exclusive prefix sum of one int per thread in thread order; `total` is the block's sum
__device__ inline int rr_scan(int v, int (*s)[RR_TPB], int& total) {
    const int t = threadIdx.x;
    int cur = 0;
    s[0][t] = v;
    __syncthreads();
    for (int off = 1; off < RR_TPB; off <<= 1) {
        int x = s[cur][t];
        if (t >= off) x += s[cur][t - off];
        s[cur ^ 1][t] = x;
        cur ^= 1;
        __syncthreads();
    }
    total = s[cur][RR_TPB - 1];
    const int incl = s[cur][t];
    __syncthreads();
    return incl - v;
}

// The round's list, RR_CAP entries at a time: this thread's `cnt` images take the places base .. base + cnt - 1 of `total`.
// entry(e, nz, d, tau) writes entry e of the chunk (s_t0[e] = k0 - tau among it); consume(n), called by the whole
// block between two barriers, adds the chunk's n entries to the taps.
template <class Column, class Entry, class Consume>
__device__ inline void rr_list(const RrTile& g, const Column& c, int cnt, int base, int total, double* s_t0, Entry entry,
                               Consume consume) {
    int cursor = 0, pos = base;
    for (int cs = 0; cs < total; cs += RR_CAP) {
        const int end = cs + RR_CAP;
        while (cursor < c.ncand && pos < end && pos < base + cnt) {
            const int nz = rr_nz(c, cursor);
            ++cursor;
            const double d = rr_distance(g, c, nz);
            const double tau = d * g.spm;
            if (!rr_reaches(g, tau)) continue;
            const int e = pos - cs;                               // >= 0: a chunk is filled before the next begins
            ++pos;
            entry(e, nz, d, tau);
        }
        const int n = total - cs < RR_CAP ? total - cs : RR_CAP;
        if (threadIdx.x < RR_UNR) s_t0[n + threadIdx.x] = 1.0e300;      // the tail of the last group of RR_UNR: in no window
        __syncthreads();
        consume(n);
        __syncthreads();
    }
}

// tap(i, t) for every entry i < n whose t = jd + t0 lies inside the window, in list order.  The call's time is this loop's,
// and it moves by a per cent or two with where the loop falls in memory.  The directive pads the code in front of the
// loop's entry to a 64-byte line, so the loop's place no longer depends on the size of what precedes it (with today's
// block layout its first block begins at byte 4 of a line; nothing but that layout ties the two).
template <class Tap>
__device__ inline void rr_consume(const double* s_t0, int n, double jd, double twd, Tap tap) {
    asm volatile(".p2align 6");
    for (int i = 0; i < n; i += RR_UNR) {
        double tt[RR_UNR];
#pragma unroll
        for (int u = 0; u < RR_UNR; ++u) tt[u] = jd + s_t0[i + u];         // one LDS latency for the group
#pragma unroll
        for (int u = 0; u < RR_UNR; ++u)
            if (fabs(tt[u]) < twd) tap(i + u, tt[u]);
    }
}

// ---------------------------------------------------------------- directivity: what an entry lambda of a DIR form adds
// the unit facing vectors of the row, from the words `w` of its record (uniform over the block)
struct RrFacing {
    double ux, uy, uz, vx, vy, vz;
};
__device__ inline RrFacing rr_facing(const double* w) { return RrFacing{w[0], w[1], w[2], w[3], w[4], w[5]}; }

// The cosines of image nz of the column at distance d: between the source image's mirrored facing vector and the ray to
// the receiver, and between the receiver's vector and the ray back to the image.  dz is rr_distance's; both 0 at d == 0.
// One reciprocal of d serves both (measured: a per cent off the single-band call against two divisions).
__device__ inline void rr_cosines(const RrFacing& f, const RrTile& g, const RrColumn<true>& c, int nz, double d, double& cos_s,
                                  double& cos_m) {
    const double dz = fma((double)(2 * nz), g.Lz, c.zo);
    const double om = fma(dz, f.vz, fma(c.dy, f.vy, c.dx * f.vx));
    const double os = fma(dz, c.pz ? -f.uz : f.uz, fma(c.dy, c.py ? -f.uy : f.uy, c.dx * (c.px ? -f.ux : f.ux)));
    const double rd = d > 0.0 ? 1.0 / d : 0.0;
    cos_m = om * rd;
    cos_s = -os * rd;
}

// signed: the rear lobe of a pattern with alpha < 1/2 is negative
__device__ inline double rr_gain(double alpha_s, double alpha_m, double cos_s, double cos_m) {
    return fma(1.0 - alpha_s, cos_s, alpha_s) * fma(1.0 - alpha_m, cos_m, alpha_m);
}

// ---------------------------------------------------------------- cmgan_rir's tap kernel
template <bool DIR>
__global__ __launch_bounds__(RR_TPB) void rir_taps(RirArgs a) {
    __shared__ double s_pw[6 * RR_PW];
    __shared__ double s_t0[RR_CAP + RR_UNR], s_sp[RR_CAP], s_ha[RR_CAP], s_hc[RR_CAP], s_hs[RR_CAP];
    __shared__ int s_scan[2][RR_TPB];
    const int t = threadIdx.x, r = blockIdx.y;
    const int k0 = blockIdx.x * RR_TILE, k = k0 + t;
    const double* rec = a.rec + (size_t)r * rr_rec_words<DIR>();
    float* out = a.rir + (size_t)r * a.ld;
    const int kr = (int)rec[RR_KR];                              // 0: an invalid row
    if (k0 >= kr) {                                              // (the whole block: nothing of this tile is a tap)
        if (k < a.K) out[k] = 0.f;
        return;
    }
    for (int i = t; i < 6 * RR_PW; i += RR_TPB) s_pw[i] = rec[RR_HEAD + i];
    const RrTile g = rr_tile(a, rec, k0, (k0 + RR_TILE < kr ? k0 + RR_TILE : kr) - 1);
    const RrFacing f = DIR ? rr_facing(rec + RR_REC) : RrFacing{};
    const double alpha_s = DIR ? rec[RR_REC + RD_ALPHA] : 1.0, alpha_m = DIR ? rec[RR_REC + RD_ALPHA + 1] : 1.0;
    __syncthreads();
    // this thread's tap: j = t
    const double twd = (double)a.tw, jd = (double)t;
    const double cj = cospi(jd / twd), sj = sinpi(jd / twd);
    double acc = 0.0;

    for (int c0 = 0; c0 < g.ncols; c0 += RR_TPB) {
        const RrColumn<DIR> c = rr_column<DIR>(g, c0 + t);
        const double cxy = s_pw[c.ax] * s_pw[c.bx] * s_pw[c.ay] * s_pw[c.by];
        const int cnt = rr_count(g, c);
        int total;
        const int base = rr_scan(cnt, s_scan, total);
        rr_list(g, c, cnt, base, total, s_t0,
                [=](int e, int nz, double d, double tau) {
                    const int ez = nz - c.pz;
                    double amp = cxy * s_pw[4 * RR_PW + (ez < 0 ? -ez : ez)] * s_pw[5 * RR_PW + (nz < 0 ? -nz : nz)]
                               / (4.0 * RR_PI * fmax(d, CMGAN_RIR_DMIN));
                    if constexpr (DIR) {
                        double cos_s, cos_m;
                        rr_cosines(f, g, c, nz, d, cos_s, cos_m);
                        amp *= rr_gain(alpha_s, alpha_m, cos_s, cos_m);
                    }
                    const double t0 = (double)k0 - tau, ha = 0.5 * amp, ang = t0 / twd;
                    s_t0[e] = t0;
                    s_sp[e] = sinpi(t0) / RR_PI;
                    s_ha[e] = ha;
                    s_hc[e] = ha * cospi(ang);
                    s_hs[e] = ha * sinpi(ang);
                },
                [=, &acc](int n) {
                    if (k < kr)
                        rr_consume(s_t0, n, jd, twd, [=, &acc](int i, double tt) {
                            const double sgn = (t & 1) ? -1.0 : 1.0;
                            const double wa = s_ha[i] + (cj * s_hc[i] - sj * s_hs[i]);
                            const double sc = tt == 0.0 ? 1.0 : sgn * s_sp[i] / tt;
                            acc = fma(wa, sc, acc);
                        });
                });
    }
    if (k < a.K) out[k] = k < kr ? (float)acc : 0.f;
}

// ---------------------------------------------------------------- cmgan_rir_bands' tap and join kernels
template <int NB, bool DIR>
__global__ __launch_bounds__(RR_TPB) void rir_bands_taps(BandArgs a) {
    __shared__ double s_t0[RR_CAP + RR_UNR], s_sp[RR_CAP], s_hc[RR_CAP], s_hs[RR_CAP];
    __shared__ double s_amp[NB][RR_CAP];
    __shared__ int s_scan[2][RR_TPB];
    const int t = threadIdx.x, r = blockIdx.y;
    const int k0 = blockIdx.x * RR_TILE, k = k0 + t;
    const int D = (a.NF - 1) / 2, KD = a.K + D;
    const double* rec = a.rec + (size_t)r * rb_rec_words<DIR>(NB);
    const double* pw = rec + RB_HEAD;                            // [NB][6][RR_PW]
    const double* facing = rec + rb_rec(NB);                     // (DIR) u, v, then [NB][2] alphas, read per image like the powers
    const int kr = (int)rec[RR_KR];                              // 0: an invalid row
    const int kq = kr > 0 ? kr + D : 0;                          // the band responses hold taps [0, kq)
    if (k0 >= kq) return;                                        // (the whole block; nothing from kq on is ever read)
    const RrTile g = rr_tile(a, rec, k0, (k0 + RR_TILE < kq ? k0 + RR_TILE : kq) - 1);
    const RrFacing f = DIR ? rr_facing(facing) : RrFacing{};
    double air[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) air[b] = rec[RB_AIR + b];
    // this thread's tap: j = t
    const double twd = (double)a.tw, jd = (double)t;
    const double cj = cospi(jd / twd), sj = sinpi(jd / twd);
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;

    for (int c0 = 0; c0 < g.ncols; c0 += RR_TPB) {
        const RrColumn<DIR> c = rr_column<DIR>(g, c0 + t);
        const int cnt = rr_count(g, c);
        int total;
        const int base = rr_scan(cnt, s_scan, total);
        double cxy[NB];                                          // the column's x / y factor per band
        if (cnt > 0) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const double* pb = pw + (size_t)b * 6 * RR_PW;
                cxy[b] = pb[c.ax] * pb[c.bx] * pb[c.ay] * pb[c.by];
            }
        } else {
#pragma unroll
            for (int b = 0; b < NB; ++b) cxy[b] = 0.0;
        }
        rr_list(g, c, cnt, base, total, s_t0,
                [=](int e, int nz, double d, double tau) {
                    const int ez = nz - c.pz;
                    const int az = ez < 0 ? -ez : ez, bz = nz < 0 ? -nz : nz;
                    const double spread = 4.0 * RR_PI * fmax(d, CMGAN_RIR_DMIN);
                    double cos_s = 0.0, cos_m = 0.0;
                    if constexpr (DIR) rr_cosines(f, g, c, nz, d, cos_s, cos_m);
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        const double* pb = pw + (size_t)b * 6 * RR_PW;
                        const double att = air[b] == 0.0 ? 1.0 : exp(-air[b] * d);
                        double amp = cxy[b] * pb[4 * RR_PW + az] * pb[5 * RR_PW + bz] * att / spread;
                        if constexpr (DIR) amp *= rr_gain(facing[RD_ALPHA + 2 * b], facing[RD_ALPHA + 2 * b + 1], cos_s, cos_m);
                        s_amp[b][e] = amp;
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
                },
                [=, &acc](int n) {
                    if (k < kq)
                        rr_consume(s_t0, n, jd, twd, [=, &acc](int i, double tt) {
                            const double sgn = (t & 1) ? -1.0 : 1.0;
                            const double w = 0.5 + (cj * s_hc[i] - sj * s_hs[i]);
                            const double sc = tt == 0.0 ? 1.0 : sgn * s_sp[i] / tt;
                            const double v = w * sc;
#pragma unroll
                            for (int b = 0; b < NB; ++b) acc[b] = fma(s_amp[b][i], v, acc[b]);
                        });
                });
    }
    if (k < kq) {
        double* hb = a.hb + (size_t)r * NB * KD;
#pragma unroll
        for (int b = 0; b < NB; ++b) hb[(size_t)b * KD + k] = acc[b];
    }
}

template <bool DIR>                                              // (the record's length is all that differs)
__global__ __launch_bounds__(RR_TPB) void rir_bands_join(BandArgs a) {
    __shared__ double s_h[RB_SPAN], s_g[RB_MAX_FILTER];
    const int t = threadIdx.x, r = blockIdx.y;
    const int k0 = blockIdx.x * RR_TILE, k = k0 + t;
    const int NF = a.NF, D = (NF - 1) / 2, KD = a.K + D;
    const int kr = (int)a.rec[(size_t)r * rb_rec_words<DIR>(a.NB) + RR_KR];   // 0: an invalid row
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

// ---------------------------------------------------------------- the host side
inline bool rr_shape_ok(int R, int K, int tw) {
    return R >= 1 && R <= 65535 && K >= 1 && K <= RR_MAX_K && tw >= 1 && tw <= RR_MAX_TW;
}

inline bool rb_shape_ok(int R, int K, int tw, int NB, int NF) {
    return rr_shape_ok(R, K, tw) && NB >= 1 && NB <= RB_MAX_BANDS && NF >= 1 && NF <= RB_MAX_FILTER && (NF & 1);
}

template <bool DIR>
inline size_t rr_rec_bytes(int R) { return up256((size_t)R * rr_rec_words<DIR>() * sizeof(double)); }
template <bool DIR>
inline size_t rb_rec_bytes(int R, int NB) { return up256((size_t)R * rb_rec_words<DIR>(NB) * sizeof(double)); }
inline size_t rb_hb_bytes(int R, int K, int NB, int NF) {
    return up256((size_t)R * NB * (size_t)(K + (NF - 1) / 2) * sizeof(double));
}

// Judges every argument but the workspace and fills `a`; `bt` is null for cmgan_rir and holds bands, filt, NB and NF for
// cmgan_rir_bands (it may be the object `a` is the base of: only the base is assigned, after the last read of `bt`); `dt`
// is null for the plain calls and holds the two tables of a directional one.  The handle is judged last: the errors
// before it need no GPU (without a handle the message is cmgan_last_error(NULL)'s).
int rr_judge(cmgan_handle* h, const char* name, const BandArgs* bt, const DirArgs* dt, const double* rooms, const int* n_taps,
             int R, int K, int fs, double c, int tw, int Nx, int Ny, int Nz, float* rir, long long ld, int* len, void* ws,
             RirArgs& a) {
    if (!rooms || !n_taps || !rir || !len || (bt && (!bt->bands || !bt->filt)) || (dt && (!dt->orient || !dt->pattern)))
        return fail(h, CMGAN_E_BADARG, "%s: null pointer", name);
    if (((uintptr_t)rooms | (bt ? (uintptr_t)bt->bands | (uintptr_t)bt->filt : 0)) & 7)
        return fail(h, CMGAN_E_BADARG, "%s: the float64 %s must be 8-byte aligned", name,
                    bt ? "room, band and filter tables" : "room table");
    if (dt && (((uintptr_t)dt->orient | (uintptr_t)dt->pattern) & 7))
        return fail(h, CMGAN_E_BADARG, "%s: the float64 orient and pattern tables must be 8-byte aligned", name);
    if (((uintptr_t)n_taps | (uintptr_t)rir | (uintptr_t)len) & 3)
        return fail(h, CMGAN_E_BADARG, "%s: float32 / int32 buffers must be 4-byte aligned", name);
    if (R < 1 || R > 65535 || K < 1 || ld < K)
        return fail(h, CMGAN_E_BADARG, "%s: need 1 <= R <= 65535, K >= 1, ld >= K (R=%d K=%d ld=%lld)", name, R, K, ld);
    if (bt && (bt->NB < 1 || bt->NB > RB_MAX_BANDS))
        return fail(h, CMGAN_E_BADARG, "%s: need 1 <= NB <= %d bands (NB=%d)", name, RB_MAX_BANDS, bt->NB);
    if (bt && (bt->NF < 1 || !(bt->NF & 1)))
        return fail(h, CMGAN_E_BADARG, "%s: the filter length must be odd and >= 1 (NF=%d)", name, bt->NF);
    if (fs < 1) return fail(h, CMGAN_E_BADARG, "%s: fs must be positive (fs=%d)", name, fs);
    if (!(c > 0.0) || !(c <= 1.0e300))
        return fail(h, CMGAN_E_BADARG, "%s: the speed of sound c must be positive and finite (%g)", name, c);
    if (tw < 1) return fail(h, CMGAN_E_BADARG, "%s: tw must be >= 1 (tw=%d)", name, tw);
    if (Nx < 0 || Ny < 0 || Nz < 0)
        return fail(h, CMGAN_E_BADARG, "%s: image ranges must be >= 0 (Nx=%d Ny=%d Nz=%d)", name, Nx, Ny, Nz);
    if (K > RR_MAX_K)
        return fail(h, CMGAN_E_UNSUPPORTED, "%s: responses of up to %d taps are supported (K=%d)", name, RR_MAX_K, K);
    if (bt && bt->NF > RB_MAX_FILTER)
        return fail(h, CMGAN_E_UNSUPPORTED, "%s: filters of up to %d taps are supported (NF=%d)", name, RB_MAX_FILTER, bt->NF);
    if (tw > RR_MAX_TW)
        return fail(h, CMGAN_E_UNSUPPORTED, "%s: a filter half-width of up to %d samples is supported (tw=%d)", name,
                    RR_MAX_TW, tw);
    if (Nx > RR_MAX_N || Ny > RR_MAX_N || Nz > RR_MAX_N)
        return fail(h, CMGAN_E_UNSUPPORTED, "%s: image ranges of up to %d are supported (Nx=%d Ny=%d Nz=%d)", name, RR_MAX_N,
                    Nx, Ny, Nz);
    if (8LL * (2 * Nx + 1) * (2 * Ny + 1) * (2 * Nz + 1) >= (1LL << 31))
        return fail(h, CMGAN_E_UNSUPPORTED, "%s: 8 (2Nx+1)(2Ny+1)(2Nz+1) must stay below 2^31 (Nx=%d Ny=%d Nz=%d)", name, Nx,
                    Ny, Nz);
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "%s: null handle", name);
    a = RirArgs{rooms, n_taps, rir, len, (double*)ws, ld, (double)fs, c, R, K, tw, Nx, Ny, Nz};
    return CMGAN_OK;
}

// the workspace of the two call families: the records, and for the banded ones the band responses behind them
template <bool DIR>
inline size_t rr_ws_bytes(int R, int K, int tw) { return rr_shape_ok(R, K, tw) ? rr_rec_bytes<DIR>(R) : 0; }
template <bool DIR>
inline size_t rb_ws_bytes(int R, int K, int tw, int NB, int NF) {
    return rb_shape_ok(R, K, tw, NB, NF) ? rb_rec_bytes<DIR>(R, NB) + rb_hb_bytes(R, K, NB, NF) : 0;
}

// cmgan_rir (`dt` null) and cmgan_rir_dir: the same judgement, the same grid; the prep kernel and the record differ
template <bool DIR>
int rr_run(cmgan_handle* h, const char* name, const DirArgs* dt, const double* rooms, const int* n_taps, int R, int K, int fs,
           double c, int tw, int Nx, int Ny, int Nz, float* rir, long long ld, int* len, void* ws, size_t ws_bytes, void* stream) {
    RirArgs a;
    if (int rc = rr_judge(h, name, nullptr, dt, rooms, n_taps, R, K, fs, c, tw, Nx, Ny, Nz, rir, ld, len, ws, a)) return rc;
    if (int rc = check_ws(h, ws, ws_bytes, rr_ws_bytes<DIR>(R, K, tw))) return rc;
    const LaunchCtx ctx = begin(h, stream);
    hipStream_t s = ctx.stream;
    const dim3 grid((K + RR_TILE - 1) / RR_TILE, R);
    if constexpr (DIR) LAUNCH(ctx, "rir_dir_prep", rir_dir_prep<<<R, RR_TPB, 0, s>>>(a, *dt));
    else LAUNCH(ctx, "rir_prep", rir_prep<<<R, RR_TPB, 0, s>>>(a));
    LAUNCH(ctx, DIR ? "rir_dir_taps" : "rir_taps", rir_taps<DIR><<<grid, RR_TPB, 0, s>>>(a));
    return check_launch(h, "rir");
}

template <bool DIR>
int rb_run(cmgan_handle* h, const char* name, const DirArgs* dt, const double* rooms, const double* bands, const int* n_taps,
           int R, int K, int NB, const double* filt, int NF, int fs, double c, int tw, int Nx, int Ny, int Nz, float* rir,
           long long ld, int* len, void* ws, size_t ws_bytes, void* stream) {
    BandArgs a;
    a.bands = bands, a.filt = filt;
    a.NB = NB, a.NF = NF;
    if (int rc = rr_judge(h, name, &a, dt, rooms, n_taps, R, K, fs, c, tw, Nx, Ny, Nz, rir, ld, len, ws, a)) return rc;
    if (int rc = check_ws(h, ws, ws_bytes, rb_ws_bytes<DIR>(R, K, tw, NB, NF))) return rc;
    const LaunchCtx ctx = begin(h, stream);
    hipStream_t s = ctx.stream;
    a.hb = (double*)((char*)ws + rb_rec_bytes<DIR>(R, NB));
    const dim3 grid_taps((K + (NF - 1) / 2 + RR_TILE - 1) / RR_TILE, R), grid_join((K + RR_TILE - 1) / RR_TILE, R);
    if constexpr (DIR) LAUNCH(ctx, "rir_bands_dir_prep", rir_bands_dir_prep<<<R, RR_TPB, 0, s>>>(a, *dt));
    else LAUNCH(ctx, "rir_bands_prep", rir_bands_prep<<<R, RR_TPB, 0, s>>>(a));
    void (*const taps[RB_MAX_BANDS])(BandArgs) = {rir_bands_taps<1, DIR>, rir_bands_taps<2, DIR>, rir_bands_taps<3, DIR>,
                                                  rir_bands_taps<4, DIR>, rir_bands_taps<5, DIR>, rir_bands_taps<6, DIR>,
                                                  rir_bands_taps<7, DIR>, rir_bands_taps<8, DIR>};
    LAUNCH(ctx, DIR ? "rir_bands_dir_taps" : "rir_bands_taps", taps[NB - 1]<<<grid_taps, RR_TPB, 0, s>>>(a));
    LAUNCH(ctx, "rir_bands_join", rir_bands_join<DIR><<<grid_join, RR_TPB, 0, s>>>(a));
    return check_launch(h, "rir_bands");
}

}  // namespace

extern "C" int cmgan_rir_tile(void) { return RR_TILE; }
extern "C" int cmgan_rir_list_capacity(void) { return RR_CAP; }
extern "C" int cmgan_rir_max_bands(void) { return RB_MAX_BANDS; }
extern "C" int cmgan_rir_max_filter(void) { return RB_MAX_FILTER; }

extern "C" size_t cmgan_rir_workspace_bytes(const cmgan_handle*, int R, int K, int tw) { return rr_ws_bytes<false>(R, K, tw); }
extern "C" size_t cmgan_rir_dir_workspace_bytes(const cmgan_handle*, int R, int K, int tw) { return rr_ws_bytes<true>(R, K, tw); }

extern "C" size_t cmgan_rir_bands_workspace_bytes(const cmgan_handle*, int R, int K, int tw, int NB, int NF) {
    return rb_ws_bytes<false>(R, K, tw, NB, NF);
}

extern "C" size_t cmgan_rir_bands_dir_workspace_bytes(const cmgan_handle*, int R, int K, int tw, int NB, int NF) {
    return rb_ws_bytes<true>(R, K, tw, NB, NF);
}

extern "C" int cmgan_rir(cmgan_handle* h, const double* rooms, const int* n_taps, int R, int K, int fs, double c, int tw,
                         int Nx, int Ny, int Nz, float* rir, long long ld, int* len, void* ws, size_t ws_bytes,
                         void* stream) {
    return rr_run<false>(h, "cmgan_rir", nullptr, rooms, n_taps, R, K, fs, c, tw, Nx, Ny, Nz, rir, ld, len, ws, ws_bytes, stream);
}

extern "C" int cmgan_rir_dir(cmgan_handle* h, const double* rooms, const double* orient, const double* pattern,
                             const int* n_taps, int R, int K, int fs, double c, int tw, int Nx, int Ny, int Nz, float* rir,
                             long long ld, int* len, void* ws, size_t ws_bytes, void* stream) {
    const DirArgs dt{orient, pattern};
    return rr_run<true>(h, "cmgan_rir_dir", &dt, rooms, n_taps, R, K, fs, c, tw, Nx, Ny, Nz, rir, ld, len, ws, ws_bytes, stream);
}

extern "C" int cmgan_rir_bands(cmgan_handle* h, const double* rooms, const double* bands, const int* n_taps, int R, int K,
                               int NB, const double* filt, int NF, int fs, double c, int tw, int Nx, int Ny, int Nz,
                               float* rir, long long ld, int* len, void* ws, size_t ws_bytes, void* stream) {
    return rb_run<false>(h, "cmgan_rir_bands", nullptr, rooms, bands, n_taps, R, K, NB, filt, NF, fs, c, tw, Nx, Ny, Nz, rir, ld,
                         len, ws, ws_bytes, stream);
}

extern "C" int cmgan_rir_bands_dir(cmgan_handle* h, const double* rooms, const double* bands, const double* orient,
                                   const double* pattern, const int* n_taps, int R, int K, int NB, const double* filt, int NF,
                                   int fs, double c, int tw, int Nx, int Ny, int Nz, float* rir, long long ld, int* len,
                                   void* ws, size_t ws_bytes, void* stream) {
    const DirArgs dt{orient, pattern};
    return rb_run<true>(h, "cmgan_rir_bands_dir", &dt, rooms, bands, n_taps, R, K, NB, filt, NF, fs, c, tw, Nx, Ny, Nz, rir, ld,
                        len, ws, ws_bytes, stream);
}
