// dynamics.hip - a compressor / limiter / automatic gain control per row of a [B, L] float32 batch on the device
// (cmgan_dynamics, include/cmgan_hip.h).  The reference has no augmentation at all (src/data/dataloader.py:13-50 replays
// pairs mixed beforehand).  The processor is the feed-forward design in the log domain with the level detector after the
// gain computer and the smooth branching peak detector (Giannoulis, Massberg and Reiss, JAES 2012).  For row b with the
// table (thr, slope, knee, a_att, a_rel, makeup) = dyn[b], n = lengths[b] and the key row k (key's, else wav's):
//
//   xg   = 20 log10(max(|k_i|, 1e-6))                 (a key sample that is not finite: c_i = 0)
//   c_i  = 0                                          if 2 (xg - thr) < -knee
//        = slope t (t / (2 knee)), t = xg - thr + knee / 2   if 2 |xg - thr| <= knee and knee > 0
//        = slope (xg - thr)                           otherwise
//   y_i  = a_att y_(i-1) + (1 - a_att) c_i  if c_i > y_(i-1)  else  a_rel y_(i-1) + (1 - a_rel) c_i,    y_(-1) = 0
//   out_i = f32(wav_i 10^((makeup - y_i) / 20)) for i < n,  0 for n <= i < L
//
// The detector is no linear recurrence, but with a_att <= a_rel a step is y -> max(A_i(y), R_i(y)) of two increasing affine
// maps, A_i(y) = a_att y + (1 - a_att) c_i and R_i(y) = a_rel y + (1 - a_rel) c_i (A - R = (a_att - a_rel)(y - c): the branch
// takes the larger one).  With a_att > a_rel it takes the smaller one, which is the same statement about -y and -c; the
// scan then runs on negated values (sg = -1 below).  Increasing maps distribute over max, so T steps compose to
//   y -> max over k = 0 .. T of (a_att^k a_rel^(T-k) y + b_k):
// one offset per NUMBER k of attack steps, because all attack maps share one slope and all release maps the other.  The
// offsets follow from a (max, +) recurrence, b_k <- max(a_att b_(k-1) + (1 - a_att) c_i, a_rel b_k + (1 - a_rel) c_i),
// over the entries that i steps can reach (k <= i before step i).  Three launches, and a fourth for peak_reduction_db;
// float64 on the VALU, no atomics, no host synchronisation:
//   dynamics_tile   a wave owns a tile of DY_T = 64 samples, lane k holds b_k (b_64, which only the last step makes, is
//                   uniform).  A step is one neighbour-lane shift (DPP wave_shr:1, in registers), two fused multiply-adds
//                   and a max.  Writes the tile's DY_T + 1 offsets.  A row's last tile is left out: nothing follows it.
//   dynamics_fold   one wave per row walks the row's tiles in ascending order: y <- max_k (p_k y + b_k), one fused
//                   multiply-add per lane and a wave max (DPP inside a row of 16 lanes, four lane reads across the rows).
//                   A serial chain of n / DY_T steps per row; the offsets of the next DY_CHUNK tiles are loaded while it
//                   runs over the chunk before them.
//                   Writes every tile's entry state, and the row's status.
//   dynamics_apply  a wave owns DY_SPAN = 64 tiles of a row.  It computes c for its 4096 samples, a sample per lane, into
//                   LDS; then lane j runs tile j's 64 steps from the tile's entry state, in the branching form above,
//                   leaving y in LDS; then a sample per lane again: the gain, the product, one rounding, the store.
//   dynamics_peak   one wave per row: the maximum of the apply blocks' largest y.
// c_i is computed twice, by the same instructions on the same operands (contraction is off in dy_want), instead of being
// kept in the workspace.  A maximum does not depend on the order it is taken in, the fold's order is the tiles', and
// every kernel judges its row from the table alone: the same bits come out from run to run, and row b's bits depend
// neither on B, nor on the other rows, nor on the strides, nor on L beyond n.  They depend on DY_T: against the serial
// loop the entry states differ by float64 roundings.
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "api_internal.h"
#include "host_ranges.h"

namespace {

constexpr int DY_T = 64;                    // samples per tile: one offset per lane
constexpr int DY_ENT = DY_T + 1;            // offsets per tile, k = 0 .. DY_T attack steps
constexpr int DY_WAVES = 4;                 // tiles per block of dynamics_tile
constexpr int DY_CHUNK = 8;                 // tiles whose offsets dynamics_fold loads ahead of the chain
constexpr int DY_SPAN = 64;                 // tiles per block of dynamics_apply: one per lane
constexpr int DY_BLOCK = DY_SPAN * DY_T;    // samples per block of dynamics_apply
constexpr int DY_PITCH = DY_T + 1;          // LDS row pitch in float64: lanes walking their tiles hit different banks
constexpr int DY_MAX_L = 0x7fffffff - DY_BLOCK;   // a block's sample indices stay in an int
static_assert(DY_T == 64, "a tile is a wave");

struct DynArgs {
    const float* wav;
    const float* key;        // null: wav is its own key
    float* out;              // may be wav (in place)
    const int* lengths;      // null: every row has L samples
    const double* dyn;       // [B][6]
    int* status;             // [B] or null
    double* peak;            // [B] or null
    double* seg;             // workspace [B][nt][DY_ENT]: a tile's offsets
    double* inc;             // workspace [B][nt]: the detector's state before a tile's first sample
    double* part;            // workspace [B][nb]: the largest y of an apply block
    long long ldw, ldk, ldo;
    int B, L, nt, nb;
};

struct DynRow {
    double thr, slope, knee, a_att, a_rel, makeup;
    int n;                   // the row's samples; 0 for an invalid row
    bool ok;
};

__device__ inline bool dy_finite(double v) { return fabs(v) <= DBL_MAX; }

__device__ inline DynRow dy_row(const DynArgs& a, int b) {
    const double* d = a.dyn + (size_t)b * 6;
    DynRow r;
    r.thr = d[0], r.slope = d[1], r.knee = d[2], r.a_att = d[3], r.a_rel = d[4], r.makeup = d[5];
    r.n = a.lengths ? a.lengths[b] : a.L;
    r.ok = dy_finite(r.thr) && dy_finite(r.makeup) && r.slope >= 0.0 && r.slope <= 1.0 && r.knee >= 0.0 && dy_finite(r.knee) &&
           r.a_att >= 0.0 && r.a_att < 1.0 && r.a_rel >= 0.0 && r.a_rel < 1.0 && r.n >= 0 && r.n <= a.L;   // a NaN compares false
    if (!r.ok) r.n = 0;
    return r;
}

__device__ inline int dy_tiles(int n) { return (n + DY_T - 1) / DY_T; }

// the wanted reduction in dB, >= 0, for one key sample.  Both kernels that call it must get the same bits: no contraction.
__device__ inline double dy_want(const DynRow& r, float k) {
#pragma clang fp contract(off)
    const double m = fabs((double)k);
    if (!(m <= (double)FLT_MAX)) return 0.0;                           // not finite: silence
    const double d = 20.0 * log10(fmax(m, 1e-6)) - r.thr;
    if (2.0 * d < -r.knee) return 0.0;
    if (2.0 * fabs(d) <= r.knee && r.knee > 0.0) {
        const double t = d + 0.5 * r.knee;
        return r.slope * (t * (t / (2.0 * r.knee)));
    }
    return r.slope * d;
}

// v of the lane that a DPP control names; a lane without a source keeps its own
template <int CTRL>
__device__ inline double dy_dpp(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

constexpr int DPP_QUAD_XOR1 = 0xB1;         // quad_perm:[1,0,3,2]
constexpr int DPP_QUAD_XOR2 = 0x4E;         // quad_perm:[2,3,0,1]
constexpr int DPP_ROW_HALF_MIRROR = 0x141;  // lane i <- lane 7 - i of its 8
constexpr int DPP_ROW_MIRROR = 0x140;       // lane i <- lane 15 - i of its 16
constexpr int DPP_WAVE_SHR1 = 0x138;        // lane i <- lane i - 1 of the wave

// v of lane `src` (wave-uniform), in every lane
__device__ inline double dy_lane(double v, int src) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}

// the largest v of the wave, in every lane (no NaN comes here)
__device__ inline double dy_wave_max(double v) {
    v = fmax(v, dy_dpp<DPP_QUAD_XOR1>(v));
    v = fmax(v, dy_dpp<DPP_QUAD_XOR2>(v));
    v = fmax(v, dy_dpp<DPP_ROW_HALF_MIRROR>(v));
    v = fmax(v, dy_dpp<DPP_ROW_MIRROR>(v));
    return fmax(fmax(dy_lane(v, 0), dy_lane(v, 16)), fmax(dy_lane(v, 32), dy_lane(v, 48)));
}

// ------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(DY_WAVES * DY_T) void dynamics_tile(DynArgs a) {
    const int lane = threadIdx.x & (DY_T - 1), b = blockIdx.y;
    const int tile = blockIdx.x * DY_WAVES + (threadIdx.x >> 6);
    const DynRow r = dy_row(a, b);
    if (tile >= dy_tiles(r.n) - 1) return;                             // past the row's end, or its last tile (wave-uniform)
    const float* key = a.key ? a.key + (size_t)b * a.ldk : a.wav + (size_t)b * a.ldw;
    const double sg = r.a_att <= r.a_rel ? 1.0 : -1.0;
    const double c = sg * dy_want(r, key[(size_t)tile * DY_T + lane]);   // a whole tile in front of the row's end
    const double ca = (1.0 - r.a_att) * c, cr = (1.0 - r.a_rel) * c;
    // before step i the entries k <= i are real (entry 0 of the identity is 0); the others hold finite values that no
    // real entry reads
    double bk = 0.0, top = 0.0;
#pragma unroll 8
    for (int i = 0; i < DY_T; ++i) {
        const double cai = dy_lane(ca, i), cri = dy_lane(cr, i);
        if (i == DY_T - 1) top = fma(r.a_att, dy_lane(bk, DY_T - 1), cai);
        const double att = fma(r.a_att, dy_dpp<DPP_WAVE_SHR1>(bk), cai), rel = fma(r.a_rel, bk, cri);
        bk = lane == 0 ? rel : (lane == i + 1 ? att : fmax(att, rel));
    }
    double* seg = a.seg + ((size_t)b * a.nt + tile) * DY_ENT;
    seg[lane] = bk;
    if (lane == 0) seg[DY_T] = top;
}

__global__ __launch_bounds__(DY_T) void dynamics_fold(DynArgs a) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const DynRow r = dy_row(a, b);
    if (lane == 0 && a.status) a.status[b] = r.ok ? 0 : 1;
    const int ntr = dy_tiles(r.n);
    if (ntr == 0) return;
    // the slopes a_att^k a_rel^(DY_T - k) of the tile map, k = lane and k = DY_T
    double p = 1.0, ptop = 1.0;
    for (int i = 0; i < DY_T; ++i) {
        p *= i < lane ? r.a_att : r.a_rel;
        ptop *= r.a_att;
    }
    const double sg = r.a_att <= r.a_rel ? 1.0 : -1.0;
    const double* seg = a.seg + (size_t)b * a.nt * DY_ENT;
    double* inc = a.inc + (size_t)b * a.nt;
    double y = 0.0;                                                    // sg x the state before tile t
    // the offsets of a chunk are loaded while the chain runs over the chunk before it.  A tile without offsets (a row's
    // last, and what lies behind it) reads those of some tile inside the plane instead, and its step is not taken
    double bk[DY_CHUNK], bt[DY_CHUNK], nk[DY_CHUNK], nb[DY_CHUNK];
    auto load = [&](int t0, double (&k)[DY_CHUNK], double (&t)[DY_CHUNK]) {
#pragma unroll
        for (int q = 0; q < DY_CHUNK; ++q) {
            const size_t at = (size_t)(t0 + q < a.nt ? t0 + q : a.nt - 1) * DY_ENT;
            k[q] = seg[at + lane];
            t[q] = seg[at + DY_T];
        }
    };
    load(0, bk, bt);
    for (int t0 = 0; t0 < ntr; t0 += DY_CHUNK) {
        load(t0 + DY_CHUNK, nk, nb);
#pragma unroll
        for (int q = 0; q < DY_CHUNK; ++q) {
            const int t = t0 + q;
            if (lane == 0 && t < ntr) inc[t] = y == 0.0 ? 0.0 : sg * y;
            const double v = dy_wave_max(fmax(fma(p, y, bk[q]), fma(ptop, y, bt[q])));
            y = t < ntr - 1 ? v : y;
        }
#pragma unroll
        for (int q = 0; q < DY_CHUNK; ++q) bk[q] = nk[q], bt[q] = nb[q];
    }
}

__global__ __launch_bounds__(DY_T) void dynamics_apply(DynArgs a) {
    __shared__ double s_c[DY_SPAN * DY_PITCH];
    const int lane = threadIdx.x, b = blockIdx.y;
    const int i0 = blockIdx.x * DY_BLOCK;                              // < L <= DY_MAX_L
    const DynRow r = dy_row(a, b);
    float* out = a.out + (size_t)b * a.ldo;
    if (i0 >= r.n) {                                                   // an invalid row, or past the row's end: zeros
        for (int q = 0; q < DY_SPAN; ++q) {
            const int i = i0 + q * DY_T + lane;
            if (i < a.L) out[i] = 0.0f;
        }
        if (lane == 0) a.part[(size_t)b * a.nb + blockIdx.x] = 0.0;
        return;
    }
    const float* wav = a.wav + (size_t)b * a.ldw;
    const float* key = a.key ? a.key + (size_t)b * a.ldk : wav;
    for (int q = 0; q < DY_SPAN; ++q) {
        const int i = i0 + q * DY_T + lane;
        s_c[q * DY_PITCH + lane] = i < r.n ? dy_want(r, key[i]) : 0.0;
    }
    __syncthreads();
    // lane j walks tile j of the block from its entry state
    double pk = 0.0;
    const int first = i0 + lane * DY_T;
    if (first < r.n) {
        const int cnt = r.n - first < DY_T ? r.n - first : DY_T;
        const double oma = 1.0 - r.a_att, omr = 1.0 - r.a_rel;
        double y = a.inc[(size_t)b * a.nt + blockIdx.x * DY_SPAN + lane];
        double* s = s_c + lane * DY_PITCH;
#pragma unroll 8
        for (int i = 0; i < cnt; ++i) {
            const double c = s[i];
            y = c > y ? fma(r.a_att, y, oma * c) : fma(r.a_rel, y, omr * c);
            s[i] = y;
            pk = fmax(pk, y);
        }
    }
    __syncthreads();
    for (int q = 0; q < DY_SPAN; ++q) {
        const int i = i0 + q * DY_T + lane;
        if (i < r.n) {
            const double g = r.makeup - s_c[q * DY_PITCH + lane];
            const double gain = g == 0.0 ? 1.0 : exp10(g / 20.0);
            out[i] = (float)((double)wav[i] * gain);
        } else if (i < a.L) {
            out[i] = 0.0f;
        }
    }
    pk = dy_wave_max(pk);
    if (lane == 0) a.part[(size_t)b * a.nb + blockIdx.x] = pk;
}

__global__ __launch_bounds__(DY_T) void dynamics_peak(DynArgs a) {
    const int lane = threadIdx.x, b = blockIdx.x;
    double pk = 0.0;
    for (int k = lane; k < a.nb; k += DY_T) pk = fmax(pk, a.part[(size_t)b * a.nb + k]);
    pk = dy_wave_max(pk);
    if (lane == 0) a.peak[b] = pk;
}

struct DynLayout {
    size_t seg, inc, part, total;   // byte offsets: float64 [B][nt][65] | float64 [B][nt] | float64 [B][nb]
    int nt, nb;
};

inline DynLayout dy_layout(int B, int L) {
    DynLayout l;
    l.nt = (L + DY_T - 1) / DY_T;
    l.nb = (L + DY_BLOCK - 1) / DY_BLOCK;
    l.seg = 0;
    l.inc = l.seg + up256((size_t)B * l.nt * DY_ENT * sizeof(double));
    l.part = l.inc + up256((size_t)B * l.nt * sizeof(double));
    l.total = l.part + up256((size_t)B * l.nb * sizeof(double));
    return l;
}

inline bool dy_shape_ok(int B, int L) { return B >= 1 && B <= 65535 && L >= 1 && L <= DY_MAX_L; }

}  // namespace

extern "C" int cmgan_dynamics_tile(void) { return DY_T; }

extern "C" size_t cmgan_dynamics_workspace_bytes(int B, int L) { return dy_shape_ok(B, L) ? dy_layout(B, L).total : 0; }

extern "C" int cmgan_dynamics(cmgan_handle* h, const float* wav, int B, int L, long long ldw, const float* key, long long ldk,
                              const int* lengths, const double* dyn, float* out, long long ldo, int* status,
                              double* peak_reduction_db, void* ws, size_t ws_bytes, void* stream) {
    // every argument is judged before the handle is, so that the errors below need no GPU (the message of a call
    // without a handle is read with cmgan_last_error(NULL))
    if (!wav || !dyn || !out) return fail(h, CMGAN_E_BADARG, "cmgan_dynamics: null pointer");
    if (((uintptr_t)wav | (uintptr_t)key | (uintptr_t)out | (uintptr_t)lengths | (uintptr_t)status) & 3)
        return fail(h, CMGAN_E_BADARG, "cmgan_dynamics: float32 / int32 buffers must be 4-byte aligned");
    if (((uintptr_t)dyn | (uintptr_t)peak_reduction_db) & 7)
        return fail(h, CMGAN_E_BADARG, "cmgan_dynamics: float64 buffers must be 8-byte aligned");
    if (B < 1 || B > 65535 || L < 1 || ldw < L || ldo < L || (key && ldk < L))
        return fail(h, CMGAN_E_BADARG,
                    "cmgan_dynamics: need 1 <= B <= 65535, L >= 1, ldw >= L, ldo >= L, ldk >= L with a key (B=%d L=%d ldw=%lld "
                    "ldo=%lld ldk=%lld)", B, L, ldw, ldo, ldk);
    if (L > DY_MAX_L)
        return fail(h, CMGAN_E_BADARG, "cmgan_dynamics: rows of up to %d samples are supported (L=%d)", DY_MAX_L, L);
    if (!((const float*)out == wav && ldo == ldw) && rows_overlap(wav, ldw, out, ldo, B, L))   // in place is the one overlap there may be
        return fail(h, CMGAN_E_BADARG, "cmgan_dynamics: wav and out overlap; only out == wav with ldo == ldw (in place) is allowed");
    if (key && !((const float*)out == key && ldo == ldk) && rows_overlap(key, ldk, out, ldo, B, L))
        return fail(h, CMGAN_E_BADARG, "cmgan_dynamics: key and out overlap; only out == key with ldo == ldk is allowed");
    const DynLayout l = dy_layout(B, L);
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < l.total)
        return fail(h, CMGAN_E_BADARG, "cmgan_dynamics: the workspace must be 256-byte aligned and hold %zu bytes (%zu given)",
                    l.total, ws ? ws_bytes : (size_t)0);
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "cmgan_dynamics: null handle");
    const LaunchCtx ctx = begin(h, stream);
    hipStream_t s = ctx.stream;
    char* w = (char*)ws;
    DynArgs a;
    a.wav = wav;
    a.key = key;
    a.out = out;
    a.lengths = lengths;
    a.dyn = dyn;
    a.status = status;
    a.peak = peak_reduction_db;
    a.seg = (double*)(w + l.seg);
    a.inc = (double*)(w + l.inc);
    a.part = (double*)(w + l.part);
    a.ldw = ldw;
    a.ldk = key ? ldk : 0;
    a.ldo = ldo;
    a.B = B;
    a.L = L;
    a.nt = l.nt;
    a.nb = l.nb;
    LAUNCH(ctx, "dynamics_tile", dynamics_tile<<<dim3((l.nt + DY_WAVES - 1) / DY_WAVES, B), DY_WAVES * DY_T, 0, s>>>(a));
    LAUNCH(ctx, "dynamics_fold", dynamics_fold<<<B, DY_T, 0, s>>>(a));
    LAUNCH(ctx, "dynamics_apply", dynamics_apply<<<dim3(l.nb, B), DY_T, 0, s>>>(a));
    if (a.peak) LAUNCH(ctx, "dynamics_peak", dynamics_peak<<<B, DY_T, 0, s>>>(a));
    return check_launch(h, "dynamics");
}
