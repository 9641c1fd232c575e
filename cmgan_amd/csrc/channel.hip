// channel.hip - the recording channel of a [B, L] float32 batch on the device (cmgan_channel, include/cmgan_hip.h): per
// row a cascade of up to 8 biquads (equaliser, microphone response, band limit) and a clipping level.  The reference
// has no augmentation at all (src/data/dataloader.py:13-50 replays pairs mixed beforehand).  For row b with
// n = clamp(lengths[b], 0, L), m = n_sections[b] and sections (b0 b1 b2 1 a1 a2), applied in order from zero state:
//
//   y_i = b0 u_i + z1,   z1 <- b1 u_i - a1 y_i + z2,   z2 <- b2 u_i - a2 y_i          (transposed direct form II, float64)
//   out_i = f32(min(max(y_i, -clip[b]), clip[b])) for i < n,  0 for n <= i < L
//
// A cascade is one linear system with the 2 m states (z1, z2 of every section) as its vector z: a segment of k samples
// run from zero state, ending in Z, acts on an incoming state as z' = A^k z + Z, where A is the system's matrix for zero
// input - block lower-triangular, a section's own block [[-a1, 1], [-a2, 0]], and below it the section's input as its
// predecessors' z1 make it.  Four launches, float64 on the VALU, no atomics, no host synchronisation:
//   channel_prepare  one block per row: judges the row (status), builds A and writes A^(CH_RUN 2^k), k = 0..7, and
//                    A^(CH_TILE 2^k), k = 0..8, to the workspace by repeated squaring.  An element's sum runs over the
//                    block columns between its own column and row only, in ascending order, so it does not depend on
//                    how many sections the batch is padded to.
//   channel_scan     a block owns a tile of CH_TILE samples of one row, a thread CH_RUN consecutive ones.  Each thread
//                    runs its samples through the row's m sections from zero state, the 256 end states are combined by
//                    an inclusive scan through LDS (mat-vecs by the tabulated powers), and the block writes the tile's
//                    end state.  Samples at i >= n are never read; they count as zeros.
//   channel_fold     one block per row: the same scan over the tiles' end states, 256 tiles at a time in ascending
//                    order, gives every tile its incoming state.
//   channel_apply    per tile: a thread's entry state is the tile's incoming state taken through its t runs (A^(CH_RUN t)
//                    composed from the table by the binary digits of t) plus the in-tile scan; then its samples in
//                    sequence, the clip, one rounding to float32 and the store.
// The kernels are templates on the padded section count SP in {1, 2, 4, 8}: the state vector is a register array with
// compile-time indices.  Sections m .. SP - 1 of a row keep the state 0 and are never run; their rows and columns of
// every matrix are exact zeros, and every sum stops at its own row's block.  So every float64 reduction runs in an order
// that depends on the tile grid alone: a row's bits depend neither on B, nor on the other rows, nor on L beyond n, nor
// on S beyond the row's own m.
#include <math.h>
#include <stdint.h>

#include "api_internal.h"
#include "host_ranges.h"

namespace {

constexpr int CH_TPB = 256;                 // threads of every kernel here
constexpr int CH_RUN_LOG2 = 3;
constexpr int CH_RUN = 1 << CH_RUN_LOG2;    // consecutive samples per thread
constexpr int CH_TILE = CH_TPB * CH_RUN;    // samples per block
constexpr int CH_MAX_S = 8;                 // sections per row
constexpr int CH_MAX_L = 0x7fffffff - CH_TILE;   // a tile's sample indices stay in an int
constexpr int CH_NPOW = 17;                 // A^(CH_RUN 2^k), k = 0..7, then A^(CH_TILE 2^k), k = 0..8
constexpr int CH_PT = 8;                    // the first of the tile powers
static_assert(CH_TPB == 256, "the scans take eight steps");
constexpr double CH_DBL_MAX = 1.79769313486231570815e308;

struct ChannelArgs {
    const float* x;
    float* y;                // may be x (in place)
    const int* lengths;      // null: every row has L samples
    const double* sos;       // [B][S][6]
    const int* n_sections;   // null: S for every row
    const double* clip;      // null: no clipping
    int* status;             // [B] or null
    int* sections;           // workspace [B]: the row's m, -1 for an invalid row
    double* pw;              // workspace [B][CH_NPOW][N][N], N = 2 SP
    double* seg;             // workspace [B][nt][N]: a tile's end state from zero state ...
    double* inc;             // ... and the state before its first sample
    long long ldx, ldy;
    int B, L, nt, S;
};

__device__ inline int ch_rows_n(const ChannelArgs& a, int b) {
    if (!a.lengths) return a.L;
    const int n = a.lengths[b];
    return n < 0 ? 0 : (n > a.L ? a.L : n);
}

__device__ inline bool ch_finite(double v) { return fabs(v) <= CH_DBL_MAX; }

// ------------------------------------------------------------------------------------------ prepare
// One block per row.  Thread (i, j) = (t / 16, t % 16) owns element (i, j) of every matrix.
__global__ __launch_bounds__(CH_TPB) void channel_prepare(ChannelArgs a, int N) {
    __shared__ double s_m[2][16][16];
    __shared__ int s_sections;
    const int t = threadIdx.x, b = blockIdx.x;
    const int i = t >> 4, j = t & 15;
    const double* sos = a.sos + (size_t)b * a.S * 6;
    s_m[0][i][j] = 0.0;
    __syncthreads();
    if (t == 0) {
        int m = a.n_sections ? a.n_sections[b] : a.S;
        bool ok = m >= 0 && m <= a.S;
        if (a.clip) ok = ok && a.clip[b] > 0.0;                              // a NaN compares false
        for (int s = 0; ok && s < m; ++s) {
            const double* c = sos + s * 6;
            for (int q = 0; q < 6; ++q) ok = ok && ch_finite(c[q]);
            ok = ok && c[3] == 1.0 && fabs(c[5]) < 1.0 && fabs(c[4]) < 1.0 + c[5];
        }
        if (!ok) m = -1;
        // A for zero input: w[q] = what z1 of section q adds to the input of section s
        double w[CH_MAX_S];
        for (int s = 0; s < m; ++s) {
            const double* c = sos + s * 6;
            const double b0 = c[0], b1 = c[1], b2 = c[2], a1 = c[4], a2 = c[5];
            const double c1 = b1 - a1 * b0, c2 = b2 - a2 * b0;                 // u enters z1' and z2' also through y
            for (int q = 0; q < s; ++q) {
                s_m[0][2 * s][2 * q] = c1 * w[q];
                s_m[0][2 * s + 1][2 * q] = c2 * w[q];
                w[q] *= b0;
            }
            w[s] = 1.0;
            s_m[0][2 * s][2 * s] = -a1;
            s_m[0][2 * s][2 * s + 1] = 1.0;
            s_m[0][2 * s + 1][2 * s] = -a2;
        }
        s_sections = m;
        a.sections[b] = m;
        if (a.status) a.status[b] = m < 0 ? 1 : 0;
    }
    __syncthreads();
    if (s_sections < 0) return;
    // A^(2^q) by squaring; element (i, j) is a sum over the columns k of its own block row and the rows of its own block
    // column: k = (j & ~1) .. (i | 1), zero above the block diagonal
    double* pw = a.pw + (size_t)b * CH_NPOW * N * N;
    const bool mine = i < N && j <= (i | 1);
    int cur = 0;
    for (int q = 1; q < CH_RUN_LOG2 + CH_NPOW; ++q) {
        double acc = 0.0;
        if (mine)
            for (int k = j & ~1; k <= (i | 1); ++k) acc = fma(s_m[cur][i][k], s_m[cur][k][j], acc);
        s_m[cur ^ 1][i][j] = acc;
        cur ^= 1;
        if (q >= CH_RUN_LOG2 && i < N && j < N) pw[(size_t)(q - CH_RUN_LOG2) * N * N + i * N + j] = acc;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------ the pieces of scan / apply
// z <- P z + add, for the sections s < m alone (the others keep exact zeros); row i sums its columns 0 .. i | 1 in
// ascending order.  P is one [N][N] matrix of the table, the same for the whole block.
template <int SP>
__device__ inline void ch_matvec(const double* __restrict__ P, int m, const double (&v)[2 * SP], double (&z)[2 * SP]) {
    constexpr int N = 2 * SP;
#pragma unroll
    for (int s = 0; s < SP; ++s) {
        if (s < m) {
            double r0 = z[2 * s], r1 = z[2 * s + 1];
#pragma unroll
            for (int j = 0; j < 2 * s + 2; ++j) {
                r0 = fma(P[(2 * s) * N + j], v[j], r0);
                r1 = fma(P[(2 * s + 1) * N + j], v[j], r1);
            }
            z[2 * s] = r0;
            z[2 * s + 1] = r1;
        }
    }
}

// Inclusive scan of 256 segments, thread t holding the end state of segment t from zero state.  Before the step with
// offset 2^k the segments of threads t >= 2^k cover 2^k units, so the step composes with P[k] = A^(unit 2^k).
template <int SP>
__device__ inline void ch_scan(const double* __restrict__ P, int m, double (&z)[2 * SP], double* s_v) {
    constexpr int N = 2 * SP;
    const int t = threadIdx.x;
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {
        const int s = 1 << k;
#pragma unroll
        for (int i = 0; i < N; ++i) s_v[i * CH_TPB + t] = z[i];
        __syncthreads();
        if (t >= s) {
            double v[N];
#pragma unroll
            for (int i = 0; i < N; ++i) v[i] = s_v[i * CH_TPB + t - s];
            ch_matvec<SP>(P + (size_t)k * N * N, m, v, z);
        }
        __syncthreads();
    }
}

// z <- A^(unit d) z with the factor composed from P[k] = A^(unit 2^k) by the binary digits of d, lowest first
template <int SP>
__device__ inline void ch_advance(const double* __restrict__ P, int m, int d, int digits, double (&z)[2 * SP]) {
    constexpr int N = 2 * SP;
#pragma unroll 1
    for (int k = 0; k < digits; ++k) {
        if ((d >> k) & 1) {
            double v[N];
#pragma unroll
            for (int i = 0; i < N; ++i) {
                v[i] = z[i];
                z[i] = 0.0;
            }
            ch_matvec<SP>(P + (size_t)k * N * N, m, v, z);
        }
    }
}

// the thread's CH_RUN samples of the tile (zeros from the row's end on)
__device__ inline void ch_load(const ChannelArgs& a, int b, int n, double (&ax)[CH_RUN]) {
    const int i0 = blockIdx.x * CH_TILE + threadIdx.x * CH_RUN;
    const float* row = a.x + (size_t)b * a.ldx;
#pragma unroll
    for (int r = 0; r < CH_RUN; ++r) ax[r] = i0 + r < n ? (double)row[i0 + r] : 0.0;
}

// The samples through the row's m sections in sequence, from state z; ax becomes the cascade's output.  Section by
// section over the run: the same operations on the same operands as sample by sample.
template <int SP>
__device__ inline void ch_run(const double* __restrict__ sos, int m, double (&ax)[CH_RUN], double (&z)[2 * SP]) {
#pragma unroll
    for (int s = 0; s < SP; ++s) {
        if (s < m) {
            const double b0 = sos[s * 6], b1 = sos[s * 6 + 1], b2 = sos[s * 6 + 2], a1 = sos[s * 6 + 4], a2 = sos[s * 6 + 5];
            double z1 = z[2 * s], z2 = z[2 * s + 1];
#pragma unroll
            for (int r = 0; r < CH_RUN; ++r) {
                const double u = ax[r];
                const double y = fma(b0, u, z1);
                z1 = fma(b1, u, fma(-a1, y, z2));
                z2 = fma(b2, u, -a2 * y);
                ax[r] = y;
            }
            z[2 * s] = z1;
            z[2 * s + 1] = z2;
        }
    }
}

// ------------------------------------------------------------------------------------------ kernels
template <int SP>
__global__ __launch_bounds__(CH_TPB) void channel_scan(ChannelArgs a) {
    constexpr int N = 2 * SP;
    __shared__ double s_v[N * CH_TPB];
    const int t = threadIdx.x, b = blockIdx.y;
    const int n = ch_rows_n(a, b), m = a.sections[b];
    double* seg = a.seg + ((size_t)b * a.nt + blockIdx.x) * N;
    if (m <= 0 || (long long)blockIdx.x * CH_TILE >= n) {              // invalid, a plain copy, or past the row's end
        if (t < N) seg[t] = 0.0;
        return;
    }
    double ax[CH_RUN], z[N];
#pragma unroll
    for (int i = 0; i < N; ++i) z[i] = 0.0;
    ch_load(a, b, n, ax);
    ch_run<SP>(a.sos + (size_t)b * a.S * 6, m, ax, z);
    ch_scan<SP>(a.pw + (size_t)b * CH_NPOW * N * N, m, z, s_v);
    if (t == CH_TPB - 1) {
#pragma unroll
        for (int i = 0; i < N; ++i) seg[i] = z[i];
    }
}

template <int SP>
__global__ __launch_bounds__(CH_TPB) void channel_fold(ChannelArgs a) {
    constexpr int N = 2 * SP;
    __shared__ double s_v[N * CH_TPB];
    const int t = threadIdx.x, b = blockIdx.x;
    const int m = a.sections[b];
    if (m <= 0) return;                                                // nothing carries a state
    const double* P = a.pw + ((size_t)b * CH_NPOW + CH_PT) * N * N;
    const size_t e0 = (size_t)b * a.nt;
    double c[N];                                                       // the state before the chunk's first tile
#pragma unroll
    for (int i = 0; i < N; ++i) c[i] = 0.0;
    for (int k0 = 0; k0 < a.nt; k0 += CH_TPB) {
        const int k = k0 + t;
        double z[N];
#pragma unroll
        for (int i = 0; i < N; ++i) z[i] = k < a.nt ? a.seg[(e0 + k) * N + i] : 0.0;
        ch_scan<SP>(P, m, z, s_v);
        // the state after tile k: the chunk's incoming state through the t + 1 tiles up to it
        double f[N];
#pragma unroll
        for (int i = 0; i < N; ++i) f[i] = c[i];
        ch_advance<SP>(P, m, t + 1, 9, f);
#pragma unroll
        for (int i = 0; i < N; ++i) f[i] += z[i];
        // all sums first: a paired LDS store must not be followed at once by a VALU write to its data registers
        // (tools/isa_lint.py), which is how the compiler schedules "store f[i] + z[i]" in a loop
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < N; ++i) s_v[i * CH_TPB + t] = f[i];
        __syncthreads();
        if (k < a.nt) {
#pragma unroll
            for (int i = 0; i < N; ++i) a.inc[(e0 + k) * N + i] = t ? s_v[i * CH_TPB + t - 1] : c[i];
        }
#pragma unroll
        for (int i = 0; i < N; ++i) c[i] = s_v[i * CH_TPB + CH_TPB - 1];
        __syncthreads();
    }
}

template <int SP>
__global__ __launch_bounds__(CH_TPB) void channel_apply(ChannelArgs a) {
    constexpr int N = 2 * SP;
    __shared__ double s_v[N * CH_TPB];
    const int t = threadIdx.x, b = blockIdx.y;
    const int n = ch_rows_n(a, b), m = a.sections[b];
    const int i0 = blockIdx.x * CH_TILE + t * CH_RUN;
    float* out = a.y + (size_t)b * a.ldy;
    if (m < 0 || (long long)blockIdx.x * CH_TILE >= n) {               // an invalid row, or past the row's end: zeros
#pragma unroll
        for (int r = 0; r < CH_RUN; ++r)
            if (i0 + r < a.L) out[i0 + r] = 0.0f;
        return;
    }
    double ax[CH_RUN];
    ch_load(a, b, n, ax);
    if (m > 0) {
        const double* sos = a.sos + (size_t)b * a.S * 6;
        const double* P = a.pw + (size_t)b * CH_NPOW * N * N;
        double u[CH_RUN], z[N];
#pragma unroll
        for (int r = 0; r < CH_RUN; ++r) u[r] = ax[r];
#pragma unroll
        for (int i = 0; i < N; ++i) z[i] = 0.0;
        ch_run<SP>(sos, m, u, z);
        ch_scan<SP>(P, m, z, s_v);
#pragma unroll
        for (int i = 0; i < N; ++i) s_v[i * CH_TPB + t] = z[i];
        __syncthreads();
        // entry state: the tile's incoming state through the t runs before this one, plus what those runs made from zero
        const double* inc = a.inc + ((size_t)b * a.nt + blockIdx.x) * N;
#pragma unroll
        for (int i = 0; i < N; ++i) z[i] = inc[i];
        ch_advance<SP>(P, m, t, 8, z);
        if (t) {
#pragma unroll
            for (int i = 0; i < N; ++i) z[i] += s_v[i * CH_TPB + t - 1];
        }
        ch_run<SP>(sos, m, ax, z);
    }
    const double lim = a.clip ? a.clip[b] : (double)INFINITY;
#pragma unroll
    for (int r = 0; r < CH_RUN; ++r) {
        double v = ax[r];
        v = v > lim ? lim : (v < -lim ? -lim : v);                      // a NaN stays one
        if (i0 + r < a.L) out[i0 + r] = i0 + r < n ? (float)v : 0.0f;
    }
}

inline int ch_tiles(int L) { return (L + CH_TILE - 1) / CH_TILE; }

inline int ch_padded(int S) { return S <= 1 ? 1 : (S <= 2 ? 2 : (S <= 4 ? 4 : 8)); }

struct ChannelLayout {
    size_t sections, pw, seg, inc, total;   // byte offsets: int32 [B] | float64 [B][17][N][N] | float64 [B][nt][N] twice
};

inline ChannelLayout ch_layout(int B, int L, int S) {
    const size_t N = 2 * (size_t)ch_padded(S);
    ChannelLayout l;
    l.sections = 0;
    l.pw = up256((size_t)B * sizeof(int));
    l.seg = l.pw + up256((size_t)B * CH_NPOW * N * N * sizeof(double));
    l.inc = l.seg + up256((size_t)B * ch_tiles(L) * N * sizeof(double));
    l.total = l.inc + up256((size_t)B * ch_tiles(L) * N * sizeof(double));
    return l;
}

inline bool ch_shape_ok(int B, int L, int S) { return B >= 1 && B <= 65535 && L >= 1 && L <= CH_MAX_L && S >= 1 && S <= CH_MAX_S; }

template <int SP>
void ch_launch(const LaunchCtx& ctx, const ChannelArgs& a) {
    hipStream_t s = ctx.stream;
    const dim3 grid(a.nt, a.B);
    LAUNCH(ctx, "channel_prepare", channel_prepare<<<a.B, CH_TPB, 0, s>>>(a, 2 * SP));
    LAUNCH(ctx, "channel_scan", channel_scan<SP><<<grid, CH_TPB, 0, s>>>(a));
    LAUNCH(ctx, "channel_fold", channel_fold<SP><<<a.B, CH_TPB, 0, s>>>(a));
    LAUNCH(ctx, "channel_apply", channel_apply<SP><<<grid, CH_TPB, 0, s>>>(a));
}

}  // namespace

extern "C" int cmgan_channel_tile(void) { return CH_TILE; }

extern "C" int cmgan_channel_max_sections(void) { return CH_MAX_S; }

extern "C" size_t cmgan_channel_workspace_bytes(int B, int L, int S) { return ch_shape_ok(B, L, S) ? ch_layout(B, L, S).total : 0; }

extern "C" int cmgan_channel(cmgan_handle* h, const float* x, int B, int L, long long ldx, const int* lengths, const double* sos,
                             const int* n_sections, int S, const double* clip, float* y, long long ldy, int* status, void* ws,
                             size_t ws_bytes, void* stream) {
    // every argument is judged before the handle is, so that the errors below need no GPU (the message of a call
    // without a handle is read with cmgan_last_error(NULL))
    if (!x || !sos || !y) return fail(h, CMGAN_E_BADARG, "cmgan_channel: null pointer");
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)lengths | (uintptr_t)n_sections | (uintptr_t)status) & 3)
        return fail(h, CMGAN_E_BADARG, "cmgan_channel: float32 / int32 buffers must be 4-byte aligned");
    if (((uintptr_t)sos | (uintptr_t)clip) & 7)
        return fail(h, CMGAN_E_BADARG, "cmgan_channel: float64 buffers must be 8-byte aligned");
    if (B < 1 || B > 65535 || L < 1 || ldx < L || ldy < L)
        return fail(h, CMGAN_E_BADARG, "cmgan_channel: need 1 <= B <= 65535, L >= 1, ldx >= L, ldy >= L (B=%d L=%d ldx=%lld ldy=%lld)",
                    B, L, ldx, ldy);
    if (L > CH_MAX_L)
        return fail(h, CMGAN_E_BADARG, "cmgan_channel: rows of up to %d samples are supported (L=%d)", CH_MAX_L, L);
    if (S < 1 || S > CH_MAX_S)
        return fail(h, CMGAN_E_BADARG, "cmgan_channel: S must lie in [1, %d] (S=%d)", CH_MAX_S, S);
    if (!((const float*)y == x && ldy == ldx)) {                       // in place is the one overlap there may be
        const uintptr_t x0 = (uintptr_t)x, x1 = x0 + ((size_t)(B - 1) * (size_t)ldx + (size_t)L) * sizeof(float);
        const uintptr_t y0 = (uintptr_t)y, y1 = y0 + ((size_t)(B - 1) * (size_t)ldy + (size_t)L) * sizeof(float);
        if (x0 < y1 && y0 < x1)
            return fail(h, CMGAN_E_BADARG, "cmgan_channel: x and y overlap; only y == x with ldy == ldx (in place) is allowed");
    }
    const ChannelLayout l = ch_layout(B, L, S);
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < l.total)
        return fail(h, CMGAN_E_BADARG, "cmgan_channel: the workspace must be 256-byte aligned and hold %zu bytes (%zu given)",
                    l.total, ws ? ws_bytes : (size_t)0);
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "cmgan_channel: null handle");
    const LaunchCtx ctx = begin(h, stream);
    char* w = (char*)ws;
    ChannelArgs a;
    a.x = x;
    a.y = y;
    a.lengths = lengths;
    a.sos = sos;
    a.n_sections = n_sections;
    a.clip = clip;
    a.status = status;
    a.sections = (int*)(w + l.sections);
    a.pw = (double*)(w + l.pw);
    a.seg = (double*)(w + l.seg);
    a.inc = (double*)(w + l.inc);
    a.ldx = ldx;
    a.ldy = ldy;
    a.B = B;
    a.L = L;
    a.nt = ch_tiles(L);
    a.S = S;
    switch (ch_padded(S)) {
        case 1: ch_launch<1>(ctx, a); break;
        case 2: ch_launch<2>(ctx, a); break;
        case 4: ch_launch<4>(ctx, a); break;
        default: ch_launch<8>(ctx, a); break;
    }
    return check_launch(h, "channel");
}
