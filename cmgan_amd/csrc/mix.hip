// mix.hip - dynamic mixing of a [B, L] float32 batch of clean speech into (noisy, target) training pairs on the device
// (cmgan_mix, include/cmgan_hip.h).  The reference only replays pairs somebody mixed before (src/data/dataloader.py:13-50
// reads clean/x.wav and noisy/x.wav); its --cut_len help names "denoise and dereverberation" as the task.
//
//   h = rir[rir_index[b], 0:K], K = rir_len[b], d = first argmax |h|        (no bank: h = [1], d = 0)
//   speech[i] = sum_{k < K} h[k] clean[b, i + d - k]                         clean = 0 outside [0, L)
//   target    = clean (early == -1) or the same sum over the taps k <= d + early
//   n[i]      = bank[noise_start[b] + (noise_off[b] + i) mod noise_len[b]]
//   Ps = mean(speech^2), Pn = mean(n^2), g = sqrt(Ps / (Pn 10^(snr_db / 10)))      (g = 0 when Ps == 0 or Pn == 0)
//   v = speech + g n, m = max |v|, s = m > peak ? peak / m : 1
//   noisy = f32(v s), target = f32(target s)                                  (s == 1, early == -1: target is clean's bits)
//
// Float32 samples in and out; every product and sum in float64 on the VALU, one rounding to float32 at the store.  Six
// launches per call (five without a bank), no host synchronisation, no atomics, and every reduction in a fixed order
// that depends on L alone, so a row's result depends neither on B nor on the other rows:
//   mix_direct   one block per row: d, the first index of the largest |h|
//   mix_conv     a block computes a tile of MX_TILE consecutive outputs of one row, MX_OPT per thread.  It walks the taps
//                that can reach a sample of the clip from its tile, k in [max(0, i0 + d - (L - 1)), min(K - 1, i0 + n - 1 +
//                d)], in chunks of MX_KC: a chunk's taps and the clean span they reach are staged in LDS as float64 (zero
//                where the clip has no sample), then every thread runs the chunk's taps in ascending order, one tap value
//                (an LDS broadcast) feeding MX_OPT speech accumulators and - for the taps k <= d + early - as many
//                target accumulators from the same loads.  K beyond the LDS span is more chunks; K > L is fewer: the
//                taps left out multiply zeros only.  The float64 speech / target rows go to the workspace, and the
//                block's sums of speech^2 and n^2 to one partial slot each.
//   mix_gain     one block per row: the partials in ascending slot order -> Ps, Pn, g
//   mix_vmax     per tile: max |speech + g n| -> one partial slot
//   mix_scale    one block per row: the partial maxima -> s
//   mix_apply    noisy = f32((speech + g n) s), target = f32(target s) or clean's bits
// The per-row tables are read on the device only.  An entry that would make a kernel read outside its bank is not
// trusted: a noise segment that leaves [0, bank_len) or has no sample counts as silence, a RIR index is clamped to
// [0, R), a RIR length to [1, Kmax].
#include <math.h>
#include <stdint.h>

#include "api_internal.h"
#include "mix_common.hip.h"

namespace {

struct MixArgs {
    const float* clean;
    const float* bank;
    const long long* n_start;
    const long long* n_len;
    const long long* n_off;
    const float* rir;
    const int* rir_index;
    const int* rir_len;
    const float* snr_db;
    float* noisy;
    float* target;
    double* g;
    double* scale;
    double* ps;
    double* pn;
    int* d;                  // workspace: direct-path index per row
    double* part_ps;         // workspace: [B][nt] each
    double* part_pn;
    double* part_m;
    double* speech;          // workspace: [B][L] float64 each
    double* tgt;
    long long ld, ld_out, bank_len;
    double peak;
    int B, L, R, Kmax, early, nt;
};

__device__ inline NoiseRow mix_noise_row(const MixArgs& a, int b) {
    return mx_segment(a.bank, a.bank_len, a.n_start[b], a.n_len[b], a.n_off[b]);
}

__device__ inline void mix_rir_row(const MixArgs& a, int b, const float*& h, int& K) {
    mx_rir_row(a.rir, a.R, a.Kmax, a.rir_index[b], a.rir_len[b], h, K);
}

// ------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(MX_TPB) void mix_direct(MixArgs a) {
    __shared__ float s_v[MX_TPB];
    __shared__ int s_i[MX_TPB];
    const int t = threadIdx.x, b = blockIdx.x;
    const float* h;
    int K;
    mix_rir_row(a, b, h, K);
    const int d = mx_direct_index(h, K, s_v, s_i);
    if (t == 0) a.d[b] = d;
}

__global__ __launch_bounds__(MX_TPB) void mix_conv(MixArgs a) {
    __shared__ double s_x[MX_TILE + MX_KC];
    __shared__ double s_h[MX_KC];
    __shared__ double s_red[MX_TPB];
    const int t = threadIdx.x, b = blockIdx.y;
    const int i0 = blockIdx.x * MX_TILE;
    const int cnt = a.L - i0 < MX_TILE ? a.L - i0 : MX_TILE;
    const float* row = a.clean + (size_t)b * a.ld;
    const float* h = nullptr;
    int K = 1, d = 0;
    if (a.rir) {
        mix_rir_row(a, b, h, K);
        d = a.d[b];
    }
    // last tap of the target: -1 none (the target is the clip itself)
    long long kt = -1;
    if (a.early >= 0) {
        kt = (long long)d + a.early;
        if (kt > K - 1) kt = K - 1;
    }
    long long k_lo = (long long)i0 + d - (a.L - 1);
    if (k_lo < 0) k_lo = 0;
    long long k_hi = (long long)i0 + cnt - 1 + d;
    if (k_hi > K - 1) k_hi = K - 1;
    double acc_s[MX_OPT], acc_t[MX_OPT];
#pragma unroll
    for (int r = 0; r < MX_OPT; ++r) acc_s[r] = acc_t[r] = 0.0;
    for (long long k0 = k_lo; k0 <= k_hi; k0 += MX_KC) {
        const int kc = k_hi - k0 + 1 < MX_KC ? (int)(k_hi - k0 + 1) : MX_KC;
        for (int j = t; j < kc; j += MX_TPB) s_h[j] = h ? (double)h[k0 + j] : 1.0;
        // s_x[q] = clean[x0 + q]: output o of the tile meets tap k0 + j at s_x[o + kc - 1 - j]
        const long long x0 = (long long)i0 + d - (k0 + kc - 1);
        for (int q = t; q < MX_TILE + kc - 1; q += MX_TPB) {
            const long long x = x0 + q;
            s_x[q] = (x >= 0 && x < a.L) ? (double)row[x] : 0.0;
        }
        __syncthreads();
        long long nb_ll = kt - k0 + 1;                       // taps of the chunk that also feed the target
        const int nb = nb_ll < 0 ? 0 : (nb_ll > kc ? kc : (int)nb_ll);
        const double* xs = s_x + t + kc - 1;
        int j = 0;
        for (; j < nb; ++j) {
            const double hv = s_h[j];
#pragma unroll
            for (int r = 0; r < MX_OPT; ++r) {
                const double xv = xs[r * MX_TPB - j];
                acc_s[r] = fma(hv, xv, acc_s[r]);
                acc_t[r] = fma(hv, xv, acc_t[r]);
            }
        }
        for (; j + 1 < kc; j += 2) {
            const double h0 = s_h[j], h1 = s_h[j + 1];
#pragma unroll
            for (int r = 0; r < MX_OPT; ++r) {
                acc_s[r] = fma(h0, xs[r * MX_TPB - j], acc_s[r]);
                acc_s[r] = fma(h1, xs[r * MX_TPB - j - 1], acc_s[r]);
            }
        }
        for (; j < kc; ++j) {
            const double hv = s_h[j];
#pragma unroll
            for (int r = 0; r < MX_OPT; ++r) acc_s[r] = fma(hv, xs[r * MX_TPB - j], acc_s[r]);
        }
        __syncthreads();
    }
    const NoiseRow nr = mix_noise_row(a, b);
    double ps = 0.0, pn = 0.0;
#pragma unroll
    for (int r = 0; r < MX_OPT; ++r) {
        const int o = t + r * MX_TPB;
        if (o < cnt) {
            const size_t e = (size_t)b * a.L + i0 + o;
            a.speech[e] = acc_s[r];
            if (a.early >= 0) a.tgt[e] = acc_t[r];
            ps = fma(acc_s[r], acc_s[r], ps);
            const double n = mix_noise(nr, i0 + o);
            pn = fma(n, n, pn);
        }
    }
    ps = block_sum(ps, s_red);
    pn = block_sum(pn, s_red);
    if (t == 0) {
        a.part_ps[(size_t)b * a.nt + blockIdx.x] = ps;
        a.part_pn[(size_t)b * a.nt + blockIdx.x] = pn;
    }
}

__global__ __launch_bounds__(MX_TPB) void mix_gain(MixArgs a) {
    __shared__ double s_red[MX_TPB];
    const int t = threadIdx.x, b = blockIdx.x;
    double ps = 0.0, pn = 0.0;
    for (int k = t; k < a.nt; k += MX_TPB) {
        ps += a.part_ps[(size_t)b * a.nt + k];
        pn += a.part_pn[(size_t)b * a.nt + k];
    }
    ps = block_sum(ps, s_red) / (double)a.L;
    pn = block_sum(pn, s_red) / (double)a.L;
    if (t == 0) {
        double g = 0.0;
        if (ps != 0.0 && pn != 0.0) g = sqrt(ps / (pn * pow(10.0, (double)a.snr_db[b] / 10.0)));
        a.ps[b] = ps;
        a.pn[b] = pn;
        a.g[b] = g;
    }
}

__global__ __launch_bounds__(MX_TPB) void mix_vmax(MixArgs a) {
    __shared__ double s_red[MX_TPB];
    const int t = threadIdx.x, b = blockIdx.y;
    const int i0 = blockIdx.x * MX_TILE;
    const NoiseRow nr = mix_noise_row(a, b);
    const double g = a.g[b];
    double m = 0.0;
#pragma unroll
    for (int r = 0; r < MX_OPT; ++r) {
        const int i = i0 + t + r * MX_TPB;
        if (i < a.L) m = fmax(m, fabs(mix_v(a.speech[(size_t)b * a.L + i], g, mix_noise(nr, i))));
    }
    m = block_max(m, s_red);
    if (t == 0) a.part_m[(size_t)b * a.nt + blockIdx.x] = m;
}

__global__ __launch_bounds__(MX_TPB) void mix_scale(MixArgs a) {
    __shared__ double s_red[MX_TPB];
    const int t = threadIdx.x, b = blockIdx.x;
    double m = 0.0;
    for (int k = t; k < a.nt; k += MX_TPB) m = fmax(m, a.part_m[(size_t)b * a.nt + k]);
    m = block_max(m, s_red);
    if (t == 0) a.scale[b] = m > a.peak ? a.peak / m : 1.0;
}

__global__ __launch_bounds__(MX_TPB) void mix_apply(MixArgs a) {
    const int t = threadIdx.x, b = blockIdx.y;
    const int i0 = blockIdx.x * MX_TILE;
    const NoiseRow nr = mix_noise_row(a, b);
    const double g = a.g[b], s = a.scale[b];
#pragma unroll
    for (int r = 0; r < MX_OPT; ++r) {
        const int i = i0 + t + r * MX_TPB;
        if (i >= a.L) continue;
        const size_t e = (size_t)b * a.L + i;
        const size_t eo = (size_t)b * a.ld_out + i;
        a.noisy[eo] = (float)(mix_v(a.speech[e], g, mix_noise(nr, i)) * s);
        if (a.early >= 0) {
            a.target[eo] = (float)(a.tgt[e] * s);
        } else {
            const float c = a.clean[(size_t)b * a.ld + i];
            a.target[eo] = s == 1.0 ? c : (float)((double)c * s);
        }
    }
}

struct MixLayout {
    size_t d, part, rows, total;       // byte offsets: d | 3 partial planes from `part` | 2 float64 row planes from `rows`
    size_t part_stride, row_stride;
};

inline MixLayout mx_layout(int B, int L) {
    MixLayout l;
    l.d = 0;
    l.part = mx_up256((size_t)B * sizeof(int));
    l.part_stride = mx_up256((size_t)B * mx_tiles(L) * sizeof(double));
    l.rows = l.part + 3 * l.part_stride;
    l.row_stride = mx_up256((size_t)B * L * sizeof(double));
    l.total = l.rows + 2 * l.row_stride;
    return l;
}

inline bool mx_shape_ok(int B, int L, int Kmax) { return B >= 1 && B <= 65535 && L >= 1 && L <= MX_MAX_L && Kmax >= 1 && Kmax <= MX_MAX_K; }

}  // namespace

extern "C" int cmgan_mix_tile(void) { return MX_TILE; }

extern "C" size_t cmgan_mix_workspace_bytes(const cmgan_handle* h, int B, int L, int Kmax) {
    (void)h;
    return mx_shape_ok(B, L, Kmax) ? mx_layout(B, L).total : 0;
}

extern "C" int cmgan_mix(cmgan_handle* h, const float* clean, int B, int L, long long ld, const float* noise_bank,
                         long long bank_len, const long long* noise_start, const long long* noise_len,
                         const long long* noise_off, const float* rir_bank, int R, int Kmax, const int* rir_index,
                         const int* rir_len, const float* snr_db, float peak, int early, float* noisy, float* target,
                         long long ld_out, double* g, double* scale, double* ps, double* pn, void* ws, size_t ws_bytes,
                         void* stream) {
    // every argument is judged before the handle is, so that the errors below need no GPU (the message of a call
    // without a handle is read with cmgan_last_error(NULL))
    if (!clean || !noise_bank || !noise_start || !noise_len || !noise_off || !snr_db || !noisy || !target || !g || !scale
        || !ps || !pn)
        return fail(h, CMGAN_E_BADARG, "cmgan_mix: null pointer");
    if (rir_bank && (!rir_index || !rir_len))
        return fail(h, CMGAN_E_BADARG, "cmgan_mix: a RIR bank needs rir_index and rir_len");
    if (((uintptr_t)clean | (uintptr_t)noise_bank | (uintptr_t)rir_bank | (uintptr_t)rir_index | (uintptr_t)rir_len
         | (uintptr_t)snr_db | (uintptr_t)noisy | (uintptr_t)target) & 3)
        return fail(h, CMGAN_E_BADARG, "cmgan_mix: float32 / int32 buffers must be 4-byte aligned");
    if (((uintptr_t)noise_start | (uintptr_t)noise_len | (uintptr_t)noise_off | (uintptr_t)g | (uintptr_t)scale
         | (uintptr_t)ps | (uintptr_t)pn) & 7)
        return fail(h, CMGAN_E_BADARG, "cmgan_mix: int64 / float64 buffers must be 8-byte aligned");
    if (B <= 0 || B > 65535 || L < 1 || ld < L || ld_out < L || bank_len < 1)
        return fail(h, CMGAN_E_BADARG, "cmgan_mix: need 0 < B <= 65535, L >= 1, ld >= L, ld_out >= L, bank_len >= 1 "
                    "(B=%d L=%d ld=%lld ld_out=%lld bank_len=%lld)", B, L, ld, ld_out, bank_len);
    if (!(peak > 0.f) || !(peak <= 3.0e38f))
        return fail(h, CMGAN_E_BADARG, "cmgan_mix: peak must be positive and finite (%g)", (double)peak);
    if (early < -1) return fail(h, CMGAN_E_BADARG, "cmgan_mix: early must be -1 (dry target) or >= 0 (%d)", early);
    if (!rir_bank) {
        R = 1;
        Kmax = 1;
    }
    if (R < 1 || Kmax < 1) return fail(h, CMGAN_E_BADARG, "cmgan_mix: a RIR bank needs R >= 1 and Kmax >= 1 (R=%d Kmax=%d)", R, Kmax);
    if (Kmax > MX_MAX_K)
        return fail(h, CMGAN_E_UNSUPPORTED, "cmgan_mix: RIRs of up to %d taps are supported (Kmax=%d)", MX_MAX_K, Kmax);
    if (L > MX_MAX_L)
        return fail(h, CMGAN_E_UNSUPPORTED, "cmgan_mix: rows of up to %d samples are supported (L=%d)", MX_MAX_L, L);
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "cmgan_mix: null handle");
    const MixLayout l = mx_layout(B, L);
    if (int rc = check_ws(h, ws, ws_bytes, l.total)) return rc;
    const LaunchCtx ctx = begin(h, stream);
    hipStream_t s = ctx.stream;
    char* w = (char*)ws;
    MixArgs a;
    a.clean = clean;
    a.bank = noise_bank;
    a.n_start = noise_start;
    a.n_len = noise_len;
    a.n_off = noise_off;
    a.rir = rir_bank;
    a.rir_index = rir_index;
    a.rir_len = rir_len;
    a.snr_db = snr_db;
    a.noisy = noisy;
    a.target = target;
    a.g = g;
    a.scale = scale;
    a.ps = ps;
    a.pn = pn;
    a.d = (int*)(w + l.d);
    a.part_ps = (double*)(w + l.part);
    a.part_pn = (double*)(w + l.part + l.part_stride);
    a.part_m = (double*)(w + l.part + 2 * l.part_stride);
    a.speech = (double*)(w + l.rows);
    a.tgt = (double*)(w + l.rows + l.row_stride);
    a.ld = ld;
    a.ld_out = ld_out;
    a.bank_len = bank_len;
    a.peak = (double)peak;
    a.B = B;
    a.L = L;
    a.R = R;
    a.Kmax = Kmax;
    a.early = early;
    a.nt = mx_tiles(L);
    const dim3 grid(a.nt, B);
    if (rir_bank) LAUNCH(ctx, "mix_direct", mix_direct<<<B, MX_TPB, 0, s>>>(a));
    LAUNCH(ctx, "mix_conv", mix_conv<<<grid, MX_TPB, 0, s>>>(a));
    LAUNCH(ctx, "mix_gain", mix_gain<<<B, MX_TPB, 0, s>>>(a));
    LAUNCH(ctx, "mix_vmax", mix_vmax<<<grid, MX_TPB, 0, s>>>(a));
    LAUNCH(ctx, "mix_scale", mix_scale<<<B, MX_TPB, 0, s>>>(a));
    LAUNCH(ctx, "mix_apply", mix_apply<<<grid, MX_TPB, 0, s>>>(a));
    return check_launch(h, "mix");
}
