// scene.hip - dynamic mixing of a [B, L] float32 batch of clean speech into (noisy, target) training pairs on the device:
// cmgan_mix and cmgan_scene (include/cmgan_hip.h), one implementation.  cmgan_mix adds one dry noise segment to the
// reverberant speech; cmgan_scene also puts up to SC_MAX_S further sources per row - point noises, interfering talkers -
// INSIDE the room, each convolved with a room response of its own and mixed in at an SNR of its own.  cmgan_mix is
// cmgan_scene with S = 0 and a dry-noise bank that must be there.  The reference only replays pairs somebody mixed before
// (src/data/dataloader.py:13-50 reads clean/x.wav and noisy/x.wav); its --cut_len help names "denoise and
// dereverberation" as the task.
//
//   h = rir[rir_index[b], 0:K], K = rir_len[b], d = first argmax |h|        (no bank: h = [1], d = 0)
//   speech[i] = sum_{k < K} h[k] clean[b, i + d - k]                         clean = 0 outside [0, L)
//   target    = clean (early == -1) or the same sum over the taps k <= d + early
//   n0[i]     = bank[noise_start[b] + (noise_off[b] + i) mod noise_len[b]]   the dry noise (cmgan_scene without a bank: none)
//   Ps = mean(speech^2), Pn = mean(n0^2), g0 = sqrt(Ps / (Pn 10^(snr_db / 10)))    (g0 = 0 when Ps == 0 or Pn == 0)
//   for j = 1 .. S_b,  S_b = clamp(n_src[b], 0, S):
//     seg_j[m] = src_bank[start_j + ((off_j + m) mod len_j)]               every integer m: the segment loops both ways
//     c_j[i]   = sum_{k < K_j} h_j[k] seg_j[i - k]                         h_j = rir[src_rir_index[b, j]], K_j = src_rir_len[b, j]
//                                                                          (no bank: h_j = [1]); the delay STAYS
//     P_j = mean(c_j^2),  g_j = sqrt(Ps / (P_j 10^(snr_j / 10)))           0 when Ps == 0 or P_j == 0
//   v = speech + g0 n0 + g_1 c_1 + ... + g_S c_S                           an fma chain in ascending j
//   m = max |v|, s = m > peak ? peak / m : 1
//   noisy = f32(v s), target = f32(target s)                                  (s == 1, early == -1: target is clean's bits)
//
// Float32 samples in and out; every product and sum in float64 on the VALU, one rounding to float32 at the store.  Six
// launches per call (five without a RIR bank), no host synchronisation, no atomics, and every reduction in a fixed order
// that depends on L alone, so a row's bits depend neither on B, nor on the other rows or their n_src, nor on what lies
// behind ld or in the source slots beyond S_b:
//   scene_direct  one block per row: d, the first index of the largest |h| of the talker's response
//   scene_conv    grid (tiles, 1 + S, B): a block computes a tile of MX_TILE consecutive outputs of one row, MX_OPT per
//                 thread.  Slice j = 0 is the talker.  It walks the taps that can reach a sample of the clip from its tile,
//                 k in [max(0, i0 + d - (L - 1)), min(K - 1, i0 + n - 1 + d)], in chunks of MX_KC: a chunk's taps and the
//                 clean span they reach are staged in LDS as float64 (zero where the clip has no sample), then every thread
//                 runs the chunk's taps in ascending order, one tap value (an LDS broadcast) feeding MX_OPT speech
//                 accumulators and - for the taps k <= d + early - as many target accumulators from the same loads.  K
//                 beyond the LDS span is more chunks; K > L is fewer: the taps left out multiply zeros only.  The float64
//                 speech / target rows go to the workspace, and the block's sums of speech^2 and n0^2 to one partial slot
//                 each.  Slice j >= 1 is source j: the same MX_TILE outputs and MX_KC-tap chunks, but ALL K_j taps reach a
//                 sample (the segment has no end), and the staged span is the LOOPED segment: a thread takes its first
//                 position mod len_j once per chunk and steps it by (MX_TPB mod len_j) with one conditional subtraction
//                 per staged sample, so a segment of 1 sample and one of 10^7 cost the same and the tap loop never sees a
//                 modulo.  c_j goes to the workspace in float64, the block's sum of c_j^2 to a partial slot.  A block of
//                 a source beyond S_b returns before it reads anything.
//   scene_gain    one block per row: the partials in ascending slot order -> Ps, Pn, g0, P_j, g_j
//   scene_vmax    per tile: max |v| -> one partial slot
//   scene_scale   one block per row: the partial maxima -> s
//   scene_apply   noisy = f32(v s), target = f32(target s) or clean's bits
// cmgan_scene_path is cmgan_scene for a talker and sources that MOVE: P waypoint columns in the RIR tables, waypoint p at
// input sample p H weighting the samples around it by u_p[m] = (H - |m - p H|) / H (held at the path's ends), so that
//   speech[i] = sum_p sum_k h_p[k] (u_p[m] clean[b, m]),  m = i + d_p - k     every waypoint's OWN direct index d_p removed
//   c_j[i]    = sum_p sum_k h_jp[k] (u_p[m] seg_j[m]),    m = i - k
// in ONE accumulator over (p, k) ascending.  scene_direct_path and scene_conv_path take the places of scene_direct and
// scene_conv; the inner tap loop, the store and every later kernel are shared, and a row with one waypoint has the static
// call's bits.  Doppler is not modelled.
// The per-row tables are read on the device only.  An entry that would make a kernel read outside its bank is not
// trusted: a segment that leaves its bank or has no sample counts as silence (c_j = 0, P_j = 0, g_j = 0), a RIR index is
// clamped to [0, R), a RIR length to [1, Kmax], offsets may be any int64.
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "api_internal.h"
#include "host_ranges.h"

namespace {

constexpr int MX_TPB = 256;                 // threads of every kernel here
constexpr int MX_OPT = 4;                   // outputs per thread of the convolutions: outputs t, t + 256, t + 512, t + 768 of the tile
constexpr int MX_TILE = MX_TPB * MX_OPT;    // outputs per block
constexpr int MX_KC = 1024;                 // taps per LDS chunk: 8 KiB of taps + 16 KiB of signal span, both float64
constexpr int MX_MAX_K = 65536;             // longest RIR (4 s at 16 kHz)
constexpr int MX_MAX_L = 0x7fffffff - MX_TILE;   // a tile's sample indices stay in an int

// a row's bank segment: valid only if it lies inside the bank; `off` is the row's offset mod len in [0, len)
struct NoiseRow {
    const float* p;
    long long len, off;
};

__device__ inline NoiseRow mx_segment(const float* bank, long long bank_len, long long st, long long len, long long off) {
    NoiseRow r;
    r.len = len;
    const bool ok = bank && st >= 0 && r.len >= 1 && st <= bank_len && r.len <= bank_len - st;
    if (!ok) {
        r.p = nullptr;
        r.len = 1;
        r.off = 0;
        return r;
    }
    r.p = bank + st;
    const long long o = off % r.len;
    r.off = o < 0 ? o + r.len : o;
    return r;
}

__device__ inline double mix_noise(const NoiseRow& r, int i) {
    return r.p ? (double)r.p[(r.off + i) % r.len] : 0.0;
}

// v = speech + g n: one expression for the maximum and the store, so both see the same bits
__device__ inline double mix_v(double speech, double g, double n) { return fma(g, n, speech); }

__device__ inline double block_sum(double v, double* red) {          // fixed order: halves folded, every thread calls
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = MX_TPB / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__device__ inline double block_max(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = MX_TPB / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = fmax(red[t], red[t + s]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// a RIR table entry is not trusted: the index is clamped to [0, R), the length to [1, Kmax]
__device__ inline void mx_rir_row(const float* rir, int R, int Kmax, int idx, int len, const float*& h, int& K) {
    idx = idx < 0 ? 0 : (idx >= R ? R - 1 : idx);
    K = len < 1 ? 1 : (len > Kmax ? Kmax : len);
    h = rir + (size_t)idx * Kmax;
}

// the direct path: the FIRST index at which |h[0:K]| is largest (all NaN: tap 0); every thread calls, thread 0 gets it
__device__ inline int mx_direct_index(const float* h, int K, float* s_v, int* s_i) {
    const int t = threadIdx.x;
    float best = -1.f;
    int at = 0x7fffffff;
    for (int k = t; k < K; k += MX_TPB) {
        const float v = fabsf(h[k]);
        if (v > best) { best = v; at = k; }                  // ascending k: the first of equals stays
    }
    s_v[t] = best;
    s_i[t] = at;
    __syncthreads();
    for (int s = MX_TPB / 2; s > 0; s >>= 1) {
        if (t < s) {
            const float v = s_v[t + s];
            const int i = s_i[t + s];
            if (v > s_v[t] || (v == s_v[t] && i < s_i[t])) { s_v[t] = v; s_i[t] = i; }
        }
        __syncthreads();
    }
    return s_i[0] < K ? s_i[0] : 0;
}

inline int mx_tiles(int L) { return (L + MX_TILE - 1) / MX_TILE; }

constexpr int SC_MAX_S = 4;                 // located sources per row

struct SceneArgs {
    const float* clean;
    const float* bank;               // dry noise (null: none)
    const long long* n_start;
    const long long* n_len;
    const long long* n_off;
    const float* snr_db;
    const float* src_bank;           // the sources' bank, tables [B, S]
    const int* n_src;
    const long long* s_start;
    const long long* s_len;
    const long long* s_off;
    const float* s_snr_db;
    const float* rir;
    const int* rir_index;
    const int* rir_len;
    const int* s_rir_index;
    const int* s_rir_len;
    float* noisy;
    float* target;
    double* g;                       // [B, 1 + S]
    double* p;                       // [B, 1 + S]: Pn, P_1 .. P_S
    double* ps;
    double* scale;
    int* d;                          // workspace: direct-path index per row
    double* part_ps;                 // workspace: [B][nt] each
    double* part_pn;
    double* part_m;
    double* part_pc;                 // workspace: [B][S][nt]
    double* speech;                  // workspace: [B][L] float64 each
    double* tgt;
    double* c;                       // workspace: [B][S][L]
    long long ld, ld_out, bank_len, src_bank_len;
    double peak;
    int B, L, R, Kmax, early, nt, S;
};

__device__ inline int scene_count(const SceneArgs& a, int b) {
    if (a.S == 0) return 0;
    const int n = a.n_src[b];
    return n < 0 ? 0 : (n > a.S ? a.S : n);
}

__device__ inline NoiseRow scene_noise_row(const SceneArgs& a, int b) {
    if (!a.bank) return mx_segment(nullptr, 0, 0, 0, 0);
    return mx_segment(a.bank, a.bank_len, a.n_start[b], a.n_len[b], a.n_off[b]);
}

// v of sample i of row b (e = b L + i): the fma chain in ascending j over the row's own sources; one expression for
// scene_vmax and scene_apply, so both see the same bits
__device__ inline double scene_v(const SceneArgs& a, int b, int sb, size_t e, int i, const NoiseRow& nr, const double* g) {
    double v = a.speech[e];
    if (a.bank) v = mix_v(v, g[0], mix_noise(nr, i));
#pragma unroll
    for (int j = 1; j <= SC_MAX_S; ++j)
        if (j <= sb) v = fma(g[j], a.c[((size_t)b * a.S + (j - 1)) * a.L + i], v);
    return v;
}

__device__ inline void scene_gains(const SceneArgs& a, int b, int sb, double* g) {
    g[0] = a.g[(size_t)b * (1 + a.S)];
#pragma unroll
    for (int j = 1; j <= SC_MAX_S; ++j) g[j] = j <= sb ? a.g[(size_t)b * (1 + a.S) + j] : 0.0;
}

// one staged chunk of kc taps, ascending, into a thread's MX_OPT accumulators; the first nb taps also feed the target.
// xs = s_x + t + kc - 1: output t + 256 r of the tile meets tap j of the chunk at xs[256 r - j]
__device__ inline void mx_chunk_taps(const double* s_h, const double* xs, int kc, int nb, double* acc_s, double* acc_t) {
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
}

// the end of a convolution block, static or along a path: the float64 rows to the workspace, the block's sums of squares
// to its partial slots; every thread calls
__device__ inline void scene_conv_store(const SceneArgs& a, int src, int b, int i0, int cnt, size_t es, const double* acc_s,
                                        const double* acc_t, double* s_red) {
    const int t = threadIdx.x;
    if (src == 0) {
        const NoiseRow nr = scene_noise_row(a, b);
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
    } else {
        double pc = 0.0;
#pragma unroll
        for (int r = 0; r < MX_OPT; ++r) {
            const int o = t + r * MX_TPB;
            if (o < cnt) {
                a.c[es * a.L + i0 + o] = acc_s[r];
                pc = fma(acc_s[r], acc_s[r], pc);
            }
        }
        pc = block_sum(pc, s_red);
        if (t == 0) a.part_pc[es * a.nt + blockIdx.x] = pc;
    }
}

// ------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(MX_TPB) void scene_direct(SceneArgs a) {
    __shared__ float s_v[MX_TPB];
    __shared__ int s_i[MX_TPB];
    const int b = blockIdx.x;
    const float* h;
    int K;
    mx_rir_row(a.rir, a.R, a.Kmax, a.rir_index[b], a.rir_len[b], h, K);
    const int d = mx_direct_index(h, K, s_v, s_i);
    if (threadIdx.x == 0) a.d[b] = d;
}

__global__ __launch_bounds__(MX_TPB) void scene_conv(SceneArgs a) {
    __shared__ double s_x[MX_TILE + MX_KC];
    __shared__ double s_h[MX_KC];
    __shared__ double s_red[MX_TPB];
    const int t = threadIdx.x, src = blockIdx.y, b = blockIdx.z;
    if (src > scene_count(a, b)) return;                     // (the whole block: src and b are its own)
    const int i0 = blockIdx.x * MX_TILE;
    const int cnt = a.L - i0 < MX_TILE ? a.L - i0 : MX_TILE;
    const float* row = a.clean + (size_t)b * a.ld;
    const float* h = nullptr;
    int K = 1, d = 0;
    long long kt = -1, k_lo = 0, k_hi;
    NoiseRow seg = mx_segment(nullptr, 0, 0, 0, 0);
    size_t es = 0;                                           // the source's slot b S + src - 1
    if (src == 0) {                                          // the talker: the taps that reach the clip
        if (a.rir) {
            mx_rir_row(a.rir, a.R, a.Kmax, a.rir_index[b], a.rir_len[b], h, K);
            d = a.d[b];
        }
        if (a.early >= 0) {
            kt = (long long)d + a.early;
            if (kt > K - 1) kt = K - 1;
        }
        k_lo = (long long)i0 + d - (a.L - 1);
        if (k_lo < 0) k_lo = 0;
        k_hi = (long long)i0 + cnt - 1 + d;
        if (k_hi > K - 1) k_hi = K - 1;
    } else {                                                 // a source: every tap meets a sample of the looping segment
        es = (size_t)b * a.S + (src - 1);
        seg = mx_segment(a.src_bank, a.src_bank_len, a.s_start[es], a.s_len[es], a.s_off[es]);
        if (a.rir) mx_rir_row(a.rir, a.R, a.Kmax, a.s_rir_index[es], a.s_rir_len[es], h, K);
        k_hi = seg.p ? K - 1 : -1;                           // silence: no tap, c = 0
    }
    double acc_s[MX_OPT], acc_t[MX_OPT];
#pragma unroll
    for (int r = 0; r < MX_OPT; ++r) acc_s[r] = acc_t[r] = 0.0;
    for (long long k0 = k_lo; k0 <= k_hi; k0 += MX_KC) {
        const int kc = k_hi - k0 + 1 < MX_KC ? (int)(k_hi - k0 + 1) : MX_KC;
        for (int j = t; j < kc; j += MX_TPB) s_h[j] = h ? (double)h[k0 + j] : 1.0;
        // s_x[q] = signal[x0 + q]: output o of the tile meets tap k0 + j at s_x[o + kc - 1 - j]
        const long long x0 = (long long)i0 + d - (k0 + kc - 1);
        if (src == 0) {
            for (int q = t; q < MX_TILE + kc - 1; q += MX_TPB) {
                const long long x = x0 + q;
                s_x[q] = (x >= 0 && x < a.L) ? (double)row[x] : 0.0;
            }
        } else {
            long long pos = (seg.off + x0 + t) % seg.len;    // the one modulo of this thread and chunk; x0 may be < 0
            if (pos < 0) pos += seg.len;
            const long long step = MX_TPB % seg.len;
            for (int q = t; q < MX_TILE + kc - 1; q += MX_TPB) {
                s_x[q] = (double)seg.p[pos];
                pos += step;
                if (pos >= seg.len) pos -= seg.len;
            }
        }
        __syncthreads();
        long long nb_ll = kt - k0 + 1;                       // taps of the chunk that also feed the target
        const int nb = nb_ll < 0 ? 0 : (nb_ll > kc ? kc : (int)nb_ll);
        mx_chunk_taps(s_h, s_x + t + kc - 1, kc, nb, acc_s, acc_t);
        __syncthreads();
    }
    scene_conv_store(a, src, b, i0, cnt, es, acc_s, acc_t, s_red);
}

// ---- cmgan_scene_path: the talker and the sources move along a path of responses.  In `a` the four RIR tables are the
// [B, P] / [B, S, P] ones and `d` is not used: the direct indices, one per waypoint, are in `dp`.
struct ScenePathArgs {
    SceneArgs a;
    const int* n_path;               // [B]
    const int* s_n_path;             // [B, S]
    int* dp;                         // workspace: [B][P]
    long long H;                     // input samples between waypoints
    int P;
};

constexpr int SP_MAX_P = 64;                    // waypoint columns
constexpr long long SP_MAX_H = 1LL << 30;       // so p H and the weights' numerators stay far inside an int64 / a double
constexpr long long SP_FAR = 1LL << 40;         // beyond every sample index and every p H

__device__ inline int path_count(const int* n_path, size_t row, int P) {
    const int n = n_path[row];
    return n < 1 ? 1 : (n > P ? P : n);
}

// u_p[m]: the triangle of half-width H around p H - an exact integer numerator, one IEEE division - that the first
// waypoint holds at 1 for m <= 0 and the last one for m >= (Pb - 1) H
__device__ inline double path_weight(long long m, int p, int Pb, long long H) {
    long long a = m - (long long)p * H;
    if (a <= 0 && p == 0) return 1.0;
    if (a >= 0 && p == Pb - 1) return 1.0;
    if (a < 0) a = -a;
    return a < H ? (double)(H - a) / (double)H : 0.0;
}

__global__ __launch_bounds__(MX_TPB) void scene_direct_path(ScenePathArgs pa) {
    __shared__ float s_v[MX_TPB];
    __shared__ int s_i[MX_TPB];
    const SceneArgs& a = pa.a;
    const int p = blockIdx.x, b = blockIdx.y;
    if (p >= path_count(pa.n_path, b, pa.P)) return;         // (the whole block) a column beyond the row's path is not read
    const size_t e = (size_t)b * pa.P + p;
    const float* h;
    int K;
    mx_rir_row(a.rir, a.R, a.Kmax, a.rir_index[e], a.rir_len[e], h, K);
    const int d = mx_direct_index(h, K, s_v, s_i);
    if (threadIdx.x == 0) pa.dp[e] = d;
}

// scene_conv along a path: the same tile, chunks, inner loop and accumulators, once per waypoint p in ascending order.
// Waypoint p weights the input samples m in (p H - H, p H + H) - the first one everything before, the last one everything
// after - so from a tile of cnt outputs it walks only the taps k = i + d_p - m that meet such a sample: at most
// cnt + 2 H - 2 of them, inside [0, K_p) and, for the talker, inside the clip.  The span is staged ALREADY weighted (one
// product per staged sample, rounded once), so the tap loop is scene_conv's.
__global__ __launch_bounds__(MX_TPB) void scene_conv_path(ScenePathArgs pa) {
    __shared__ double s_x[MX_TILE + MX_KC];
    __shared__ double s_h[MX_KC];
    __shared__ double s_red[MX_TPB];
    const SceneArgs& a = pa.a;
    const int t = threadIdx.x, src = blockIdx.y, b = blockIdx.z;
    if (src > scene_count(a, b)) return;                     // (the whole block: src and b are its own)
    const int i0 = blockIdx.x * MX_TILE;
    const int cnt = a.L - i0 < MX_TILE ? a.L - i0 : MX_TILE;
    const float* row = a.clean + (size_t)b * a.ld;
    const long long H = pa.H;
    NoiseRow seg = mx_segment(nullptr, 0, 0, 0, 0);
    size_t es = 0, pe;                                       // the source's slot b S + src - 1; its row of the path tables
    int Pb;
    if (src == 0) {
        pe = (size_t)b * pa.P;
        Pb = path_count(pa.n_path, b, pa.P);
    } else {
        es = (size_t)b * a.S + (src - 1);
        seg = mx_segment(a.src_bank, a.src_bank_len, a.s_start[es], a.s_len[es], a.s_off[es]);
        pe = es * pa.P;
        Pb = seg.p ? path_count(pa.s_n_path, es, pa.P) : 0;  // silence: no waypoint, c = 0
    }
    double acc_s[MX_OPT], acc_t[MX_OPT];
#pragma unroll
    for (int r = 0; r < MX_OPT; ++r) acc_s[r] = acc_t[r] = 0.0;
    for (int p = 0; p < Pb; ++p) {
        // the input samples this waypoint weights
        long long m_lo = p == 0 ? -SP_FAR : (long long)p * H - H + 1;
        long long m_hi = p == Pb - 1 ? SP_FAR : (long long)p * H + H - 1;
        const float* h;
        int K, d = 0;
        long long kt = -1;
        if (src == 0) {
            if (m_lo < 0) m_lo = 0;
            if (m_hi > a.L - 1) m_hi = a.L - 1;
            if (m_lo > m_hi) continue;                       // (p, Pb, H and L are the block's own: no thread skips a barrier)
            mx_rir_row(a.rir, a.R, a.Kmax, a.rir_index[pe + p], a.rir_len[pe + p], h, K);
            d = pa.dp[pe + p];
            if (a.early >= 0) {
                kt = (long long)d + a.early;
                if (kt > K - 1) kt = K - 1;
            }
        } else {
            mx_rir_row(a.rir, a.R, a.Kmax, a.s_rir_index[pe + p], a.s_rir_len[pe + p], h, K);
        }
        long long k_lo = (long long)i0 + d - m_hi;
        if (k_lo < 0) k_lo = 0;
        long long k_hi = (long long)i0 + cnt - 1 + d - m_lo;
        if (k_hi > K - 1) k_hi = K - 1;
        for (long long k0 = k_lo; k0 <= k_hi; k0 += MX_KC) {
            const int kc = k_hi - k0 + 1 < MX_KC ? (int)(k_hi - k0 + 1) : MX_KC;
            for (int j = t; j < kc; j += MX_TPB) s_h[j] = (double)h[k0 + j];
            // s_x[q] = u_p[x0 + q] signal[x0 + q]: output o of the tile meets tap k0 + j at s_x[o + kc - 1 - j]
            const long long x0 = (long long)i0 + d - (k0 + kc - 1);
            if (src == 0) {
                for (int q = t; q < MX_TILE + kc - 1; q += MX_TPB) {
                    const long long x = x0 + q;
                    s_x[q] = (x >= 0 && x < a.L) ? path_weight(x, p, Pb, H) * (double)row[x] : 0.0;
                }
            } else {
                long long pos = (seg.off + x0 + t) % seg.len;    // the one modulo of this thread and chunk; x0 may be < 0
                if (pos < 0) pos += seg.len;
                const long long step = MX_TPB % seg.len;
                for (int q = t; q < MX_TILE + kc - 1; q += MX_TPB) {
                    s_x[q] = path_weight(x0 + q, p, Pb, H) * (double)seg.p[pos];
                    pos += step;
                    if (pos >= seg.len) pos -= seg.len;
                }
            }
            __syncthreads();
            long long nb_ll = kt - k0 + 1;                   // taps of the chunk that also feed the target
            const int nb = nb_ll < 0 ? 0 : (nb_ll > kc ? kc : (int)nb_ll);
            mx_chunk_taps(s_h, s_x + t + kc - 1, kc, nb, acc_s, acc_t);
            __syncthreads();
        }
    }
    scene_conv_store(a, src, b, i0, cnt, es, acc_s, acc_t, s_red);
}

__global__ __launch_bounds__(MX_TPB) void scene_gain(SceneArgs a) {
    __shared__ double s_red[MX_TPB];
    const int t = threadIdx.x, b = blockIdx.x;
    const int sb = scene_count(a, b);
    double ps = 0.0, pn = 0.0;
    for (int k = t; k < a.nt; k += MX_TPB) {
        ps += a.part_ps[(size_t)b * a.nt + k];
        pn += a.part_pn[(size_t)b * a.nt + k];
    }
    ps = block_sum(ps, s_red) / (double)a.L;
    pn = block_sum(pn, s_red) / (double)a.L;
    double* g = a.g + (size_t)b * (1 + a.S);
    double* p = a.p + (size_t)b * (1 + a.S);
    if (t == 0) {
        double g0 = 0.0;
        if (a.bank && ps != 0.0 && pn != 0.0) g0 = sqrt(ps / (pn * pow(10.0, (double)a.snr_db[b] / 10.0)));
        a.ps[b] = ps;
        p[0] = pn;
        g[0] = g0;
    }
    for (int j = 1; j <= a.S; ++j) {
        double pc = 0.0, gj = 0.0;
        if (j <= sb) {                                       // (sb is the block's own: no thread skips the barrier)
            const size_t es = (size_t)b * a.S + (j - 1);
            for (int k = t; k < a.nt; k += MX_TPB) pc += a.part_pc[es * a.nt + k];
            pc = block_sum(pc, s_red) / (double)a.L;
            if (t == 0 && ps != 0.0 && pc != 0.0) gj = sqrt(ps / (pc * pow(10.0, (double)a.s_snr_db[es] / 10.0)));
        }
        if (t == 0) {
            p[j] = pc;
            g[j] = gj;
        }
    }
}

__global__ __launch_bounds__(MX_TPB) void scene_vmax(SceneArgs a) {
    __shared__ double s_red[MX_TPB];
    const int t = threadIdx.x, b = blockIdx.y;
    const int i0 = blockIdx.x * MX_TILE;
    const int sb = scene_count(a, b);
    const NoiseRow nr = scene_noise_row(a, b);
    double g[1 + SC_MAX_S];
    scene_gains(a, b, sb, g);
    double m = 0.0;
#pragma unroll
    for (int r = 0; r < MX_OPT; ++r) {
        const int i = i0 + t + r * MX_TPB;
        if (i < a.L) m = fmax(m, fabs(scene_v(a, b, sb, (size_t)b * a.L + i, i, nr, g)));
    }
    m = block_max(m, s_red);
    if (t == 0) a.part_m[(size_t)b * a.nt + blockIdx.x] = m;
}

__global__ __launch_bounds__(MX_TPB) void scene_scale(SceneArgs a) {
    __shared__ double s_red[MX_TPB];
    const int t = threadIdx.x, b = blockIdx.x;
    double m = 0.0;
    for (int k = t; k < a.nt; k += MX_TPB) m = fmax(m, a.part_m[(size_t)b * a.nt + k]);
    m = block_max(m, s_red);
    if (t == 0) a.scale[b] = m > a.peak ? a.peak / m : 1.0;
}

__global__ __launch_bounds__(MX_TPB) void scene_apply(SceneArgs a) {
    const int t = threadIdx.x, b = blockIdx.y;
    const int i0 = blockIdx.x * MX_TILE;
    const int sb = scene_count(a, b);
    const NoiseRow nr = scene_noise_row(a, b);
    double g[1 + SC_MAX_S];
    scene_gains(a, b, sb, g);
    const double s = a.scale[b];
#pragma unroll
    for (int r = 0; r < MX_OPT; ++r) {
        const int i = i0 + t + r * MX_TPB;
        if (i >= a.L) continue;
        const size_t e = (size_t)b * a.L + i;
        const size_t eo = (size_t)b * a.ld_out + i;
        a.noisy[eo] = (float)(scene_v(a, b, sb, e, i, nr, g) * s);
        if (a.early >= 0) {
            a.target[eo] = (float)(a.tgt[e] * s);
        } else {
            const float c = a.clean[(size_t)b * a.ld + i];
            a.target[eo] = s == 1.0 ? c : (float)((double)c * s);
        }
    }
}

struct SceneLayout {
    // byte offsets: d | the partial planes Ps, Pn, m, then S of P_j | the float64 row planes speech, target, then S of c_j
    size_t d, part, rows, total;
    size_t part_stride, row_stride;
};

inline SceneLayout sc_layout(int B, int L, int S) {
    SceneLayout l;
    l.d = 0;
    l.part = up256((size_t)B * sizeof(int));
    l.part_stride = up256((size_t)B * mx_tiles(L) * sizeof(double));
    l.rows = l.part + (3 + (size_t)S) * l.part_stride;
    l.row_stride = up256((size_t)B * L * sizeof(double));
    l.total = l.rows + (2 + (size_t)S) * l.row_stride;
    return l;
}

inline bool sc_shape_ok(int B, int L, int Kmax, int S) {
    return B >= 1 && B <= 65535 && L >= 1 && L <= MX_MAX_L && Kmax >= 1 && Kmax <= MX_MAX_K && S >= 0 && S <= SC_MAX_S;
}

// what cmgan_scene_path has beyond cmgan_scene; its workspace is that call's with the plane d [B, P] behind it
struct PathSpec {
    int P;
    long long H;
    const int* n_path;
    const int* src_n_path;
};

inline size_t sp_total(int B, int L, int S, int P) { return sc_layout(B, L, S).total + up256((size_t)B * P * sizeof(int)); }

// cmgan_scene, and cmgan_mix as its S = 0 case: `api` is the name of the entry point that was called, for the messages.
// Every argument is judged before the handle is, so that the errors below need no GPU (the message of a call without a
// handle is read with cmgan_last_error(NULL)).  With a `path` the call is cmgan_scene_path: the RIR tables have P columns
// per row and per source, and scene_direct_path / scene_conv_path take the places of scene_direct / scene_conv.
int mix_scene(const char* api, cmgan_handle* h, const float* clean, int B, int L, long long ld, const float* noise_bank,
              long long bank_len, const long long* noise_start, const long long* noise_len, const long long* noise_off,
              const float* snr_db, const float* src_bank, long long src_bank_len, int S, const int* n_src,
              const long long* src_start, const long long* src_len, const long long* src_off, const float* src_snr_db,
              const float* rir_bank, int R, int Kmax, const int* rir_index, const int* rir_len, const int* src_rir_index,
              const int* src_rir_len, float peak, int early, float* noisy, float* target, long long ld_out, double* g,
              double* p, double* ps, double* scale, void* ws, size_t ws_bytes, void* stream, const PathSpec* path = nullptr) {
    if (!clean || !noisy || !target || !g || !p || !ps || !scale) return fail(h, CMGAN_E_BADARG, "%s: null pointer", api);
    if (noise_bank && (!noise_start || !noise_len || !noise_off || !snr_db))
        return fail(h, CMGAN_E_BADARG, "%s: a dry-noise bank needs noise_start, noise_len, noise_off and snr_db", api);
    if (S < 0 || S > SC_MAX_S)
        return fail(h, CMGAN_E_BADARG, "%s: 0 <= S <= %d located sources per row (S=%d)", api, SC_MAX_S, S);
    if (S > 0 && (!src_bank || !n_src || !src_start || !src_len || !src_off || !src_snr_db))
        return fail(h, CMGAN_E_BADARG, "%s: S > 0 needs src_bank, n_src, src_start, src_len, src_off and src_snr_db", api);
    if (rir_bank && (!rir_index || !rir_len))
        return fail(h, CMGAN_E_BADARG, "%s: a RIR bank needs rir_index and rir_len", api);
    if (rir_bank && S > 0 && (!src_rir_index || !src_rir_len))
        return fail(h, CMGAN_E_BADARG, "%s: a RIR bank with S > 0 needs src_rir_index and src_rir_len", api);
    if (((uintptr_t)clean | (uintptr_t)noise_bank | (uintptr_t)snr_db | (uintptr_t)src_bank | (uintptr_t)n_src
         | (uintptr_t)src_snr_db | (uintptr_t)rir_bank | (uintptr_t)rir_index | (uintptr_t)rir_len | (uintptr_t)src_rir_index
         | (uintptr_t)src_rir_len | (uintptr_t)noisy | (uintptr_t)target) & 3)
        return fail(h, CMGAN_E_BADARG, "%s: float32 / int32 buffers must be 4-byte aligned", api);
    if (((uintptr_t)noise_start | (uintptr_t)noise_len | (uintptr_t)noise_off | (uintptr_t)src_start | (uintptr_t)src_len
         | (uintptr_t)src_off | (uintptr_t)g | (uintptr_t)p | (uintptr_t)ps | (uintptr_t)scale) & 7)
        return fail(h, CMGAN_E_BADARG, "%s: int64 / float64 buffers must be 8-byte aligned", api);
    if (B <= 0 || B > 65535 || L < 1 || ld < L || ld_out < L)
        return fail(h, CMGAN_E_BADARG, "%s: need 0 < B <= 65535, L >= 1, ld >= L, ld_out >= L (B=%d L=%d ld=%lld "
                    "ld_out=%lld)", api, B, L, ld, ld_out);
    if ((noise_bank && bank_len < 1) || (S > 0 && src_bank_len < 1))
        return fail(h, CMGAN_E_BADARG, "%s: a bank needs at least one sample (bank_len=%lld src_bank_len=%lld)", api,
                    bank_len, src_bank_len);
    if (!(peak > 0.f) || !(peak <= 3.0e38f))
        return fail(h, CMGAN_E_BADARG, "%s: peak must be positive and finite (%g)", api, (double)peak);
    if (early < -1) return fail(h, CMGAN_E_BADARG, "%s: early must be -1 (dry target) or >= 0 (%d)", api, early);
    if (!rir_bank) {
        R = 1;
        Kmax = 1;
    }
    if (R < 1 || Kmax < 1) return fail(h, CMGAN_E_BADARG, "%s: a RIR bank needs R >= 1 and Kmax >= 1 (R=%d Kmax=%d)", api, R, Kmax);
    if (Kmax > MX_MAX_K)
        return fail(h, CMGAN_E_UNSUPPORTED, "%s: RIRs of up to %d taps are supported (Kmax=%d)", api, MX_MAX_K, Kmax);
    if (L > MX_MAX_L)
        return fail(h, CMGAN_E_UNSUPPORTED, "%s: rows of up to %d samples are supported (L=%d)", api, MX_MAX_L, L);
    const SceneLayout l = sc_layout(B, L, S);
    if (path) {
        if (path->P < 1 || path->P > SP_MAX_P || path->H < 1 || path->H > SP_MAX_H)
            return fail(h, CMGAN_E_BADARG, "%s: need 1 <= P <= %d waypoints and a hop 1 <= H <= 2^30 (P=%d H=%lld)", api,
                        SP_MAX_P, path->P, path->H);
        if (!rir_bank) return fail(h, CMGAN_E_BADARG, "%s: a path needs a RIR bank", api);
        if (!path->n_path || (S > 0 && !path->src_n_path))
            return fail(h, CMGAN_E_BADARG, "%s: a path needs n_path and, with S > 0, src_n_path", api);
        if (((uintptr_t)path->n_path | (uintptr_t)path->src_n_path) & 3)
            return fail(h, CMGAN_E_BADARG, "%s: float32 / int32 buffers must be 4-byte aligned", api);
        const size_t need = sp_total(B, L, S, path->P);
        if (!ws || ((uintptr_t)ws & 255) != 0 || ws_bytes < need)
            return fail(h, CMGAN_E_BADARG, "%s: the workspace must be 256-byte aligned and hold %zu bytes (%zu given)", api,
                        need, ws ? ws_bytes : (size_t)0);
    }
    if (!h) return fail(nullptr, CMGAN_E_BADARG, "%s: null handle", api);
    if (!path)
        if (int rc = check_ws(h, ws, ws_bytes, l.total)) return rc;
    const LaunchCtx ctx = begin(h, stream);
    hipStream_t s = ctx.stream;
    char* w = (char*)ws;
    SceneArgs a;
    a.clean = clean;
    a.bank = noise_bank;
    a.n_start = noise_start;
    a.n_len = noise_len;
    a.n_off = noise_off;
    a.snr_db = snr_db;
    a.src_bank = src_bank;
    a.n_src = n_src;
    a.s_start = src_start;
    a.s_len = src_len;
    a.s_off = src_off;
    a.s_snr_db = src_snr_db;
    a.rir = rir_bank;
    a.rir_index = rir_index;
    a.rir_len = rir_len;
    a.s_rir_index = src_rir_index;
    a.s_rir_len = src_rir_len;
    a.noisy = noisy;
    a.target = target;
    a.g = g;
    a.p = p;
    a.ps = ps;
    a.scale = scale;
    a.d = (int*)(w + l.d);
    a.part_ps = (double*)(w + l.part);
    a.part_pn = (double*)(w + l.part + l.part_stride);
    a.part_m = (double*)(w + l.part + 2 * l.part_stride);
    a.part_pc = (double*)(w + l.part + 3 * l.part_stride);
    a.speech = (double*)(w + l.rows);
    a.tgt = (double*)(w + l.rows + l.row_stride);
    a.c = (double*)(w + l.rows + 2 * l.row_stride);
    a.ld = ld;
    a.ld_out = ld_out;
    a.bank_len = bank_len;
    a.src_bank_len = src_bank_len;
    a.peak = (double)peak;
    a.B = B;
    a.L = L;
    a.R = R;
    a.Kmax = Kmax;
    a.early = early;
    a.nt = mx_tiles(L);
    a.S = S;
    const dim3 grid(a.nt, B);
    if (path) {
        const ScenePathArgs pa{a, path->n_path, path->src_n_path, (int*)(w + l.total), path->H, path->P};
        LAUNCH(ctx, "scene_direct_path", scene_direct_path<<<dim3(path->P, B), MX_TPB, 0, s>>>(pa));
        LAUNCH(ctx, "scene_conv_path", scene_conv_path<<<dim3(a.nt, 1 + S, B), MX_TPB, 0, s>>>(pa));
    } else {
        if (rir_bank) LAUNCH(ctx, "scene_direct", scene_direct<<<B, MX_TPB, 0, s>>>(a));
        LAUNCH(ctx, "scene_conv", scene_conv<<<dim3(a.nt, 1 + S, B), MX_TPB, 0, s>>>(a));
    }
    LAUNCH(ctx, "scene_gain", scene_gain<<<B, MX_TPB, 0, s>>>(a));
    LAUNCH(ctx, "scene_vmax", scene_vmax<<<grid, MX_TPB, 0, s>>>(a));
    LAUNCH(ctx, "scene_scale", scene_scale<<<B, MX_TPB, 0, s>>>(a));
    LAUNCH(ctx, "scene_apply", scene_apply<<<grid, MX_TPB, 0, s>>>(a));
    return check_launch(h, api + 6);                         // "mix" / "scene" / "scene_path": the name without its cmgan_
}

}  // namespace

extern "C" int cmgan_mix_tile(void) { return MX_TILE; }

extern "C" int cmgan_scene_max_sources(void) { return SC_MAX_S; }

extern "C" size_t cmgan_scene_workspace_bytes(const cmgan_handle* h, int B, int L, int Kmax, int S) {
    (void)h;
    return sc_shape_ok(B, L, Kmax, S) ? sc_layout(B, L, S).total : 0;
}

extern "C" size_t cmgan_mix_workspace_bytes(const cmgan_handle* h, int B, int L, int Kmax) {
    return cmgan_scene_workspace_bytes(h, B, L, Kmax, 0);
}

extern "C" int cmgan_scene(cmgan_handle* h, const float* clean, int B, int L, long long ld, const float* noise_bank,
                           long long bank_len, const long long* noise_start, const long long* noise_len,
                           const long long* noise_off, const float* snr_db, const float* src_bank, long long src_bank_len,
                           int S, const int* n_src, const long long* src_start, const long long* src_len,
                           const long long* src_off, const float* src_snr_db, const float* rir_bank, int R, int Kmax,
                           const int* rir_index, const int* rir_len, const int* src_rir_index, const int* src_rir_len,
                           float peak, int early, float* noisy, float* target, long long ld_out, double* g, double* p,
                           double* ps, double* scale, void* ws, size_t ws_bytes, void* stream) {
    return mix_scene("cmgan_scene", h, clean, B, L, ld, noise_bank, bank_len, noise_start, noise_len, noise_off, snr_db,
                     src_bank, src_bank_len, S, n_src, src_start, src_len, src_off, src_snr_db, rir_bank, R, Kmax, rir_index,
                     rir_len, src_rir_index, src_rir_len, peak, early, noisy, target, ld_out, g, p, ps, scale, ws, ws_bytes,
                     stream);
}

extern "C" int cmgan_scene_max_waypoints(void) { return SP_MAX_P; }

extern "C" size_t cmgan_scene_path_workspace_bytes(const cmgan_handle* h, int B, int L, int Kmax, int S, int P) {
    (void)h;
    return sc_shape_ok(B, L, Kmax, S) && P >= 1 && P <= SP_MAX_P ? sp_total(B, L, S, P) : 0;
}

extern "C" int cmgan_scene_path(cmgan_handle* h, const float* clean, int B, int L, long long ld, const float* noise_bank,
                                long long bank_len, const long long* noise_start, const long long* noise_len,
                                const long long* noise_off, const float* snr_db, const float* src_bank, long long src_bank_len,
                                int S, const int* n_src, const long long* src_start, const long long* src_len,
                                const long long* src_off, const float* src_snr_db, const float* rir_bank, int R, int Kmax,
                                int P, int H, const int* n_path, const int* rir_index, const int* rir_len,
                                const int* src_n_path, const int* src_rir_index, const int* src_rir_len, float peak, int early,
                                float* noisy, float* target, long long ld_out, double* g, double* p, double* ps, double* scale,
                                void* ws, size_t ws_bytes, void* stream) {
    const PathSpec path{P, H, n_path, src_n_path};
    return mix_scene("cmgan_scene_path", h, clean, B, L, ld, noise_bank, bank_len, noise_start, noise_len, noise_off, snr_db,
                     src_bank, src_bank_len, S, n_src, src_start, src_len, src_off, src_snr_db, rir_bank, R, Kmax, rir_index,
                     rir_len, src_rir_index, src_rir_len, peak, early, noisy, target, ld_out, g, p, ps, scale, ws, ws_bytes,
                     stream, &path);
}

// the scene without located sources whose dry noise and outputs must all be there; its [B, 1 + S] tables g and p are
// this call's [B] vectors g and pn
extern "C" int cmgan_mix(cmgan_handle* h, const float* clean, int B, int L, long long ld, const float* noise_bank,
                         long long bank_len, const long long* noise_start, const long long* noise_len,
                         const long long* noise_off, const float* rir_bank, int R, int Kmax, const int* rir_index,
                         const int* rir_len, const float* snr_db, float peak, int early, float* noisy, float* target,
                         long long ld_out, double* g, double* scale, double* ps, double* pn, void* ws, size_t ws_bytes,
                         void* stream) {
    if (!clean || !noise_bank || !noise_start || !noise_len || !noise_off || !snr_db || !noisy || !target || !g || !scale
        || !ps || !pn)
        return fail(h, CMGAN_E_BADARG, "cmgan_mix: null pointer");
    return mix_scene("cmgan_mix", h, clean, B, L, ld, noise_bank, bank_len, noise_start, noise_len, noise_off, snr_db,
                     nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, rir_bank, R, Kmax, rir_index, rir_len, nullptr,
                     nullptr, peak, early, noisy, target, ld_out, g, pn, ps, scale, ws, ws_bytes, stream);
}
