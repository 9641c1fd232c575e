// in_running.hip - RUNNING InstanceNorm statistics for carried-state streaming (include/cmgan_hip.h, "Streaming";
// cmgan_stream_encoder_running / cmgan_stream_decoder_running).
//
// A running stream carries, per norm and per (row, channel), fp64 sums {n, S1 = sum x, S2 = sum x^2} of the norm's
// INPUT (the conv output, bias included).  A step adds the frames [hist, T) of its call - the history frames in front
// were counted by an earlier step - then turns the sums into the (scale, shift) pair the next consumer normalises on
// load with, the arithmetic of in_finalize_kernel (conv.hip): mean = S1 / n, var = max(S2 / n - mean^2, 0), eps 1e-5.
//
// The conv epilogues' tile partials cannot be reused (a 128-position tile straddles frames), so the raw output the
// conv already stored is read again: a partial pass (one block per chunk of a row's new positions, fp64 per block,
// fixed order) and a finalize pass (one block per row, the chunks in a fixed order).  No atomics: a graph replay and an
// eager call give the same bits.  The fold2 norm of the complex decoder (channel c owns conv channels c and c + 64,
// generator.py:112-119, 148) needs no variant of its own: the pixel-shuffled output [B, T, 2F', 64] IS the folded
// layout, so it is reduced as a 64-channel tensor with 2F' positions per frame.
#include "kernels.h"

#define IRN_CHUNK 512          // positions per partial block (64-channel norms)
#define IRN_MCHUNK 2048        // positions per partial block (the mask head's one-channel norm)
#define IRN_MAXCH 256          // partial blocks per row at most
#define IRN_NP 16              // threads per channel in the finalize pass

// x channels-last [B, T*PF, 64]; block (k, b) sums positions [k chunk, (k + 1) chunk) of row b's n new positions
// (which start at position pos0 of the row) into part[b][k][64][2]
__global__ __launch_bounds__(256) void in_running_partial_kernel(const float* __restrict__ x, long row_pos, long pos0,
                                                                 long n, long chunk, double* __restrict__ part) {
    __shared__ double red[16][64][2];
    const int c4 = threadIdx.x & 15, pl = threadIdx.x >> 4;   // 16 lanes x float4 = one 256 B row; 16 rows in flight
    const int b = blockIdx.y;
    const long lo = (long)blockIdx.x * chunk;
    const long hi = lo + chunk < n ? lo + chunk : n;
    const float* xb = x + ((long)b * row_pos + pos0) * 64 + c4 * 4;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    for (long p0 = lo + pl; p0 < hi; p0 += 16 * 4) {          // 4 independent loads in flight per thread
        f32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long p = p0 + 16 * k;
            v[k] = p < hi ? ldg4(xb + p * 64) : splat4(0.f);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)v[k][e];
                s1[e] += d;
                s2[e] += d * d;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        red[pl][c4 * 4 + e][0] = s1[e];
        red[pl][c4 * 4 + e][1] = s2[e];
    }
    __syncthreads();
    if (threadIdx.x < 128) {
        const int c = threadIdx.x >> 1, w = threadIdx.x & 1;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 16; q += 4)                        // fixed order: groups of four, then the groups
            s += (red[q][c][w] + red[q + 1][c][w]) + (red[q + 2][c][w] + red[q + 3][c][w]);
        part[(((long)b * gridDim.x + blockIdx.x) * 64 + c) * 2 + w] = s;
    }
}

// the mask head's norm input: conv_1 over (f, f + 1) + bias, from the tail projections dm [B, T*(F+1), 4]
// (the same expression as mask_raw in conv.hip)
__device__ __forceinline__ float irn_mask_raw(const float* __restrict__ dm, long base, float bias) {
    return dm[base * 4 + 0] + dm[(base + 1) * 4 + 1] + bias;
}

// block (k, b) sums the mask values of positions [k chunk, (k + 1) chunk) of row b's n = (T - hist) F new ones
__global__ __launch_bounds__(256) void mask_running_partial_kernel(const float* __restrict__ dm,
                                                                   const float* __restrict__ scalars, int T, int F,
                                                                   int hist, long n, long chunk,
                                                                   double* __restrict__ part) {
    __shared__ double r1[256], r2[256];
    const int b = blockIdx.y;
    const int W = F + 1;
    const float bias = scalars[0];
    const long lo = (long)blockIdx.x * chunk;
    const long hi = lo + chunk < n ? lo + chunk : n;
    double s1 = 0.0, s2 = 0.0;
    for (long i0 = lo + threadIdx.x; i0 < hi; i0 += 256 * 4) {
        float mv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long i = i0 + 256 * k < hi ? i0 + 256 * k : hi - 1;
            const int t = hist + (int)(i / F), f = (int)(i % F);
            mv[k] = irn_mask_raw(dm, ((long)b * T + t) * W + f, bias);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + 256 * k < hi) {
                s1 += (double)mv[k];
                s2 += (double)mv[k] * (double)mv[k];
            }
        }
    }
    r1[threadIdx.x] = s1;
    r2[threadIdx.x] = s2;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) {
            r1[threadIdx.x] += r1[threadIdx.x + st];
            r2[threadIdx.x] += r2[threadIdx.x + st];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[((long)b * gridDim.x + blockIdx.x) * 2 + 0] = r1[0];
        part[((long)b * gridDim.x + blockIdx.x) * 2 + 1] = r2[0];
    }
}

// one block per row: chunks in a fixed order, + the carried sums {n, S1, S2} [B][C][3] (written back), -> the pair.
// C = 64: nscale / nshift [B][64] from the affine weights gb = {gamma[64], beta[64]};
// C = 1 (mask head): mstat [B][2] = {mean, 1 / sqrt(var + eps)}, the layout final_combine_kernel reads.
template <int C>
__global__ __launch_bounds__(64 * IRN_NP) void in_running_finalize_kernel(const double* __restrict__ part, int nch,
                                                                          double count, double* __restrict__ sums,
                                                                          const float* __restrict__ gb,
                                                                          float* __restrict__ nscale,
                                                                          float* __restrict__ nshift,
                                                                          float* __restrict__ mstat) {
    __shared__ double acc[IRN_NP][64][2];
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int b = blockIdx.x;
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        for (int k = q; k < nch; k += IRN_NP) {
            const double* p = part + (((long)b * nch + k) * C + c) * 2;
            s1 += p[0];
            s2 += p[1];
        }
    }
    acc[q][c][0] = s1;
    acc[q][c][1] = s2;
    __syncthreads();
    if (q == 0 && c < C) {
        s1 = 0.0; s2 = 0.0;
#pragma unroll
        for (int r = 0; r < IRN_NP; r += 4) {
            s1 += (acc[r][c][0] + acc[r + 1][c][0]) + (acc[r + 2][c][0] + acc[r + 3][c][0]);
            s2 += (acc[r][c][1] + acc[r + 1][c][1]) + (acc[r + 2][c][1] + acc[r + 3][c][1]);
        }
        double* sm = sums + ((long)b * C + c) * 3;
        const double n = sm[0] + count;
        s1 += sm[1];
        s2 += sm[2];
        sm[0] = n;
        sm[1] = s1;
        sm[2] = s2;
        const double mean = s1 / n;
        double var = s2 / n - mean * mean;
        if (var < 0.0) var = 0.0;
        const double rstd = 1.0 / sqrt(var + 1e-5);
        if (C == 1) {
            mstat[b * 2 + 0] = (float)mean;
            mstat[b * 2 + 1] = (float)rstd;
        } else {
            const double sc = (double)gb[c] * rstd;
            nscale[b * 64 + c] = (float)sc;
            nshift[b * 64 + c] = (float)((double)gb[64 + c] - mean * sc);
        }
    }
}

// partial blocks per row: ~`chunk` positions each, at most IRN_MAXCH and at most what `part_doubles` holds
static int irn_chunks(long n, long chunk, int B, int C, size_t part_doubles) {
    long nch = (n + chunk - 1) / chunk;
    nch = std::min<long>(nch, IRN_MAXCH);
    nch = std::min<long>(nch, (long)(part_doubles / ((size_t)B * C * 2)));
    return (int)std::max<long>(nch, 1);
}

void launch_in_running(LaunchCtx ctx, const float* x, int B, int T, int PF, int hist, double* part,
                       size_t part_doubles, double* sums, const float* gb, float* nscale, float* nshift) {
    const long n = (long)(T - hist) * PF;
    const int nch = irn_chunks(n, IRN_CHUNK, B, 64, part_doubles);
    const long chunk = (n + nch - 1) / nch;
    LAUNCH(ctx, "in_running_partial", (in_running_partial_kernel<<<dim3(nch, B), 256, 0, ctx.stream>>>(
                                          x, (long)T * PF, (long)hist * PF, n, chunk, part)));
    LAUNCH(ctx, "in_running_finalize", (in_running_finalize_kernel<64><<<B, 64 * IRN_NP, 0, ctx.stream>>>(
                                           part, nch, (double)n, sums, gb, nscale, nshift, nullptr)));
}

void launch_mask_running(LaunchCtx ctx, const float* dm, const float* scalars, int B, int T, int F, int hist,
                         double* part, size_t part_doubles, double* sums, float* mstat) {
    const long n = (long)(T - hist) * F;
    const int nch = irn_chunks(n, IRN_MCHUNK, B, 1, part_doubles);
    const long chunk = (n + nch - 1) / nch;
    LAUNCH(ctx, "mask_running_partial", (mask_running_partial_kernel<<<dim3(nch, B), 256, 0, ctx.stream>>>(
                                            dm, scalars, T, F, hist, n, chunk, part)));
    LAUNCH(ctx, "mask_running_finalize", (in_running_finalize_kernel<1><<<B, 64 * IRN_NP, 0, ctx.stream>>>(
                                             part, nch, (double)n, sums, nullptr, nullptr, nullptr, mstat)));
}
