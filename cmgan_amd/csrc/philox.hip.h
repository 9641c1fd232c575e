// philox.hip.h - Philox4x32-10 (Salmon et al. 2011), the counter-based generator torch's own dropout uses: the one
// definition behind the dropout masks of train.hip and the noise of rir_tail.hip.  c is the 128-bit counter as four words,
// (k0, k1) the 64-bit key; on return c holds the block's four 32-bit outputs.
#pragma once

__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
