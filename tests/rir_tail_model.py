"""The plain-numpy statement of cmgan_rir_tail (include/cmgan_hip.h, "The diffuse reverberant tail"): a response extended
from its junction k_x by noise under an exponential envelope that follows a given 60 dB decay time band by band, the level
fitted to the W samples in front of the junction.  It shares no code with the kernels: the Philox below is numpy's integer
arithmetic, every sum is in np.longdouble (64 mantissa bits on x86; its own error is 2^-11 of a float64 rounding and is
left out below).  The GPU tests compare Engine.rir_tail with it, the host tests compare it with a naive loop, closed forms
and literal values.

The noise nu is EXACT in the model and on the device alike: an integer below 2^34 divided once, IEEE's division, by one
float64 literal.  Besides each value `rir_tail_row` returns a DERIVED BOUND on |device - model|, one term per rounding source
(u = 2^-53; the scheme of rir_bands_model.rir_bands_row and rir_stats_model):
  x(q)   an exponent -delta_b (q - k_x) (or twice that in S_b): delta_b is a literal divided by a rounded product, the
         exponent a rounded product, and exp is the device's.  By the project's convention (rir_model.bound) the computed
         exp(x) is taken as good to rx(x) = 64 u max(1, |x|), relative
  z_b    NF fused multiply-adds in ascending j: |dz| <= bz = (NF + 1) u sum_j |g_b[j] h[k + D - j]|
  E_b    sum of z^2 over W terms in whatever order: |dE| <= bE = sum be + (W + 1) u (E + sum be), be = (2 |z| bz + bz^2) (1 + u) + u z^2
  G_b    relative rG = (NF + 1) u;  S_b: relative rS = max_k rx(2 x(k)) + (W + 1) u
  A_b    sqrt(E / (G S)): relative rA = 0.505 (bE / E + rG + rS) + 67 u (a product, a quotient, and 64 ulps for the device's
         sqrt), infinite unless bE / E + rG + rS < 0.5.  E_b = 0 with bE = 0 is exactly 0 on the device too
  e_b    (A_b exp(x)) nu[q]: relative re(q) = rA + rx(x(q)) + 2 u
  y[k]   NB NF fused multiply-adds: |dy| <= sum_b sum_j |g_b[j] e_b[q]| re_b(q) + (NB NF + 1) u sum_b sum_j |g_b[j] e_b[q]|, q = k + D - j
  f32    2^-24 |y[k]| + 2^-150 for the one rounding to float32
These are bounds, not measurements: nothing here was fitted to what the kernels give.  They are generous on purpose - a
wrong Philox word, counter, envelope index, filter index or band is wrong by the size of the value itself."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
NOTHING, WINDOW, DECAY, NONFINITE = 1, 2, 4, 8
THREE_LN10 = 6.907755278982137          # CMGAN_RIR_TAIL_3LN10
NOISE_DIV = 2479700524.506239           # CMGAN_RIR_TAIL_NOISE_DIV = sqrt((2^64 - 1) / 3)


def philox4x32_10(c0, seed):
    """numpy Philox4x32-10 (Salmon et al. 2011) at the counter words (c0, 0, 0, 0) under the 64-bit key `seed`: four
    uint64 arrays that hold the block's 32-bit words."""
    M0, M1, W0, W1, LO, S = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85, np.uint64(0xffffffff), np.uint64(32)
    c0 = np.asarray(c0).astype(np.uint64)
    c = [c0, np.zeros_like(c0), np.zeros_like(c0), np.zeros_like(c0)]
    seed = int(seed) & 0xffffffffffffffff
    k0, k1 = seed & 0xffffffff, seed >> 32
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S) ^ c[1] ^ np.uint64(k0), p1 & LO, (p0 >> S) ^ c[3] ^ np.uint64(k1), p0 & LO]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return c


def noise(seed, q):
    """nu[q], float64, for an integer array q: 0 where q < 0."""
    q = np.asarray(q, dtype=np.int64)
    w = philox4x32_10(np.maximum(q, 0), seed)
    total = (w[0] + w[1] + w[2] + w[3]).astype(np.int64) - 2 * (2 ** 32 - 1)
    return np.where(q >= 0, total.astype(np.float64) / NOISE_DIV, 0.0)


def delta(decay, fs):
    return LD(THREE_LN10) / (LD(decay) * LD(fs))


def _rx(x):
    return 64 * U * np.maximum(1.0, np.abs(np.asarray(x, dtype=np.float64)))


def level_fit(h, kx, g, decay, W, fs, real=LD):
    """One band's fit on the float32 row h (zero outside [0, kx)): (A, its bound, E, G, S), in `real` but the bound."""
    LD = real
    NF = len(g)
    D = (NF - 1) // 2
    k_lo = kx - D - W
    assert k_lo >= 0 and NF % 2 == 1
    g = np.asarray(g, dtype=LD)
    span = np.zeros(W + NF - 1, dtype=LD)                          # span[i] = h[k_lo - D + i]
    lo = k_lo - D
    span[max(-lo, 0):] = np.asarray(h[max(lo, 0):kx], dtype=LD)
    z = np.convolve(span, g)[NF - 1:NF - 1 + W]                    # z[m] = sum_j g[j] span[m + 2 D - j]
    mag = np.convolve(np.abs(span), np.abs(g))[NF - 1:NF - 1 + W]
    bz = (NF + 1) * U * mag
    e = z * z
    be = (2 * np.abs(z) * bz + bz * bz) * (1 + U) + U * e
    E = np.sum(e)
    bE = np.sum(be) + (W + 1) * U * (E + np.sum(be))
    G = np.sum(g * g)
    d = LD(delta(decay, fs))
    x = -2 * d * (np.arange(k_lo, k_lo + W) - kx).astype(LD)
    S = np.sum(np.exp(x))
    if E == 0:
        return LD(0), (0.0 if bE == 0 else float(np.sqrt(bE / (G * S)))), E, G, S
    rel = float(bE / E) + (NF + 1) * U + float(np.max(_rx(x))) + (W + 1) * U
    A = np.sqrt(E / (G * S))
    return A, (float(A) * (0.505 * rel + 67 * U) if rel < 0.5 else np.inf), E, G, S


def rir_tail_row(h, kx, n_taps, decay, seed, filt=None, W=480, fs=16000, nu=noise, real=LD):
    """One row.  h: the float32 [K] row on entry; kx: len[r] on entry; n_taps: the wanted length; decay: [NB'] seconds;
    filt: float64 [NB, NF] or None.  `nu(seed, q)` is the noise (replaced by the host tests); `real` = np.float64 trades
    the model's extra precision for speed where no bound is asked of it.  Returns a dict: y float64
    [K], the row on return before its one rounding to float32 (the input where the row is left alone or below the
    junction, zeros from k_end on); bound [K] (0 where the device must give y's bits exactly); gain, gain_bound
    [NB']; status; length (len[r] on return); kx, kend (clamped)."""
    LD = real
    h = np.asarray(h, dtype=np.float32)
    K = len(h)
    filt = np.ones((1, 1)) if filt is None else np.asarray(filt, dtype=np.float64)
    NB, NF = filt.shape
    assert NF % 2 == 1
    D = (NF - 1) // 2
    decay = np.asarray(decay, dtype=np.float64).reshape(NB)
    kx_in = int(kx)
    kx, kend = min(max(kx_in, 1), K), min(max(int(n_taps), 1), K)
    out = {"y": h.astype(np.float64), "bound": np.zeros(K), "gain": np.zeros(NB), "gain_bound": np.zeros(NB), "status": 0,
           "length": kx_in, "kx": kx, "kend": kend}
    status = 0
    if kend <= kx:
        status |= NOTHING
    if kx - D - W < 0:
        status |= WINDOW
    if not np.all(np.isfinite(decay) & (decay > 0)):
        status |= DECAY
    if kx - D - W >= 0 and not np.all(np.isfinite(h[max(kx - W - 2 * D, 0):kx])):
        status |= NONFINITE
    out["status"] = status
    if status:
        return out
    n = kend - kx
    q = np.arange(kx - D, kend + D)                                # e[i] = e_b[kx - D + i]
    v = nu(seed, q).astype(LD)
    y, err, mag = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    for b in range(NB):
        A, bA, _, _, _ = level_fit(h, kx, filt[b], decay[b], W, fs, real)
        out["gain"][b], out["gain_bound"][b] = float(A), bA
        x = -LD(delta(decay[b], fs)) * (q - kx).astype(LD)
        env = np.exp(x)
        e = A * env * v
        # the relative error of A where A > 0; where the model's A is 0 the device's may be as large as its bound
        de = np.abs(e) * ((bA / float(A) if A > 0 else 0.0) + _rx(x) + 2 * U) + (0.0 if A > 0 else bA * np.abs(env * v))
        g = filt[b].astype(LD)
        y += np.convolve(e, g)[2 * D:2 * D + n]                    # y[k] = sum_j g[j] e[(k - kx) + 2 D - j]
        err += np.convolve(de, np.abs(g))[2 * D:2 * D + n]
        mag += np.convolve(np.abs(e), np.abs(g))[2 * D:2 * D + n]
    out["y"][kx:kend] = y.astype(np.float64)
    out["y"][kend:] = 0.0
    out["bound"][kx:kend] = (err + (NB * NF + 1) * U * mag).astype(np.float64) + 2.0 ** -24 * np.abs(out["y"][kx:kend]) + 2.0 ** -150
    out["length"] = max(kx, kend)
    return out


def rir_tail(bank, length, n_taps, decay, seed, filt=None, W=480, fs=16000):
    """Rows of rir_tail_row, as a list of its dicts."""
    decay = np.asarray(decay, dtype=np.float64).reshape(len(bank), -1)
    return [rir_tail_row(bank[r], length[r], n_taps[r], decay[r], seed[r], filt, W, fs) for r in range(len(bank))]
