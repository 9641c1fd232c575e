"""The numpy model of the auxiliary losses (cmgan_amd/csrc/auxloss.hip; include/cmgan_hip.h, "Auxiliary losses"), shared by
tests/test_auxloss_host.py and tests/test_gpu_auxloss.py.  Nothing here imports the library.

For an estimate row e and a reference row r of L float32 samples and a resolution n (hop h = n / 4, F = n / 2 + 1, T = 1 + L //
h, w[k] = 0.5 - 0.5 cos(2 pi k / n), frames centred with reflect padding of n / 2):

    X_x[t, f] = sum_k w[k] x~[t h + k] e^{-2 pi i f k / n};   m_x = sqrt(max(|X_x|^2, 1e-7)), derivative 0 below the clamp
    N = sum (m_r - m_e)^2,  D = sum m_r^2,  sc = sqrt(N) / sqrt(D) (0 with a zero derivative where N == 0)
    lm = mean |ln m_r - ln m_e| (sign(0) = 0);   MR = mean over the resolutions of (sc + lm)
    x' = x - mean x,  a = <e', r'> / (<r', r'> + 1e-8),  s = a r',  q = e' - s,  SISDR = 10 log10((<s, s> + 1e-8) / (<q, q> + 1e-8))
    A_row = k_mr MR - k_si SISDR (a term of weight 0 is left out),  g = dA_row / de, with the adjoint of the reflect padding

The gradient is written out by hand (`resolution`, `si_sdr`); tests/test_auxloss_host.py holds it against float64 autograd
through torch.stft.  Everything is evaluated three ways: w in np.longdouble (scipy.fft keeps that precision), the value a
device output is judged against; d in float64 with scipy.fft; d2 in float64 with a direct DFT product.

Acceptance rule (suppress_model's, transmit_model's).  Exact zeros and bit copies are compared for EQUALITY.  A device
gradient sample g is accepted against w when |g - w| <= ulp32(w) / 2 + E with E = 8 x max(|d - w|, |d2 - w|) per row, from
the model alone.  The float64 `rows` values are held to `value_bounds`: first-order bounds from the transform's norm-wise
error 4 (log2 n + 2) u per frame, the term counts of the sums and the conditioning of SI-SDR, u = 2^-53 - nothing in them
comes from device output.  CONDITIONS of a registered row, checked without a GPU by the host test: E <= 2^-10 x
ulp32(rms of w) / 2; no cell with 0 < |ln m_r - ln m_e| < 2^-20; no cell with |X|^2 within a factor 1 +- 2^-20 of the
clamp; SI-SDR between -20 and 40 dB."""
from functools import lru_cache
from typing import NamedTuple

import numpy as np
import scipy.fft

from transmit_model import speech
from warp_model import LD, PI_LD, ulp32

N_FFTS = (256, 512, 1024, 2048)
CLAMP, EPS = 1e-7, 1e-8
U = 2.0 ** -53
SI_TILE = 4096                      # samples per partial sum of the SI-SDR kernel
KINK, NEAR = 2.0 ** -20, 2.0 ** -20


def hann(n, T):
    k = np.arange(n)
    if T is LD:
        return LD(0.5) - LD(0.5) * np.cos(LD(2) * PI_LD * k.astype(LD) / LD(n))
    return 0.5 - 0.5 * np.cos(2 * np.pi * k / n)


def dft_matrix(n):
    """e^{-2 pi i f k / n}, float64 [F, n], from the angle reduced exactly (f k mod n)."""
    m = (np.arange(n // 2 + 1)[:, None] * np.arange(n)[None, :]) % n
    return np.cos(2 * np.pi * m / n) - 1j * np.sin(2 * np.pi * m / n)


def n_frames(L, n):
    return 1 + L // (n // 4)


class Resolution(NamedTuple):
    sc: object              # in the evaluation's precision
    lm: object
    g: np.ndarray           # [L] d(sc + lm) / de
    P_e: np.ndarray         # [T, F] |X|^2 of both signals
    P_r: np.ndarray
    dl: np.ndarray          # [T, F] ln m_r - ln m_e


def resolution(e, r, n, T=np.float64, direct=False) -> Resolution:
    """sc, lm and the hand-written gradient of their sum with respect to e, at one resolution."""
    L, h, half = len(e), n // 4, n // 2
    assert L > half
    nt = n_frames(L, n)
    src = np.pad(np.arange(L), half, mode="reflect")                    # padded position -> sample
    idx = np.arange(nt)[:, None] * h + np.arange(n)[None, :]            # [T, n] padded positions of the frames
    win = hann(n, T)
    M = dft_matrix(n) if direct else None

    def spectrum(x):
        fr = np.asarray(x).astype(T)[src][idx] * win[None, :]
        return fr @ M.T if direct else scipy.fft.rfft(fr, axis=1)

    Xe, Xr = spectrum(e), spectrum(r)
    Pe, Pr = Xe.real ** 2 + Xe.imag ** 2, Xr.real ** 2 + Xr.imag ** 2
    me, mr = np.sqrt(np.maximum(Pe, T(CLAMP))), np.sqrt(np.maximum(Pr, T(CLAMP)))
    N, D = np.sum((mr - me) ** 2), np.sum(mr ** 2)
    sc = np.sqrt(N) / np.sqrt(D) if N != 0 else T(0)
    dl = np.log(mr) - np.log(me)
    cells = T(dl.size)
    lm = np.sum(np.abs(dl)) / cells
    # d(sc + lm) / dm_e, then through m = |X| (0 below the clamp) to the one-sided spectrum
    dm = -np.sign(dl) / (cells * me)
    if N != 0:
        dm = dm + (me - mr) / (np.sqrt(N) * np.sqrt(D))
    G = np.where(Pe < T(CLAMP), T(0), dm / me) * Xe
    # d / d frame sample k = sum_f Re(G_f e^{+2 pi i f k / n}) over the F one-sided bins, each once
    if direct:
        z = G.real @ M.real - G.imag @ (-M.imag)
    else:
        H = G * T(0.5)
        H[:, 0], H[:, -1] = G[:, 0].real, G[:, -1].real
        z = scipy.fft.irfft(H, n=n, axis=1) * T(n)
    gp = np.zeros(L + n, dtype=T)
    np.add.at(gp, idx, z * win[None, :])                                # overlap-add onto the padded signal
    g = np.zeros(L, dtype=T)
    np.add.at(g, src, gp)                                               # the adjoint of the reflect padding
    return Resolution(sc, lm, g, Pe, Pr, dl)


class SiSdr(NamedTuple):
    db: object
    g: np.ndarray           # [L] dSISDR / de
    parts: tuple            # (Ee, Rr, Er, alpha, S, Q, mean_e, mean_r) for the bounds


def si_sdr(e, r, T=np.float64) -> SiSdr:
    e, r = np.asarray(e).astype(T), np.asarray(r).astype(T)
    L = T(len(e))
    mu_e, mu_r = np.sum(e) / L, np.sum(r) / L
    ec, rc = e - mu_e, r - mu_r
    Ee, Rr, Er = np.sum(ec * ec), np.sum(rc * rc), np.sum(ec * rc)
    eps = T(EPS)
    a = Er / (Rr + eps)
    q = ec - a * rc
    S, Q = a * a * Rr + eps, np.sum(q * q) + eps
    db = T(10) * np.log10(S / Q)
    k = T(10) / np.log(T(10))
    ce = -T(2) / Q
    cr = T(2) * a * Rr / ((Rr + eps) * S) + (T(2) * a / Q) * (T(1) + eps / (Rr + eps))
    return SiSdr(db, k * (ce * ec + cr * rc), (Ee, Rr, Er, a, S, Q, mu_e, mu_r))


# ------------------------------------------------------------------ registered rows
LENGTHS = (1100, 1700, 3200)        # just above the 2048 window's reflect limit | a multiple of no hop | plain
N_FFT_SETS = ((256,), (2048,), (512, 1024, 2048), (256, 512, 1024, 2048))
B = 3
W_MR, W_SI = 1.0, 0.05
WEIGHTS = ((W_MR, 0.0), (0.0, W_SI), (W_MR, W_SI))
#: (kind, SNR in dB) of the three rows of a batch
ROWS = (("speech", 20.0), ("gauss", 5.0), ("speech", -3.0))


#: the draw of every registered row: the first few seeds 100 L + b + 1000 t were tried in order of t against the CONDITIONS
#: above (the model's own, no device in the loop), and the one with the most room under the bound on E is kept
DRAW = {(1100, 0): 2, (1100, 1): 1, (1100, 2): 0, (1700, 0): 5, (1700, 1): 4, (1700, 2): 2, (3200, 0): 1, (3200, 1): 1,
        (3200, 2): 2}


@lru_cache(maxsize=None)
def pair(L, b):
    """(est, ref) float32 [L] of row b: est = ref + white noise at the row's SNR."""
    kind, snr = ROWS[b]
    seed = 100 * L + b + 1000 * DRAW[(L, b)]
    rng = np.random.default_rng(seed)
    ref = speech(seed % 97, L) if kind == "speech" else (0.1 * rng.standard_normal(L)).astype(np.float32)
    noise = rng.standard_normal(L)
    noise *= np.sqrt(np.mean(ref.astype(np.float64) ** 2) / np.mean(noise ** 2)) * 10.0 ** (-snr / 20.0)
    return (ref + noise).astype(np.float32), ref


def batch(L):
    """(est, ref) float32 [B, L]."""
    return tuple(np.stack([pair(L, b)[i] for b in range(B)]) for i in (0, 1))


_WAYS = {"w": (LD, False), "d": (np.float64, False), "d2": (np.float64, True)}


@lru_cache(maxsize=None)
def _res(key, n, way):
    T, direct = _WAYS[way]
    return resolution(*_PAIRS[key], n, T, direct)


@lru_cache(maxsize=None)
def _si(key, way):
    return si_sdr(*_PAIRS[key], _WAYS[way][0])


_PAIRS = {}


def register(key, est, ref):
    """Make the row (est, ref) known under `key` (hashable); the evaluations below are cached per key."""
    _PAIRS[key] = (np.asarray(est, dtype=np.float32), np.asarray(ref, dtype=np.float32))
    return key


def registered(L, b):
    return register((L, b), *pair(L, b))


class RowModel(NamedTuple):
    rows: np.ndarray        # long double [2 R + 1]: (sc, lm) per resolution, SI-SDR
    a: object               # long double: the row's share of the total (and its two parts)
    a_mr: object
    a_si: object
    g: np.ndarray           # long double [L]
    E: float                # the gradient's slack 8 x max(|d - w|, |d2 - w|)
    bounds: np.ndarray      # float64 [2 R + 1]: what a device value of `rows` may be off by


def _combine(key, n_ffts, k_mr, k_si, way):
    T = _WAYS[way][0]
    R = len(n_ffts)
    res = [_res(key, n, way) for n in n_ffts]
    si = _si(key, way)
    L = len(_PAIRS[key][0])
    g = np.zeros(L, dtype=T)
    a_mr = a_si = T(0)
    if k_mr != 0:
        for x in res:
            g = g + (T(k_mr) / T(R)) * x.g
        a_mr = T(k_mr) * (sum((x.sc + x.lm for x in res), T(0)) / T(R))
    if k_si != 0:
        g = g - T(k_si) * si.g
        a_si = -T(k_si) * si.db
    rows = np.array([v for x in res for v in (x.sc, x.lm)] + [si.db], dtype=T)
    return rows, a_mr, a_si, g


def row_model(key, n_ffts, k_mr, k_si) -> RowModel:
    rows, a_mr, a_si, w = _combine(key, n_ffts, k_mr, k_si, "w")
    E = 0.0
    for way in ("d", "d2"):
        g = _combine(key, n_ffts, k_mr, k_si, way)[3]
        E = max(E, 8.0 * float(np.max(np.abs(g.astype(LD) - w), initial=0.0)))
    return RowModel(rows, a_mr + a_si, a_mr, a_si, w, E, value_bounds(key, n_ffts))


def value_bounds(key, n_ffts) -> np.ndarray:
    """What a float64 evaluation by radix-2 transforms and blocked sums may be off by, per entry of `rows`; from the long
    double evaluation alone.  Per frame the transform of a windowed frame is off by at most gam u ||X_t||_2 in any bin (the
    norm-wise bound of log2 n butterfly stages, window and twiddles included), gam = 4 (log2 n + 2); m = |X| moves by no more,
    and not at all below the clamp (condition: no cell near it).  A sum of K non-negative terms in blocks is off by (16 +
    T) u, relatively (at most 5 cells a thread, 8 tree levels, T frames in sequence)."""
    est, ref = _PAIRS[key]
    L = len(est)
    out = []
    for n in n_ffts:
        x = _res(key, n, "w")
        Pe, Pr = x.P_e.astype(np.float64), x.P_r.astype(np.float64)
        nt, F = Pe.shape
        gam = 4.0 * (np.log2(n) + 2.0) * U
        # ||X_t||_2 over all n bins from the one-sided ones
        de = gam * np.sqrt(2.0 * Pe.sum(axis=1))[:, None] * (Pe >= CLAMP)
        dr = gam * np.sqrt(2.0 * Pr.sum(axis=1))[:, None] * (Pr >= CLAMP)
        me, mr = np.sqrt(np.maximum(Pe, CLAMP)), np.sqrt(np.maximum(Pr, CLAMP))
        de, dr = de + 2 * U * me, dr + 2 * U * mr                       # the square root and the sum of squares under it
        D = float(np.sum(mr ** 2))
        delta = float(np.sqrt(np.sum((de + dr) ** 2)))                  # of sqrt(N), and more than sqrt(D)'s
        sums = (16.0 + nt) * U
        sc, lm = float(x.sc), float(x.lm)
        out.append((1.0 + sc) * delta / np.sqrt(D) + (sums + 8 * U) * sc)
        per_cell = de / me + dr / mr + 4 * U * (np.abs(np.log(me)) + np.abs(np.log(mr)))
        out.append(float(np.mean(per_cell)) + (sums + 8 * U) * lm)
    Ee, Rr, Er, a, S, Q, mu_e, mu_r = (float(v) for v in _si(key, "w").parts)
    e64, r64 = est.astype(np.float64), ref.astype(np.float64)
    See, Srr = float(np.sum(e64 * e64)), float(np.sum(r64 * r64))
    cs = (32.0 + -(-L // SI_TILE)) * U                                  # 16 samples a thread, 8 tree levels, the tiles
    dE, dR, dX = 4 * cs * See, 4 * cs * Srr, 4 * cs * np.sqrt(See * Srr)        # the centred sums, from the raw ones
    da = (dX + abs(a) * dR) / (Rr + EPS) + 2 * U * abs(a)
    ss = a * a * Rr
    dss = 2 * abs(a) * Rr * da + a * a * dR + 4 * U * ss
    dqq = dE + 2 * abs(a) * dX + 2 * abs(Er) * da + dss + 4 * U * (Ee + 2 * abs(a * Er) + ss)
    k = 10.0 / np.log(10.0)
    db = k * (np.log(S) - np.log(Q))
    out.append(k * (dss / S + dqq / Q) + k * 4 * U * (abs(np.log(S)) + abs(np.log(Q))) + 4 * U * abs(db))
    return np.array(out)


def conditions(key, n_ffts, k_mr, k_si) -> dict:
    """The four conditions of a registered row, as numbers the host test asserts on."""
    m = row_model(key, n_ffts, k_mr, k_si)
    rms = float(np.sqrt(np.mean(m.g.astype(np.float64) ** 2)))
    kink, near = False, False
    for n in n_ffts:
        x = _res(key, n, "w")
        a = np.abs(x.dl.astype(np.float64))
        kink |= bool(np.any((a > 0) & (a < KINK)))
        for P in (x.P_e, x.P_r):
            ratio = P.astype(np.float64) / CLAMP
            near |= bool(np.any((ratio > 1 - NEAR) & (ratio < 1 + NEAR)))
    return {"E": m.E, "E_max": 2.0 ** -10 * float(ulp32(rms)) / 2, "kink": kink, "near_clamp": near, "si_sdr": float(m.rows[-1])}


def accept(got, m: RowModel):
    """(ok, worst excess over half an ulp as a fraction of E) of a device gradient row against its model."""
    w = m.g.astype(np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - m.g).astype(np.float64)
    over = err - ulp32(w) / 2
    ok = bool(np.all(over <= m.E)) and bool(np.all(np.isfinite(got)))
    return ok, float(np.max(over, initial=0.0) / m.E) if m.E > 0 else (0.0 if ok else np.inf)
