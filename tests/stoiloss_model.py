"""The numpy model of the intelligibility loss (cmgan_amd/csrc/stoiloss.hip; include/cmgan_hip.h, "Intelligibility loss"),
shared by tests/test_stoiloss_host.py and tests/test_gpu_stoiloss.py.  Written from the formulas of the header; the only
thing it takes from the library is what the header defines by it: tables 2 (band edges), 3 (inner Hann) and 4 (resample_poly
taps) of cmgan_metrics_table, float64 values that every evaluation below widens as they are.

For an estimate row e and a reference row r of L samples at 16 kHz, in the header's notation: x10 = resample_poly(x, 5, 8);
frame levels of r10 read one sample early; the keep rule ((level - max) + 40) > 0; the overlap-add xs of the K kept frames;
envelope frames j < K - 1 with their 15 band envelopes; windows w < K - 30 of 30 frames; d_w as STOI (alpha, the clipped
min, the normalised correlation, sum over the bands / 15) or as ESTOI (rows, then columns, mean-removed and normalised;
sum of the products / 30); value = mean_w d_w; A_row = -k value; g = dA_row / de with r, the keep mask and all made of r
constant, the derivative of min following the selected branch (the estimate's at a tie).  A row with K < 31 has status 1,
one whose value is not finite status 2; either has value NaN, A_row = 0 and g = 0.

`evaluate` is generic in the number type and is run three ways per registered row: w in np.longdouble (scipy.fft keeps
that precision), the value a device output is judged against; d in float64 with scipy.fft; d2 in float64 with a direct DFT
product.

Acceptance rule (auxloss_model's).  Exact zeros, counts and status words are compared for EQUALITY.  A device gradient
sample g is accepted against w when |g - w| <= ulp32(w) / 2 + E with E = 8 x max(|d - w|, |d2 - w|) per row, from the model
alone.  The float64 value is held to `bound` = 8 x max(|d - w|, |d2 - w|) + 4096 u, u = 2^-53: the value is built from sums
of at most a few thousand terms of magnitude <= 1, each rounded once, on top of what the three evaluations differ by (the
device makes its own taps and window with its own cos / sin / Bessel series, an ulp from the table's).  Nothing in either
comes from device output.

MARGINS of a row, the two conditions under which a long-double model and a float64 kernel take the same branch everywhere:
`level_margin` = min over the frames of |(level - max) + 40| in dB (>= 1e-6 required), `min_margin` = min over every
(window, band, frame) of |Y alpha - X (1 + c)| / max(Y alpha, X (1 + c)) (>= 1e-9 required; inf for ESTOI, which has no
min).  A further condition keeps the rule from hiding a wrong sample: E <= 2^-10 x ulp32(rms of w) / 2.  Case (c), est == ref,
sits at the maximum of every correlation: its true gradient is 0 and every evaluation of it is rounding noise, so its E is
judged against the rms of case (a)'s gradient (the same kind of row at the same amplitude and length): `conditions(...,
scale_of=)`."""
import ctypes
from functools import lru_cache
from typing import NamedTuple

import numpy as np
import scipy.fft

from metrics_signals import speechlike
from warp_model import LD, PI_LD, ulp32

U = 2.0 ** -53
FS = 16000
N, HOP, NFFT, J, SEG = 256, 128, 512, 15, 30
UP, DOWN, PRE_REMOVE = 5, 8, 11
DYN = 40.0
MIN_L = 6554
LEVEL_MARGIN, MIN_MARGIN = 1e-6, 1e-9


@lru_cache(maxsize=None)
def tables():
    """(taps h [169], inner Hann [256], band edges [(first, end)] x 15) as the library exports them (no GPU needed)."""
    from cmgan_amd import _lib
    lib = _lib.load()
    fn = lib.cmgan_metrics_table
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]

    def table(which):
        n = fn(FS, which, None, 0)
        out = np.zeros(n)
        assert fn(FS, which, out.ctypes.data, n) == n
        return out
    edges = table(2)
    assert int(edges[0]) == J and len(edges) == 1 + 2 * J
    bands = tuple((int(edges[1 + 2 * b]), int(edges[2 + 2 * b])) for b in range(J))
    h, hann = table(4), table(3)
    assert len(h) == 169 and len(hann) == N
    return h, hann, bands


def n10_of(L):
    return -(-UP * L // DOWN)


def frames_of(L):
    return -(-(n10_of(L) - N) // HOP)


@lru_cache(maxsize=None)
def _resample_index(L):
    """(i [N10, 34], tap [N10, 34], valid): x10[n] = sum over the valid (i, tap) of x[i] h[tap], i ascending."""
    n10 = n10_of(L)
    pos = (np.arange(n10) + PRE_REMOVE) * DOWN
    i = pos[:, None] // UP - np.arange(33, -1, -1)[None, :]            # ascending in i along the row
    tap = pos[:, None] - UP * i
    ok = (i >= 0) & (i < L) & (tap >= 0) & (tap <= 168)
    return np.where(ok, i, 0), np.where(ok, tap, 0), ok


def _dft(T):
    """e^{-2 pi i k n / 512}, [257, 256], from the angle reduced exactly."""
    m = (np.arange(NFFT // 2 + 1)[:, None] * np.arange(N)[None, :]) % NFFT
    if T is LD:
        a = LD(2) * PI_LD * m.astype(LD) / LD(NFFT)
    else:
        a = 2 * np.pi * m / NFFT
    return np.cos(a), -np.sin(a)


class Eval(NamedTuple):
    value: object           # in the evaluation's precision; NaN with a status
    kept: int
    status: int
    a: object               # the row's share of the total: -k value, 0 with a status
    g: np.ndarray           # [L] dA_row / de
    level_margin: float
    min_margin: float
    clipped: float          # the share of (window, band, frame) cells where min took the clipped branch (STOI)


def evaluate(est, ref, extended, k, T=np.float64, direct=False) -> Eval:
    h64, hann64, bands = tables()
    h, hann = h64.astype(T), hann64.astype(T)
    e, r = np.asarray(est).astype(T), np.asarray(ref).astype(T)
    L = len(e)
    assert L >= MIN_L and len(r) == L
    n10, nS = n10_of(L), frames_of(L)
    ii, tap, ok = _resample_index(L)
    hm = np.where(ok, h[tap], T(0))
    e10, r10 = np.sum(e[ii] * hm, axis=1), np.sum(r[ii] * hm, axis=1)
    # the keep rule, from the reference alone
    starts = np.arange(nS) * HOP
    idx = (starts[:, None] - 1 + np.arange(N)[None, :]) % n10
    with np.errstate(divide="ignore"):
        level = T(20) * np.log10(np.sqrt(np.sum((r10[idx] * hann) ** 2, axis=1)) / T(16))
    rule = (level - np.max(level)) + T(DYN)
    keep = np.flatnonzero(rule > 0)
    level_margin = float(np.min(np.abs(rule)))
    K = len(keep)
    zero = np.zeros(L, dtype=T)
    if K < SEG + 1:
        return Eval(T(np.nan), K, 1, T(0), zero, level_margin, np.inf, 0.0)
    grab = starts[keep][:, None] + np.arange(N)[None, :]
    put = starts[:K][:, None] + np.arange(N)[None, :]
    rs, es = np.zeros((K + 1) * HOP, dtype=T), np.zeros((K + 1) * HOP, dtype=T)
    np.add.at(rs, put, r10[grab] * hann)
    np.add.at(es, put, e10[grab] * hann)
    nE = K - 1
    fidx = (np.arange(nE) * HOP)[:, None] + np.arange(N)[None, :]
    ws = np.sum(hann)
    if direct:
        C, S = _dft(T)

        def spectrum(x):
            fr = x[fidx] * hann
            return fr @ C.T + 1j * (fr @ S.T)
    else:
        def spectrum(x):
            return scipy.fft.rfft(x[fidx] * hann, NFFT, axis=1)
    Xs, Ys = spectrum(rs), spectrum(es)

    def envelopes(spec):
        p = (spec.real / ws) ** 2 + (spec.imag / ws) ** 2
        return np.stack([np.sqrt(np.sum(p[:, lo:hi], axis=1)) for lo, hi in bands])       # [15, nE]
    X, Y = envelopes(Xs), envelopes(Ys)
    nW = K - SEG
    win = np.arange(nW)[:, None] + np.arange(SEG)[None, :]
    Xw, Yw = X[:, win], Y[:, win]                                       # [15, nW, 30]
    min_margin, clipped = np.inf, 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        if not extended:
            c1 = T(1) + T(10) ** (T(15) / T(20))
            sy2 = np.sum(Yw * Yw, axis=2, keepdims=True)
            alpha = np.sqrt(np.sum(Xw * Xw, axis=2, keepdims=True) / sy2)
            ya, xc = Yw * alpha, Xw * c1
            own = ya <= xc                                              # a tie follows the estimate's branch
            yp = np.where(own, ya, xc)
            yp = np.where(np.isnan(ya) | np.isnan(xc), T(np.nan), yp)
            big = np.maximum(np.abs(ya), np.abs(xc))
            rel = np.abs(ya - xc) / big
            if np.all(np.isfinite(rel)):
                min_margin, clipped = float(np.min(rel)), float(np.mean(~own))
            xu = Xw - np.mean(Xw, axis=2, keepdims=True)
            yu = yp - np.mean(yp, axis=2, keepdims=True)
            nx, ny = np.sqrt(np.sum(xu * xu, axis=2, keepdims=True)), np.sqrt(np.sum(yu * yu, axis=2, keepdims=True))
            xn, yn = xu / nx, yu / ny
            s = np.sum(xn * yn, axis=2, keepdims=True)                  # [15, nW, 1]
            d = np.sum(s[:, :, 0], axis=0) / T(J)
            u = (xn - yn * s) / ny
            q = u - np.mean(u, axis=2, keepdims=True)
            Tq = np.sum(np.where(own, q * Yw, T(0)), axis=2, keepdims=True)
            D = (np.where(own, q * alpha, T(0)) - (alpha / sy2) * Tq * Yw) / T(J)
        else:
            def rows_then_columns(V):
                u = V - np.mean(V, axis=2, keepdims=True)
                n = np.sqrt(np.sum(u * u, axis=2, keepdims=True))
                a = u / n
                v = a - np.mean(a, axis=0, keepdims=True)
                nu = np.sqrt(np.sum(v * v, axis=0, keepdims=True))
                return a, n, v / nu, nu
            _, _, cx, _ = rows_then_columns(Xw)
            ya_, n, cy, nu = rows_then_columns(Yw)
            d = np.sum(np.sum(cx * cy, axis=0), axis=1) / T(SEG)
            dc = cx / T(SEG)
            u = (dc - cy * np.sum(cy * dc, axis=0, keepdims=True)) / nu
            da = u - np.mean(u, axis=0, keepdims=True)
            v = (da - ya_ * np.sum(ya_ * da, axis=2, keepdims=True)) / n
            D = v - np.mean(v, axis=2, keepdims=True)
        value = np.sum(d) / T(nW)
    if not np.isfinite(value):
        return Eval(T(np.nan), K, 2, T(0), zero, level_margin, min_margin, clipped)
    # 1. the windows of a frame   2. the envelope's adjoint   3. overlap-add and silence removal   4. the resampler
    gY = np.zeros((J, nE), dtype=T)
    np.add.at(gY, (np.arange(J)[:, None, None], win[None, :, :]), D)
    gY *= -T(k) / T(nW)
    G = np.zeros((nE, NFFT // 2 + 1), dtype=Ys.dtype)
    for b, (lo, hi) in enumerate(bands):
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(Y[b] == 0, T(0), gY[b] / (ws * ws * Y[b]))
        G[:, lo:hi] = c[:, None] * Ys[:, lo:hi]
    if direct:
        z = G.real @ C - G.imag @ (-S)
    else:
        assert bands[0][0] > 0 and bands[-1][1] <= NFFT // 2            # no DC, no Nyquist bin in a band
        z = scipy.fft.irfft(G * T(0.5), n=NFFT, axis=1)[:, :N] * T(NFFT)
    ges = np.zeros_like(es)
    np.add.at(ges, fidx, z * hann)
    g10 = np.zeros(n10, dtype=T)
    np.add.at(g10, grab, ges[put] * hann)
    g = np.zeros(L, dtype=T)
    np.add.at(g, ii[ok], (g10[:, None] * hm)[ok])
    return Eval(value, K, 0, -T(k) * value, g, level_margin, min_margin, clipped)


# ------------------------------------------------------------------ registered rows
_WAYS = {"w": (LD, False), "d": (np.float64, False), "d2": (np.float64, True)}
_PAIRS = {}


def register(key, est, ref):
    """Make the row (est, ref) known under `key` (hashable); the evaluations below are cached per key."""
    _PAIRS[key] = (np.asarray(est, dtype=np.float32), np.asarray(ref, dtype=np.float32))
    return key


@lru_cache(maxsize=None)
def _eval(key, extended, k, way):
    T, direct = _WAYS[way]
    return evaluate(*_PAIRS[key], extended, k, T, direct)


class RowModel(NamedTuple):
    value: object           # long double; NaN with a status
    kept: int
    status: int
    a: object               # long double: the row's share of the total
    g: np.ndarray           # long double [L]
    E: float                # the gradient's slack
    bound: float            # what a device value may be off by
    level_margin: float
    min_margin: float
    clipped: float


def row_model(key, extended, k) -> RowModel:
    w = _eval(key, bool(extended), float(k), "w")
    E = dv = 0.0
    for way in ("d", "d2"):
        x = _eval(key, bool(extended), float(k), way)
        assert (x.kept, x.status) == (w.kept, w.status), (key, way)
        E = max(E, 8.0 * float(np.max(np.abs(x.g.astype(LD) - w.g), initial=0.0)))
        if w.status == 0:
            dv = max(dv, 8.0 * float(abs(LD(x.value) - w.value)))
    return RowModel(w.value, w.kept, w.status, w.a, w.g, E, dv + 4096 * U, w.level_margin, w.min_margin, w.clipped)


def conditions(key, extended, k, scale_of=None) -> dict:
    m = row_model(key, extended, k)
    scale = m if scale_of is None else row_model(scale_of, extended, k)
    rms = float(np.sqrt(np.mean(scale.g.astype(np.float64) ** 2)))
    return {"level_margin": m.level_margin, "min_margin": m.min_margin, "E": m.E,
            "E_max": 2.0 ** -10 * float(ulp32(rms)) / 2 if rms > 0 else 0.0, "kept": m.kept, "status": m.status}


def accept(got, m: RowModel):
    """(ok, worst excess over half an ulp as a fraction of E) of a device gradient row against its model."""
    w = m.g.astype(np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - m.g).astype(np.float64)
    over = err - ulp32(w) / 2
    ok = bool(np.all(over <= m.E)) and bool(np.all(np.isfinite(got)))
    return ok, float(np.max(over, initial=0.0) / m.E) if m.E > 0 else (0.0 if ok else np.inf)


# ------------------------------------------------------------------ the six cases
L_SHORT, L_LONG = 9600, 16000
K_WEIGHT = 0.5                       # the weight the GPU cases run at (k = K_WEIGHT / 4)
#: (seed of the reference, SNR of the estimate in dB, seed of its noise) per case; the seeds were tried in order against
#: the two margins and the bound on E by the model alone (no device in the loop) and the first that met all is frozen
SEEDS = {"a": (11, 5.0, 111), "b": (12, 8.0, 112), "c": (13, None, 0), "d": (14, 10.0, 114), "e": (15, 10.0, 115),
         "f": (16, None, 0), "a16": (17, 0.0, 117)}
#: first silent 16 kHz sample of the references of (d) and (e): chosen so that exactly 31 and 30 frames are kept
CUT = {"d": 6350, "e": 6150}
GAP = (6000, 10000)                 # the 0.25 s of near-silence in the middle of (b)'s 16000 samples


def _noisy(ref, snr, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    noise = g.standard_normal(len(ref))
    noise *= np.sqrt(np.mean(ref.astype(np.float64) ** 2) / np.mean(noise ** 2)) * 10.0 ** (-snr / 20.0)
    return (ref + noise).astype(np.float32)


def _voiced(n, seed):
    """A row with no pause of its own: voiced harmonics under a slow tremolo on the recording floor of speechlike()."""
    g = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / FS
    f0 = g.uniform(100, 180) * (1 + 0.03 * np.sin(2 * np.pi * 5 * t))
    ph = 2 * np.pi * np.cumsum(f0) / FS
    s = sum(np.sin(k * ph) / k ** 1.2 for k in range(1, 25)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.1 * t + g.uniform(0, 6)))
    return s / np.max(np.abs(s)) * 9000.0 + 4.0 * g.standard_normal(n)


@lru_cache(maxsize=None)
def case(name):
    """(est, ref) float32 of a case, at int16-like amplitude."""
    seed, snr, nseed = SEEDS[name]
    if name in ("a", "c", "f"):
        L = L_SHORT if name != "f" else L_LONG
        ref = _voiced(L, seed)
    elif name == "a16":
        ref = speechlike(L_LONG, FS, seed)
    elif name == "b":
        ref = _voiced(L_LONG, seed)
        g = np.random.Generator(np.random.PCG64(seed + 500))
        ref[GAP[0]:GAP[1]] = 4.0 * g.standard_normal(GAP[1] - GAP[0])
    else:
        ref = _voiced(L_SHORT, seed)
        g = np.random.Generator(np.random.PCG64(seed + 500))
        ref[CUT[name]:] = 4.0 * g.standard_normal(L_SHORT - CUT[name])
    ref = ref.astype(np.float32)
    if name == "c":
        est = ref.copy()
    elif name == "f":
        est = np.zeros_like(ref)
    else:
        est = _noisy(ref, snr, nseed)
    return est, ref


BATCHES = {L_SHORT: ("a", "c", "d", "e"), L_LONG: ("b", "f", "a16", "b")}


def registered(name):
    return register(name, *case(name))


def batch(L):
    """(est, ref) float32 [4, L] and the cases' names."""
    names = BATCHES[L]
    return tuple(np.stack([case(n)[i] for n in names]) for i in (0, 1)) + (names,)
