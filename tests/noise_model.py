"""The plain-numpy statement of cmgan_noise (include/cmgan_hip.h, "Synthetic noise"), in float64 and in long double, and
the rows the GPU tests use.  It shares no code with the kernels: Philox is numpy's integer arithmetic (the constants and the
round of tests/rir_tail_model.py, with all four counter words), the sums are plain loops over the taps.

What is EXACT in the model and on the device alike, and therefore the same float64 in both of the model's precisions:
  nu[q]   an integer below 2^34 divided once, IEEE's division, by one float64 literal
  imp[q]  an integer divided by 2^31 (exact), times the amplitude (one rounding); e[q] = nu[q] + imp[q] (one rounding)
  x       fma(nu_m, (double)n, phi_m): ONE rounding of the exact value.  numpy has no fma and the product has up to 94
          significant bits, so the model takes the exact rational (fractions.Fraction) and rounds it once; at n near 2^40
          a product rounded on its own would be off by 2^-13 cycles.  frac(x) = x - floor(x) and 2 frac are exact.
What is ROUNDED differently by the two precisions, and by the device (one fma where the float64 model rounds a product and a
sum): the NF terms of s, the envelope's difference, quotient and interpolation, sinpi, the tones' sum, and g s + t.

Acceptance, the rule of the channel and dynamics tests: a GPU sample g is accepted against the float64 model's w when
|g - w| <= ulp32(w) / 2 + E, with E = 8 max|model64 - model_ld| over the row (`case_model`, from the model alone) plus CAP = 2^-40
times the sum of the row's tone amplitudes for the device's sinpi.  CAP is a cap, not a measurement: it is eleven binary
orders above any plausible double-precision sinpi error and fifteen below what a phase off by one sample does at 50 Hz.
The host tests assert for every row below that the measured part of E is under 2^-20 ulp32 of the row's peak."""
import functools
from fractions import Fraction

import numpy as np

import rir_tail_model as T

LD = np.longdouble
NOISE_DIV = T.NOISE_DIV
TILE, MAX_FILTER, MAX_TONES, MAX_POINTS, MAX_INDEX = 256, 1023, 8, 4096, 2 ** 40
CAP = 2.0 ** -40
PI_LD = LD(4) * np.arctan(LD(1))


def philox4x32_10(c, seed):
    """numpy Philox4x32-10 at the counter words c = (c0, c1, c2, c3) (arrays or ints) under the 64-bit key `seed`: four
    uint64 arrays that hold the block's 32-bit words."""
    M0, M1, W0, W1, LO, S = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85, np.uint64(0xffffffff), np.uint64(32)
    shape = np.broadcast(*c).shape
    c = [np.broadcast_to(np.asarray(w).astype(np.uint64), shape) for w in c]
    seed = int(seed) & 0xffffffffffffffff
    k0, k1 = seed & 0xffffffff, seed >> 32
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S) ^ c[1] ^ np.uint64(k0), p1 & LO, (p0 >> S) ^ c[3] ^ np.uint64(k1), p0 & LO]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return c


def _words(q):
    q = np.maximum(np.asarray(q, dtype=np.int64), 0).astype(np.uint64)
    return q & np.uint64(0xffffffff), q >> np.uint64(32)


def nu(seed, q):
    """nu[q], float64, for an int64 array q: 0 where q < 0."""
    q = np.asarray(q, dtype=np.int64)
    lo, hi = _words(q)
    w = philox4x32_10((lo, hi, 0, 0), seed)
    total = (w[0] + w[1] + w[2] + w[3]).astype(np.int64) - 2 * (2 ** 32 - 1)
    return np.where(q >= 0, total.astype(np.float64) / NOISE_DIV, 0.0)


def excitation(seed, q, imp=None):
    """e[q] = nu[q] + imp[q], float64; imp = (thr, amp) or None."""
    q = np.asarray(q, dtype=np.int64)
    e = nu(seed, q)
    if imp is None or int(imp[0]) == 0:
        return e
    lo, hi = _words(q)
    v = philox4x32_10((lo, hi, 1, 0), seed)
    unit = (v[1].astype(np.int64) - 2 ** 31).astype(np.float64) / 2.0 ** 31
    click = np.where(v[0] < np.uint64(int(imp[0])), np.float64(imp[1]) * unit, 0.0)
    return np.where(q >= 0, e + click, 0.0)


def _sinpi(y, real):
    """sin(pi y) for y in [0, 2), reduced exactly to |z| <= 1/2 first."""
    y = np.asarray(y, dtype=np.float64)
    z = np.where(y <= 0.5, y, np.where(y <= 1.5, 1.0 - y, y - 2.0))
    return np.sin((np.pi if real is np.float64 else PI_LD) * z.astype(real))


def phase(nu_m, phi, n):
    """frac(fma(nu_m, n, phi)) for the int array n, float64: the exact value rounded once, then x - floor(x)."""
    a, b = Fraction(float(nu_m)), Fraction(float(phi))
    x = np.array([float(a * int(k) + b) for k in n], dtype=np.float64)
    return x - np.floor(x)


def invalid(row, K, M):
    """Whether the kernels must refuse the row (status 1, K zeros)."""
    n_tones = row["n_tones"]
    if not 0 <= row["len"] <= K or not 0 <= n_tones <= M or row["start"] < 0 or row["start"] + K > MAX_INDEX:
        return True
    if not np.all(np.isfinite(row["fir"])) or (row["env"] is not None and not np.all(np.isfinite(row["env"]))):
        return True
    t = row["tones"][:n_tones] if row["tones"] is not None else np.zeros((0, 3))
    if not np.all(np.isfinite(t)) or np.any(t[:, 0] < 0.0) or np.any(t[:, 0] > 0.5):
        return True
    if row["imp"] is not None:
        thr, amp = row["imp"]
        if not (np.isfinite(thr) and np.isfinite(amp) and 0.0 <= thr < 2.0 ** 32 and thr == np.floor(thr)):
            return True
    return False


def row_model(row, H, real=np.float64, first=0, count=None):
    """Samples first .. first + count - 1 (default: all len) of a VALID row before their rounding to float32, in `real`."""
    n_len = row["len"] - first if count is None else count
    fir = np.asarray(row["fir"], dtype=np.float64)
    NF = len(fir)
    n = row["start"] + first + np.arange(n_len, dtype=np.int64)
    if n_len == 0:
        return np.zeros(0, dtype=real)
    e = excitation(row["seed"], np.arange(n[0] - (NF - 1), n[-1] + 1, dtype=np.int64), row["imp"]).astype(real)
    s = np.zeros(n_len, dtype=real)
    for j in range(NF):                                            # e[n - j] = e_arr[k + NF - 1 - j]
        s = s + real(fir[j]) * e[NF - 1 - j:NF - 1 - j + n_len]
    g = real(1.0)
    if row["env"] is not None:
        env = np.asarray(row["env"], dtype=np.float64)
        P = len(env)
        p0 = np.minimum(n // H, P - 1)
        p1 = np.minimum(p0 + 1, P - 1)
        frac = (n - p0 * H).astype(real) / real(H)
        g = (env[p1].astype(real) - env[p0].astype(real)) * frac + env[p0].astype(real)
    t = np.zeros(n_len, dtype=real)
    if row["tones"] is not None:
        for nu_m, amp, phi in np.asarray(row["tones"], dtype=np.float64)[:row["n_tones"]]:
            t = t + real(amp) * _sinpi(2.0 * phase(nu_m, phi, n), real)
    return g * s + t


@functools.lru_cache(maxsize=None)
def case_model(name):
    """`model_of` the case `name`: computed once, shared, read-only."""
    return model_of(get(name))


def model_of(c):
    """Per row of the case: (w float64 [K] - what the device's float32 row is compared with, zeros past len and for an
    invalid row - the measured E, CAP x the tones' amplitudes, status)."""
    out = []
    for row in rows_of(c):
        w = np.zeros(c["K"])
        if invalid(row, c["K"], c["M"]):
            out.append((w, 0.0, 0.0, 1))
            continue
        m64, mld = row_model(row, c["H"]), row_model(row, c["H"], LD)
        w[:row["len"]] = m64
        E = 8.0 * float(np.max(np.abs(m64.astype(LD) - mld), initial=0.0))
        cap = CAP * float(np.sum(np.abs(row["tones"][:row["n_tones"], 1]))) if row["tones"] is not None else 0.0
        w.setflags(write=False)
        out.append((w, E, cap, 0))
    return out


@functools.lru_cache(maxsize=None)
def get(name):
    """The case `name`, built once; its arrays are shared and read-only."""
    c = CASES[name]()
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def ulp32(w):
    """The float32 spacing at |w| (w float64): 2^(e - 24) for |w| in [2^(e-1), 2^e), at least the denormal 2^-149."""
    w = np.abs(np.asarray(w, dtype=np.float64))
    _, e = np.frexp(w)
    return np.where(w == 0.0, 2.0 ** -149, np.ldexp(1.0, np.maximum(e - 24, -149)))


def excess(g, w, E):
    """The worst |g - w| - ulp32(w) / 2 - E over a row (accepted when <= 0).  g float32, w float64."""
    return float(np.max(np.abs(np.asarray(g, dtype=np.float64) - w) - 0.5 * ulp32(w) - E, initial=-np.inf))


# ------------------------------------------------------------------ the rows of the GPU tests
def rows_of(c):
    """The case's rows as dicts of their own table entries (len and start filled in where the case leaves them out)."""
    N = len(c["seed"])
    pick = lambda key, r: None if c[key] is None else np.asarray(c[key][r])
    return [dict(seed=int(c["seed"][r]), start=0 if c["start"] is None else int(c["start"][r]),
                 len=c["K"] if c["len"] is None else int(c["len"][r]), fir=np.asarray(c["fir"][r]), env=pick("env", r),
                 tones=pick("tones", r), n_tones=(c["M"] if c["n_tones"] is None else int(c["n_tones"][r])) if c["tones"] is not None else 0,
                 imp=pick("imp", r)) for r in range(N)]


def colour(rng, N, NF):
    """N random filters of NF taps with sum h^2 = 1 (decaying taps, so that the rows are coloured)."""
    h = rng.standard_normal((N, NF)) * np.exp(-np.arange(NF) / max(NF / 4.0, 1.0))[None, :]
    return h / np.sqrt((h * h).sum(axis=1, keepdims=True))


def case(seed, K, fir, start=None, length=None, env=None, H=0, tones=None, n_tones=None, imp=None):
    f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    c = dict(seed=np.ascontiguousarray(seed, dtype=np.int64), K=int(K), fir=f64(fir),
             start=None if start is None else np.ascontiguousarray(start, dtype=np.int64),
             len=None if length is None else np.ascontiguousarray(length, dtype=np.int32), env=f64(env), H=int(H),
             tones=f64(tones), n_tones=None if n_tones is None else np.ascontiguousarray(n_tones, dtype=np.int32), imp=f64(imp))
    c["M"] = 0 if tones is None else c["tones"].shape[1]
    c["NF"], c["P"] = c["fir"].shape[1], 0 if env is None else c["env"].shape[1]
    return c


EDGES = (0, 1, 255, 256, 257, 513)
FILTERS = (1, 2, 9, 1023)
HOPS = {1: 100, 7: 50, 256: 3, 5000: 2}                           # H -> P; 600 samples outlast every (P - 1) H but the last


def _seeds(rng, N):
    return rng.integers(-2 ** 63, 2 ** 63 - 1, N, dtype=np.int64)


def _edge(K):
    rng = np.random.default_rng(100 + K)
    lens = [n for n in EDGES if n <= K]
    return case(_seeds(rng, len(lens)), K, colour(rng, len(lens), 9), length=lens)


def _filter(NF):
    rng = np.random.default_rng(200 + NF)
    return case(_seeds(rng, 3), 513, colour(rng, 3, NF), start=[0, 1, 300])


def _far():
    """The counter's word boundary inside a tile, and the last index there is; envelope, tones and clicks ride along."""
    rng = np.random.default_rng(300)
    K = 300
    tones = np.array([[[50.0 / 16000.0, 0.3, 0.25], [0.5, 0.1, 0.0]]] * 2)
    return case(_seeds(rng, 2), K, colour(rng, 2, 9), start=[2 ** 32 - 100, 2 ** 40 - K], env=[[0.5, 1.5, 0.75]] * 2, H=5000,
                tones=tones, imp=[[2.0 ** 29, 4.0]] * 2)


def _hop(H):
    rng = np.random.default_rng(400 + H)
    P = HOPS[H]
    return case(_seeds(rng, 2), 600, colour(rng, 2, 9), start=[0, 3], env=0.25 + rng.random((2, P)) * 2.0, H=H)


def _one_point():
    rng = np.random.default_rng(450)
    return case(_seeds(rng, 2), 300, colour(rng, 2, 2), env=[[0.5], [2.0]], H=7)


def _tones():
    """n_tones 0 and 8; nu 0, 0.5 and 50 / 16000; phases that make frac cross 1, negative and large; unused columns NaN."""
    rng = np.random.default_rng(500)
    M, nan = 8, np.nan
    t = np.full((4, M, 3), nan)
    t[1] = [[0.0, 0.2, 0.25], [0.5, 0.3, 0.25], [50.0 / 16000.0, 0.5, 0.999], [50.0 / 16000.0, 0.4, -0.3], [0.123, 0.1, 12345.678],
            [0.25, 0.1, 0.75], [0.499, 0.2, 0.9999999], [1e-9, 1.0, 1.0 - 2.0 ** -53]]
    t[2, :2] = [[60.0 / 16000.0, 0.7, 0.5], [120.0 / 16000.0, 0.35, 0.9]]
    t[3, :1] = [[0.5, 1.0, 0.25]]
    return case(_seeds(rng, 4), 513, colour(rng, 4, 9), start=[0, 300, 0, 7], tones=t, n_tones=[0, 8, 2, 1])


def _clicks():
    rng = np.random.default_rng(600)
    thr = [0.0, 1.0, 2.0 ** 31, 2.0 ** 32 - 1.0, 2.0 ** 26]
    return case(_seeds(rng, 5), 513, colour(rng, 5, 9), start=[0, 0, 5, 0, 300], imp=[[v, 8.0] for v in thr])


def _whole():
    """One row of 1000 samples with everything on: the chunking case."""
    rng = np.random.default_rng(700)
    return case(_seeds(rng, 1), 1000, colour(rng, 1, 63), env=0.5 + rng.random((1, 6)), H=256,
                tones=[[[50.0 / 16000.0, 0.3, 0.1], [100.0 / 16000.0, 0.15, 0.6]]], imp=[[2.0 ** 27, 6.0]])


def _mixed():
    """Three rows with everything on and lengths of their own: the rows of the invariance and invalid-row tests."""
    rng = np.random.default_rng(800)
    t = np.array([[[50.0 / 16000.0, 0.3, 0.1], [0.25, 0.1, 0.4]], [[60.0 / 16000.0, 0.2, 0.7], [0.4, 0.1, 0.2]],
                  [[0.01, 0.5, 0.0], [0.02, 0.25, 0.5]]])
    return case(_seeds(rng, 3), 300, colour(rng, 3, 9), start=[0, 40, 1000], length=[300, 257, 100], env=0.5 + rng.random((3, 4)),
                H=100, tones=t, n_tones=[2, 1, 2], imp=[[2.0 ** 28, 5.0], [0.0, 1.0], [2.0 ** 30, 3.0]])


CASES = {**{f"edge-{K}": functools.partial(_edge, K) for K in EDGES},
         **{f"filter-{NF}": functools.partial(_filter, NF) for NF in FILTERS},
         **{f"hop-{H}": functools.partial(_hop, H) for H in HOPS},
         "far": _far, "one-point": _one_point, "tones": _tones, "clicks": _clicks, "whole": _whole, "mixed": _mixed}
