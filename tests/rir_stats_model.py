"""The plain-numpy statement of cmgan_rir_stats (include/cmgan_hip.h, "What a room impulse response measures as"): the
Schroeder decay curve, EDT / T20 / T30, DRR, C50 / C80, D50 and Ts of one response, broad-band and in the bands of an FIR
filterbank.  It shares no code with the kernels: every sum is in np.longdouble (64 mantissa bits on x86, its own error is
2^-11 of a float64 rounding and is left out below).  The GPU tests compare Engine.rir_stats with it, the host tests compare
it with closed forms, hand-computed responses and a naive loop.

Besides each value `rir_stats_row` returns a DERIVED BOUND on |device - model|, from the arithmetic the header prescribes
(u = 2^-53; the scheme of rir_bands_model.rir_bands_row):
  band signal  y[k] is NF fused multiply-adds in ascending j: |dy| <= by = (NF + 1) u sum_j |g[j] h[k + D - j]|; slice 0 is
               h itself, by = 0.  e = y^2: |de| <= be = (2 |y| by + by^2) (1 + u) + u y^2
  sums         any sum X of the non-negative e over a range, in whatever order: |dX| <= bX = sum be + (n + 1) u (X + sum be).
               That covers E, EDC[k], the DRR window and its outside, the early sums; Ts's numerator has the exact integer
               weights k - k0 on e and be, and (n + 2) u for the products' roundings
  log10        the device's log10 is taken as good to 64 ulps of its result, as in test_gpu_level.py: for x with relative
               error rel, |d 10 log10 x| <= 10 (1.01 rel / ln 10 + 64 u |log10 x|) + 2 u |10 log10 x|.  That is the bound of
               L[k] (rel = bEDC/EDC + bE/E + 2 u) and of DRR, C50, C80
  slope        S = sum (k - kbar) L[k]: |dS| <= bS = sum |k - kbar| bL[k] + (m + 2) u sum |(k - kbar) L[k]|, i.e. the per-sample
               bound on L times sum |k - kbar|, with m (m^2 - 1) / 12 exact; time = -60 / slope: |dT| <= |T| r / (1 - r),
               r = bS / |S| + 6 u
These are bounds, not measurements: nothing here was fitted to what the kernels give.

`guard_hits` counts the DECISIONS of the row that lie within their bound of flipping, in which case device and model may
legitimately differ by more than a rounding: every comparison EDC[k] <= c_x E at k < ka(x) and at ka(x) itself (the device
takes the smallest k that passes, so an early pass anywhere before the crossing would move it; the margin is the two sides'
bounds, bEDC[k] + c_x bE + u c_x E), the sign of each fitted slope (bS against |S|), and an exactly empty denominator whose
bound is not empty.  k0 is decided on float32 values without any arithmetic: its bound is 0, a tie falls to the first index
in device and model alike, and it never counts.  A GPU comparison is meaningful where guard_hits == 0: a condition on the
inputs, which the tests assert first."""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
P = 10
E_, K0, DRR, C50, C80, D50, TS, EDT, T20, T30 = range(P)
NONFINITE, ZERO, NO_EDT, NO_T20, NO_T30 = 1, 2, 4, 8, 16
DOWN = (0.31622776601683794, 0.1, 0.0031622776601683794, 0.00031622776601683794)     # 10^(-x/10), x = 5, 10, 25, 35: the header's literals
LN10 = math.log(10.0)


def offsets(fs, direct_ms):
    """(w, round(0.05 fs), round(0.08 fs)) with round(x) = floor(x + 1/2), the last two in whole numbers."""
    return int(math.floor(direct_ms * float(fs) / 1000.0 + 0.5)), (fs + 10) // 20, (4 * fs + 25) // 50


def band_signal(h, g):
    """(y, mag) of one band on 0 <= k < n: y[k] = sum_j g[j] h[k + D - j], mag[k] = sum_j |g[j] h[k + D - j]|, h = 0 outside."""
    n, D = len(h), (len(g) - 1) // 2
    h, g = np.asarray(h, dtype=LD), np.asarray(g, dtype=LD)
    return np.convolve(h, g)[D:D + n], np.convolve(np.abs(h), np.abs(g))[D:D + n]


def _sum_bound(X, bsum, n):
    return bsum + (n + 1) * U * (X + bsum)


def _db(x, rel):
    """(10 log10 x, its bound) for x > 0 known to the relative error rel."""
    if not (rel < 0.5):
        return float(10.0 * np.log10(x)), math.inf
    v = 10.0 * np.log10(LD(x))
    return float(v), float(10.0 * (1.01 * rel / LN10 + 64 * U * abs(np.log10(LD(x)))) + 2 * U * abs(v))


def _ratio_db(num, bnum, den, bden):
    """10 log10(num / den) with an empty denominator giving +inf: (value, bound, guard hits)."""
    if den == 0:
        return math.inf, 0.0, int(bden > 0)
    if num == 0:
        return -math.inf, 0.0, int(bnum > 0)
    v, b = _db(num / den, float(bnum / num + bden / den) + 2 * U)
    return v, b, 0


def slice_stats(y, by, k0, n, fs, w, o50, o80):
    """One slice from its band signal y and the bound by on it: (values [P], bounds [P], status, ka [4], EDC [n], bEDC [n],
    guard hits).  ka[x] = n where it does not exist."""
    y, by = np.asarray(y, dtype=LD), np.asarray(by, dtype=LD)
    e = y * y
    be = (2 * np.abs(y) * by + by * by) * (1 + U) + U * e
    edc = np.cumsum(e[::-1])[::-1]
    bedc = _sum_bound(edc, np.cumsum(be[::-1])[::-1], n)
    E, bE = edc[0], bedc[0]
    val, bnd = np.full(P, np.nan), np.zeros(P)
    ka = [n] * 4
    if not np.isfinite(float(E)):
        return val, bnd, NO_EDT | NO_T20 | NO_T30, ka, edc.astype(np.float64), bedc.astype(np.float64), 0
    if E == 0:
        val[E_] = 0.0
        return val, bnd, ZERO | NO_EDT | NO_T20 | NO_T30, ka, edc.astype(np.float64), bedc.astype(np.float64), 0
    hits = 0
    for x, c in enumerate(DOWN):
        thr, bthr = LD(c) * E, c * bE + U * c * E
        under = np.nonzero(edc <= thr)[0]
        ka[x] = int(under[0]) if under.size else n
        before = slice(1, ka[x])                                   # (the device sets EDC[0] = E: k = 0 never passes)
        hits += int(np.count_nonzero(edc[before] - thr <= bedc[before] + bthr))
        if ka[x] < n:
            hits += int(thr - edc[ka[x]] <= bedc[ka[x]] + bthr)
    status = 0
    k = np.arange(n)
    for col, bit, beg, end in ((EDT, NO_EDT, 0, ka[1]), (T20, NO_T20, ka[0], ka[2]), (T30, NO_T30, ka[0], ka[3])):
        m = end - beg
        if end >= n or m < 2:
            status |= bit
            continue
        r = edc[beg:end] / E
        L = 10.0 * np.log10(r)
        rel = (bedc[beg:end] / edc[beg:end] + bE / E + 2 * U).astype(np.float64)
        bL = 10.0 * (1.01 * rel / LN10 + 64 * U * np.abs(np.log10(r)).astype(np.float64)) + 2 * U * np.abs(L).astype(np.float64)
        bL = np.where(rel < 0.5, bL, np.inf)
        dk = (k[beg:end] - LD(0.5) * (beg + end - 1)).astype(LD)
        S = np.sum(dk * L)
        with np.errstate(invalid="ignore"):                        # (0 inf = nan: counted as a hit below)
            bS = float(np.sum(np.abs(dk).astype(np.float64) * bL)) + (m + 2) * U * float(np.sum(np.abs(dk * L)))
        if not bS < abs(float(S)):
            hits += 1                                              # the slope's sign is within reach of rounding
        slope = fs * S / (LD(m) * (LD(m) * m - 1) / 12)
        if not slope < 0:
            status |= bit
            continue
        val[col] = float(-60.0 / slope)
        rr = bS / abs(float(S)) + 6 * U
        bnd[col] = abs(val[col]) * rr / (1 - rr) if rr < 1 else math.inf
    lo, hi = max(k0 - w, 0), min(k0 + w, n - 1)
    k50, k80 = min(k0 + o50, n), min(k0 + o80, n)
    part = lambda a, b: (np.sum(e[a:b]), _sum_bound(np.sum(e[a:b]), np.sum(be[a:b]), n))
    A, bA = part(lo, hi + 1)
    (pre, bpre), (post, bpost) = part(0, lo), part(hi + 1, n)
    val[E_], bnd[E_] = float(E), float(bE)
    val[K0] = float(k0)
    val[DRR], bnd[DRR], g = _ratio_db(A, bA, pre + post, bpre + bpost + U * (pre + post))
    hits += g
    for col, kx in ((C50, k50), (C80, k80)):
        early, bearly = part(0, kx)
        late, blate = (edc[kx], bedc[kx]) if kx < n else (LD(0), LD(0))
        val[col], bnd[col], g = _ratio_db(early, bearly, late, blate)
        hits += g
        if col == C50:
            val[D50] = float(early / E)
            bnd[D50] = float(bearly / E + (early / E) * (bE / E + 2 * U))
    wt = np.maximum(k - k0, 0).astype(LD)
    num = np.sum(wt * e)
    bnum = float(np.sum(wt * be)) + (n + 2) * U * float(num + np.sum(wt * be))
    val[TS] = float(num / (fs * E))
    bnd[TS] = float(bnum / (fs * E)) + val[TS] * float(bE / E + 4 * U)
    return val, bnd, status, ka, edc.astype(np.float64), bedc.astype(np.float64), hits


def rir_stats_row(h, n=None, filt=None, fs=16000, direct_ms=2.5):
    """One row.  h: the float32 response (only h[:n] is looked at, n clamped to [1, len(h)]); filt: float64 [NB, NF] or
    None.  Returns a dict: values, bounds float64 [NB + 1, P]; status int [NB + 1]; ka int [NB + 1, 4] (n where a
    threshold index does not exist); k0; n; edc, edc_bound float64 [NB + 1, n]; guard_hits."""
    h = np.asarray(h, dtype=np.float32)
    n = len(h) if n is None else min(max(int(n), 1), len(h))
    h = h[:n]
    filt = np.zeros((0, 1)) if filt is None else np.asarray(filt, dtype=np.float64)
    NB, NF = filt.shape
    assert NF % 2 == 1
    S = NB + 1
    out = {"values": np.full((S, P), np.nan), "bounds": np.zeros((S, P)), "status": np.zeros(S, dtype=np.int64),
           "ka": np.full((S, 4), n, dtype=np.int64), "k0": 0, "n": n, "edc": np.full((S, n), np.nan),
           "edc_bound": np.zeros((S, n)), "guard_hits": 0}
    if not np.all(np.isfinite(h)):
        out["status"][:] = NONFINITE | NO_EDT | NO_T20 | NO_T30
        return out
    k0 = int(np.argmax(np.abs(h)))                                 # the first of the maxima
    out["k0"] = k0
    w, o50, o80 = offsets(fs, direct_ms)
    for s in range(S):
        if s == 0:
            y, by = h.astype(LD), np.zeros(n, dtype=LD)
        else:
            y, mag = band_signal(h, filt[s - 1])
            by = (NF + 1) * U * mag
        v, b, st, ka, edc, bedc, hits = slice_stats(y, by, k0, n, fs, w, o50, o80)
        out["values"][s], out["bounds"][s], out["status"][s], out["ka"][s] = v, b, st, ka
        out["edc"][s], out["edc_bound"][s] = edc, bedc
        out["guard_hits"] += hits
    return out


def decaying_noise(seed, n, db_per_sample=0.01, k0=0, spike=4.0):
    """The test responses, as float32: a direct spike at k0 (larger than any noise sample can be: the unique maximum),
    behind it seeded Gaussian noise whose level falls `db_per_sample` per sample, and 40 dB weaker noise before it."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    x = rng.standard_normal(n) * 0.25 * np.where(k < k0, 0.01, 10.0 ** (-db_per_sample * np.maximum(k - k0, 0) / 20.0))
    x[k0] = spike if rng.random() < 0.5 else -spike
    return x.astype(np.float32)
