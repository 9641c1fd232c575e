"""Float64 statement of the active speech level that cmgan_speech_level computes (include/cmgan_hip.h, "Active speech
level"): the level meter of ITU-T P.56, method B, as its published description gives it.  It shares no code with the
kernels: the envelope is the sample-by-sample recurrence in plain Python floats, the activity counts come from the
index of the last crossing, the selection is the closed form of the header.

    g   = exp(-1 / (0.03 fs))              I = ceil(0.2 fs)              c_j = 2^(j-15), j = 0..14
    p_i = g p_{i-1} + (1-g) |x_i|,  q_i = g q_{i-1} + (1-g) p_i,          p_{-1} = q_{-1} = 0
    a_j = #{ i < n : q_i' >= c_j for some i' in [i-I, i] }
    sq  = sum x_i^2,  ms = sq / n,  A_j = 10 log10(sq / a_j),  D_j = A_j - 20 log10(c_j),  M = 15.9
    A*  = A_0 if D_0 <= M; else A_{j-1} + t (A_j - A_{j-1}), t = (D_{j-1} - M) / (D_{j-1} - D_j), at the first j < J with
          D_j <= M; else A_{J-1}                                           (J = #{ j : a_j > 0 })
    active_ms = 10^(A* / 10),  activity = ms / active_ms

The guard.  A threshold decision q_i >= c_j is the one place where a rounding error could change an integer, so the
comparison tests only use inputs on which no decision is within reach of rounding: guard_hits(...) == 0, with

    delta = max(2^-40, 12 / (1 - g) * 2^-53) * max|x|.

Where the second term comes from (u = 2^-53, X = max|x|, so p, q <= X).  One step of p = g p + (1-g)|x| rounds at most
three times, each by at most u X, and an error made at a step decays by g per later step: the sequential loop's p is
within 3 u X / (1-g) of the exact recurrence, and its q - which takes p's error over with gain (1-g) / (1-g) = 1 and adds as
much of its own - within 6 u X / (1-g).  The kernels use fma (two roundings a step: 2 u X / (1-g) for p, 4 u X / (1-g) for
q), and their g = exp(-1 / (0.03 fs)) may differ from this file's by an ulp: the gain at DC stays exactly 1, the transient
moves by at most u X / (1-g) in p and 2 u X / (1-g) in q.  On top of that the tile form rounds where the sequential loop
does not: a thread's run of samples from zero state, eight composition steps of the in-tile scan, eight of the tile fold
and the two entry states, each a few roundings of at most u X with coefficients g^m = exp(-m / (0.03 fs)) that are good
to (2 + m / (0.03 fs)) u - under 64 u X in all, because none of these is amplified: every later step only decays it.
Sum: (6 + 4 + 2) u X / (1-g) + 64 u X.  At fs = 16000, 1 / (1-g) = 480.5 and the sum is 5.8e3 u X = 6.5e-13 X, inside
2^-40 X = 9.1e-13 X; at 8000 it is half that.  Above about 22 kHz the derived term is the larger one and widens the guard.
"""
import math

import numpy as np

N_THRESHOLDS = 15
THRESHOLDS = np.array([2.0 ** (j - 15) for j in range(N_THRESHOLDS)])
MARGIN_DB = 15.9
U64 = 2.0 ** -53


def constants(fs):
    """(g, I) of the definition."""
    return math.exp(-1.0 / (0.03 * fs)), -(-int(fs) // 5)


def envelope(x, fs):
    """q of the definition for every sample of x: the two one-pole smoothers in sequence, float64."""
    g, _ = constants(fs)
    omg = 1.0 - g
    q = np.empty(len(x))
    p_prev = q_prev = 0.0
    for i, v in enumerate(np.abs(np.asarray(x, dtype=np.float64)).tolist()):
        p_prev = g * p_prev + omg * v
        q_prev = g * q_prev + omg * p_prev
        q[i] = q_prev
    return q


def activity_counts(q, fs):
    """a_0 .. a_14 of an envelope: sample i is active for threshold j when the last crossing at or before i is at most
    I samples back."""
    _, hang = constants(fs)
    n = len(q)
    idx = np.arange(n)
    a = np.zeros(N_THRESHOLDS, dtype=np.int64)
    for j, c in enumerate(THRESHOLDS):
        last = np.maximum.accumulate(np.where(q >= c, idx, -(hang + 1) * 2))
        a[j] = int(np.count_nonzero(idx - last <= hang))
    return a


def select(sq, a, n):
    """(ms, active_ms, activity) from the sum of squares, the counts and the length."""
    if n == 0:
        return 0.0, 0.0, 0.0
    if not math.isfinite(sq):
        return math.nan, math.nan, math.nan
    J = int(np.count_nonzero(np.asarray(a) > 0))
    if sq == 0.0 or J == 0:
        return 0.0, 0.0, 0.0
    A = [10.0 * math.log10(sq / float(a[j])) for j in range(J)]
    D = [A[j] - 20.0 * math.log10(THRESHOLDS[j]) for j in range(J)]
    star = A[J - 1]
    if D[0] <= MARGIN_DB:
        star = A[0]
    else:
        for j in range(1, J):
            if D[j] <= MARGIN_DB:
                t = (D[j - 1] - MARGIN_DB) / (D[j - 1] - D[j])
                star = A[j - 1] + t * (A[j] - A[j - 1])
                break
    ms = sq / n
    active = 10.0 ** (star / 10.0)
    return ms, active, ms / active


def level(x, n, fs):
    """-> (ms, active_ms, activity, counts int64 [16] = a_0 .. a_14 and n, q float64 [n]) of the first n samples of x."""
    n = min(max(int(n), 0), len(x))
    x = np.asarray(x[:n], dtype=np.float64)
    q = envelope(x, fs)
    a = activity_counts(q, fs)
    with np.errstate(over="ignore", invalid="ignore"):
        sq = float(np.sum(x * x))
    ms, active, frac = select(sq, a, n)
    return ms, active, frac, np.concatenate([a, [n]]).astype(np.int64), q


def guard_delta(fs):
    """delta / max|x| (the derivation is in this file's docstring)."""
    g, _ = constants(fs)
    return max(2.0 ** -40, 12.0 / (1.0 - g) * U64)


def guard_hits(q, x, counts, fs=16000):
    """The number of (i, j), i < n = counts[15], with |q_i - c_j| <= delta: threshold decisions within reach of rounding."""
    n = int(counts[N_THRESHOLDS])
    if n == 0:
        return 0
    delta = guard_delta(fs) * float(np.max(np.abs(np.asarray(x[:n], dtype=np.float64))))
    q = np.asarray(q[:n], dtype=np.float64)
    return int(sum(np.count_nonzero(np.abs(q - c) <= delta) for c in THRESHOLDS))


def tolerance(n):
    """Relative bound on ms, active_ms and activity: n roundings of the sum plus 64 ulps for the device's log10 / pow."""
    return (n + 64) * U64


def bursts(seed, L, peak=0.4, fs=16000):
    """Seeded Gaussian bursts: stretches of noise at levels that spread over the thresholds, with pauses between them."""
    rng = np.random.default_rng(seed)
    x = np.zeros(L)
    i = 0
    while i < L:
        m = int(rng.integers(fs // 100, fs // 16))
        amp = 10.0 ** (-float(rng.uniform(0.0, 3.5))) if rng.random() < 0.7 else 0.0
        seg = rng.standard_normal(min(m, L - i)) * amp * 0.3
        x[i:i + m] = seg
        i += m
    x = np.clip(x, -1.0, 1.0)
    top = float(np.max(np.abs(x)))
    if top > 0.0:
        x *= peak / top
    return x.astype(np.float32)
