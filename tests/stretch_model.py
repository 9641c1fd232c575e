"""The numpy model of the tempo perturbation (cmgan_amd/csrc/stretch.hip; include/cmgan_hip.h, "Tempo perturbation"), shared
by tests/test_stretch_host.py and tests/test_gpu_stretch.py.  Nothing here imports the library.

WSOLA.  For a row x with n float32 samples (x reads as 0 outside [0, n)), a rate r (input time per output time), a hop H
and a search range D:

    M   = #{i >= 0 : fl(i r) < n}  (warp_model.count; the kernel takes min(N, M)),   K = ceil(M / H) frames
    p_k = floor(fl((k H) r)),   q_0 = c_0 = 0,   c_k = q_{k-1} + H
    q_k = c_k                          if |c_k - p_k| <= D and 0 <= c_k < n (no search)
        = p_k + d, |d| <= D, 0 <= p_k + d < n, with the largest score s(d) = 2 C - E otherwise,
          C = sum_i x[q + i] x[c_k + i], E = sum_i x[q + i]^2: float64 sums in ascending i; a NaN score counts as -inf;
          among equal maxima the earliest of d = 0, -1, +1, -2, +2, ... wins
    f[i] = 0.5 - 0.5 cospi(i / H),  g[i] = fl(1 - f[i]),   y[k H + i] = f[i] x[q_k + i] + g[i] x[c_k + i]   (k H + i < M)

positions        the definition: (q [K], c [K], searched [K] bool) with SEQUENTIAL ascending sums (np.cumsum(...)[-1]; np.sum
                 would add pairwise).  A product of two float32 values is exact in float64, so these are the sums the kernel's
                 fused multiply-adds make, bit for bit, and q is compared with the kernel's for EQUALITY.
positions_brute  the same in plain Python loops (short rows).
direct           the cross-fade in float64 from given positions, before the rounding to float32.
direct_ld        the same in np.longdouble from the same float64 f, g and positions: the value w a device sample is judged
                 against.

Acceptance rule for samples (warp_model's, the channel's).  A device sample g is accepted against w = direct_ld when
|g - w| <= ulp32(w) / 2 + E, with E = 8 x max |direct - w| per row from the model alone (`slack`); the factor 8 covers the
FMA contraction of the device build and the device's own cospi.  CONDITION: a row may be used only if
E <= 2^-10 x ulp32(rms of w) / 2 (`condition`), so that the rule cannot hide a wrong sample.  Positions, out_len, searched
and status are compared for equality."""
import math
from typing import NamedTuple

import numpy as np

from warp_model import LD, MAX_RATE, MIN_RATE, condition, cospi, count, excess, ulp32, valid   # noqa: F401 (re-exported)

HOP, SEARCH = 256, 160       # the defaults of Engine.stretch
H_S, D_S = 32, 20            # the small frames most rows use: the model stays fast


# ------------------------------------------------------------------ the definition
def seg(x, n, s, H, dtype=np.float64):
    """x[s .. s + H) as `dtype`, zeros outside [0, n)."""
    out = np.zeros(H, dtype=dtype)
    lo, hi = max(s, 0), min(s + H, n)
    if hi > lo:
        out[lo - s:hi - s] = x[lo:hi]
    return out


def fade(H):
    """(f, g) float64 [H]: f[i] = 0.5 - 0.5 cospi(i / H) and g[i] = fl(1 - f[i])."""
    f = 0.5 - 0.5 * cospi(np.arange(H, dtype=np.float64) / float(H))
    return f, 1.0 - f


def nominal(k, r, H):
    return int(math.floor(float(k * H) * float(r)))


def order(D):
    """The visiting order of the offsets: 0, -1, +1, -2, +2, ..."""
    return [0] + [s * d for d in range(1, D + 1) for s in (-1, 1)]


def rank(d):
    return 0 if d == 0 else (-2 * d - 1 if d < 0 else 2 * d)


def scores(x, n, p, c, H, D):
    """(d [m], s [m]): the valid offsets in ascending d and their scores, NaN already mapped to -inf."""
    d = np.arange(max(-D, -p), min(D, n - 1 - p) + 1)
    span = seg(x, n, p + int(d[0]), len(d) - 1 + H)
    a = np.lib.stride_tricks.sliding_window_view(span, H)                # a[j, i] = x[p + d[j] + i]
    b = seg(x, n, c, H)
    with np.errstate(invalid="ignore", over="ignore"):
        C = np.cumsum(a * b, axis=1)[:, -1]
        E = np.cumsum(a * a, axis=1)[:, -1]
        s = 2.0 * C - E
    return d, np.where(np.isnan(s), -np.inf, s)


def positions(x, n, r, H=HOP, D=SEARCH, N=None):
    """(q, c, searched) of the frames of a row, int64 / int64 / bool [K]."""
    M = count(n, r) if N is None else min(count(n, r), N)
    K = -(-M // H)
    q, c, srch = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64), np.zeros(K, dtype=bool)
    for k in range(1, K):
        p = nominal(k, r, H)
        assert 0 <= p < n
        ck = int(q[k - 1]) + H
        c[k] = ck
        if abs(ck - p) <= D and 0 <= ck < n:
            q[k] = ck
            continue
        srch[k] = True
        d, s = scores(x, n, p, ck, H, D)
        best = s.max()
        ties = d[s == best]
        q[k] = p + int(min(ties, key=lambda v: rank(int(v))))
    return q, c, srch


def positions_brute(x, n, r, H, D):
    """The same, one product at a time (short rows)."""
    M = count(n, r)
    K = -(-M // H)
    xs = [float(v) for v in np.asarray(x[:n], dtype=np.float64)]
    at = lambda i: xs[i] if 0 <= i < n else 0.0
    q, c, srch = [0] * K, [0] * K, [False] * K
    for k in range(1, K):
        p = nominal(k, r, H)
        ck = q[k - 1] + H
        c[k] = ck
        if abs(ck - p) <= D and 0 <= ck < n:
            q[k] = ck
            continue
        srch[k] = True
        best, q[k] = -math.inf, p
        for d in order(D):
            cand = p + d
            if cand < 0 or cand >= n:
                continue
            C = E = 0.0
            for i in range(H):
                with np.errstate(invalid="ignore", over="ignore"):
                    C = float(np.float64(C) + np.float64(at(cand + i)) * np.float64(at(ck + i)))
                    E = float(np.float64(E) + np.float64(at(cand + i)) * np.float64(at(cand + i)))
            s = 2.0 * C - E
            if math.isnan(s):
                s = -math.inf
            if s > best:
                best, q[k] = s, cand
    return np.array(q, dtype=np.int64), np.array(c, dtype=np.int64), np.array(srch, dtype=bool)


def _fade_sums(x, n, r, H, q, c, N, F):
    M = count(n, r) if N is None else min(count(n, r), N)
    f, g = (v.astype(F) for v in fade(H))
    y = np.zeros(len(q) * H, dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(len(q)):
            y[k * H:(k + 1) * H] = f * seg(x, n, int(q[k]), H, F) + g * seg(x, n, int(c[k]), H, F)
    return y[:M]


def direct(x, n, r, H=HOP, D=SEARCH, N=None, pos=None):
    """The min(M, N) outputs in float64, before the rounding to float32; pos = (q, c, ...) of `positions`, if at hand."""
    q, c = (positions(x, n, r, H, D, N) if pos is None else pos)[:2]
    return _fade_sums(x, n, r, H, q, c, N, np.float64)


def direct_ld(x, n, r, H=HOP, D=SEARCH, N=None, pos=None):
    q, c = (positions(x, n, r, H, D, N) if pos is None else pos)[:2]
    return _fade_sums(x, n, r, H, q, c, N, LD)


def slack(x, n, r, H=HOP, D=SEARCH, N=None, pos=None):
    """(E, w): E = 8 x max |direct - w| over the row's outputs, and w = direct_ld."""
    pos = positions(x, n, r, H, D, N) if pos is None else pos
    w = direct_ld(x, n, r, H, D, N, pos)
    if w.size == 0:
        return 0.0, w
    return 8.0 * float(np.max(np.abs(direct(x, n, r, H, D, N, pos).astype(LD) - w))), w


# ------------------------------------------------------------------ signals
def voiced(seed, L, period=57.3, sigma=0.02):
    """Seeded noise plus a harmonic tone (six harmonics of 1 / period), so that the scores have a clear maximum."""
    t = np.arange(L, dtype=np.float64)
    tone = sum(np.sin(2.0 * np.pi * h * t / period + 0.7 * h) / h for h in range(1, 7))
    return (0.1 * tone + sigma * np.random.default_rng(seed).standard_normal(L)).astype(np.float32)


def periodic(seed, L, P):
    """An exact period of P samples: every window that starts a multiple of P apart holds the same float32 values."""
    return np.tile((0.3 * np.random.default_rng(seed).standard_normal(P)).astype(np.float32), -(-L // P))[:L]


def edge_length(M, r):
    """The shortest n with count(n, r) == M, for a rate >= 1 (one more input sample adds at most one output)."""
    n = int(math.floor(float(M - 1) * r)) + 1
    assert count(n, r) == M and count(n - 1, r) == M - 1
    return n


def match_row(seed, sign, r=2.0, H=H_S, D=D_S, L=400):
    """A row whose first searched frame (frame 1 at r = 2: p = 2 H, c = H) finds a perfect copy of its continuation at
    p - D (sign < 0; the copy overlaps the continuation, so the stretch x[c .. p - D + H) has the period p - D - c) or at
    p + D (sign > 0)."""
    x = voiced(seed, L, sigma=0.05)
    p, c = nominal(1, r, H), H
    assert abs(c - p) > D
    if sign < 0:
        P = p - D - c
        assert P > 0
        for i in range(c + P, p - D + H):
            x[i] = x[i - P]
    else:
        x[p + D:p + D + H] = x[c:c + H]
    return x


# ------------------------------------------------------------------ the rows the GPU tests judge
class Row(NamedTuple):
    x: np.ndarray            # float32 [n] (read-only)
    n: int
    r: float
    H: int
    D: int
    N: int                   # the n_out of the call the row is used in


ROWS = {}
_CASES = {}
RATES = (1.0, 1.0001, 0.9, 1.1, 0.5, 2.0, 0.25, 4.0, 1.0371, 0.9412)
EDGE_RATE = 1.1
EDGE_FRAMES = (1, 2, 5)
HOP_SEARCH = ((16, 0), (16, 1024), (1024, 0), (1024, 1024), (256, 160))
INVALID_NEIGHBOURS = 6
CUT_RATE = 0.3               # frame 1 is searched with p - D < 0, and the last frames with p + D >= n and c + H > n


def _register(key, x, r, N, H=H_S, D=D_S):
    assert key not in ROWS
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    ROWS[key] = Row(x, len(x), float(r), int(H), int(D), int(N))
    return key


def build_rows():
    """Every row a GPU test accepts under the rule, registered once (read-only, shared); tests/test_stretch_host.py checks
    the condition E <= 2^-10 x ulp32(rms) / 2 on each of them without a GPU."""
    if ROWS:
        return ROWS
    seed = 100
    for k in EDGE_FRAMES:                                                # 1. frame edges: M = kH - 1, kH, kH + 1; N = M, M - 1
        for M in (k * H_S - 1, k * H_S, k * H_S + 1):
            seed += 1
            x = voiced(seed, edge_length(M, EDGE_RATE))
            for N in (M, M - 1):
                _register(f"edge-{M}-{N}", x, EDGE_RATE, N)
    for n, r in ((1, 0.9), (H_S - 1, 1.1), (D_S - 10, 0.5)):              #    and rows shorter than a frame / than D
        seed += 1
        _register(f"short-{n}", voiced(seed, n), r, count(n, r))
    for i, r in enumerate(RATES):                                        # 2. the rates in one batch
        _register(f"rates-{i}", voiced(200 + i, 3000), r, count(3000, MIN_RATE))
    _register("tie-silence", np.zeros(1000, dtype=np.float32), 1.1, 1000)             # 3. ties and windows
    _register("tie-constant", np.full(1000, 0.25, dtype=np.float32), 0.9, 1200)
    _register("tie-period", periodic(301, 1000, 8), 1.25, 1000)          # k H r = 40 k: every p_k is a multiple of the period
    _register("match-lo", match_row(302, -1), 2.0, 256)
    _register("match-hi", match_row(303, +1), 2.0, 256)
    _register("cut", voiced(304, 300), CUT_RATE, count(300, CUT_RATE))
    for H, D in HOP_SEARCH:                                              # 4. every (hop, search) edge
        _register(f"hd-{H}-{D}", voiced(400 + H + D, 6000), 1.9, count(6000, 1.9), H, D)
    _register("long", voiced(500, 70000), 1.03, count(70000, 1.03), HOP, SEARCH)       # 5. a long row at the defaults
    for i in range(INVALID_NEIGHBOURS):                                  # 6. the valid neighbours of invalid rows
        _register(f"inv-ok-{i}", voiced(600 + i, 400), 0.85 + 0.06 * i, 500)
    _register("nf-a", voiced(610, 600), 1.0371, 700)                     #    and of a row with non-finite samples
    _register("nf-b", voiced(611, 600), 0.9412, 700)
    for i, (n, r) in enumerate(zip((900, 777, 513, 300, 1), (1.0371, 0.9412, 1.0001, 2.5, 0.8))):   # 7. bits
        _register(f"bits-{i}", voiced(700 + i, n), r, 1000)
    for i, (n, r) in enumerate(((600, 1.05), (500, 0.95))):              #    graph replay
        _register(f"graph-{i}", voiced(800 + i, n), r, 640)
    return ROWS


def case(key):
    """(pos, E, w) of a registered row, computed once: pos = positions (q, c, searched), w = direct_ld on its min(M, N)
    outputs and E = slack."""
    if key not in _CASES:
        row = ROWS[key]
        pos = positions(row.x, row.n, row.r, row.H, row.D, row.N)
        E, w = slack(row.x, row.n, row.r, row.H, row.D, row.N, pos)
        _CASES[key] = (pos, E, w)
    return _CASES[key]
