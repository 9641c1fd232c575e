"""The numpy model of the transmission stage (cmgan_amd/csrc/transmit.hip; include/cmgan_hip.h, "Transmission"), shared by
tests/test_transmit_host.py and tests/test_gpu_transmit.py.  Nothing here imports the library.

For a row x with n float32 samples, a table of lost frames, a codec, a concealment switch and the host values F (frame),
pmin .. pmax (lags), W (matching window) and A (fade unit):

    z[i] = codec(x[i])     0: x itself; 1 .. 3 from q = sat16(rint(x 32768)) (half to even, NaN -> 0): q / 32768,
                           ulaw2lin(lin2ulaw(q)) / 32768, alaw2lin(lin2alaw(q)) / 32768 - audioop's maps at width 2
    a run of lost frames k0 .. k1 - 1, s = k0 F, e = min(k1 F, n), in ascending order; h(i) = y[i] as it stands, 0 for i < 0
    plc = 0: y[s .. e) = 0
    plc = 1: P = the lag in pmin .. pmax with the largest 2 C - E, C = sum_{i<W} h(s-W+i) h(s-W-P+i), E = sum_{i<W}
             h(s-W-P+i)^2 (float64, ascending; NaN counts as -inf; the smallest P among equal maxima); Q = floor(P / 4);
             v[i] = h(s-P+i) for i < P - Q, else fl(1-t) h(s-P+i) + t h(s-2P+i) with t = (i-(P-Q)+1) / (Q+1);
             g(j) = min(1, max(0, (6A - j) / (5A)));  y[s+j] = g(j) v[j mod P] for j < e - s;  and if e < n, with R =
             min(Q, F, n-e), M = e - s, t = (i+1) / (R+1):  y[e+i] = fl(1-t) g(M+i) v[(M+i) mod P] + t z[e+i] for i < R

ulaw_encode .. alaw_decode   the four G.711 maps in closed form on integer arrays (the segment is a bit length).
codec                        z of a float32 array, float32: exact, compared with the kernel's for EQUALITY.
transmit                     the whole row, written serially: the decisions (scores, lags) in float64 with SEQUENTIAL ascending
                             sums (np.cumsum(...)[-1]); every stored sample three times - w in np.longdouble, the value a
                             device sample is judged against; d, the same expression in float64; and y = f32(w), the row the
                             chain goes on from.  Also, per searched run, the margin of the best score over the runner-up
                             and the energy sum_{i<W} h(s-W+i)^2 of the window.

Acceptance rule (stretch_model's).  Lags, status and zeros are compared for EQUALITY.  A device sample g is accepted
against w when |g - w| <= ulp32(w) / 2 + E, with E = 8 x max |d - w| per row from the model alone.  CONDITIONS, checked
without a GPU by the host test on every registered row: E <= 2^-10 x ulp32(rms of w) / 2, and - because the chain runs
on ROUNDED float32 output, where a device sample may differ from the model's by one ulp - every searched run is either an
exact tie by construction (the row is registered with tie=True) or its best score beats the runner-up by at least 2^-12 x
sum_{i<W} h(s-W+i)^2: one ulp of a history sample moves a score by about 2^-22 of that sum, so the decision cannot flip."""
from typing import NamedTuple

import numpy as np

from warp_model import LD, ulp32

FS = 16000
F_D, PMIN_D, PMAX_D, W_D, A_D = 320, 80, 240, 320, 160         # the defaults of Engine.transmit at 16 kHz
NONE, PCM16, ULAW, ALAW = 0, 1, 2, 3
MARGIN = 2.0 ** -12


# ------------------------------------------------------------------ G.711 in closed form
def _bit_length(v):
    """The bit length of the non-negative integers v (0 -> 0)."""
    v = np.asarray(v, dtype=np.int64)
    return np.where(v > 0, np.floor(np.log2(np.maximum(v, 1))).astype(np.int64) + 1, 0)


def ulaw_encode(q):
    """lin2ulaw at width 2: int16 values -> codes 0 .. 255."""
    v = np.asarray(q, dtype=np.int64) >> 2                               # the 14-bit value (floor)
    neg = v < 0
    m = np.minimum(np.where(neg, -v, v), 8159) + 33
    seg = _bit_length(m) - 6                                             # m >= 33: the segment is its bit length
    code = np.where(seg >= 8, 0x7F, (seg << 4) | ((m >> (seg + 1)) & 0xF))
    return (code ^ np.where(neg, 0x7F, 0xFF)) & 0xFF


def ulaw_decode(code):
    u = ~np.asarray(code, dtype=np.int64) & 0xFF
    t = (((u & 0xF) << 3) + 0x84) << ((u & 0x70) >> 4)
    return np.where(u & 0x80, 0x84 - t, t - 0x84)


def alaw_encode(q):
    """lin2alaw at width 2: int16 values -> codes 0 .. 255."""
    v = np.asarray(q, dtype=np.int64) >> 3                               # the 13-bit value (floor)
    neg = v < 0
    m = np.where(neg, -v - 1, v)
    seg = np.maximum(_bit_length(m) - 5, 0)
    code = (seg << 4) | ((m >> np.where(seg < 2, 1, seg)) & 0xF)
    return (code ^ np.where(neg, 0x55, 0xD5)) & 0xFF


def alaw_decode(code):
    a = (np.asarray(code, dtype=np.int64) ^ 0x55) & 0xFF
    t, seg = (a & 0xF) << 4, (a & 0x70) >> 4
    t = np.where(seg == 0, t + 8, np.where(seg == 1, t + 0x108, (t + 0x108) << np.maximum(seg - 1, 0)))
    return np.where(a & 0x80, t, -t)


def quantise(x):
    """q = sat16(rint(x 32768)) of float32 values, int64: half to even, NaN -> 0, +-inf saturate."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.asarray(x, dtype=np.float32).astype(np.float64) * 32768.0
        s = np.where(np.isnan(s), 0.0, np.clip(s, -32768.0, 32767.0))
        return np.rint(s).astype(np.int64)


def codec(x, kind):
    """z of the float32 array x, float32 (every value is exact)."""
    x = np.asarray(x, dtype=np.float32)
    if kind == NONE:
        return x.copy()
    q = quantise(x)
    if kind == ULAW:
        q = ulaw_decode(ulaw_encode(q))
    elif kind == ALAW:
        q = alaw_decode(alaw_encode(q))
    else:
        assert kind == PCM16
    return (q.astype(np.float64) / 32768.0).astype(np.float32)


# ------------------------------------------------------------------ the definition, serially
def runs(lost, K):
    """[(k0, k1)]: the maximal runs of lost frames among the first K table columns, ascending."""
    out, k = [], 0
    while k < K:
        if lost[k]:
            k0 = k
            while k < K and lost[k]:
                k += 1
            out.append((k0, k))
        else:
            k += 1
    return out


def hist(y, lo, hi, dtype=np.float64):
    """h(lo .. hi) of the row as it stands, zeros for i < 0; hi <= len(y)."""
    out = np.zeros(hi - lo, dtype=dtype)
    a = max(lo, 0)
    if hi > a:
        out[a - lo:] = y[a:hi]
    return out


def lag_scores(y, s, pmin, pmax, W):
    """(scores float64 [pmax - pmin + 1] with NaN mapped to -inf, the window's energy) of the run that starts at s."""
    span = hist(y, s - W - pmax, s)                                      # span[j] = h(s - W - pmax + j)
    a = span[pmax:]                                                      # h(s - W + i)
    b = np.lib.stride_tricks.sliding_window_view(span, W)[pmax - np.arange(pmin, pmax + 1)]   # row P: h(s - W - P + i)
    with np.errstate(invalid="ignore", over="ignore"):
        C = np.cumsum(a[None, :] * b, axis=1)[:, -1]
        E = np.cumsum(b * b, axis=1)[:, -1]
        sc = 2.0 * C - E
        energy = float(np.cumsum(a * a)[-1])
    return np.where(np.isnan(sc), -np.inf, sc), energy


def gain(j, A):
    """g(j), float64: one IEEE division of exact integers, clamped to [0, 1]."""
    g = (6.0 * A - np.asarray(j, dtype=np.float64)) / (5.0 * A)
    return np.minimum(1.0, np.maximum(0.0, g))


class Run(NamedTuple):
    k0: int
    k1: int
    lag: int                 # 0 when the run is not concealed (plc = 0)
    margin: float            # best score - runner-up (inf with one lag; nan when not concealed)
    energy: float            # sum_{i<W} h(s-W+i)^2


class Result(NamedTuple):
    y: np.ndarray            # float32 [n]: f32(w), the chain the decisions were made on
    w: np.ndarray            # long double [n]
    d: np.ndarray            # float64 [n]: the same expressions in float64
    lag: np.ndarray          # int32 [K]
    runs: list


def transmit(x, n, lost, kind, plc, F=F_D, pmin=PMIN_D, pmax=PMAX_D, W=W_D, A=A_D):
    x = np.asarray(x, dtype=np.float32)[:n]
    K = -(-n // F)
    z = codec(x, kind)
    y = z.copy()
    w, d = z.astype(LD), z.astype(np.float64)
    lag, found = np.zeros(K, dtype=np.int32), []
    for k0, k1 in runs(lost, K):
        s, e = k0 * F, min(k1 * F, n)
        if not plc:
            y[s:e], w[s:e], d[s:e] = 0.0, 0.0, 0.0
            found.append(Run(k0, k1, 0, np.nan, np.nan))
            continue
        sc, energy = lag_scores(y, s, pmin, pmax, W)
        P = pmin + int(np.argmax(sc))                                    # (argmax: the first, so the smallest, of equal maxima)
        rest = np.delete(sc, P - pmin)
        with np.errstate(invalid="ignore"):
            margin = float(sc[P - pmin] - rest.max()) if rest.size else np.inf
        found.append(Run(k0, k1, P, margin, energy))
        lag[k0] = P
        Q = P // 4
        i = np.arange(P - Q, P)
        t = (i - (P - Q) + 1).astype(np.float64) / float(Q + 1)
        M, R = e - s, (min(Q, F, n - e) if e < n else 0)
        j = np.arange(M + R)
        g = gain(j, A)
        tb = np.arange(1, R + 1, dtype=np.float64) / float(R + 1)
        with np.errstate(invalid="ignore", over="ignore"):
            for T, dst in ((LD, w), (np.float64, d)):
                v = hist(y, s - P, s, T)
                v[P - Q:] = (1.0 - t).astype(T) * v[P - Q:] + t.astype(T) * hist(y, s - 2 * P + P - Q, s - P, T)
                a = g.astype(T) * v[j % P]
                dst[s:e] = a[:M]
                if R:
                    dst[e:e + R] = (1.0 - tb).astype(T) * a[M:] + tb.astype(T) * z[e:e + R].astype(T)
            y[s:e + R] = w[s:e + R].astype(np.float32)
    return Result(y, w, d, lag, found)


def slack(res):
    """E = 8 x max |d - w| over the row (NaN samples, where both are NaN, do not count)."""
    if res.w.size == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        diff = np.abs(res.d.astype(LD) - res.w).astype(np.float64)
    diff = diff[~np.isnan(diff)]
    return 8.0 * float(diff.max()) if diff.size else 0.0


def condition(res):
    """The bound E must respect for the row to be used: 2^-10 x ulp32(rms of the finite w) / 2."""
    v = res.w.astype(np.float64)
    v = v[np.isfinite(v)]
    rms = float(np.sqrt(np.mean(v ** 2))) if v.size else 0.0
    return 2.0 ** -10 * float(ulp32(rms)) / 2.0


def excess(g, w, E):
    """The worst |g - w| - ulp32(w) / 2 - E over the samples (accepted when <= 0); g float32, w long double.  A sample
    that is NaN in one of the two and not in the other is +inf beyond; NaN in both is accepted."""
    if len(w) == 0:
        return -np.inf
    g = np.asarray(g)
    gn, wn = np.isnan(g), np.isnan(w.astype(np.float64))
    if not np.array_equal(gn, wn):
        return np.inf
    keep = ~wn
    if not keep.any():
        return -np.inf
    with np.errstate(invalid="ignore"):
        err = np.abs(g[keep].astype(LD) - w[keep]).astype(np.float64)
        err = np.where(g[keep].astype(np.float64) == w[keep].astype(np.float64), 0.0, err)      # (equal infinities)
    return float(np.max(err - 0.5 * ulp32(w[keep].astype(np.float64)) - E))


def margins_ok(res, tie=False):
    """Whether every searched run of the row is decided beyond the reach of one ulp of its history (or is a tie by
    construction)."""
    return tie or all(r.lag == 0 or r.margin >= MARGIN * r.energy for r in res.runs)


# ------------------------------------------------------------------ signals
def speech(seed, L, f0=123.0, sigma=0.002, glide=20.0):
    """Eleven harmonics of a pitch that glides by +-`glide` Hz around f0 under a 3 Hz envelope, noise at -34 dB (the clips
    of tools/stretch_bench.py)."""
    t = np.arange(L) / FS
    f = f0 + glide * np.sin(2 * np.pi * (1.0 + 0.1 * seed) * t)
    ph = 2 * np.pi * np.cumsum(f) / FS
    tone = sum(np.sin(h * ph) / h for h in range(1, 12))
    return (0.1 * tone * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + sigma * np.random.default_rng(seed).standard_normal(L)).astype(np.float32)


def periodic(seed, L, P):
    """An exact period of P samples, bit for bit."""
    return np.tile((0.3 * np.random.default_rng(seed).standard_normal(P)).astype(np.float32), -(-L // P))[:L]


def near_periodic(seed, L, P, sigma=0.01):
    """A period of P samples of noise, repeated, plus independent noise: one lag stands far above the others."""
    return (periodic(seed, L, P) + sigma * np.random.default_rng(seed + 1).standard_normal(L)).astype(np.float32)


def table(K, *frames):
    """uint8 [K]: 1 at the given frames (negative ones count from the end)."""
    t = np.zeros(K, dtype=np.uint8)
    for k in frames:
        t[k] = 1
    return t


# ------------------------------------------------------------------ the rows the GPU tests judge
class Row(NamedTuple):
    x: np.ndarray            # float32 [n] (read-only)
    n: int
    lost: np.ndarray         # uint8 [K]
    codec: int
    plc: int
    F: int
    pmin: int
    pmax: int
    W: int
    A: int
    tie: bool


ROWS = {}
_CASES = {}
N_ROW = 8000
FRAMES = (160, 320)


def _register(key, x, lost, codec=ULAW, plc=1, F=F_D, pmin=PMIN_D, pmax=PMAX_D, W=W_D, A=A_D, tie=False):
    assert key not in ROWS
    x = np.ascontiguousarray(x, dtype=np.float32)
    lost = np.ascontiguousarray(lost, dtype=np.uint8)
    assert len(lost) == -(-len(x) // F)
    x.setflags(write=False)
    lost.setflags(write=False)
    ROWS[key] = Row(x, len(x), lost, int(codec), int(plc), int(F), int(pmin), int(pmax), int(W), int(A), bool(tie))
    return key


def build_rows():
    """Every row a GPU test accepts under the rule, registered once (read-only, shared); tests/test_transmit_host.py checks
    the two conditions of the module docstring on each of them without a GPU."""
    if ROWS:
        return ROWS
    seed = 0
    for F in FRAMES:                                                     # 1. the runs, at both frame sizes
        K = -(-N_ROW // F)
        kw = dict(F=F, A=F // 2)
        part = N_ROW - 3 * F // 4 - 7                                    # n is no multiple of F: the last frame is partial
        Kp = -(-part // F)
        for name, n, frames in (("first", N_ROW, (0,)), ("second", N_ROW, (1,)), ("last-partial", part, (Kp - 1,)),
                                ("apart", N_ROW, (10, 12)), ("mid", N_ROW, (7, 8))):
            seed += 1
            _register(f"run-{F}-{name}", speech(seed, n), table(-(-n // F), *frames), **kw)
        seed += 1                                                        #    a partial good frame shorter than Q behind the run
        n = (K - 2) * F + 9
        _register(f"run-{F}-short-good", speech(seed, n), table(-(-n // F), -(-n // F) - 2), **kw)
        seed += 1
        _register(f"run-{F}-all", speech(seed, N_ROW), np.ones(K, dtype=np.uint8), **kw)
        seed += 1
        _register(f"run-{F}-none", speech(seed, N_ROW), np.zeros(K, dtype=np.uint8), codec=NONE, **kw)
        seed += 1
        _register(f"run-{F}-gap", speech(seed, N_ROW), table(K, 3, 9, 10), plc=0, **kw)
        seed += 1
        _register(f"run-{F}-plc", speech(seed, N_ROW), table(K, 3, 9, 10), plc=1, **kw)
    K = -(-N_ROW // 320)
    _register("long-run", speech(30, N_ROW), table(K, 10, 11, 12, 13, 14))          #    5 frames = 1600 > 6 A = 960: exact zeros
    _register("bench-pattern", speech(31, N_ROW), table(K, 1, 5, 10, 11, 12, 13, 14, 16, 24))
    for i, kind in enumerate((NONE, PCM16, ULAW, ALAW)):                 #    every codec in front of a concealed run
        _register(f"codec-{kind}", speech(40 + i, N_ROW), table(K, 6, 7, 15), codec=kind)
    tiled = periodic(50, N_ROW, 100)                                     # 2. ties and non-finite rows
    _register("tie-period", tiled, table(K, 9), codec=NONE, tie=True)
    _register("tie-silence", np.zeros(N_ROW, dtype=np.float32), table(K, 4, 20), codec=NONE, tie=True)
    x = speech(51, N_ROW).copy()
    x[320 * 8 - 100] = np.nan
    _register("nan-window", x, table(K, 8), codec=NONE, tie=True)
    _register("edge-one-lag", speech(60, N_ROW), table(K, 5, 11), pmin=130, pmax=130)              # 3. range edges
    _register("edge-1024", near_periodic(61, N_ROW, 700), table(K, 12, 20), pmin=512, pmax=1024, W=1024)
    _register("edge-f16", speech(62, 2000, f0=400.0), table(125, 40, 41, 80, 124), F=16, pmin=16, pmax=64, W=64, A=8)
    kw = dict(F=16, pmin=16, pmax=64, W=64, A=8)                         #    tables longer than one pass of the kernel's walk (64 and 256 frames)
    _register("walk-64", speech(63, 1024, f0=400.0), table(64, 20, 60, 61, 62, 63), **kw)           # a run that ends at K = 64
    _register("walk-256", speech(64, 4096, f0=400.0), table(256, 62, 63, 64, 65, 127, 192, 250, 251, 252, 253, 254, 255), **kw)
    _register("walk-513", speech(65, 8200, f0=400.0), table(513, 0, 63, 128, 129, 254, 255, 256, 257, 258, 383, 384, 511, 512), **kw)
    for i, n in enumerate((8000, 7777, 5000, 321, 0)):                   # 4. per-row lengths
        _register(f"len-{i}", speech(70 + i, n), table(-(-n // 320), *((2,) if n > 960 else ())))
    for i in range(4):                                                   # 5. neighbours of invalid rows, bits, graph replay
        _register(f"inv-ok-{i}", speech(80 + i, 2000), table(7, 2 + i))
    for i, n in enumerate((8000, 6001, 3333)):
        _register(f"bits-{i}", speech(90 + i, n), table(-(-n // 320), 3, 4, 8), codec=(ULAW, ALAW, PCM16)[i])
    for i in range(4):
        _register(f"graph-{i}", speech(100 + i, 4000), table(13, 2 + i, 7 + (i & 1)), codec=i, plc=1 - (i & 1) if i < 2 else 1)
    return ROWS


def case(key):
    """(result, E) of a registered row, computed once."""
    if key not in _CASES:
        row = ROWS[key]
        res = transmit(row.x, row.n, row.lost, row.codec, row.plc, row.F, row.pmin, row.pmax, row.W, row.A)
        _CASES[key] = (res, slack(res))
    return _CASES[key]
