"""The numpy model of the speed perturbation (cmgan_amd/csrc/warp.hip; include/cmgan_hip.h, "Speed perturbation"), shared
by tests/test_warp_host.py and tests/test_gpu_warp.py.  Nothing here imports the library.

For a row x with n samples, a rate r (input samples per output sample), `zeros` and `rolloff`, in float64:

    t_i = fl(i r),   M = #{i >= 0 : t_i < n},   fc = rolloff (r > 1 ? 1 / r : 1),   W = zeros / fc
    h(d) = fc sinc(fc d) (0.5 + 0.5 cospi(d / W)) for |d| < W,   sinc(z) = sinpi(z) / (pi z), sinc(0) = 1
    y_i = sum_k x[k] h(t_i - k)  over the integers k with |t_i - k| < W and 0 <= k < n, in ascending k

direct      the definition in float64; sinpi / cospi by exact reduction (z = q / 2 + f with |f| <= 1 / 4, then sin or cos
            of pi f), so that they are exactly 0 / +-1 at the integers and half-integers.
direct_ld   the same in np.longdouble, from the same float64 t_i, fc and W and the same set of taps: the value w a device
            sample is judged against.
as_kernel   float64 with the kernel's shortcuts and summation order: sinpi / cospi at an output's first tap only, then
            both (sin, cos) pairs turned by the angle-addition identities with cospi / sinpi of the constant step
            (fc for the sinc, 1 / W for the window); the taps with |d| < 1 take sinpi(fc d) and cospi(d / W) directly.

All three return the sums before the rounding to float32, for the outputs `ns` (default: all M of them).

Acceptance rule (the channel's).  A device sample g is accepted against w = direct_ld when |g - w| <= ulp32(w) / 2 + E,
with E per row from the model alone: E = 8 x max_i max(|direct - w|, |as_kernel - w|) (`slack`).  The factor 8 covers
the FMA contraction of the device build and the device's own sinpi / cospi.  CONDITION: a row may be used only if
E <= 2^-10 x ulp32(rms of w) / 2 (`condition`), so that the rule cannot hide a wrong sample."""
import math
from typing import NamedTuple, Optional

import numpy as np

LD = np.longdouble
PI_LD = LD("3.14159265358979323846264338327950288")
MIN_RATE, MAX_RATE = 0.25, 4.0


# ------------------------------------------------------------------ sinpi / cospi by exact reduction
def _reduced(z):
    """z = q / 2 + f exactly, |f| <= 1 / 4: (q mod 4, sin(pi f), cos(pi f)) in z's own precision."""
    z = np.asarray(z)
    F = z.dtype.type
    q = np.rint(z * F(2))
    f = z - q / F(2)
    a = (PI_LD if F is LD else F(math.pi)) * f
    return np.mod(q, F(4)).astype(np.int64), np.sin(a), np.cos(a)


def sinpi(z):
    m, s, c = _reduced(z)
    return np.choose(m, [s, c, -s, -c])


def cospi(z):
    m, s, c = _reduced(z)
    return np.choose(m, [c, -s, -c, s])


# ------------------------------------------------------------------ geometry
def valid(r, n, L):
    return bool(np.isfinite(r) and MIN_RATE <= r <= MAX_RATE and 0 <= n <= L)


def geometry(r, zeros, rolloff):
    """(fc, W) as the float64 values the definition names."""
    r = float(r)
    fc = float(rolloff) * (1.0 / r if r > 1.0 else 1.0)
    return fc, float(zeros) / fc


def count(n, r):
    """M = #{i >= 0 : fl(i r) < n}: ceil(n / r) corrected by single steps until fl((M - 1) r) < n <= fl(M r)."""
    n, r = int(n), float(r)
    if n <= 0:
        return 0
    M = int(math.ceil(n / r))
    while M > 0 and float(M - 1) * r >= n:
        M -= 1
    while float(M) * r < n:
        M += 1
    return M


def count_brute(n, r):
    """The same count by looking at every time (short rows only)."""
    i = np.arange(0, 4 * int(n) + 16, dtype=np.float64)
    return int(np.count_nonzero(i * float(r) < n))


def support(t, W, n):
    """(k0, k1), int64: the integers k with |t - k| < W judged on the float64 difference, clamped to [0, n)."""
    t = np.asarray(t, dtype=np.float64)
    a = np.floor(t - W).astype(np.int64)
    for _ in range(3):
        a = np.where(t - a < W, a, a + 1)
    for _ in range(3):
        a = np.where(t - (a - 1) < W, a - 1, a)
    b = np.ceil(t + W).astype(np.int64)
    for _ in range(3):
        b = np.where(t - b > -W, b, b - 1)
    for _ in range(3):
        b = np.where(t - (b + 1) > -W, b + 1, b)
    assert np.all((t - a < W) & ~(t - (a - 1) < W) & (t - b > -W) & ~(t - (b + 1) > -W))
    return np.maximum(a, 0), np.minimum(b, int(n) - 1)


# ------------------------------------------------------------------ the three forms
def _sums(x, n, r, zeros, rolloff, ns, mode):
    M = count(n, r)
    ns = np.arange(M, dtype=np.int64) if ns is None else np.asarray(ns, dtype=np.int64)
    assert ns.size == 0 or (ns.min() >= 0 and ns.max() < M)
    F = LD if mode == "ld" else np.float64
    if ns.size == 0:
        return np.zeros(0, dtype=F)
    fc, W = geometry(r, zeros, rolloff)
    t = ns.astype(np.float64) * float(r)                                 # one rounded float64 product each
    k0, k1 = support(t, W, n)
    xs = np.asarray(x[:n]).astype(F)
    tF, fcF, WF = t.astype(F), F(fc), F(W)
    pi = PI_LD if F is LD else F(math.pi)
    acc = np.zeros(ns.size, dtype=F)
    if mode == "kernel":
        cd, sd, cwd, swd = cospi(fcF), sinpi(fcF), cospi(F(1) / WF), sinpi(F(1) / WF)
        d0 = tF - k0.astype(F)
        s, c, ws, wc = sinpi(fcF * d0), cospi(fcF * d0), sinpi(d0 / WF), cospi(d0 / WF)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(int((k1 - k0).max()) + 1):
            k = k0 + j
            live = k <= k1
            d = tF - k.astype(F)
            if mode == "kernel":
                near = np.abs(d) < 1
                sj = np.where(near, sinpi(fcF * d), s)
                wj = np.where(near, cospi(d / WF), wc)
            else:
                sj, wj = sinpi(fcF * d), cospi(d / WF)
            zero = d == 0
            sinc = np.where(zero, F(1), sj / np.where(zero, F(1), pi * (fcF * d)))
            h = fcF * sinc * (F(0.5) + F(0.5) * wj)
            acc = np.where(live, acc + xs[np.minimum(k, n - 1)] * h, acc)
            if mode == "kernel":
                s, c = s * cd - c * sd, c * cd + s * sd
                ws, wc = ws * cwd - wc * swd, wc * cwd + ws * swd
    return acc


def direct(x, n, r, zeros=24, rolloff=0.95, ns=None):
    return _sums(x, n, r, zeros, rolloff, ns, "direct")


def direct_ld(x, n, r, zeros=24, rolloff=0.95, ns=None):
    return _sums(x, n, r, zeros, rolloff, ns, "ld")


def as_kernel(x, n, r, zeros=24, rolloff=0.95, ns=None):
    return _sums(x, n, r, zeros, rolloff, ns, "kernel")


def holders(n, r, zeros, rolloff, k, N=None):
    """The outputs i < min(M, N) whose support holds sample k: a bool array."""
    M = count(n, r) if N is None else min(count(n, r), N)
    fc, W = geometry(r, zeros, rolloff)
    k0, k1 = support(np.arange(M, dtype=np.float64) * float(r), W, n)
    return (k0 <= k) & (k <= k1)


def noise(seed, L, sigma=0.3):
    return (sigma * np.random.default_rng(seed).standard_normal(L)).astype(np.float32)


# ------------------------------------------------------------------ the acceptance rule
def ulp32(w):
    """The float32 spacing at |w| (w float64): 2^(e - 24) for |w| in [2^(e-1), 2^e), at least the denormal 2^-149."""
    w = np.abs(np.asarray(w, dtype=np.float64))
    _, e = np.frexp(w)
    return np.where(w == 0.0, 2.0 ** -149, np.ldexp(1.0, np.maximum(e - 24, -149)))


def slack(x, n, r, zeros=24, rolloff=0.95, ns=None):
    """(E, w): E = 8 x max(|direct - w|, |as_kernel - w|) over the outputs `ns`, and w = direct_ld."""
    w = direct_ld(x, n, r, zeros, rolloff, ns)
    if w.size == 0:
        return 0.0, w
    a = np.max(np.abs(direct(x, n, r, zeros, rolloff, ns).astype(LD) - w))
    b = np.max(np.abs(as_kernel(x, n, r, zeros, rolloff, ns).astype(LD) - w))
    return 8.0 * float(max(a, b)), w


def condition(E, w):
    """The bound E must respect for the row to be used: 2^-10 x ulp32(rms of w) / 2."""
    rms = float(np.sqrt(np.mean(np.asarray(w, dtype=np.float64) ** 2)))
    return 2.0 ** -10 * float(ulp32(rms)) / 2.0


def case(key):
    """(E, w, ns) of a registered row, computed once: the outputs `ns` it is judged on (all min(M, N) of them unless the
    row names some), w = direct_ld there and E = slack."""
    if key not in _CASES:
        row = ROWS[key]
        ns = row.ns if row.ns is not None else np.arange(min(count(row.n, row.r), row.N), dtype=np.int64)
        E, w = slack(row.x, row.n, row.r, row.zeros, row.rolloff, ns)
        _CASES[key] = (E, w, ns)
    return _CASES[key]


def excess(g, w, E):
    """The worst |g - w| - ulp32(w) / 2 - E over the samples (accepted when <= 0); g float32, w long double."""
    if len(w) == 0:
        return -np.inf
    err = np.abs(np.asarray(g).astype(LD) - w).astype(np.float64)
    return float(np.max(err - 0.5 * ulp32(w.astype(np.float64)) - E))


# ------------------------------------------------------------------ the rows the GPU tests judge by the rule
class Row(NamedTuple):
    x: np.ndarray            # float32 [n] (read-only)
    n: int
    r: float
    zeros: int
    rolloff: float
    N: int                   # the n_out of the call the row is used in
    ns: Optional[np.ndarray] = None


ROWS = {}
_CASES = {}
RATES = (1.0, 1.0 + 1e-4, 1.0 - 1e-4, 0.8, 1.25, 0.25, 4.0, 2.5)
EDGE_RATES = (1.1, 2.5)      # >= 1: one more input sample adds at most one output, so every M can be hit
INVALID_NEIGHBOURS = 9
NONFINITE_AT = 333          # where the rows of the non-finite test hold their bad sample


def _register(key, x, r, N, zeros=24, rolloff=0.95, ns=None):
    assert key not in ROWS
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    ROWS[key] = Row(x, len(x), float(r), int(zeros), float(rolloff), int(N), ns)
    return key


def edge_lengths(N, r):
    """(the shortest n with count(n, r) >= N, the longest n with count(n, r) == N - 1) for a rate >= 1."""
    full = int(math.floor(float(N - 1) * r)) + 1
    assert count(full, r) == N and count(full - 1, r) == N - 1
    return full, full - 1


def edge_cases(T):
    return [1, T - 1, T, T + 1, 2 * T + 1]


def build_rows(T):
    """Every row a GPU test accepts under the rule, registered once (read-only, shared); tests/test_warp_host.py checks
    the condition E <= 2^-10 x ulp32(rms) / 2 on each of them without a GPU."""
    if ROWS:
        return ROWS
    seed = 1000
    for N in edge_cases(T):                                              # 1. tile edges: M = N and M = N - 1
        for r in EDGE_RATES:
            for kind, n in zip(("full", "short"), edge_lengths(N, r)):
                seed += 1
                if n > 0:
                    _register(f"edge-{N}-{r}-{kind}", noise(seed, n), r, N)
    for r in (1.1, 0.8):                                                 # 2. rows shorter than the filter
        W = geometry(r, 24, 0.95)[1]
        for n in (1, 2, int(2 * W) - 1):
            seed += 1
            _register(f"short-{r}-{n}", noise(seed, n), r, count(n, r))
    for zeros in (4, 24, 64):                                            # 3. the rates, for every filter
        for rolloff in (0.5, 0.95, 1.0):
            for i, r in enumerate(RATES):
                _register(f"rates-{zeros}-{rolloff}-{i}", noise(2000 + i, 300), r, count(300, MIN_RATE), zeros, rolloff)
    M = count(70000, 1.0001)                                             # 4. a long row: its first and its last tile
    last = (M - 1) // T * T
    _register("long", noise(3000, 70000), 1.0001, M, ns=np.concatenate([np.arange(T), np.arange(last, M)]))
    for i, (n, r) in enumerate(zip((900, 777, 513, 300, 1), (1.0371, 0.9412, 1.0001, 2.5, 0.8))):   # 5. bits
        _register(f"bits-{i}", noise(4000 + i, n), r, 1000)
    for i in range(INVALID_NEIGHBOURS):                                  # 6. the valid neighbours of invalid rows
        _register(f"inv-ok-{i}", noise(5000 + i, 400), 0.9 + 0.02 * i, 500)
    for i, (name, v, r) in enumerate((("nan", np.nan, 1.1), ("inf", np.inf, 0.9), ("-inf", -np.inf, 2.5))):   # 7.
        x = noise(6000 + i, 600)
        x[NONFINITE_AT] = v
        _register(f"nf-{name}", x, r, 700, ns=np.flatnonzero(~holders(600, r, 24, 0.95, NONFINITE_AT, 700)))
    _register("nf-a", noise(6010, 600), 1.0371, 700)
    _register("nf-b", noise(6011, 600), 0.9412, 700)
    for i, (n, r) in enumerate(((600, 1.05), (500, 0.95))):              # 8. graph replay
        _register(f"graph-{i}", noise(7000 + i, n), r, 640)
    return ROWS

