"""The numpy model of the noise-suppressor stage (cmgan_amd/csrc/suppress.hip; include/cmgan_hip.h, "Suppression"), shared
by tests/test_suppress_host.py and tests/test_gpu_suppress.py.  Nothing here imports the library.

For a row x with n float32 samples, a key row of the same length (x itself without one), a table row (rule, a_dd, a_n, D,
bias, g_min, xi_min) and n_fft = N (h = N / 2, F = N / 2 + 1, T_b = ceil(n / h) + 1, w[k] = sin(pi k / N)):

    Y_t[f] = sum_k x~[(t-1) h + k] w[k] e^{-2 pi i f k / N},  K_t the same from the key,  A_t[f] = |K_t[f]|^2
    P_t = a_n P_{t-1} + (1 - a_n) A_t (P_{-1} = A_0);  lam_t = max(bias min_{t-D < u <= t} P_u, 2^-60);  gam_t = min(A_t / lam_t, 40)
    xi_t = max(a_dd G_{t-1}^2 gam_{t-1} + (1 - a_dd) max(gam_t - 1, 0), xi_min)  (t = 0: without the first term);  q = xi_t / (1 + xi_t)
    G = q | sqrt(q) | min(q exp(E1(max(q gam_t, 2^-30)) / 2), 1)  for rule 1 | 2 | 3;  G_t = max(G, g_min)
    z_t = irfft(G_t Y_t);  y[t h + r] = f32(z_t[r + h] w[r + h] + z_{t+1}[r] w[r])

e1_d            E1 by the header's fixed formulas in float64, term for term: below E1_SPLIT the series -gamma - ln x + x (c_1 + x
                (c_2 + ... x c_K)) with c_k = (-1)^(k+1) / (k k!) and K = E1_TERMS, from there the continued fraction e^-x /
                (x + 1 - 1 / (x + 3 - 4 / (x + 5 - ...))) cut at depth E1_DEPTH and run backwards as a ratio n / d.
e1_w            E1 converged in long double (a longer series, a much deeper fraction).
suppress        the whole row three times: w in np.longdouble (scipy.fft keeps that precision) with e1_w, the value a device
                sample is judged against; d, the same in float64 with scipy.fft and e1_d; and d2, float64 with a direct DFT
                product in place of scipy.fft.

Acceptance rule (transmit_model's).  Status words, zeros and bit copies are compared for EQUALITY.  A device sample g is
accepted against w when |g - w| <= ulp32(w) / 2 + E with E = 8 x max(|d - w|, |d2 - w|) per row, from the model alone; a
device gain when |G - G_w| <= E_G = 8 x max(|G_d - G_w|, |G_d2 - G_w|).  CONDITIONS, checked without a GPU by the host test
on every registered row: E <= 2^-10 x ulp32(rms of w) / 2 and E_G <= 2^-30."""
from typing import NamedTuple, Optional

import numpy as np
import scipy.fft

from transmit_model import speech
from warp_model import LD, PI_LD, ulp32

FS = 16000
OFF, WIENER, SPECSUB, LOGMMSE = 0, 1, 2, 3
N_FFTS = (256, 512, 1024)
MAX_WINDOW = 128                  # = cmgan_suppress_max_window()
GAMMA_MAX, LAM_MIN, V_MIN = 40.0, 2.0 ** -60, 2.0 ** -30
E1_SPLIT, E1_TERMS, E1_DEPTH = 2.0, 26, 40
EULER_LD = LD("0.57721566490153286060651209008240243")
EG_MAX = 2.0 ** -30


# ------------------------------------------------------------------ the exponential integral
def e1_coefficients():
    """c_1 .. c_K = (-1)^(k+1) / (k k!) in float64, k! by a running float64 product: the kernel's table."""
    c, fact = np.empty(E1_TERMS), 1.0
    for k in range(1, E1_TERMS + 1):
        fact = fact * float(k)
        c[k - 1] = (1.0 if k & 1 else -1.0) / (float(k) * fact)
    return c


def e1_d(x):
    """The header's E1 in float64, for x > 0 (array)."""
    x = np.asarray(x, dtype=np.float64)
    c = e1_coefficients()
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        s = np.full_like(x, c[-1])
        for k in range(E1_TERMS - 2, -1, -1):
            s = s * x + c[k]
        series = (-float(np.float64(EULER_LD)) - np.log(x)) + s * x
        n, d = x + float(2 * E1_DEPTH + 1), np.ones_like(x)
        for k in range(E1_DEPTH, 0, -1):
            n, d = (x + float(2 * k - 1)) * n - float(k * k) * d, n
        frac = np.exp(-x) * (d / n)
    return np.where(x < E1_SPLIT, series, frac)


def e1_w(x):
    """E1 converged in long double, for x > 0 (array): 60 series terms below 2, a fraction of depth 400 from there."""
    x = np.asarray(x, dtype=LD)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        xs = np.minimum(x, LD(2.0))
        s, term = np.zeros_like(xs), np.ones_like(xs)
        for k in range(1, 61):
            term = term * (-xs) / LD(k)
            s = s - term / LD(k)
        series = -EULER_LD - np.log(xs) + s
        xf = np.maximum(x, LD(2.0))
        f = xf + LD(801)
        for k in range(400, 0, -1):
            f = (xf + LD(2 * k - 1)) - LD(k * k) / f
        frac = np.exp(-xf) / f
    return np.where(x < LD(2.0), series, frac)


# ------------------------------------------------------------------ the definition
def window(N, T):
    k = np.arange(N)
    return np.sin(PI_LD * k.astype(LD) / LD(N)).astype(T) if T is LD else np.sin(np.pi * k / N)


def n_frames(n, N):
    return -(-n // (N // 2)) + 1 if n > 0 else 0


def frames(x, n, N, T):
    """[T_b, N]: the windowed frames of the first n samples of x, in T."""
    h, Tb = N // 2, n_frames(n, N)
    pad = np.zeros((Tb + 1) * h, dtype=T)
    pad[h:h + n] = np.asarray(x[:n]).astype(T)
    idx = np.arange(Tb)[:, None] * h + np.arange(N)[None, :]
    return pad[idx] * window(N, T)[None, :]


def dft_matrix(N):
    """e^{-2 pi i f k / N}, float64 [F, N], from the angle reduced exactly (f k mod N)."""
    m = (np.arange(N // 2 + 1)[:, None] * np.arange(N)[None, :]) % N
    return np.cos(2 * np.pi * m / N) - 1j * np.sin(2 * np.pi * m / N)


def rfft(s, direct=False):
    if direct:
        return s @ dft_matrix(s.shape[1]).T
    return scipy.fft.rfft(s, axis=1)


def irfft(Z, N, direct=False):
    if direct:                                                          # the real inverse of a one-sided spectrum, 1 / N included
        M = dft_matrix(N)
        c = np.full(N // 2 + 1, 2.0)
        c[0] = c[-1] = 1.0
        return ((Z.real * c) @ M.real + (Z.imag * c) @ M.imag) / N
    return scipy.fft.irfft(Z, n=N, axis=1)


def gains(A, p, T, e1):
    """G [T_b, F] and lam [T_b, F] in T from A [T_b, F] and the table row p."""
    rule, D = int(p[0]), int(p[3])
    a_dd, a_n, bias, g_min, xi_min = (T(float(v)) for v in (p[1], p[2], p[4], p[5], p[6]))
    one = T(1.0)
    G, lam_all = np.empty_like(A), np.empty_like(A)
    P = np.empty_like(A)
    prev, Gp, gp = A[0] if len(A) else None, None, None
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for t in range(len(A)):
            P[t] = a_n * prev + (one - a_n) * A[t]
            prev = P[t]
            lam = np.maximum(bias * P[max(0, t - D + 1):t + 1].min(axis=0), T(LAM_MIN))
            gam = np.minimum(A[t] / lam, T(GAMMA_MAX))
            xi = (one - a_dd) * np.maximum(gam - one, T(0.0))
            if t > 0:
                xi = a_dd * (Gp * Gp) * gp + xi
            xi = np.maximum(xi, xi_min)
            q = xi / (one + xi)
            if rule == WIENER:
                g = q
            elif rule == SPECSUB:
                g = np.sqrt(q)
            else:
                g = np.minimum(q * np.exp(e1(np.maximum(q * gam, T(V_MIN))) / T(2.0)), one)
            G[t] = Gp = np.maximum(g, g_min)
            gp, lam_all[t] = gam, lam
    return G, lam_all


class Result(NamedTuple):
    y: np.ndarray            # float32 [n]: f32(w)
    w: np.ndarray            # long double [n]
    d: np.ndarray            # float64 [n], scipy.fft
    d2: np.ndarray           # float64 [n], direct DFT product
    G: np.ndarray            # long double [T_b, F]
    G_d: np.ndarray          # float64
    G_d2: np.ndarray         # float64
    lam: np.ndarray          # long double [T_b, F]


def _one(x, key, n, p, N, T, e1, direct=False):
    h = N // 2
    Tb = n_frames(n, N)
    s = frames(x, n, N, T)
    Y = rfft(s, direct)
    K = Y if key is None else rfft(frames(key, n, N, T), direct)
    A = K.real * K.real + K.imag * K.imag
    G, lam = gains(A, p, T, e1)
    z = irfft(G * Y, N, direct) * window(N, T)[None, :]
    # sample i = t h + r sits at h + i of the padded row: the second half of frame t (the earlier one, added first) plus the
    # first half of frame t + 1
    early = np.concatenate([np.zeros(h, dtype=T), z[:, h:].reshape(-1)])
    late = np.concatenate([z[:, :h].reshape(-1), np.zeros(h, dtype=T)])
    return (early + late)[h:h + n], G, lam


def suppress(x, n, p, N, key=None):
    """The row: Result.  Rule 0 is the copy (w = d = x, gains 1)."""
    x = np.asarray(x, dtype=np.float32)[:n]
    key = None if key is None else np.asarray(key, dtype=np.float32)[:n]
    Tb, F = n_frames(n, N), N // 2 + 1
    if int(p[0]) == OFF or n == 0:
        one = np.ones((Tb, F))
        return Result(x.copy(), x.astype(LD), x.astype(np.float64), x.astype(np.float64), one.astype(LD), one, one.copy(),
                      np.zeros((Tb, F), dtype=LD))
    w, G, lam = _one(x, key, n, p, N, LD, e1_w)
    d, G_d, _ = _one(x, key, n, p, N, np.float64, e1_d)
    d2, G_d2, _ = _one(x, key, n, p, N, np.float64, e1_d, direct=True)
    with np.errstate(over="ignore", invalid="ignore"):
        y = w.astype(np.float32)
    return Result(y, w, d, d2, G, G_d, G_d2, lam)


def _worst(a, b):
    with np.errstate(invalid="ignore"):
        diff = np.abs(a.astype(LD) - b).astype(np.float64)
    diff = diff[~np.isnan(diff)]
    return float(diff.max()) if diff.size else 0.0


def slack(res):
    """E = 8 x max(|d - w|, |d2 - w|) over the row."""
    return 8.0 * max(_worst(res.d, res.w), _worst(res.d2, res.w))


def gain_slack(res):
    """E_G = 8 x max(|G_d - G_w|, |G_d2 - G_w|) over the row's frames and bins."""
    return 8.0 * max(_worst(res.G_d, res.G), _worst(res.G_d2, res.G))


def condition(res):
    """The bound E must respect for the row to be used: 2^-10 x ulp32(rms of the finite w) / 2."""
    v = res.w.astype(np.float64)
    v = v[np.isfinite(v)]
    rms = float(np.sqrt(np.mean(v ** 2))) if v.size else 0.0
    return 2.0 ** -10 * float(ulp32(rms)) / 2.0


def excess(g, w, E):
    """The worst |g - w| - ulp32(w) / 2 - E over the samples (accepted when <= 0); g float32, w long double."""
    if len(w) == 0:
        return -np.inf
    g = np.asarray(g)
    gn, wn = np.isnan(g), np.isnan(w.astype(np.float64))
    if not np.array_equal(gn, wn):
        return np.inf
    keep = ~wn
    if not keep.any():
        return -np.inf
    err = np.abs(g[keep].astype(LD) - w[keep]).astype(np.float64)
    return float(np.max(err - 0.5 * ulp32(w[keep].astype(np.float64)) - E))


def gain_excess(G, G_w, E_G):
    """The worst |G - G_w| - E_G over frames and bins (accepted when <= 0); G float64 [T_b, F]."""
    if G_w.size == 0:
        return -np.inf
    return float(np.max(np.abs(np.asarray(G).astype(LD) - G_w).astype(np.float64))) - E_G


# ------------------------------------------------------------------ table rows and signals
def params(rule=LOGMMSE, a_dd=0.98, a_n=0.8, D=20, bias=1.5, g_min=0.1, xi_min=10.0 ** -2.5):
    return np.array([rule, a_dd, a_n, D, bias, g_min, xi_min], dtype=np.float64)


def noisy(seed, L, sigma=0.02, scale=1.0):
    """transmit_model.speech with broadband noise at -14 dB of the tone's peak, so that no judged bin sits at rounding level."""
    return (scale * speech(seed, L, sigma=sigma)).astype(np.float32)


def white(seed, L, sigma=0.05):
    return (sigma * np.random.default_rng(seed).standard_normal(L)).astype(np.float32)


class Row(NamedTuple):
    x: np.ndarray            # float32 [n] (read-only)
    n: int
    p: np.ndarray            # float64 [7]
    N: int
    key: Optional[np.ndarray]


ROWS = {}
_CASES = {}
H = 128                       # the hop at N = 256
LENGTHS = (1, H - 1, H, H + 1, 2 * H, 5 * H + 37, 2000, 0)


def _register(name, x, p, N=256, key=None):
    assert name not in ROWS
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    if key is not None:
        key = np.ascontiguousarray(key, dtype=np.float32)
        assert len(key) == len(x)
        key.setflags(write=False)
    p = np.array(p, dtype=np.float64)
    p.setflags(write=False)
    ROWS[name] = Row(x, len(x), p, int(N), key)
    return name


def build_rows():
    """Every row a GPU test accepts under the rule, registered once (read-only, shared); tests/test_suppress_host.py checks
    the conditions of the module docstring on each of them without a GPU."""
    if ROWS:
        return ROWS
    for i, n in enumerate(LENGTHS):                                      # 1. lengths, the rules in turn
        _register(f"len-{n}", noisy(1 + i, n), params(rule=1 + i % 3, D=3))
    for rule in (OFF, WIENER, SPECSUB, LOGMMSE):                         # 2. every rule in one batch
        _register(f"rule-{rule}", noisy(20 + rule, 1500), params(rule=rule, D=5))
    for D in (1, 3, 128):                                                # 3. the window: none, sliding out, longer than the row
        _register(f"D-{D}", noisy(30 + D, 1800), params(rule=LOGMMSE, D=D))
    _register("a_dd-0", noisy(40, 1200), params(rule=WIENER, a_dd=0.0))  # 4. extreme values
    _register("a_n-0", noisy(41, 1200), params(rule=LOGMMSE, a_n=0.0, D=4))
    _register("g_min-1", noisy(42, 1200), params(rule=SPECSUB, g_min=1.0))
    _register("xi_min-0", noisy(43, 1200), params(rule=LOGMMSE, xi_min=0.0, D=4))
    _register("xi_min-1", noisy(44, 1200), params(rule=WIENER, xi_min=1.0))
    x = noisy(50, 2000).copy()                                           # 5. digital silence: at the start, and inside
    x[:700] = 0.0
    _register("silence-start", x, params(rule=LOGMMSE, D=3))
    x = noisy(51, 2000).copy()
    x[600:1300] = 0.0
    _register("silence-inside", x, params(rule=WIENER, D=3, xi_min=0.0))
    x = noisy(52, 2000)                                                  # 6. a loud row: peak 4.0
    _register("loud", (x * (4.0 / np.abs(x).max())).astype(np.float32), params(rule=LOGMMSE, D=6))
    for N in (512, 1024):                                                # 7. the other sizes, rows of 3 h + 5
        for j, rule in enumerate((WIENER, SPECSUB, LOGMMSE)):
            _register(f"N-{N}-{rule}", noisy(60 + j + N // 512, 3 * (N // 2) + 5), params(rule=rule, D=2), N=N)
    for j, rule in enumerate((WIENER, SPECSUB, LOGMMSE)):                # 8. a key that is not the signal
        _register(f"key-{rule}", noisy(70 + j, 1500, sigma=0.002), params(rule=rule, D=5), key=noisy(70 + j, 1500, sigma=0.05))
    for i, n in enumerate((2000, 1777, 900, 129)):                       # 9. per-row lengths, bits, independence, graph
        _register(f"rowlen-{i}", noisy(80 + i, n), params(rule=1 + i % 3, D=4))
    for i in range(4):
        _register(f"ok-{i}", noisy(90 + i, 1000), params(rule=1 + i % 3, D=3))
    for i in range(4):
        _register(f"graph-{i}", noisy(100 + i, 1100), params(rule=i, D=2 + i))
    return ROWS


def case(name):
    """(result, E, E_G) of a registered row, computed once."""
    if name not in _CASES:
        row = ROWS[name]
        res = suppress(row.x, row.n, row.p, row.N, row.key)
        _CASES[name] = (res, slack(res), gain_slack(res))
    return _CASES[name]
