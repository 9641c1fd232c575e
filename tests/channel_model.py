"""The float64 model of the recording channel (cmgan_amd/csrc/channel.hip; include/cmgan_hip.h, "Recording channel"),
shared by tests/test_channel_host.py and tests/test_gpu_channel.py.  Nothing here imports the library.

filt      the definition: scipy.signal.sosfilt section by section in float64, then the clip.  sosfilt IS the reference.
filt_ld   the same transposed-direct-form-II loop in np.longdouble (scipy.signal.lfilter keeps long double; it adds
          z2 + b1 u - a1 y in another order than the loop written out in Python, `loop_ld`, and the host tests bound
          the difference: a few long-double roundings, far below the float64 errors E is made of).
tiled     a numpy restatement of the method the kernels are prescribed: runs of `tile / 256` samples from zero state, an
          inclusive scan of the 256 end states of a tile by mat-vecs with A^(run 2^k), a fold over the tiles 256 at a
          time with A^(tile 2^k), and every run again from its entry state (the tile's incoming state through the runs
          before it, composed by the binary digits of the run's index, plus the in-tile scan).

Acceptance rule.  A GPU sample g is accepted against the model's float64 value w when |g - w| <= ulp32(w) / 2 + E, and a
sample the model clips by more than E must equal f32(+-clip) exactly.  E is not a constant: per case it is
8 x max(|filt - filt_ld|, |tiled - filt_ld|) over the case's samples (`slack`), computed from the three functions above
alone.  The factor 8 covers the FMA contraction of the device build and a different association in its scans."""
import math
import warnings

import numpy as np
from scipy import signal

FS = 16000
IDENTITY = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])


# ------------------------------------------------------------------ designs (numpy; the audio-EQ-cookbook formulas)
def peaking(f0, gain_db, q, fs=FS):
    w0 = 2.0 * math.pi * f0 / fs
    alpha, A = math.sin(w0) / (2.0 * q), 10.0 ** (gain_db / 40.0)
    a0 = 1.0 + alpha / A
    return np.array([(1.0 + alpha * A) / a0, -2.0 * math.cos(w0) / a0, (1.0 - alpha * A) / a0, 1.0,
                     -2.0 * math.cos(w0) / a0, (1.0 - alpha / A) / a0])


def highpass(f0, q, fs=FS):
    w0 = 2.0 * math.pi * f0 / fs
    alpha, c = math.sin(w0) / (2.0 * q), math.cos(w0)
    a0 = 1.0 + alpha
    return np.array([0.5 * (1.0 + c) / a0, -(1.0 + c) / a0, 0.5 * (1.0 + c) / a0, 1.0, -2.0 * c / a0, (1.0 - alpha) / a0])


def hard_cascade(fs=FS):
    """The S = 8 cascade the method was checked on: two low-frequency high-Q peaking sections, an 8th-order Butterworth
    low-pass at 3.8 kHz (scipy's own design) and two more peaking sections.  max ||A^k|| is about 255."""
    sos = np.concatenate([[peaking(25.0, 12.0, 4.0, fs), peaking(40.0, -12.0, 8.0, fs)],
                          signal.butter(8, 3800.0, output="sos", fs=fs),
                          [peaking(7000.0, 6.0, 1.0, fs), peaking(300.0, -6.0, 2.0, fs)]])
    assert sos.shape == (8, 6) and np.all(sos[:, 3] == 1.0)
    return sos


def sampler_like(seed, m, fs=FS):
    """m sections of the kind a ChannelSampler draws: a high-pass first, then peaking sections."""
    rng = np.random.default_rng(seed)
    rows = []
    for s in range(m):
        if s == 0:
            rows.append(highpass(float(np.exp(rng.uniform(np.log(20.0), np.log(120.0)))), math.sqrt(0.5), fs))
        else:
            rows.append(peaking(float(np.exp(rng.uniform(np.log(50.0), np.log(0.45 * fs)))), float(rng.uniform(-6.0, 6.0)),
                                float(rng.uniform(0.5, 2.0)), fs))
    return np.array(rows).reshape(m, 6)


def padded(sos, S):
    """sos [m, 6] -> [S, 6], the identity section after the row's own."""
    out = np.tile(IDENTITY, (S, 1))
    out[:len(sos)] = sos
    return out


def noise(seed, L, sigma=0.3):
    return (sigma * np.random.default_rng(seed).standard_normal(L)).astype(np.float32)


# ------------------------------------------------------------------ the definition
def _clip(y, clip):
    return y if clip is None or np.isposinf(clip) else np.clip(y, -clip, clip)


def filt(x, n, sos, m, clip=None):
    """Row x[:n] through sections 0 .. m-1 of sos in float64, limited to [-clip, clip]: float64 [n]."""
    y = np.array(x[:n], dtype=np.float64)                                # copies: sosfilt wants writeable buffers
    for s in range(m if n else 0):
        y = signal.sosfilt(np.array(sos[s:s + 1], dtype=np.float64), y)
    return _clip(y, clip)


def filt_ld(x, n, sos, m, clip=None):
    """The same loop in long double: np.longdouble [n]."""
    y = np.asarray(x[:n], dtype=np.longdouble)
    for s in range(m if n else 0):
        c = np.asarray(sos[s], dtype=np.longdouble)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", DeprecationWarning)      # scipy is to drop long double from lfilter
                out = signal.lfilter(c[:3], c[3:], y)
        except (TypeError, ValueError, NotImplementedError):
            out = None
        y = out if out is not None and out.dtype == np.longdouble else loop_ld(y, n, sos[s:s + 1], 1)
    return _clip(y, None if clip is None else np.longdouble(clip))


def loop_ld(x, n, sos, m):
    """filt_ld written out: y = b0 u + z1, z1 <- b1 u - a1 y + z2, z2 <- b2 u - a2 y.  Slow; for short rows."""
    y = np.asarray(x[:n], dtype=np.longdouble).copy()
    for s in range(m):
        b0, b1, b2, _, a1, a2 = (np.longdouble(v) for v in sos[s])
        z1 = z2 = np.longdouble(0)
        for i in range(n):
            u = y[i]
            v = b0 * u + z1
            z1 = b1 * u - a1 * v + z2
            z2 = b2 * u - a2 * v
            y[i] = v
    return y


# ------------------------------------------------------------------ the prescribed method, restated
def system_matrix(sos, m):
    """A of z' = A z for zero input, z = (z1, z2) of every section in order: block lower-triangular."""
    A = np.zeros((2 * m, 2 * m))
    w = np.zeros(m)
    for s in range(m):
        b0, b1, b2, _, a1, a2 = sos[s]
        c1, c2 = b1 - a1 * b0, b2 - a2 * b0
        for q in range(s):
            A[2 * s, 2 * q] = c1 * w[q]
            A[2 * s + 1, 2 * q] = c2 * w[q]
            w[q] *= b0
        w[s] = 1.0
        A[2 * s, 2 * s], A[2 * s, 2 * s + 1], A[2 * s + 1, 2 * s] = -a1, 1.0, -a2
    return A


def _run(sos, m, u, z):
    """u [R, run] through the cascade from states z [R, 2m] (both changed in place): outputs in u, end states in z."""
    for r in range(u.shape[1]):
        v = u[:, r].copy()
        for s in range(m):
            b0, b1, b2, _, a1, a2 = sos[s]
            y = b0 * v + z[:, 2 * s]
            z[:, 2 * s] = b1 * v - a1 * y + z[:, 2 * s + 1]
            z[:, 2 * s + 1] = b2 * v - a2 * y
            v = y
        u[:, r] = v


def _scan(v, P):
    """Inclusive scan along axis 1 (256 segments of states v [G, 256, N]): step k composes with P[k] = A^(unit 2^k)."""
    for k in range(8):
        s = 1 << k
        v[:, s:] = v[:, :-s] @ P[k].T + v[:, s:]
    return v


def _advance(z, d, P, digits):
    """z [R, N] <- A^(unit d) z, the factor composed from P[k] by the binary digits of d [R], lowest first."""
    for k in range(digits):
        on = ((d >> k) & 1).astype(bool)
        z[on] = z[on] @ P[k].T
    return z


def tiled(x, n, sos, m, clip=None, tile=2048):
    assert tile % 256 == 0 and tile >= 256
    run = tile // 256
    assert run & (run - 1) == 0
    x = np.asarray(x[:n], dtype=np.float64)
    if m == 0 or n == 0:
        return _clip(x.copy(), clip)
    N = 2 * m
    A = system_matrix(sos, m)
    P, cur = [], np.linalg.matrix_power(A, run)
    for _ in range(17):
        P.append(cur)
        cur = cur @ cur
    PR, PT = P[:8], P[8:]
    nt = -(-n // tile)
    xp = np.zeros(nt * tile)
    xp[:n] = x
    runs = xp.reshape(nt * 256, run)
    z = np.zeros((nt * 256, N))
    _run(sos, m, runs.copy(), z)
    incl = _scan(z.reshape(nt, 256, N), PR)                              # in-tile scan of the runs' end states
    seg = incl[:, 255].copy()
    inc = np.zeros((nt, N))
    c = np.zeros(N)
    for k0 in range(0, nt, 256):                                         # the fold, 256 tiles at a time
        chunk = np.zeros((1, 256, N))
        nk = min(256, nt - k0)
        chunk[0, :nk] = seg[k0:k0 + nk]
        sc = _scan(chunk, PT)[0]
        f = _advance(np.tile(c, (256, 1)), np.arange(1, 257), PT, 9) + sc
        inc[k0] = c
        inc[k0 + 1:k0 + nk] = f[:nk - 1]
        c = f[255]
    t = np.tile(np.arange(256), nt)
    entry = _advance(np.repeat(inc, 256, axis=0), t, PR, 8)
    excl = np.zeros((nt, 256, N))
    excl[:, 1:] = incl[:, :-1]
    entry += excl.reshape(nt * 256, N)
    out = runs.copy()
    _run(sos, m, out, entry)
    return _clip(out.reshape(-1)[:n], clip)


# ------------------------------------------------------------------ the acceptance rule
def ulp32(w):
    """The float32 spacing at |w| (w float64): 2^(e - 24) for |w| in [2^(e-1), 2^e), at least the denormal 2^-149."""
    w = np.abs(np.asarray(w, dtype=np.float64))
    _, e = np.frexp(w)
    return np.where(w == 0.0, 2.0 ** -149, np.ldexp(1.0, np.maximum(e - 24, -149)))


def slack(x, n, sos, m, tile=2048):
    """E of a case's row: 8 x max(|filt - filt_ld|, |tiled - filt_ld|), from the model alone (no clip)."""
    if n == 0:
        return 0.0
    ref = filt_ld(x, n, sos, m)
    a = np.max(np.abs(filt(x, n, sos, m).astype(np.longdouble) - ref))
    b = np.max(np.abs(tiled(x, n, sos, m, None, tile).astype(np.longdouble) - ref))
    return 8.0 * float(max(a, b))


def excess(g, x, n, sos, m, clip, E):
    """The worst |g - w| - ulp32(w) / 2 - E over the row (accepted when <= 0), and whether every sample that the model
    clips by more than E is f32(+-clip) exactly.  g float32 [n]."""
    raw = filt(x, n, sos, m)
    w = _clip(raw, clip)
    if n == 0:
        return -np.inf, True
    worst = float(np.max(np.abs(g.astype(np.float64) - w) - 0.5 * ulp32(w) - E))
    exact = True
    if clip is not None and not np.isposinf(clip):
        hi, lo = raw > clip + E, raw < -clip - E
        exact = bool(np.all(g[hi] == np.float32(clip)) and np.all(g[lo] == np.float32(-clip)))
    return worst, exact
