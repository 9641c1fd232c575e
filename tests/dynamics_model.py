"""The float64 model of the gain control (cmgan_amd/csrc/dynamics.hip; include/cmgan_hip.h, "Dynamics"), shared by
tests/test_dynamics_host.py and tests/test_gpu_dynamics.py.  Nothing here imports the library.

serial    the definition: the wanted reduction c per sample (vectorised), the branching attack / release loop sample by
          sample, the gain and the product - in float64, or in np.longdouble with dtype=.
tiled     a numpy restatement of the method the kernels are prescribed: per tile of T samples the T + 1 offsets b_k of
          y -> max_k (a_att^k a_rel^(T-k) y + b_k) by the (max, +) recurrence, a fold of the tile maps in ascending order
          for every tile's entry state, and every tile again from its entry state in the branching form.

Acceptance rule (that of tests/channel_model.py).  A GPU sample g is accepted against the model's float64 value w when
|g - w| <= ulp32(w) / 2 + E.  E is not a constant: per row it is 8 x max(|serial64 - serial_ld|, |tiled64 - serial_ld|)
over the row's samples (`slack`), computed from the functions above alone.  The factor 8 covers the fused multiply-adds
of the device build and its own log10 and 10^x.  Every sample of every row is judged; a sample the model makes NaN or
+-inf must be the same on the GPU."""
import numpy as np

FS = 16000
TILE = 64          # cmgan_dynamics_tile(); the host tests assert that the library says the same


# ------------------------------------------------------------------ tables and signals
def coeff(ms, fs=FS):
    """exp(-1 / (t fs)) for a time constant of `ms` milliseconds; 0 ms is instant (0)."""
    return 0.0 if ms == 0 else float(np.exp(-1000.0 / (ms * fs)))


def params(thr_db, ratio, knee_db, attack_ms, release_ms, makeup_db=0.0, fs=FS):
    """One row of the table: (thr_db, slope, knee_db, a_att, a_rel, makeup_db)."""
    slope = 1.0 if np.isinf(ratio) else 1.0 - 1.0 / ratio
    return np.array([thr_db, slope, knee_db, coeff(attack_ms, fs), coeff(release_ms, fs), makeup_db], dtype=np.float64)


def bursts(seed, L, quiet=0.003, loud=0.5):
    """Float32 noise whose level jumps every 40 .. 400 samples between `quiet` and `loud` (log-uniform): onsets, pauses
    and everything a knee can meet in between."""
    rng = np.random.default_rng(seed)
    env = np.empty(L)
    i = 0
    while i < L:
        k = int(rng.integers(40, 401))
        env[i:i + k] = np.exp(rng.uniform(np.log(quiet), np.log(loud)))
        i += k
    return (env * rng.standard_normal(L)).astype(np.float32)


# ------------------------------------------------------------------ the definition
def want(key, thr, slope, knee, dtype=np.float64):
    """c: the wanted reduction in dB per key sample, >= 0; a sample that is not finite counts as silence (0)."""
    k = np.asarray(key, dtype=dtype)
    thr, slope, knee = dtype(thr), dtype(slope), dtype(knee)
    finite = np.isfinite(k)
    m = np.abs(np.where(finite, k, dtype(1)))
    d = dtype(20) * np.log10(np.maximum(m, dtype(1e-6))) - thr
    t = d + dtype(0.5) * knee
    with np.errstate(divide="ignore", invalid="ignore"):
        soft = slope * (t * (t / (dtype(2) * knee)))
    c = np.where(dtype(2) * d < -knee, dtype(0), np.where((dtype(2) * np.abs(d) <= knee) & (knee > 0), soft, slope * d))
    return np.where(finite, c, dtype(0)).astype(dtype)


def detect(c, a_att, a_rel, y0=0.0, dtype=np.float64):
    """y: the branching peak detector over c from the state y0, sample by sample."""
    a_att, a_rel = dtype(a_att), dtype(a_rel)
    oma, omr = dtype(1) - a_att, dtype(1) - a_rel
    y, out = dtype(y0), np.empty(len(c), dtype=dtype)
    for i, ci in enumerate(c):
        y = a_att * y + oma * ci if ci > y else a_rel * y + omr * ci
        out[i] = y
    return out


def _apply(wav, y, makeup, dtype):
    g = dtype(makeup) - y
    with np.errstate(over="ignore", invalid="ignore"):
        gain = np.where(g == 0, dtype(1), np.power(dtype(10), g / dtype(20)))
        return np.asarray(wav, dtype=dtype) * gain


def serial(wav, key, n, dyn, dtype=np.float64):
    """(out [n], y [n]) of the row wav[:n] with the level taken from key[:n] (None: from wav), in `dtype`."""
    thr, slope, knee, a_att, a_rel, makeup = (float(v) for v in dyn)
    k = wav if key is None else key
    y = detect(want(k[:n], thr, slope, knee, dtype), a_att, a_rel, 0.0, dtype)
    return _apply(wav[:n], y, makeup, dtype), y


# ------------------------------------------------------------------ the prescribed method, restated
def tile_maps(c, a_att, a_rel):
    """c [nt, T] -> the offsets b [nt, T + 1] of every tile's map, b_k for k attack steps (needs a_att <= a_rel)."""
    nt, T = c.shape
    b = np.zeros((nt, T + 1))
    for i in range(T):                       # before step i the entries k <= i are real; the others are never read by them
        ci = c[:, i:i + 1]
        att = np.zeros_like(b)
        att[:, 1:] = a_att * b[:, :-1] + (1.0 - a_att) * ci
        rel = a_rel * b + (1.0 - a_rel) * ci
        new = np.maximum(att, rel)
        new[:, 0] = rel[:, 0]
        new[:, i + 1] = att[:, i + 1]
        b = new
    return b


def tile_slopes(a_att, a_rel, T):
    """a_att^k a_rel^(T - k), k = 0 .. T, by T products in the order the kernels take them."""
    k, p = np.arange(T + 1), np.ones(T + 1)
    for i in range(T):
        p = p * np.where(i < k, a_att, a_rel)
    return p


def entry_states(c, a_att, a_rel, T=TILE):
    """The detector's state before every tile of c [n] (the last one may be short): float64 [ceil(n / T)]."""
    n = len(c)
    nt = -(-n // T)
    sg = 1.0 if a_att <= a_rel else -1.0     # attack slower than release: min instead of max, so the negated problem
    full = (sg * c[:(nt - 1) * T]).reshape(nt - 1, T)
    b, p = tile_maps(full, a_att, a_rel), tile_slopes(a_att, a_rel, T)
    inc, y = np.zeros(nt), 0.0
    for t in range(nt):
        inc[t] = sg * y if y != 0.0 else 0.0
        if t < nt - 1:
            y = float(np.max(p * y + b[t]))
    return inc


def tiled(wav, key, n, dyn, T=TILE):
    """(out [n], y [n]) by the tiled method, float64."""
    thr, slope, knee, a_att, a_rel, makeup = (float(v) for v in dyn)
    k = wav if key is None else key
    if n == 0:
        return np.zeros(0), np.zeros(0)
    c = want(k[:n], thr, slope, knee)
    nt = -(-n // T)
    cp = np.zeros(nt * T)
    cp[:n] = c
    cp = cp.reshape(nt, T)
    y, ys = entry_states(c, a_att, a_rel, T), np.empty((nt, T))
    for i in range(T):                       # every tile from its entry state, all tiles at once
        ci = cp[:, i]
        y = np.where(ci > y, a_att * y + (1.0 - a_att) * ci, a_rel * y + (1.0 - a_rel) * ci)
        ys[:, i] = y
    ys = ys.reshape(-1)[:n]
    return _apply(wav[:n], ys, makeup, np.float64), ys


# ------------------------------------------------------------------ the acceptance rule
def ulp32(w):
    """The float32 spacing at |w| (w float64): 2^(e - 24) for |w| in [2^(e-1), 2^e), at least the denormal 2^-149."""
    w = np.abs(np.asarray(w, dtype=np.float64))
    _, e = np.frexp(w)
    return np.where(w == 0.0, 2.0 ** -149, np.ldexp(1.0, np.maximum(e - 24, -149)))


def slack(wav, key, n, dyn, T=TILE):
    """(E, Ey) of a row: 8 x max(|serial64 - serial_ld|, |tiled64 - serial_ld|) over its finite output samples, and the
    same over the detector's y (for peak_reduction_db).  From the model alone."""
    if n == 0:
        return 0.0, 0.0
    (o64, y64), (old, yld), (ot, yt) = serial(wav, key, n, dyn), serial(wav, key, n, dyn, np.longdouble), tiled(wav, key, n, dyn, T)
    ok = np.isfinite(old)
    def dist(a, ref, m):
        with np.errstate(invalid="ignore"):
            return float(np.max(np.abs(a.astype(np.longdouble) - ref)[m], initial=0.0))
    every = np.ones(n, dtype=bool)
    return (8.0 * max(dist(o64, old, ok), dist(ot, old, ok)), 8.0 * max(dist(y64, yld, every), dist(yt, yld, every)))


def excess(g, wav, key, n, dyn, E):
    """The worst |g - w| - ulp32(w) / 2 - E over the row's finite samples (accepted when <= 0), and whether every sample
    that the model makes NaN or +-inf is the same in g.  g float32 [n]."""
    if n == 0:
        return -np.inf, True
    w, _ = serial(wav, key, n, dyn)
    ok = np.isfinite(w)
    same = bool(np.array_equal(g[~ok].astype(np.float64), w[~ok], equal_nan=True))
    with np.errstate(invalid="ignore"):
        worst = float(np.max((np.abs(g.astype(np.float64) - w) - 0.5 * ulp32(w) - E)[ok], initial=-np.inf))
    return worst, same


# ------------------------------------------------------------------ the rows of the GPU tests
def mix_rows():
    """The per-row parameter mixes of one batch: name -> table row."""
    return {
        "limiter": params(-20.0, np.inf, 0.0, 1.0, 100.0),
        "hard_knee": params(-25.0, 4.0, 0.0, 5.0, 200.0, 3.0),
        "wide_knee": params(-25.0, 3.0, 24.0, 10.0, 300.0, 2.0),
        "slope0": params(-30.0, 1.0, 6.0, 5.0, 100.0),
        "slow_attack": params(-30.0, 8.0, 6.0, 40.0, 10.0, 4.0),
        "instant_attack": params(-20.0, 10.0, 3.0, 0.0, 150.0),
        "equal_times": params(-28.0, 6.0, 6.0, 30.0, 30.0, 1.0),
        "instant_release": params(-22.0, 5.0, 2.0, 10.0, 0.0),
    }


def edge_lengths(T=TILE):
    """Row lengths at every edge the kernels have: the tile, the 4 tiles of a dynamics_tile block, the 8 tiles of a fold
    chunk (the row's last tile is not folded, so 9 tiles are the first to need a second chunk), the 64 tiles of a
    dynamics_apply block."""
    return [1, T - 1, T, T + 1, 2 * T + 1, 4 * T, 4 * T + 1, 8 * T + 1, 9 * T, 9 * T + 1, 16 * T + 1, 17 * T + 1, 64 * T - 1, 64 * T,
            64 * T + 1, 65 * T + 1]
