"""The numpy model of cmgan_scene_path (cmgan_amd/csrc/scene.hip; include/cmgan_hip.h, "Paths"), shared by
tests/test_path_host.py and tests/test_gpu_path.py.  Nothing here imports the library.

A row is the row of tests/scene_model.py with a PATH of responses for the talker and for every source: waypoint p sits at
input sample p H and weights the input samples around it,

    u_p[m] = float64(H - |m - p H|) / float64(H) where positive, else 0;  u_0[m] = 1 for m <= 0,
    u_{Pb-1}[m] = 1 for m >= (Pb - 1) H                              (an exact integer numerator, one IEEE division)
    xw_p[m] = u_p[m] * float64(x[m])                                  rounded once to float64 - in ALL three forms: it is
                                                                      part of the definition, not of the arithmetic judged
    speech[i] = sum_p sum_k h_p[k] xw_p[i + d_p - k]                  d_p the first argmax of |h_p|; x = clean, 0 outside [0, L)
    target[i] = the same over k <= d_p + early                        (early == -1: the clean row)
    c_j[i]    = sum_p sum_k h_jp[k] xw_p[i - k]                       x = seg_j, looping both ways; every integer m weighted

and everything after the convolutions is scene_model's: powers, gains, v = speech + g0 n0 + g_1 c_1 + ..., the peak guard.

direct      float64 by the definition: np.convolve per waypoint, the waypoints added in ascending p; np.mean, np.max.
direct_ld   the same in np.longdouble: the value w a device sample is judged against.
as_kernel   float64 in the kernel's order: ONE accumulator over (p ascending, k ascending), the powers and the maximum
            through scene_model's tile / tree reductions.

The acceptance rule and its condition are scene_model's, unchanged (`slack`, `condition`, `excess`, `ulp32` are its own):
|g - w| <= ulp32(w) / 2 + E with E = 8 x max(|direct - w|, |as_kernel - w|) per row, usable only if
E <= 2^-10 x ulp32(rms w) / 2.  Every judged row is one of BATCHES (`build_batches`)."""
from typing import NamedTuple, Optional

import numpy as np

import mix_model
import scene_model as S

LD = S.LD
condition, excess, ulp32 = S.condition, S.excess, S.ulp32


# ------------------------------------------------------------------ one row's inputs
class PathSource(NamedTuple):
    start: int
    length: int
    off: int
    snr_db: np.float32
    hs: tuple                        # float32 taps per waypoint, the source's own count of them


class PathRowIn(NamedTuple):
    clean: np.ndarray                # float32 [L]
    hs: tuple                        # the talker's taps per waypoint (Pb of them)
    H: int
    noise_bank: Optional[np.ndarray]
    noise: Optional[tuple]           # (start, length, off, snr_db), None: no dry noise
    src_bank: Optional[np.ndarray]
    sources: tuple                   # of PathSource
    peak: float
    early: int


def weights(p, Pb, H, m):
    """u_p[m], float64, for an int64 array m of any sign."""
    m = np.asarray(m, dtype=np.int64)
    a = m - np.int64(p) * np.int64(H)
    u = np.where(np.abs(a) < H, (np.int64(H) - np.abs(a)).astype(np.float64) / np.float64(H), 0.0)
    if p == 0:
        u = np.where(a <= 0, 1.0, u)
    if p == Pb - 1:
        u = np.where(a >= 0, 1.0, u)
    return u


def _along(x, lo, hs, ds, H, L, mode, early=None):
    """out[i] = sum_p sum_k h_p[k] u_p[m] x[m], m = i + d_p - k, for 0 <= i < L.  The float32 array x holds the signal at
    the input indices lo .. lo + len(x) - 1 and is zero elsewhere; early: the target's prefix k <= d_p + early.  With one
    waypoint these are scene_model's own operations on its own arrays, so the values are its values."""
    F = LD if mode == "ld" else np.float64
    Pb, pad = len(hs), max(len(h) for h in hs)
    m = lo + np.arange(len(x), dtype=np.int64)
    out = np.zeros(L, dtype=F)
    i = np.arange(L)
    for p, (h, d) in enumerate(zip(hs, ds)):
        K = len(h) if early is None else min(d + int(early), len(h) - 1) + 1
        xw = weights(p, Pb, H, m) * x.astype(np.float64)              # the one float64 rounding of the definition
        hh = h.astype(F)
        if mode == "kernel":
            xp = np.concatenate([np.zeros(pad), xw, np.zeros(pad)])   # xp[pad + q] = xw[q]
            for k in range(K):
                out = out + hh[k] * xp[pad + i + d - k - lo]
        else:
            full = np.convolve(xw.astype(F), hh[:K])                  # full[n] = sum_k h[k] xw[n - k]: out[i] = full[i + d - lo]
            n = min(L, full.size - (d - lo))
            if n > 0:
                out[:n] = out[:n] + full[d - lo:d - lo + n]
    return out


def _row(r: PathRowIn, mode):
    F = LD if mode == "ld" else np.float64
    clean = np.asarray(r.clean, dtype=np.float32)
    L, H = clean.size, int(r.H)
    hs = [np.asarray(h, dtype=np.float32) for h in r.hs]
    ds = [mix_model.direct_path(h) for h in hs]
    power = S._power_kernel if mode == "kernel" else (lambda x: F(np.mean(x * x)))
    peak_of = S._max_kernel if mode == "kernel" else (lambda x: F(np.max(np.abs(x))))
    speech = _along(clean, 0, hs, ds, H, L, mode)
    target = clean.astype(F) if r.early < 0 else _along(clean, 0, hs, ds, H, L, mode, r.early)
    ps = power(speech)
    ten = F(10)

    def gain(p, snr_db):
        if ps == 0 or p == 0:
            return F(0)
        return np.sqrt(ps / (p * ten ** (F(float(np.float32(snr_db))) / ten)))

    v = speech.copy()
    g, P, cs = [F(0)], [F(0)], []
    if r.noise is not None:
        st, ln, off, snr = r.noise
        n0 = S.looped(r.noise_bank, st, ln, off, np.arange(L)).astype(F) if S.segment_ok(r.noise_bank, st, ln) else np.zeros(L, dtype=F)
        P[0] = power(n0)
        g[0] = gain(P[0], snr)
        v = v + g[0] * n0
    for s in r.sources:
        hj = [np.asarray(h, dtype=np.float32) for h in s.hs]
        if S.segment_ok(r.src_bank, s.start, s.length):
            back = max(len(h) for h in hj) - 1                       # the furthest a tap reaches back
            sig = S.looped(r.src_bank, s.start, s.length, s.off, np.arange(-back, L))          # sig[back + m] = seg[m]
            c = _along(sig, -back, hj, [0] * len(hj), H, L, mode)
        else:
            c = np.zeros(L, dtype=F)
        pc = power(c)
        gj = gain(pc, s.snr_db)
        v = v + gj * c
        g.append(gj)
        P.append(pc)
        cs.append(c)
    m = peak_of(v)
    pk = F(float(np.float32(r.peak)))
    scale = pk / m if m > pk else F(1)
    return {"noisy": v * scale, "target": target * scale, "g": g, "P": P, "Ps": ps, "scale": scale, "c": cs, "d": ds,
            "speech": speech}


def direct(r):
    return _row(r, "direct")


def direct_ld(r):
    return _row(r, "ld")


def as_kernel(r):
    return _row(r, "kernel")


def slack(r: PathRowIn):
    """scene_model.slack for a path row: {"noisy": (E, w), "target": (E, w)} and the long-double row."""
    ld, a, b = direct_ld(r), direct(r), as_kernel(r)
    out = {}
    for key in ("noisy", "target"):
        w = ld[key]
        e = max(np.max(np.abs(a[key].astype(LD) - w)), np.max(np.abs(b[key].astype(LD) - w)))
        out[key] = (8.0 * float(e), w)
    return out, ld


# ------------------------------------------------------------------ batches: the arguments of one Engine.scene_path call
class PathBatch(NamedTuple):
    clean: np.ndarray                        # float32 [B, L]
    H: int
    n_path: np.ndarray                       # int32 [B]
    rir: np.ndarray                          # float32 [R, Kmax]
    rir_index: np.ndarray                    # int32 [B, P]
    rir_len: np.ndarray
    noise_bank: Optional[np.ndarray]         # None: no dry noise
    noise_start: Optional[np.ndarray]
    noise_len: Optional[np.ndarray]
    noise_off: Optional[np.ndarray]
    snr_db: Optional[np.ndarray]
    n_src: Optional[np.ndarray]              # int32 [B], None: S = 0
    src_bank: Optional[np.ndarray]
    src_start: Optional[np.ndarray]          # int64 [B, S] ...
    src_len: Optional[np.ndarray]
    src_off: Optional[np.ndarray]
    src_snr_db: Optional[np.ndarray]
    src_n_path: Optional[np.ndarray]         # int32 [B, S]
    src_rir_index: Optional[np.ndarray]      # int32 [B, S, P]
    src_rir_len: Optional[np.ndarray]
    peak: float
    early: int


def _path(rir, idx, length, n):
    P = len(idx)
    return tuple(S._taps(rir, idx[p], length[p]) for p in range(min(max(int(n), 1), P)))


def row_of(bt: PathBatch, b: int) -> PathRowIn:
    """Row b as the model takes it: the clamps of the untrusted tables applied (n_path to [1, P], indices, lengths), the
    sources beyond n_src and the waypoints beyond a path's own count dropped."""
    ns = 0 if bt.n_src is None else bt.src_start.shape[1]
    sb = 0 if bt.n_src is None else min(max(int(bt.n_src[b]), 0), ns)
    srcs = tuple(PathSource(int(bt.src_start[b, j]), int(bt.src_len[b, j]), int(bt.src_off[b, j]), bt.src_snr_db[b, j],
                            _path(bt.rir, bt.src_rir_index[b, j], bt.src_rir_len[b, j], bt.src_n_path[b, j]))
                 for j in range(sb))
    noise = None if bt.noise_bank is None else (int(bt.noise_start[b]), int(bt.noise_len[b]), int(bt.noise_off[b]), bt.snr_db[b])
    return PathRowIn(bt.clean[b], _path(bt.rir, bt.rir_index[b], bt.rir_len[b], bt.n_path[b]), int(bt.H), bt.noise_bank, noise,
                     bt.src_bank, srcs, bt.peak, bt.early)


def static_batch(bt: PathBatch) -> S.Batch:
    """The scene_model.Batch of column 0 of the path tables: what Engine.scene takes for a batch that stands still."""
    col = lambda t: None if t is None else np.ascontiguousarray(t[..., 0])
    return S.Batch(bt.clean, bt.noise_bank, bt.noise_start, bt.noise_len, bt.noise_off, bt.snr_db, bt.n_src, bt.src_bank,
                   bt.src_start, bt.src_len, bt.src_off, bt.src_snr_db, bt.rir, col(bt.rir_index), col(bt.rir_len),
                   col(bt.src_rir_index), col(bt.src_rir_len), bt.peak, bt.early)


BATCHES = {}
_CASES = {}


def case(name, b):
    """(slack dict, long-double row) of row b of a registered batch, computed once."""
    if (name, b) not in _CASES:
        _CASES[(name, b)] = slack(row_of(BATCHES[name], b))
    return _CASES[(name, b)]


def response(K, d, rng, sign=1.0):
    """A decaying-noise response of K taps whose largest tap is at min(d, K - 1)."""
    h = 0.5 * rng.standard_normal(K) * np.exp(-np.arange(K) / (0.15 * K + 1.0))
    h[min(d, K - 1)] = 1.5 * sign
    return h.astype(np.float32)


DIRECTS = (0, 5, 40)             # the direct indices the waypoints of one path cycle through


def make_batch(seed, L, H, P, early, n_path, talker_K, n_src, src_n_path, src_K, src_len, src_off, dry=True, peak=0.99,
               bank_len=6000):
    """A batch of len(n_path) rows with P waypoint columns and 2 source columns.  talker_K: [B] response lengths (all the
    waypoints of a row), src_K / src_len / src_off / src_n_path: [B][2].  Waypoint p of row b has its direct path at
    DIRECTS[(b + p) % 3] (clipped to its length), so neighbouring waypoints of a path differ; every (row, waypoint) and
    (row, source, waypoint) has a bank row of its own, the columns beyond a path included."""
    rng = np.random.default_rng(seed)
    B, NS = len(n_path), 2
    src_K, src_len, src_off = (np.asarray(v, dtype=np.int64).reshape(B, NS) for v in (src_K, src_len, src_off))
    Kmax = int(max(max(talker_K), src_K.max())) + 3
    rir = np.zeros((B * P + B * NS * P, Kmax), dtype=np.float32)
    rir_len = np.zeros((B, P), dtype=np.int32)
    src_rir_len = np.zeros((B, NS, P), dtype=np.int32)
    for b in range(B):
        for p in range(P):
            K = int(talker_K[b])
            rir[b * P + p, :K] = response(K, DIRECTS[(b + p) % 3], rng, (-1.0) ** p)
            rir_len[b, p] = K
            for j in range(NS):
                K = int(src_K[b, j])
                rir[B * P + (b * NS + j) * P + p, :K] = response(K, DIRECTS[(b + j + p) % 3], rng)
                src_rir_len[b, j, p] = K
    bank = rng.standard_normal(bank_len).astype(np.float32)
    src_bank = (0.5 * rng.standard_normal(bank_len)).astype(np.float32)
    src_start = np.array([[int(rng.integers(0, bank_len - max(int(src_len[b, j]), 1) + 1)) for j in range(NS)] for b in range(B)],
                         dtype=np.int64)
    return S._freeze(PathBatch(
        clean=(0.1 * rng.standard_normal((B, L))).astype(np.float32), H=int(H), n_path=np.asarray(n_path, dtype=np.int32), rir=rir,
        rir_index=np.arange(B * P, dtype=np.int32).reshape(B, P), rir_len=rir_len,
        noise_bank=bank if dry else None,
        noise_start=rng.integers(0, 100, B).astype(np.int64) if dry else None,
        noise_len=rng.integers(1, bank_len - 100, B).astype(np.int64) if dry else None,
        noise_off=rng.integers(-10 ** 6, 10 ** 6, B).astype(np.int64) if dry else None,
        snr_db=rng.uniform(0.0, 20.0, B).astype(np.float32) if dry else None,
        n_src=np.asarray(n_src, dtype=np.int32), src_bank=src_bank, src_start=src_start, src_len=src_len.copy(),
        src_off=src_off.copy(), src_snr_db=rng.uniform(-5.0, 15.0, (B, NS)).astype(np.float32),
        src_n_path=np.asarray(src_n_path, dtype=np.int32).reshape(B, NS),
        src_rir_index=(B * P + np.arange(B * NS * P, dtype=np.int32)).reshape(B, NS, P), src_rir_len=src_rir_len, peak=peak,
        early=early))


KBIG = 1300                      # more than scene_model.KC taps: two staged chunks per waypoint


def _walk(seed, L, H, P, early, dry=True):
    """Six rows that take the walk everywhere it can go for one (L, H, P, early):
      0  every column, long responses (two chunks; K > L at the short L); sources of 1 sample and of a 3-sample loop, the
         second with a path shorter than the talker's
      1  STATIC between moving rows: n_path = 1, both sources with one waypoint
      2  half the columns (the last one holds), K = 40; a source of K taps at a negative offset, one invalid segment
      3  n_path = 0 (clamped to 1) with moving sources, one of them with src_n_path = P + 3
      4  n_path = P + 3 (clamped to P), K = 1: no reverberation at all, d = 0 everywhere; no source
      5  two columns, K = 200; one source"""
    half = max(P // 2, 2)
    return make_batch(
        seed, L, H, P, early, n_path=[P, 1, half, 0, P + 3, 2], talker_K=[KBIG, 40, 40, 60, 1, 200], n_src=[2, 2, 2, 2, 0, 1],
        src_n_path=[[P, 2], [1, 1], [half, P], [3, P + 3], [P, P], [0, 1]],
        src_K=[[40, 300], [KBIG, 1], [40, 40], [1, 90], [40, 40], [60, 40]],
        src_len=[[1, 3], [700, 5000], [333, 0], [L + 50, 7], [9, 9], [2000, 9]],
        src_off=[[0, -2], [-5, 10 ** 9 + 1], [-(10 ** 7) - 3, 0], [-1, 4], [0, 0], [-777, 0]], dry=dry)


def build_batches(T):
    """Every batch whose rows a GPU test accepts under the rule, registered once (read-only, shared).  T: cmgan_mix_tile().
    With KC = 1024 taps per staged chunk:
      h37    L = T - 1,           H = 37 (28 waypoints inside the one tile; (P - 1) H < L: the last one holds), early = 0
      htile  L = 2 T + T / 2 + 7, H = T,   P = 5: the window of column 4 starts behind the clip - never reached; early = 200
      h1500  L = 2 T + T / 2 + 7, H = 1500 (straddles tiles, no multiple of anything), P = 3; dry target; no dry noise
      hfar   L = T - 1,           H = 4000 > L: only the first cross-fade begins; early >= every K"""
    if BATCHES:
        return BATCHES
    assert T == S.TPB * S.OPT
    long_L = 2 * T + T // 2 + 7
    BATCHES["h37"] = _walk(1100, T - 1, 37, 28, 0)
    BATCHES["htile"] = _walk(1200, long_L, T, 5, 200)
    BATCHES["h1500"] = _walk(1300, long_L, 1500, 3, -1, dry=False)
    BATCHES["hfar"] = _walk(1400, T - 1, 4000, 3, 5000)
    # graph replay: the tables before and after they are rewritten (other paths, other lengths, other sources)
    g0 = _walk(1500, 900, 250, 4, 30)
    BATCHES["graph-0"] = g0
    BATCHES["graph-1"] = S._freeze(g0._replace(
        n_path=np.array([2, 4, 1, 3, 1, 4], dtype=np.int32), rir_index=g0.rir_index[::-1].copy(),
        rir_len=np.maximum(g0.rir_len[::-1] - 7, 1).astype(np.int32), src_n_path=g0.src_n_path[::-1].copy(),
        src_rir_index=g0.src_rir_index[:, ::-1].copy(), n_src=np.array([1, 0, 2, 2, 2, 2], dtype=np.int32),
        src_off=g0.src_off + 12345, noise_off=g0.noise_off - 77))
    return BATCHES
