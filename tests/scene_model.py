"""The numpy model of cmgan_scene (cmgan_amd/csrc/scene.hip; include/cmgan_hip.h, "Scenes"), shared by
tests/test_scene_host.py and tests/test_gpu_scene.py.  Nothing here imports the library.

For one row - a float32 clip of L samples, the talker's response h (None: [1]), an optional dry noise segment and up to
four located sources, each a looping bank segment with a response and an SNR of its own:

    speech, target, d   as tests/mix_model.py (direct-path delay removed, `early` samples of reflections in the target)
    n0[i]  = bank[start0 + (off0 + i) mod len0]
    seg_j[m] = src_bank[start_j + ((off_j + m) mod len_j)]        every integer m
    c_j[i] = sum_{k < K_j} h_j[k] seg_j[i - k]                    no delay removal
    P_j = mean(c_j^2),  g_j = sqrt(Ps / (P_j 10^(snr_j / 10)))    0 when Ps == 0 or P_j == 0
    v = speech + g0 n0 + g_1 c_1 + ...;  m = max |v|, s = m > peak ? peak / m : 1;  noisy = v s, target = target s

direct      the definition in float64: np.convolve for the sums, np.mean for the powers - the expressions of mix_model.
direct_ld   the same in np.longdouble: the value w a device sample is judged against.
as_kernel   float64 in the kernel's order: taps accumulated in ascending k, the powers and the maximum through the
            per-thread sums of a tile (samples t, t + 256, t + 512, t + 768), the halving tree over the 256 threads, the
            partials of a row strided over the threads and the tree again.

All three return the values BEFORE the rounding to float32.  A segment that is empty or leaves its bank is silence; RIR
indices are clamped to [0, R) and lengths to [1, Kmax] (`row_of`).

Acceptance rule (the channel's and the warp's).  A device sample g is accepted against w = direct_ld when
|g - w| <= ulp32(w) / 2 + E, with E per row from the model alone: E = 8 x max_i max(|direct - w|, |as_kernel - w|).  The
factor 8 covers the fused multiply-adds of the device build and its own pow and sqrt.  CONDITION: a row may be used only if
E <= 2^-10 x ulp32(rms of w) / 2 (`condition`), so that the rule cannot hide a wrong sample.  Every judged row is one of
BATCHES (`build_batches`); tests/test_scene_host.py checks the condition on each."""
from typing import NamedTuple, Optional

import numpy as np

import mix_model

LD = np.longdouble
TPB, OPT = 256, 4            # threads per block and outputs per thread of the kernels
KC = 1024                    # taps per staged chunk


# ------------------------------------------------------------------ one row's inputs
class Source(NamedTuple):
    start: int
    length: int
    off: int
    snr_db: np.float32
    h: Optional[np.ndarray]          # float32 taps (None: [1])


class RowIn(NamedTuple):
    clean: np.ndarray                # float32 [L]
    h: Optional[np.ndarray]          # the talker's taps
    noise_bank: Optional[np.ndarray]
    noise: Optional[tuple]           # (start, length, off, snr_db), None: no dry noise
    src_bank: Optional[np.ndarray]
    sources: tuple                   # of Source
    peak: float
    early: int


def segment_ok(bank, start, length):
    n = 0 if bank is None else len(bank)
    return bool(bank is not None and start >= 0 and length >= 1 and start <= n and length <= n - start)


def looped(bank, start, length, off, m):
    """seg[m] for an int64 array m of any sign (numpy's % is the mathematical one for a positive modulus)."""
    idx = (int(off) % int(length) + np.asarray(m, dtype=np.int64)) % int(length)
    return np.asarray(bank)[int(start) + idx]


# ------------------------------------------------------------------ the kernel's reductions
def _tree(red, op):
    red = red.copy()
    s = TPB // 2
    while s > 0:
        red[:s] = op(red[:s], red[s:2 * s])
        s //= 2
    return red[0]


def _tiles(L):
    return (L + TPB * OPT - 1) // (TPB * OPT)


def _row_reduce(x, op, square):
    """mean-of-squares numerator (square) or maximum of x in the kernels' order: per tile a partial, then the partials."""
    L, T = len(x), TPB * OPT
    parts = np.zeros(_tiles(L))
    for k in range(_tiles(L)):
        pad = np.zeros(T)
        seg = x[k * T:(k + 1) * T]
        pad[:len(seg)] = seg
        per = pad.reshape(OPT, TPB)                              # per[r, t] = sample t + 256 r of the tile
        acc = np.zeros(TPB)
        for r in range(OPT):
            acc = acc + per[r] * per[r] if square else op(acc, np.abs(per[r]))
        parts[k] = _tree(acc, op)
    acc = np.zeros(TPB)
    for k0 in range(0, len(parts), TPB):
        chunk = parts[k0:k0 + TPB]
        acc[:len(chunk)] = op(acc[:len(chunk)], chunk)
    return _tree(acc, op)


def _power_kernel(x):
    return float(_row_reduce(x, np.add, True) / float(len(x)))


def _max_kernel(x):
    return float(_row_reduce(x, np.maximum, False))


def _taps_kernel(sig, h, first, L, last_tap=None):
    """out[i] = sum_k h[k] sig[first + i - k] with the taps accumulated in ascending k; sig is indexed from its own 0."""
    acc = np.zeros(L)
    K = len(h) if last_tap is None else last_tap + 1
    i = np.arange(L)
    for k in range(K):
        acc = acc + h[k] * sig[first + i - k]
    return acc


# ------------------------------------------------------------------ the three forms
def _row(r: RowIn, mode):
    F = LD if mode == "ld" else np.float64
    clean = np.asarray(r.clean, dtype=np.float32)
    L = clean.size
    h = np.ones(1, dtype=np.float32) if r.h is None else np.asarray(r.h, dtype=np.float32)
    d = mix_model.direct_path(h)
    power = _power_kernel if mode == "kernel" else (lambda x: F(np.mean(x * x)))
    peak_of = _max_kernel if mode == "kernel" else (lambda x: F(np.max(np.abs(x))))
    x, hh = clean.astype(F), h.astype(F)
    kt = None if r.early < 0 else min(d + int(r.early), h.size - 1)
    if mode == "kernel":
        K = h.size
        pad = np.concatenate([np.zeros(K), x, np.zeros(K)])      # pad[K + n] = clean[n]
        speech = _taps_kernel(pad, hh, K + d, L)
        target = x.copy() if kt is None else _taps_kernel(pad, hh, K + d, L, kt)
    else:
        def reverb(taps):
            full = np.convolve(x, taps)
            out = np.zeros(L, dtype=F)
            n = min(L, full.size - d)
            if n > 0:
                out[:n] = full[d:d + n]
            return out
        speech = reverb(hh)
        target = x.copy() if kt is None else reverb(hh[:kt + 1])
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
        n0 = looped(r.noise_bank, st, ln, off, np.arange(L)).astype(F) if segment_ok(r.noise_bank, st, ln) else np.zeros(L, dtype=F)
        P[0] = power(n0)
        g[0] = gain(P[0], snr)
        v = v + g[0] * n0
    for s in r.sources:
        hj = (np.ones(1, dtype=np.float32) if s.h is None else np.asarray(s.h, dtype=np.float32)).astype(F)
        K = hj.size
        if segment_ok(r.src_bank, s.start, s.length):
            sig = looped(r.src_bank, s.start, s.length, s.off, np.arange(-(K - 1), L)).astype(F)      # sig[K - 1 + m] = seg[m]
            c = _taps_kernel(sig, hj, K - 1, L) if mode == "kernel" else np.convolve(sig, hj)[K - 1:K - 1 + L]
        else:
            c = np.zeros(L, dtype=F)
        pj = power(c)
        gj = gain(pj, s.snr_db)
        v = v + gj * c
        g.append(gj)
        P.append(pj)
        cs.append(c)
    m = peak_of(v)
    pk = F(float(np.float32(r.peak)))
    scale = pk / m if m > pk else F(1)
    return {"noisy": v * scale, "target": target * scale, "g": g, "P": P, "Ps": ps, "scale": scale, "c": cs, "d": d,
            "speech": speech}


def direct(r):
    return _row(r, "direct")


def direct_ld(r):
    return _row(r, "ld")


def as_kernel(r):
    return _row(r, "kernel")


# ------------------------------------------------------------------ the acceptance rule
def ulp32(w):
    """The float32 spacing at |w| (w float64): 2^(e - 24) for |w| in [2^(e-1), 2^e), at least the denormal 2^-149."""
    w = np.abs(np.asarray(w, dtype=np.float64))
    _, e = np.frexp(w)
    return np.where(w == 0.0, 2.0 ** -149, np.ldexp(1.0, np.maximum(e - 24, -149)))


def condition(w):
    """The bound E must respect for the row to be used: 2^-10 x ulp32(rms of w) / 2."""
    rms = float(np.sqrt(np.mean(np.asarray(w, dtype=np.float64) ** 2)))
    return 2.0 ** -10 * float(ulp32(rms)) / 2.0


def excess(g, w, E):
    """The worst |g - w| - ulp32(w) / 2 - E over the samples (accepted when <= 0); g float32, w long double."""
    err = np.abs(np.asarray(g).astype(LD) - w).astype(np.float64)
    return float(np.max(err - 0.5 * ulp32(w.astype(np.float64)) - E))


def slack(r: RowIn):
    """{"noisy": (E, w), "target": (E, w)} and the long-double row: E = 8 x max(|direct - w|, |as_kernel - w|)."""
    ld, a, b = direct_ld(r), direct(r), as_kernel(r)
    out = {}
    for key in ("noisy", "target"):
        w = ld[key]
        e = max(np.max(np.abs(a[key].astype(LD) - w)), np.max(np.abs(b[key].astype(LD) - w)))
        out[key] = (8.0 * float(e), w)
    return out, ld


# ------------------------------------------------------------------ batches: the arguments of one Engine.scene call
class Batch(NamedTuple):
    clean: np.ndarray                        # float32 [B, L]
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
    rir: Optional[np.ndarray]                # float32 [R, Kmax]
    rir_index: Optional[np.ndarray]
    rir_len: Optional[np.ndarray]
    src_rir_index: Optional[np.ndarray]
    src_rir_len: Optional[np.ndarray]
    peak: float
    early: int


def _taps(rir, idx, length):
    if rir is None:
        return None
    R, Kmax = rir.shape
    return rir[min(max(int(idx), 0), R - 1), :min(max(int(length), 1), Kmax)]


def row_of(bt: Batch, b: int) -> RowIn:
    """Row b of a batch as the model takes it: the clamps of the untrusted tables applied, the sources beyond n_src dropped."""
    S = 0 if bt.n_src is None else bt.src_start.shape[1]
    sb = 0 if bt.n_src is None else min(max(int(bt.n_src[b]), 0), S)
    srcs = tuple(Source(int(bt.src_start[b, j]), int(bt.src_len[b, j]), int(bt.src_off[b, j]), bt.src_snr_db[b, j],
                        None if bt.rir is None else _taps(bt.rir, bt.src_rir_index[b, j], bt.src_rir_len[b, j]))
                 for j in range(sb))
    noise = None if bt.noise_bank is None else (int(bt.noise_start[b]), int(bt.noise_len[b]), int(bt.noise_off[b]), bt.snr_db[b])
    h = None if bt.rir is None else _taps(bt.rir, bt.rir_index[b], bt.rir_len[b])
    return RowIn(bt.clean[b], h, bt.noise_bank, noise, bt.src_bank, srcs, bt.peak, bt.early)


BATCHES = {}
_CASES = {}


def case(name, b):
    """(slack dict, long-double row) of row b of a registered batch, computed once."""
    if (name, b) not in _CASES:
        _CASES[(name, b)] = slack(row_of(BATCHES[name], b))
    return _CASES[(name, b)]


def rirs(R, K, rng):
    """R decaying-noise responses of K taps, the largest tap at the front, inside and at the end in turn."""
    h = rng.standard_normal((R, K)) * np.exp(-np.arange(K) / (0.15 * K + 1.0))
    for r in range(R):
        h[r, [0, K // 3, K - 1][r % 3]] = 1.5 * (-1) ** r
    return h.astype(np.float32)


def _freeze(bt: Batch) -> Batch:
    for a in bt:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return bt


def make_batch(seed, L, n_src, src_K, src_len, src_off, talker_K=40, dry=True, peak=0.99, early=20, src_snr=None, snr=None,
               bank_len=6000):
    """A batch of len(n_src) rows with S = 4 source columns.  src_K / src_len / src_off: [B][4] response lengths, segment
    lengths and offsets (a response length of 0 stands for the one-tap response [1]).  The RIR bank has one row per
    (row, source) and one per talker; segments start at arbitrary places of a bank of `bank_len` samples."""
    rng = np.random.default_rng(seed)
    B, S = len(n_src), 4
    src_K, src_len, src_off = (np.asarray(v, dtype=np.int64).reshape(B, S) for v in (src_K, src_len, src_off))
    Kmax = int(max(src_K.max(), talker_K, 1)) + 3                 # rows padded with zeros beyond their own length
    rir = np.zeros((B + B * S, Kmax), dtype=np.float32)
    rir[:B, :talker_K] = rirs(B, talker_K, rng)
    for b in range(B):
        for j in range(S):
            K = int(src_K[b, j])
            rir[B + b * S + j, :max(K, 1)] = rirs(1, K, rng)[0] if K > 0 else 1.0
    bank_len = max(bank_len, int(src_len.max()) + 50)
    bank = rng.standard_normal(bank_len).astype(np.float32)
    src_bank = (0.5 * rng.standard_normal(bank_len)).astype(np.float32)
    src_start = np.array([[int(rng.integers(0, bank_len - int(src_len[b, j]) + 1)) for j in range(S)] for b in range(B)],
                         dtype=np.int64)
    return _freeze(Batch(
        clean=(0.1 * rng.standard_normal((B, L))).astype(np.float32),
        noise_bank=bank if dry else None,
        noise_start=rng.integers(0, 100, B).astype(np.int64) if dry else None,
        noise_len=rng.integers(1, bank_len - 100, B).astype(np.int64) if dry else None,
        noise_off=rng.integers(-10 ** 6, 10 ** 6, B).astype(np.int64) if dry else None,
        snr_db=(rng.uniform(0.0, 20.0, B).astype(np.float32) if snr is None else np.asarray(snr, dtype=np.float32)) if dry else None,
        n_src=np.asarray(n_src, dtype=np.int32), src_bank=src_bank, src_start=src_start, src_len=src_len.copy(),
        src_off=src_off.copy(),
        src_snr_db=rng.uniform(-5.0, 15.0, (B, S)).astype(np.float32) if src_snr is None else np.asarray(src_snr, dtype=np.float32).reshape(B, S),
        rir=rir, rir_index=np.arange(B, dtype=np.int32), rir_len=np.full(B, talker_K, dtype=np.int32),
        src_rir_index=(B + np.arange(B * S, dtype=np.int32)).reshape(B, S),
        src_rir_len=np.maximum(src_K, 1).astype(np.int32), peak=peak, early=early))


def tile_lengths(T):
    return [1, T - 1, T, T + 1, 2 * T + T // 2 + 7]


def build_batches(T):
    """Every batch whose rows a GPU test accepts under the rule, registered once (read-only, shared).  T: cmgan_mix_tile()."""
    if BATCHES:
        return BATCHES
    assert T == TPB * OPT
    for n, L in enumerate(tile_lengths(T)):
        # 1. L around the output tile; rows of 0, 1 and 4 sources; K of 1 and 40; segments of 1 sample, of 7 under 40
        #    taps, of L and longer than L + K; offsets that are negative and far beyond the segment
        BATCHES[f"tile-{L}"] = make_batch(
            100 + n, L, n_src=[0, 1, 4, 4],
            src_K=[[40, 40, 40, 40], [40, 1, 1, 1], [0, 40, 40, 1], [40, 40, 0, 40]],
            src_len=[[9, 9, 9, 9], [7, 9, 9, 9], [1, 7, L, L + 40 + 13], [L + 57, 1, 7, L]],
            src_off=[[0, 0, 0, 0], [-3, 0, 0, 0], [5, -10 ** 9 - 7, 3 * L + 1, -1], [10 ** 12 + 5, -2, 6, L]])
    # 2. K around the staged chunk, in two tiles; a 7-sample segment under KC + 1 taps wraps ~150 times inside a chunk
    BATCHES["chunk"] = make_batch(
        200, T + 1, n_src=[4, 2], talker_K=KC + 1,
        src_K=[[KC - 1, KC, KC + 1, 2 * KC + 50], [KC + 1, 40, 40, 40]],
        src_len=[[300, T + 1, 3 * T + 2 * KC, 1000], [7, 1, 5, 5]],
        src_off=[[-1, 17, -(10 ** 7), 999], [10 ** 5, 0, 0, 0]])
    # 3. bad table entries: segments that are empty, start before the bank or leave it; RIR indices and lengths out of range
    bt = make_batch(300, 700, n_src=[4, 3, 9, -2], src_K=[[40] * 4] * 4, src_len=[[50, 60, 70, 80]] * 4, src_off=[[1, -2, 3, -4]] * 4)
    bad = {k: getattr(bt, k).copy() for k in ("noise_start", "noise_len", "src_start", "src_len", "rir_index", "rir_len",
                                              "src_rir_index", "src_rir_len")}
    bad["src_len"][0, 0] = 0
    bad["src_start"][0, 1] = -1
    bad["src_start"][0, 2] = len(bt.src_bank) - 10
    bad["src_len"][1, 0] = -5
    bad["src_start"][1, 1] = len(bt.src_bank)
    bad["src_len"][2, 3] = 2 ** 62
    bad["noise_len"][1] = 0
    bad["noise_start"][2] = 2 ** 40
    bad["rir_index"][0], bad["rir_len"][0] = -3, 0
    bad["rir_index"][1], bad["rir_len"][1] = 10 ** 6, 10 ** 6
    bad["src_rir_index"][2] = [-1, 10 ** 5, 3, 4]
    bad["src_rir_len"][2] = [-7, 10 ** 5, 0, 41]
    BATCHES["bad"] = _freeze(bt._replace(**bad))
    # 4. the peak guard: sources 25 dB above the speech under a peak that speech and dry noise alone stay below
    BATCHES["peak"] = make_batch(400, 1500, n_src=[2, 4], src_K=[[40] * 4] * 2, src_len=[[900, 2000, 30, 40]] * 2,
                                 src_off=[[0, 5, -6, 7]] * 2, src_snr=[[-25.0] * 4] * 2, snr=[20.0, 20.0], peak=2.5)
    # 5. no dry noise: every noise is located
    BATCHES["located"] = make_batch(500, 1300, n_src=[1, 3, 0], src_K=[[40, 0, 40, 40]] * 3, src_len=[[500, 1300, 7, 1]] * 3,
                                    src_off=[[-9, 8, 7, 6]] * 3, dry=False, early=-1)
    # 6. determinism and graph replay: the rows before and after the tables are rewritten
    BATCHES["bits"] = make_batch(600, T + 77, n_src=[4, 0, 2, 1, 3], src_K=[[200, 40, 1100, 1]] * 5,
                                 src_len=[[333, 7, 4000, 1]] * 5, src_off=[[-1, 2, -3, 4]] * 5)
    BATCHES["graph-0"] = make_batch(700, 900, n_src=[1, 4, 2], src_K=[[40, 30, 20, 10]] * 3, src_len=[[100, 200, 7, 1000]] * 3,
                                    src_off=[[1, -2, 3, -4]] * 3)
    g0 = BATCHES["graph-0"]
    BATCHES["graph-1"] = _freeze(g0._replace(
        n_src=np.array([3, 0, 4], dtype=np.int32), src_off=g0.src_off + 12345, src_len=np.maximum(g0.src_len // 2, 1),
        src_snr_db=(g0.src_snr_db - 3.0).astype(np.float32), src_rir_len=np.maximum(g0.src_rir_len - 5, 1).astype(np.int32),
        src_rir_index=g0.src_rir_index[::-1].copy(), noise_off=g0.noise_off - 77))
    return BATCHES
