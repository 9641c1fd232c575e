"""The float64 statement of cmgan_mix (include/cmgan_hip.h, "Dynamic mixing"): plain numpy, one row at a time,
np.convolve for the sums.  Nothing here is shared with the kernels; the tests compare them against this."""
import numpy as np


def direct_path(h):
    """First index at which |h| is largest."""
    return int(np.argmax(np.abs(np.asarray(h, dtype=np.float64))))


def reverb(clean, h, d, last_tap=None):
    """out[i] = sum_{k <= last_tap} h[k] clean[i + d - k], 0 <= i < L, clean zero outside [0, L): float64."""
    x = np.asarray(clean, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    if last_tap is not None:
        h = h[:last_tap + 1]
    full = np.convolve(x, h)                                   # full[j] = sum_k h[k] x[j - k], j < L + K - 1
    out = np.zeros(x.size, dtype=np.float64)
    n = min(x.size, full.size - d)
    if n > 0:
        out[:n] = full[d:d + n]
    return out


def wrap_noise(bank, start, length, off, L):
    """n[i] = bank[start + (off + i) mod length]"""
    idx = (int(off) + np.arange(L, dtype=np.int64)) % int(length)
    return np.asarray(bank, dtype=np.float64)[int(start) + idx]


def gain(ps, pn, snr_db):
    if ps == 0.0 or pn == 0.0:
        return 0.0
    return float(np.sqrt(ps / (pn * 10.0 ** (float(snr_db) / 10.0))))


def mix_row(clean, bank, start, length, off, snr_db, h=None, peak=0.99, early=-1):
    """One row -> dict(noisy, target float64 BEFORE the float32 rounding; g, scale, Ps, Pn; speech, d)."""
    clean = np.asarray(clean, dtype=np.float32)
    L = clean.size
    h = np.ones(1) if h is None else np.asarray(h, dtype=np.float64)
    d = direct_path(h)
    speech = reverb(clean, h, d)
    if early < 0:
        target = clean.astype(np.float64)
    else:
        target = reverb(clean, h, d, last_tap=min(d + int(early), h.size - 1))
    n = wrap_noise(bank, start, length, off, L)
    ps, pn = float(np.mean(speech * speech)), float(np.mean(n * n))
    g = gain(ps, pn, np.float32(snr_db))
    v = speech + g * n
    m = float(np.max(np.abs(v)))
    pk = float(np.float32(peak))
    s = pk / m if m > pk else 1.0
    return {"noisy": v * s, "target": target * s, "g": g, "scale": s, "Ps": ps, "Pn": pn, "speech": speech, "d": d,
            "noise": n}


def mix_batch(clean, bank, start, length, off, snr_db, rir=None, rir_index=None, rir_len=None, peak=0.99, early=-1):
    """Rows of mix_row for a [B, L] batch; rir [R, Kmax] with per-row index / length, or None."""
    rows = []
    for b in range(len(clean)):
        h = None if rir is None else np.asarray(rir)[int(rir_index[b]), :int(rir_len[b])]
        rows.append(mix_row(clean[b], bank, start[b], length[b], off[b], snr_db[b], h, peak, early))
    return rows
