"""The float64 statement of cmgan_rir_bands (include/cmgan_hip.h, "Room impulse responses in frequency bands"): the
image-source method in NB frequency bands joined by a filterbank, in plain numpy.  It shares no code with the kernels
(the image enumeration is rir_model.images, once per band): the GPU tests compare Engine.rir_bands with it, the host
tests compare it with a naive loop and with known answers."""
import numpy as np

import rir_model as M


def row_is_valid(room, bands) -> bool:
    room, bands = np.asarray(room, dtype=np.float64), np.asarray(bands, dtype=np.float64).reshape(-1, 7)
    return bool(np.all(np.isfinite(room[0:9])) and np.all(room[0:3] > 0) and np.all(np.isfinite(bands)) and np.all(bands >= 0)
                and np.all(bands[:, 0:6] <= 1))


def band_taps(room, band, kq, n, N, fs, c, tw, chunk=40000):
    """One band: (h_b, A_b) float64 [n], the taps 0 <= q < kq (0 from kq on) and A_b[q] = sum |a_b| over the images whose
    window reaches q."""
    table = np.array(room, dtype=np.float64)
    table[9:15] = band[0:6]
    d, num = M.images(table, N)
    tau = d * fs / c
    keep = tau - tw < kq
    d, num, tau = d[keep], num[keep], tau[keep]
    a = num * np.exp(-band[6] * d) / (4 * np.pi * np.maximum(d, M.DMIN))
    h, A = np.zeros(n), np.zeros(n)
    span = np.arange(0, 2 * tw + 2)[None, :]
    for i in range(0, tau.size, chunk):
        ta, aa = tau[i:i + chunk, None], a[i:i + chunk, None]
        q = np.floor(ta).astype(np.int64) - tw + span
        t = q - ta
        inside = (np.abs(t) < tw) & (q >= 0) & (q < kq)
        with np.errstate(invalid="ignore", divide="ignore"):
            sinc = np.where(t == 0, 1.0, np.sin(np.pi * t) / (np.pi * t))
        w = 0.5 * (1 + np.cos(np.pi * t / tw))
        h += np.bincount(q[inside], weights=(aa * w * sinc)[inside], minlength=n)
        A += np.bincount(q[inside], weights=np.broadcast_to(np.abs(aa), q.shape)[inside], minlength=n)
    return h, A


def rir_bands_row(room, bands, n_taps, K, N, filt, fs=16000, c=343.0, tw=40):
    """(h [K], bound [K], h_b [NB, K + D], A_b [NB, K + D], k_r) of one row, float64.  Taps k >= k_r are 0 in h and bound;
    an invalid row gives zeros and k_r = 1.  bound is the per-tap bound of the GPU tests:
        2^-24 |h[k]| + sum_b sum_j |g_b[j]| 64 2^-53 (K + D + tw) A_b[k + D - j] + (NB NF + 1) 2^-53 sum_b sum_j |g_b[j] h_b[k + D - j]|
    the float32 rounding, rir_model.bound's delay term carried through the filters, and the join's float64 sum."""
    bands, filt = np.asarray(bands, dtype=np.float64).reshape(-1, 7), np.asarray(filt, dtype=np.float64)
    NB, NF = filt.shape
    assert bands.shape[0] == NB and NF % 2 == 1
    D = (NF - 1) // 2
    h, bound, hb, Ab = np.zeros(K), np.zeros(K), np.zeros((NB, K + D)), np.zeros((NB, K + D))
    if not row_is_valid(room, bands):
        return h, bound, hb, Ab, 1
    kr = int(min(max(int(n_taps), 1), K))
    for b in range(NB):
        hb[b], Ab[b] = band_taps(room, bands[b], kr + D, K + D, N, fs, c, tw)
    delay = mag = 0.0
    for b in range(NB):                                          # h[k] = sum_j g[j] h_b[k + D - j] = (g * h_b)[k + D]
        h[:kr] += np.convolve(hb[b], filt[b])[D:D + kr]
        delay = delay + np.convolve(Ab[b], np.abs(filt[b]))[D:D + kr]
        mag = mag + np.convolve(np.abs(hb[b]), np.abs(filt[b]))[D:D + kr]
    bound[:kr] = 2.0 ** -24 * np.abs(h[:kr]) + 64 * 2.0 ** -53 * (K + D + tw) * delay + (NB * NF + 1) * 2.0 ** -53 * mag
    return h, bound, hb, Ab, kr


def rir_bands(rooms, bands, n_taps, K, N, filt, fs=16000, c=343.0, tw=40):
    """Rows of rir_bands_row: (h [R, K], bound [R, K], len int32 [R])."""
    rooms = np.asarray(rooms, dtype=np.float64).reshape(-1, 15)
    bands = np.asarray(bands, dtype=np.float64).reshape(rooms.shape[0], -1, 7)
    out = [rir_bands_row(rooms[r], bands[r], n_taps[r], K, N, filt, fs, c, tw) for r in range(rooms.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[4] for o in out], dtype=np.int32)
