"""The float64 statement of cmgan_rir_dir and cmgan_rir_bands_dir (include/cmgan_hip.h, "Room impulse responses of
directional sources and receivers") in plain numpy: rir_model's image grid extended by the offsets' components and the
mirror signs, so that every image gets its gain g = (alpha_s + (1 - alpha_s) cos_s) (alpha_m + (1 - alpha_m) cos_m).  It
shares no code with the kernels: the GPU tests compare Engine.rir(orient=, pattern=) and Engine.rir_bands with it, the
host tests compare it with a naive triple loop, with rir_model (all alpha = 1: bit for bit) and with known answers."""
import numpy as np

import rir_bands_model as BM
import rir_model as M

MAX_COMPONENT = 1e100

# What the gain's own rounding adds to rir_model.bound, in units of 2^-53 A (A = sum |a| BEFORE the gains, |g| <= 1),
# from the arithmetic and not from any output.  With u = 2^-53: a unit vector costs a three-term sum, a square root and
# a division (<= 3 u per component); o . w is three products and two sums on terms whose magnitudes add up to at most
# d (1 + 3 u) (<= 3 u d, fused or not); d itself is within 2 u, so the kernel's reciprocal 1 / d is within 3 u and the
# product with it adds u (the division here: 2 u + u): |delta cos| <= 10 u.  A factor alpha + (1 - alpha) cos adds the
# rounding of 1 - alpha and its own (<= 2 u): <= 12 u, and it is at most 1 in magnitude, so g = f_s f_m is within
# 12 u + 12 u + u = 25 u, and a g within 26 u |a|.  Kernel and model both err at most that much: 52 u.
GAIN_ULPS = 52


def unit(v):
    """v / |v| with |v| = sqrt(x x + y y + z z); the zero vector stays zero."""
    v = np.asarray(v, dtype=np.float64)
    n = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return v / n if n > 0 else np.zeros(3)


def dirs_are_valid(orient, pattern) -> bool:
    """orient [6], pattern [NB, 2]: finite, alphas in [0, 1], components within 1e100, and a vector that is not zero at
    an end that has some alpha < 1."""
    orient, pattern = np.asarray(orient, dtype=np.float64), np.asarray(pattern, dtype=np.float64).reshape(-1, 2)
    if not (np.all(np.isfinite(orient)) and np.all(np.isfinite(pattern))):
        return False
    if not (np.all(pattern >= 0) and np.all(pattern <= 1) and np.all(np.abs(orient) <= MAX_COMPONENT)):
        return False
    for end in (0, 1):
        v = orient[3 * end:3 * end + 3]
        if np.any(pattern[:, end] < 1) and not np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) > 0:
            return False
    return True


def cosines(room, N, orient):
    """(cos_s, cos_m) of every image, flat float64 arrays in the order of rir_model.images (nx, ny, px, py, pz, nz):
    cos_m = (o . v^) / d and cos_s = -(o . u^_p) / d with u^_p = (1 - 2 p) u^ per axis; both 0 where d == 0."""
    room = np.asarray(room, dtype=np.float64)
    L, s, m = room[0:3], room[3:6], room[6:9]
    u, v = unit(orient[0:3]), unit(orient[3:6])
    off, up = [], []
    for ax in range(3):
        n = np.arange(-N[ax], N[ax] + 1, dtype=np.float64)[:, None]
        p = np.array([0.0, 1.0])[None, :]
        off.append((1 - 2 * p) * s[ax] + 2 * n * L[ax] - m[ax])                       # [2N+1, 2], rir_model.images' offsets
        up.append(np.broadcast_to((1 - 2 * p) * u[ax], off[-1].shape))
    # axes of the grid: nx, ny, px, py, pz, nz
    ox, ux = off[0][:, None, :, None, None, None], up[0][:, None, :, None, None, None]
    oy, uy = off[1][None, :, None, :, None, None], up[1][None, :, None, :, None, None]
    oz, uz = off[2].T[None, None, None, None, :, :], up[2].T[None, None, None, None, :, :]
    d = np.sqrt(ox * ox + oy * oy + oz * oz)
    with np.errstate(invalid="ignore", divide="ignore"):
        cos_m = np.where(d > 0, (ox * v[0] + oy * v[1] + oz * v[2]) / d, 0.0)
        cos_s = np.where(d > 0, -(ox * ux + oy * uy + oz * uz) / d, 0.0)
    return cos_s.ravel(), cos_m.ravel()


def gain(cos_s, cos_m, alpha_s, alpha_m):
    return (alpha_s + (1 - alpha_s) * cos_s) * (alpha_m + (1 - alpha_m) * cos_m)


def _taps(d, a, g, k_end, n, fs, c, tw, chunk=40000):
    """The sum of rir_model.rir_row / rir_bands_model.band_taps with a gain per image: (h, A) float64 [n] over taps
    0 <= k < k_end, A from |a| before the gains."""
    tau = d * fs / c
    keep = tau - tw < k_end
    a, g, tau = a[keep], g[keep], tau[keep]
    ag = a * g
    h, A = np.zeros(n), np.zeros(n)
    span = np.arange(0, 2 * tw + 2)[None, :]
    for i in range(0, tau.size, chunk):
        ta, aa, gg = tau[i:i + chunk, None], a[i:i + chunk, None], ag[i:i + chunk, None]
        k = np.floor(ta).astype(np.int64) - tw + span
        t = k - ta
        inside = (np.abs(t) < tw) & (k >= 0) & (k < k_end)
        with np.errstate(invalid="ignore", divide="ignore"):
            sinc = np.where(t == 0, 1.0, np.sin(np.pi * t) / (np.pi * t))
        w = 0.5 * (1 + np.cos(np.pi * t / tw))
        kk = k[inside]
        h += np.bincount(kk, weights=(gg * w * sinc)[inside], minlength=n)
        A += np.bincount(kk, weights=np.broadcast_to(np.abs(aa), k.shape)[inside], minlength=n)
    return h, A


def rir_dir_row(room, orient, pattern, n_taps, K, N, fs=16000, c=343.0, tw=40):
    """(h float64 [K], A float64 [K], k_r) of one row of cmgan_rir_dir; pattern = (alpha_s, alpha_m).  A[k] = sum |a| over
    the images whose window reaches tap k, BEFORE the gains.  An invalid row gives zeros and k_r = 1."""
    pattern = np.asarray(pattern, dtype=np.float64).reshape(-1)
    if not (M.row_is_valid(room) and dirs_are_valid(orient, pattern)):
        return np.zeros(K), np.zeros(K), 1
    kr = int(min(max(int(n_taps), 1), K))
    d, num = M.images(room, N)
    a = num / (4 * np.pi * np.maximum(d, M.DMIN))
    g = gain(*cosines(room, N, np.asarray(orient, dtype=np.float64)), pattern[0], pattern[1])
    h, A = _taps(d, a, g, kr, K, fs, c, tw)
    return h, A, kr


def rir_dir(rooms, orient, pattern, n_taps, K, N, fs=16000, c=343.0, tw=40):
    """Rows of rir_dir_row: (h [R, K], A [R, K], len int32 [R])."""
    rooms = np.asarray(rooms, dtype=np.float64).reshape(-1, 15)
    orient = np.asarray(orient, dtype=np.float64).reshape(-1, 6)
    pattern = np.asarray(pattern, dtype=np.float64).reshape(-1, 2)
    out = [rir_dir_row(rooms[r], orient[r], pattern[r], n_taps[r], K, N, fs, c, tw) for r in range(rooms.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32)


def bound(h, A, K, tw):
    """rir_model.bound on the A before the gains, plus the gains' own rounding (GAIN_ULPS)."""
    return M.bound(h, A, K, tw) + GAIN_ULPS * 2.0 ** -53 * A


def rir_bands_dir_row(room, bands, orient, pattern, n_taps, K, N, filt, fs=16000, c=343.0, tw=40):
    """(h [K], bound [K], k_r) of one row of cmgan_rir_bands_dir, float64; pattern [NB, 2].  The bound is
    rir_bands_model.rir_bands_row's on the A_b before the gains, plus GAIN_ULPS 2^-53 A_b carried through the filters."""
    bands, filt = np.asarray(bands, dtype=np.float64).reshape(-1, 7), np.asarray(filt, dtype=np.float64)
    pattern = np.asarray(pattern, dtype=np.float64).reshape(-1, 2)
    NB, NF = filt.shape
    assert bands.shape[0] == NB and pattern.shape[0] == NB and NF % 2 == 1
    D = (NF - 1) // 2
    h, bnd = np.zeros(K), np.zeros(K)
    if not (BM.row_is_valid(room, bands) and dirs_are_valid(orient, pattern)):
        return h, bnd, 1
    kr = int(min(max(int(n_taps), 1), K))
    cos_s, cos_m = cosines(room, N, np.asarray(orient, dtype=np.float64))
    delay = mag = 0.0
    for b in range(NB):
        table = np.array(room, dtype=np.float64)
        table[9:15] = bands[b, 0:6]
        d, num = M.images(table, N)
        a = num * np.exp(-bands[b, 6] * d) / (4 * np.pi * np.maximum(d, M.DMIN))
        hb, Ab = _taps(d, a, gain(cos_s, cos_m, pattern[b, 0], pattern[b, 1]), kr + D, K + D, fs, c, tw)
        h[:kr] += np.convolve(hb, filt[b])[D:D + kr]
        delay = delay + np.convolve(Ab, np.abs(filt[b]))[D:D + kr]
        mag = mag + np.convolve(np.abs(hb), np.abs(filt[b]))[D:D + kr]
    bnd[:kr] = (2.0 ** -24 * np.abs(h[:kr]) + (64 * (K + D + tw) + GAIN_ULPS) * 2.0 ** -53 * delay
                + (NB * NF + 1) * 2.0 ** -53 * mag)
    return h, bnd, kr


def rir_bands_dir(rooms, bands, orient, pattern, n_taps, K, N, filt, fs=16000, c=343.0, tw=40):
    """Rows of rir_bands_dir_row: (h [R, K], bound [R, K], len int32 [R])."""
    rooms = np.asarray(rooms, dtype=np.float64).reshape(-1, 15)
    R = rooms.shape[0]
    bands = np.asarray(bands, dtype=np.float64).reshape(R, -1, 7)
    orient = np.asarray(orient, dtype=np.float64).reshape(R, 6)
    pattern = np.asarray(pattern, dtype=np.float64).reshape(R, -1, 2)
    out = [rir_bands_dir_row(rooms[r], bands[r], orient[r], pattern[r], n_taps[r], K, N, filt, fs, c, tw) for r in range(R)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32)
