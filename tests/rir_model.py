"""The float64 statement of cmgan_rir (include/cmgan_hip.h, "Room impulse responses"): the image-source method for a
shoe-box room in plain numpy, vectorised over images.  It shares no code with the kernels: the GPU tests compare
Engine.rir with it, the host tests compare it with a naive triple loop and with known answers."""
import numpy as np

DMIN = 0.01            # CMGAN_RIR_DMIN


def row_is_valid(room) -> bool:
    room = np.asarray(room, dtype=np.float64)
    return bool(np.all(np.isfinite(room)) and np.all(room[0:3] > 0) and np.all(room[9:15] >= 0) and np.all(room[9:15] <= 1))


def images(room, N):
    """Every image (n, p), |n_axis| <= N_axis, p in {0,1}^3, in the order (nx, ny, px, py, pz, nz) ascending:
    (distance d, numerator of the amplitude prod b0^|n-p| b1^|n|), flat float64 arrays."""
    room = np.asarray(room, dtype=np.float64)
    L, s, m, b = room[0:3], room[3:6], room[6:9], room[9:15].reshape(3, 2)
    off, coef = [], []
    for ax in range(3):
        n = np.arange(-N[ax], N[ax] + 1, dtype=np.float64)[:, None]
        p = np.array([0.0, 1.0])[None, :]
        off.append((1 - 2 * p) * s[ax] + 2 * n * L[ax] - m[ax])                       # [2N+1, 2]
        coef.append(b[ax, 0] ** np.abs(n - p) * b[ax, 1] ** np.abs(n))
    # axes of the grid: nx, ny, px, py, pz, nz
    ox, cx = off[0][:, None, :, None, None, None], coef[0][:, None, :, None, None, None]
    oy, cy = off[1][None, :, None, :, None, None], coef[1][None, :, None, :, None, None]
    oz, cz = off[2].T[None, None, None, None, :, :], coef[2].T[None, None, None, None, :, :]
    d = np.sqrt(ox * ox + oy * oy + oz * oz)
    num = cx * cy * cz
    return d.ravel(), np.broadcast_to(num, d.shape).ravel()


def rir_row(room, n_taps, K, N, fs=16000, c=343.0, tw=40, chunk=40000):
    """(h float64 [K], A float64 [K], k_r): the taps, A[k] = sum |a| over the images whose window reaches tap k, and the
    length.  Taps k >= k_r are 0 in both.  An invalid row gives zeros and k_r = 1."""
    h, A = np.zeros(K), np.zeros(K)
    if not row_is_valid(room):
        return h, A, 1
    kr = int(min(max(int(n_taps), 1), K))
    d, num = images(room, N)
    tau = d * fs / c
    keep = tau - tw < K
    d, num, tau = d[keep], num[keep], tau[keep]
    a = num / (4 * np.pi * np.maximum(d, DMIN))
    span = np.arange(0, 2 * tw + 2)[None, :]
    for i in range(0, tau.size, chunk):
        ta, aa = tau[i:i + chunk, None], a[i:i + chunk, None]
        k = np.floor(ta).astype(np.int64) - tw + span                                  # covers every k with |k - tau| < tw
        t = k - ta
        inside = (np.abs(t) < tw) & (k >= 0) & (k < kr)
        with np.errstate(invalid="ignore", divide="ignore"):
            sinc = np.where(t == 0, 1.0, np.sin(np.pi * t) / (np.pi * t))
        w = 0.5 * (1 + np.cos(np.pi * t / tw))
        kk = k[inside]
        h += np.bincount(kk, weights=(aa * w * sinc)[inside], minlength=K)
        A += np.bincount(kk, weights=np.broadcast_to(np.abs(aa), k.shape)[inside], minlength=K)
    return h, A, kr


def rir(rooms, n_taps, K, N, fs=16000, c=343.0, tw=40):
    """Rows of rir_row: (h [R, K], A [R, K], len int32 [R])."""
    rooms = np.asarray(rooms, dtype=np.float64).reshape(-1, 15)
    out = [rir_row(rooms[r], n_taps[r], K, N, fs, c, tw) for r in range(rooms.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32)


def bound(h, A, K, tw):
    """The per-tap bound of the GPU tests: one float32 rounding plus 64 ulps of a delay of up to K + tw samples on A."""
    return 2.0 ** -24 * np.abs(h) + 64 * 2.0 ** -53 * (K + tw) * A
