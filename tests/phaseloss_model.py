"""The numpy model of the phase loss (cmgan_amd/csrc/phaseloss.hip; include/cmgan_hip.h, "Phase loss"), shared by
tests/test_phaseloss_host.py and tests/test_gpu_phaseloss.py.  Written from the formulas of the header and from nothing else.

For one row - est_real, est_imag, clean_re, clean_im float32 [T, F] - in the header's notation: p = atan2(est_imag, est_real),
q = atan2(clean_im, clean_re); r(x) = the IEEE remainder of x by TWO_PI, the double nearest 2 pi; AW = |r|; a cell is void
when re^2 + im^2 of either spectrum (float64: exact squares, one rounding) is 0 or below floor * floor or an input is not
finite; ip / gd / iaf are the means of AW over the non-void cells / frequency pairs / time pairs; a_row = sum_i k_i value_i
(k_i == 0 left out); D = c_ip s_ip + c_gd (s_gd[t,f] - s_gd[t,f+1]) + c_iaf (s_iaf[t,f] - s_iaf[t+1,f]), c_i = k_i / N_i;
g_real = D (-im / |z|^2), g_imag = D (re / |z|^2).  The void map is decided in float64 in every evaluation (it is defined
there); everything else is generic in the number type and is run two ways: w in np.longdouble, the value a device output is
judged against, and d in float64.

Acceptance rule.  Exact zeros, counts and status words are compared for EQUALITY.  A device gradient sample g is accepted
against w when |g - w| <= ulp32(w) / 2 + E.  E comes from the float64 roundings of the formula alone: c_i = k_i / N_i is
rounded once, c_i s is exact (s is 0, +-1, +-2), the two additions of D round twice, the sum of the exact squares once, the
quotient once and the last product once - at most six relative roundings of u = 2^-53 on quantities no larger than
S |x| / |z|^2 with S = |c_ip| + 2 |c_gd| + 2 |c_iaf| and x the other component - so E = 8 u S |x| / |z|^2 per sample (8 for
6 and the second-order terms).  The host tests check that the float64 evaluation itself lies inside E of the long-double one.

Values.  A row value is a mean of n terms of at most pi.  The kernel adds them in a fixed tree (header): a thread's chain of
TILE_FRAMES x ceil(F / BLOCK) terms, 8 halvings, the row's tiles ascending, one division - `depth` roundings in all, each
at most u x the partial sum, so the summation costs at most depth x u x pi.  The one unknown is the device's float64 atan2:
four of them and three subtractions make a term, and its error is allowed ATAN2_ALLOWANCE x u x pi per term (so as much in
the mean).  bound = (depth + ATAN2_ALLOWANCE) u pi.  ATAN2_ALLOWANCE is four times the worst row-value error seen against
the long-double model on the first MI355X run, in units of u pi (DESIGN.md 9v has both figures).  Whatever it is, no value
may differ by more than VALUE_CAP = 1e-12: more is a wrong term, not rounding.

MARGINS of a row, under which a long-double model and a float64 kernel take the same branch everywhere: `branch_margin` =
min over the non-void terms of min(|r|, pi - |r|) (the sign of r and the wrap), inf for a row whose every r is exactly 0
(est == clean, est = 2 clean: both evaluate to exact zeros); `floor_margin` = min over the cells and both spectra of
|m2 - floor^2| / floor^2 (inf at floor = 0, where the test is m2 == 0 and exact)."""
from functools import lru_cache
from typing import NamedTuple

import numpy as np

from warp_model import LD, PI_LD, ulp32

U = 2.0 ** -53
TWO_PI = 2.0 * np.pi                 # the double nearest 2 pi (np.pi is the double nearest pi)
TILE_FRAMES, BLOCK = 8, 256          # cmgan_phase_loss_tile_frames() and the threads of a tile
#: worst |device row value - w| over every judged row of tests/test_gpu_phaseloss.py on the first MI355X run, in units of
#: u pi (1.144: the row with the NaN at T = 17, F = 201; 4.0e-16 absolute), and four times it
ATAN2_WORST_SEEN = 1.15
ATAN2_ALLOWANCE = 4 * ATAN2_WORST_SEEN
VALUE_CAP = 1e-12
BRANCH_MARGIN, FLOOR_MARGIN = 1e-9, 1e-6


def remainder(x, T):
    """The IEEE remainder of x by TWO_PI for |x| < 2 TWO_PI, exact in T: fmod is exact, and so is the one subtraction."""
    y = T(TWO_PI)
    r = np.fmod(x, y)
    half = y / T(2)
    return np.where(r > half, r - y, np.where(r < -half, r + y, r))


class Eval(NamedTuple):
    values: np.ndarray      # [3] in the evaluation's precision
    counts: np.ndarray      # [3] int64
    status: int
    a: object               # the row's share of the total
    parts: np.ndarray       # [3]: k_i value_i
    g_real: np.ndarray      # [T, F]
    g_imag: np.ndarray
    E_real: np.ndarray      # [T, F] float64: the slack of a gradient sample
    E_imag: np.ndarray
    void: np.ndarray        # [T, F] bool
    branch_margin: float
    floor_margin: float


def void_map(er, ei, cr, ci, floor):
    """(void [T, F], floor_margin) in float64, as the header defines them."""
    a, b, c, d = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (er, ei, cr, ci))
    with np.errstate(invalid="ignore", over="ignore"):
        me, mc = a * a + b * b, c * c + d * d
        fl2 = float(floor) * float(floor)
        finite = np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & np.isfinite(d)
        void = ~finite | ~(me > 0) | ~(mc > 0) | (me < fl2) | (mc < fl2)
        margin = np.inf
        if fl2 > 0:
            m = np.concatenate([me[finite], mc[finite]])
            margin = float(np.min(np.abs(m - fl2) / fl2, initial=np.inf))
    return void, margin


def evaluate(er, ei, cr, ci, k3, floor=0.0, T=np.float64, shift=None) -> Eval:
    """One row.  `shift` = (d_real, d_imag) in T is added to the estimate after it has been widened (central differences);
    the void map stays that of the float32 inputs."""
    void, floor_margin = void_map(er, ei, cr, ci, floor)
    ok = ~void
    a, b, c, d = (np.where(ok, np.asarray(x, dtype=np.float32).astype(np.float64), 1.0).astype(T) for x in (er, ei, cr, ci))
    if shift is not None:
        a, b = a + np.where(ok, shift[0], T(0)), b + np.where(ok, shift[1], T(0))
    nT, nF = a.shape
    p, q = np.arctan2(b, a), np.arctan2(d, c)
    r_ip, v_ip = remainder(p - q, T), ok
    r_gd, v_gd = remainder((p[:, 1:] - p[:, :-1]) - (q[:, 1:] - q[:, :-1]), T), ok[:, 1:] & ok[:, :-1]
    r_iaf, v_iaf = remainder((p[1:] - p[:-1]) - (q[1:] - q[:-1]), T), ok[1:] & ok[:-1]
    values, counts, status, margin, signs, coef = [], [], 0, np.inf, [], []
    for i, (r, v) in enumerate(((r_ip, v_ip), (r_gd, v_gd), (r_iaf, v_iaf))):
        n = int(np.count_nonzero(v))
        aw = np.abs(r[v])
        values.append(np.sum(aw) / T(n) if n else T(0))
        counts.append(n)
        status |= 0 if n else 1 << i
        if n and np.any(aw != 0):
            margin = min(margin, float(np.min(np.minimum(aw, T(PI_LD) - aw))))
        signs.append(np.where(v, np.sign(r), T(0)))
        coef.append(T(k3[i]) / T(n) if (k3[i] != 0 and n) else T(0))
    values = np.array(values, dtype=T)
    parts = np.array([T(k3[i]) * values[i] if k3[i] != 0 else T(0) for i in range(3)], dtype=T)
    s_gd, s_iaf = np.zeros((nT, nF), dtype=T), np.zeros((nT, nF), dtype=T)
    s_gd[:, 1:] += signs[1]
    s_gd[:, :-1] -= signs[1]
    s_iaf[1:] += signs[2]
    s_iaf[:-1] -= signs[2]
    D = coef[0] * signs[0]
    D = D + coef[1] * s_gd
    D = D + coef[2] * s_iaf
    m2 = a * a + b * b
    g_real, g_imag = np.where(ok, D * (-b / m2), T(0)), np.where(ok, D * (a / m2), T(0))
    S = float(abs(coef[0]) + 2 * abs(coef[1]) + 2 * abs(coef[2]))
    m64 = m2.astype(np.float64)
    E_real = np.where(ok, 8 * U * S * np.abs(b.astype(np.float64)) / m64, 0.0)
    E_imag = np.where(ok, 8 * U * S * np.abs(a.astype(np.float64)) / m64, 0.0)
    return Eval(values, np.array(counts), status, (parts[0] + parts[1]) + parts[2], parts, g_real, g_imag, E_real, E_imag, void,
                margin, floor_margin)


def value_bound(nT, nF):
    """What a device row value may be off by (module docstring)."""
    depth = TILE_FRAMES * -(-nF // BLOCK) + 8 + -(-nT // TILE_FRAMES) + 1
    return (depth + ATAN2_ALLOWANCE) * U * np.pi


def accept(got_real, got_imag, m: Eval):
    """(ok, worst excess over half an ulp as a fraction of the sample's E) of a device gradient row against its model."""
    worst, ok = 0.0, True
    for got, w, E in ((got_real, m.g_real, m.E_real), (got_imag, m.g_imag, m.E_imag)):
        got = np.asarray(got, dtype=np.float64)
        err = np.abs(got.astype(LD) - w).astype(np.float64)
        over = err - ulp32(w.astype(np.float64)) / 2
        ok = ok and bool(np.all(np.isfinite(got))) and bool(np.all(over <= E)) and not got[m.void].any()
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = np.where(over > 0, over / E, 0.0)
        worst = max(worst, float(np.max(frac, initial=0.0)))
    return ok, worst


# ------------------------------------------------------------------ the rows of the GPU cases
#: (T, F): T = 1, 2, 3; T = 17 = two whole tiles of TILE_FRAMES = 8 frames and one of a single frame, so that pairs cross a tile
#: edge twice and the last tile is all halo but one frame; F = 601 = two whole passes of the 256 threads along f and a part
#: of a third (201 bins are less than one pass), at T = 2
SHAPES = ((1, 201), (2, 201), (3, 201), (17, 201), (2, 601))
FLOOR = 1e-2
K_WEIGHTS = (0.7, 0.45, 1.3)          # (w_ip, w_gd, w_iaf) of the GPU cases
#: seed per kind of row; the seeds were tried in order against the two margins by the model alone (no device in the loop)
#: and the first that met both at every shape is frozen
SEEDS = {"rand": 1, "rand2": 2, "zeros": 3, "same": 4, "double": 5, "nan": 6, "void": 7, "floor": 8, "floor2": 9}
KINDS = tuple(SEEDS)
#: the batches of a shape: rows and the floor of the call
BATCHES = {"main": (("rand", "zeros", "same"), 0.0), "odd": (("double", "nan", "void"), 0.0),
           "floor": (("floor", "rand2", "floor2"), FLOOR), "lone": (("rand",), 0.0)}


def zero_cells(nT, nF):
    """((t, f) zeroed in est, (t, f) zeroed in clean): the four corners, an interior cell and a pair of neighbours."""
    tm, fm = nT // 2, nF // 2
    est = {(0, 0), (nT - 1, nF - 1), (tm, fm), (tm, fm + 1), (nT - 1, 57)}
    clean = {(0, nF - 1), (nT - 1, 0), (tm, fm + 3), (0, 100), (tm, 1)}
    return sorted(est), sorted(clean)


@lru_cache(maxsize=None)
def row(kind, nT, nF):
    """(est_real, est_imag, clean_re, clean_im) float32 [T, F] of a kind of row."""
    g = np.random.Generator(np.random.PCG64(1000 * SEEDS[kind] + 7 * nT + nF))
    er, ei, cr, ci = (g.standard_normal((nT, nF)).astype(np.float32) * np.float32(0.5) for _ in range(4))
    if kind == "zeros":
        ze, zc = zero_cells(nT, nF)
        for t, f in ze:
            er[t, f] = ei[t, f] = 0.0
        for t, f in zc:
            cr[t, f] = ci[t, f] = 0.0
    elif kind == "same":
        er, ei = cr.copy(), ci.copy()
    elif kind == "double":
        er, ei = cr * np.float32(2), ci * np.float32(2)
    elif kind == "nan":
        er[nT // 2, 5] = np.nan
        ci[0, nF - 2] = np.inf
        ei[nT - 1, 77] = -np.inf
    elif kind == "void":
        er[:], ei[:] = 0.0, 0.0
    elif kind in ("floor", "floor2"):
        # a tenth of the cells of each spectrum at a magnitude of 1e-3 .. 5e-3, below the floor of 1e-2; the rest stay
        small_e, small_c = g.random((nT, nF)) < 0.1, g.random((nT, nF)) < 0.1
        scale = (g.uniform(1e-3, 5e-3, (nT, nF)) / np.maximum(np.hypot(er, ei), 1e-6)).astype(np.float32)
        er, ei = np.where(small_e, er * scale, er), np.where(small_e, ei * scale, ei)
        scale = (g.uniform(1e-3, 5e-3, (nT, nF)) / np.maximum(np.hypot(cr, ci), 1e-6)).astype(np.float32)
        cr, ci = np.where(small_c, cr * scale, cr), np.where(small_c, ci * scale, ci)
    out = tuple(np.ascontiguousarray(x, dtype=np.float32) for x in (er, ei, cr, ci))
    for x in out:
        x.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def row_model(kind, nT, nF, k3, floor, way="w") -> Eval:
    return evaluate(*row(kind, nT, nF), k3, floor, LD if way == "w" else np.float64)


def batch(name, nT, nF):
    """(est_real [B, 1, T, F], est_imag, clean_spec [B, 2, T, F], the rows' kinds, the call's floor) of a batch."""
    kinds, floor = BATCHES[name]
    rows = [row(k, nT, nF) for k in kinds]
    est_real = np.stack([r[0] for r in rows])[:, None]
    est_imag = np.stack([r[1] for r in rows])[:, None]
    clean = np.stack([np.stack([r[2], r[3]]) for r in rows])
    return est_real, est_imag, clean, kinds, floor
