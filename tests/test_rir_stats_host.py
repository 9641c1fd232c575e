"""CPU side of the room-response meter (cmgan_amd/csrc/rir_stats.hip; include/cmgan_hip.h, "What a room impulse response
measures as"): the long-double model the GPU tests compare the kernels with (tests/rir_stats_model.py) against closed
forms, hand-computed responses and a naive loop, the library's symbols and workspace formula, and every argument error of
cmgan_rir_stats, Engine.rir_stats, RirBank.where and DynamicMixer(room_stats=), all of which are judged before a handle or
a GPU is needed."""
import math

import numpy as np
import pytest
import torch

import rir_stats_model as M
from cmgan_amd import _lib
from cmgan_amd.engine import RIR_MAX_BANDS, RIR_MAX_FILTER, RIR_STATS_COLUMNS, RirStats, check_rir_stats_args
from cmgan_amd.mixing import DynamicMixer, NoiseBank, RirBank

BADARG, UNSUPPORTED = -1, -3
CPU = torch.device("cpu")
LD = np.longdouble


# ------------------------------------------------------------------ the model against closed forms
@pytest.mark.parametrize("db_per_sample,n", [(0.013, 12000), (0.047, 3000)])
def test_geometric_response_has_the_closed_form_curve_and_times(db_per_sample, n):
    fs = 16000
    r = LD(10.0) ** (LD(-db_per_sample) / 20)
    k = np.arange(n)
    y = r ** k.astype(LD)
    w, o50, o80 = M.offsets(fs, 2.5)
    val, bnd, status, ka, edc, bedc, hits = M.slice_stats(y, np.zeros(n, dtype=LD), 0, n, fs, w, o50, o80)
    closed = r ** (2 * k.astype(LD)) * (1 - r ** (2 * (n - k).astype(LD))) / (1 - r * r)
    assert float(np.max(np.abs(edc - closed.astype(np.float64)) / closed.astype(np.float64))) <= 1e-12
    assert status == 0 and hits == 0
    # ka(x): the smallest k with r^2k (1 - r^2(n-k)) <= c_x (1 - r^2n)
    for x, c in enumerate(M.DOWN):
        want = int(np.nonzero(closed <= LD(c) * closed[0])[0][0])
        assert ka[x] == want and abs(want - (5, 10, 25, 35)[x] / db_per_sample) <= 2
    k50 = o50
    tail = 1 - r ** (2 * LD(n - k50))
    assert abs(val[M.C50] - float(10 * np.log10((1 - r ** (2 * LD(k50))) / (r ** (2 * LD(k50)) * tail)))) <= 1e-10
    assert abs(val[M.D50] - float((1 - r ** (2 * LD(k50))) / (1 - r ** (2 * LD(n))))) <= 1e-13
    assert val[M.E_] == float(closed[0]) and val[M.K0] == 0.0
    # the curve bends down towards its end (the sum stops at n), so the fitted time lies a little below the limit
    limit = -3.0 / (fs * math.log10(float(r)))
    assert limit == pytest.approx(60.0 / (db_per_sample * fs))
    for col in (M.EDT, M.T20, M.T30):
        assert 0.999 * limit < val[col] <= limit * (1 + 1e-12), (col, val[col], limit)
    assert np.all(bnd[[M.EDT, M.T20, M.T30]] < 1e-9)


def test_t30_tends_to_the_limit_as_the_response_grows():
    fs, db = 16000, 0.02
    r = LD(10.0) ** (LD(-db) / 20)
    limit = -3.0 / (fs * math.log10(float(r)))
    gap = []
    for n in (2000, 3000, 6000):                                  # 40, 60, 120 dB of decay within the response
        y = r ** np.arange(n).astype(LD)
        val = M.slice_stats(y, np.zeros(n, dtype=LD), 0, n, fs, *M.offsets(fs, 2.5))[0]
        gap.append(limit - val[M.T30])
    assert gap[0] > gap[1] > gap[2] >= 0.0 and gap[2] < 1e-9 * limit


# ------------------------------------------------------------------ special responses
def test_single_impulse():
    h = np.zeros(100, dtype=np.float32)
    h[10] = -0.5
    m = M.rir_stats_row(h, fs=16000)
    v = m["values"][0]
    assert m["k0"] == 10 and v[M.K0] == 10.0 and v[M.E_] == 0.25
    assert v[M.DRR] == math.inf and v[M.C50] == math.inf and v[M.C80] == math.inf and v[M.D50] == 1.0 and v[M.TS] == 0.0
    assert m["status"][0] == M.NO_EDT | M.NO_T20 | M.NO_T30 and np.all(np.isnan(v[[M.EDT, M.T20, M.T30]]))
    assert m["ka"][0].tolist() == [11] * 4                        # the curve is E up to the impulse and 0 after it
    assert np.all(m["edc"][0][:11] == 0.25) and not m["edc"][0][11:].any()


def test_two_impulses_by_hand():
    fs = 16000
    h = np.zeros(2000, dtype=np.float32)
    h[5], h[1005] = 1.0, 0.5                                     # 62.5 ms apart: outside the direct window, after k50 and k80
    v = M.rir_stats_row(h, fs=fs)["values"][0]
    assert v[M.E_] == 1.25 and v[M.K0] == 5.0
    assert v[M.DRR] == pytest.approx(10 * math.log10(4.0), abs=1e-12)
    assert v[M.C50] == pytest.approx(10 * math.log10(4.0), abs=1e-12)
    assert v[M.C80] == math.inf                                   # k80 = 5 + 1280 lies behind the echo
    assert v[M.D50] == pytest.approx(0.8, abs=1e-15)
    assert v[M.TS] == pytest.approx(1000 * 0.25 / (fs * 1.25), abs=1e-15)
    # a wider direct window takes the echo in: nothing is left outside it
    assert M.rir_stats_row(h, fs=fs, direct_ms=62.5)["values"][0][M.DRR] == math.inf
    assert M.offsets(fs, 2.5) == (40, 800, 1280) and M.offsets(8000, 0.0) == (0, 400, 640) and M.offsets(10, 50.0)[0] == 1


def test_zero_and_non_finite_rows():
    m = M.rir_stats_row(np.zeros(50, dtype=np.float32))
    assert m["status"][0] == M.ZERO | M.NO_EDT | M.NO_T20 | M.NO_T30
    assert m["values"][0][M.E_] == 0.0 and np.all(np.isnan(m["values"][0][1:]))
    for bad in (np.nan, np.inf):
        h = M.decaying_noise(1, 300, 0.5)
        h[200] = bad
        filt = np.zeros((2, 3))
        filt[:, 1] = 1.0
        m = M.rir_stats_row(h, filt=filt)
        assert np.all(m["status"] == M.NONFINITE | M.NO_EDT | M.NO_T20 | M.NO_T30) and np.all(np.isnan(m["values"]))
        assert M.rir_stats_row(h, n=200)["status"][0] & M.NONFINITE == 0      # the sample beyond n is not looked at


def test_tie_for_the_maximum_falls_to_the_first_index():
    h = M.decaying_noise(3, 400, k0=100)
    h[300] = -h[100]
    assert M.rir_stats_row(h)["k0"] == 100


# ------------------------------------------------------------------ the model's band path against a naive loop
def test_band_signal_equals_the_naive_double_loop():
    rng = np.random.default_rng(5)
    n, NF = 40, 5
    D = (NF - 1) // 2
    h = rng.standard_normal(n).astype(np.float32)
    g = rng.standard_normal(NF)
    y, mag = M.band_signal(h, g)
    for k in range(n):
        acc = mg = 0.0
        for j in range(NF):
            q = k + D - j
            v = float(h[q]) if 0 <= q < n else 0.0
            acc += g[j] * v
            mg += abs(g[j] * v)
        assert abs(float(y[k]) - acc) <= 8 * 2.0 ** -53 * mg and abs(float(mag[k]) - mg) <= 8 * 2.0 ** -53 * mg
    # a delta filterbank reproduces the broad-band slice, with a bound that is no longer zero
    delta = np.zeros((1, NF))
    delta[0, D] = 1.0
    x = M.decaying_noise(2, 600, 0.2)
    m = M.rir_stats_row(x, filt=delta)
    assert m["guard_hits"] == 0 and np.array_equal(m["values"][0], m["values"][1], equal_nan=True)
    assert np.all(m["bounds"][1][[M.E_, M.DRR, M.T30]] > m["bounds"][0][[M.E_, M.DRR, M.T30]])


def test_guard_counts_decisions_within_reach_of_rounding():
    n, fs = 3000, 16000
    y = (LD(10.0) ** (LD(-0.047) / 20)) ** np.arange(n).astype(LD)
    args = (0, n, fs, *M.offsets(fs, 2.5))
    assert M.slice_stats(y, np.zeros(n, dtype=LD), *args)[6] == 0
    # an error bound on the band signal as large as the signal leaves every decision open
    assert M.slice_stats(y, np.abs(y), *args)[6] > 4
    # a flat stretch that sits on a threshold within a rounding
    z = np.zeros(400, dtype=LD)
    z[0], z[300] = 1.0, math.sqrt(0.1 / 0.9)                      # EDC falls from E to 0.1 E (1 + O(u)) at k = 1
    hits = M.slice_stats(z, np.zeros(400, dtype=LD), *((0, 400, fs) + M.offsets(fs, 2.5)))[6]
    assert hits >= 1


# ------------------------------------------------------------------ the library without a GPU
def test_symbols_columns_tile_and_abi():
    lib = _lib.load()
    for name in ("cmgan_rir_stats", "cmgan_rir_stats_workspace_bytes", "cmgan_rir_stats_tile", "cmgan_rir_stats_columns"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.cmgan_rir_stats_columns() == RIR_STATS_COLUMNS == M.P == len(RirStats._fields) - 1 == 10
    assert lib.cmgan_rir_stats_tile() == 1024
    assert lib.cmgan_rir_max_bands() == RIR_MAX_BANDS and lib.cmgan_rir_max_filter() == RIR_MAX_FILTER
    assert lib.cmgan_abi_version() == _lib.ABI_VERSION >= 16
    assert RirStats._fields == ("energy", "direct", "drr_db", "c50_db", "c80_db", "d50", "ts", "edt", "t20", "t30", "status")


def _ws_formula(R, K, NB):
    up = lambda v: (v + 255) & ~255
    nt = (K + 1023) // 1024
    return 2 * up(R * (NB + 1) * nt * 1024 * 8) + up(R * (NB + 1) * nt * 8)


def test_workspace_formula():
    lib = _lib.load()
    ws = lambda R, K, NB, NF: int(lib.cmgan_rir_stats_workspace_bytes(None, R, K, NB, NF))
    for R in (1, 5, 32, 65535):
        for K in (1, 1023, 1024, 1025, 8000, 65536):
            for NB, NF in ((0, 1), (1, 3), (7, 511), (8, 1023)):
                assert ws(R, K, NB, NF) == _ws_formula(R, K, NB) > 0 and ws(R, K, NB, NF) % 256 == 0, (R, K, NB, NF)
    base = (4, 3000, 3, 511)
    for i, more in enumerate((5, 3001 + 1024, 4, 513)):
        grown = list(base)
        grown[i] = more
        assert ws(*base) <= ws(*grown), (i, more)
    assert ws(4, 3000, 3, 511) < ws(5, 3000, 3, 511) and ws(4, 3000, 3, 511) < ws(4, 3000, 4, 511)
    for bad in ((0, 100, 0, 1), (-1, 100, 0, 1), (65536, 100, 0, 1), (1, 0, 0, 1), (1, 65537, 0, 1), (1, 100, -1, 1),
                (1, 100, 9, 1), (1, 100, 1, 0), (1, 100, 1, 4), (1, 100, 1, 1025), (1, 100, 1, -3)):
        assert ws(*bad) == 0, bad


def test_library_rejects_bad_arguments_before_it_needs_a_handle():
    lib = _lib.load()
    rir = np.zeros(8192, dtype=np.float32)
    length = np.zeros(8, dtype=np.int32)
    filt = np.zeros(4096, dtype=np.float64)
    stats = np.zeros(1024, dtype=np.float64)
    status = np.zeros(64, dtype=np.int32)
    edc = np.zeros(1 << 16, dtype=np.float64)
    raw = np.zeros(1 << 20, dtype=np.uint8)
    base = (raw.ctypes.data + 255) & ~255
    pr, pl, pf, pv, pt, pe = (a.ctypes.data for a in (rir, length, filt, stats, status, edc))

    def call(rir=pr, R=2, K=1500, ld=1500, length=pl, filt=pf, NB=2, NF=511, fs=16000, direct_ms=2.5, stats=pv, status=pt,
             edc=pe, ws=base, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = _ws_formula(R, K, NB) if 1 <= R <= 2 and 1 <= K <= 2048 and 0 <= NB <= 8 else 4096
        rc = lib.cmgan_rir_stats(None, rir, R, K, ld, length, filt, NB, NF, fs, direct_ms, stats, status, edc, ws, ws_bytes, None)
        return rc, (lib.cmgan_last_error(None) or b"").decode()

    cases = {
        "null pointer": [dict(rir=None), dict(stats=None)],
        "4-byte aligned": [dict(rir=pr + 2), dict(length=pl + 1), dict(status=pt + 2)],
        "8-byte aligned": [dict(filt=pf + 4), dict(stats=pv + 4), dict(edc=pe + 4)],
        "need 1 <= R": [dict(R=0), dict(R=-3), dict(R=65536), dict(K=0), dict(K=-1), dict(ld=1499)],
        "need 0 <= NB": [dict(NB=-1), dict(NB=9)],
        "must be null with NB = 0 and only then": [dict(filt=None), dict(NB=0)],
        "filter length must be odd": [dict(NF=0), dict(NF=-1), dict(NF=510), dict(NF=1024)],
        "fs must be positive": [dict(fs=0), dict(fs=-16000)],
        "direct_ms must be finite": [dict(direct_ms=-0.5), dict(direct_ms=math.inf), dict(direct_ms=math.nan)],
        "workspace": [dict(ws=None), dict(ws=base + 64), dict(ws_bytes=_ws_formula(2, 1500, 2) - 1), dict(ws_bytes=0)],
    }
    for text, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == BADARG and text in msg, (kw, rc, msg)
    for text, kw in (("responses of up to 65536 taps", dict(K=65537, ld=65537)), ("filters of up to 1023 taps", dict(NF=1025))):
        rc, msg = call(**kw)
        assert rc == UNSUPPORTED and text in msg, (kw, rc, msg)
    # everything in order: only the handle is missing - nothing was enqueued, nothing was written
    for kw in (dict(), dict(length=None), dict(status=None), dict(edc=None), dict(filt=None, NB=0, NF=1), dict(direct_ms=0.0),
               dict(NF=1), dict(NF=1023), dict(NB=8, R=1), dict(ld=4096), dict(fs=1)):
        rc, msg = call(**kw)
        assert rc == BADARG and "null handle" in msg, (kw, rc, msg)
    assert not stats.any() and not status.any() and not edc.any()


# ------------------------------------------------------------------ Engine.rir_stats' argument rules
def test_check_rir_stats_args():
    ok = torch.zeros(3, 2000)
    filt = torch.zeros(7, 511, dtype=torch.float64)
    assert check_rir_stats_args(CPU, ok) == (3, 2000, 0, 1)
    assert check_rir_stats_args(CPU, ok, torch.zeros(3, dtype=torch.int32), filt, 8000, 0.0) == (3, 2000, 7, 511)
    assert check_rir_stats_args(CPU, torch.zeros(3, 2500)[:, :2000], None, filt[:1, :1].contiguous()) == (3, 2000, 1, 1)
    with pytest.raises(TypeError, match="rir: expected a torch.Tensor"):
        check_rir_stats_args(CPU, np.zeros((3, 2000), dtype=np.float32))
    with pytest.raises(TypeError, match="rir: expected float32"):
        check_rir_stats_args(CPU, ok.double())
    with pytest.raises(RuntimeError, match="rir: tensor is on cpu"):
        check_rir_stats_args(torch.device("cuda:0"), ok)
    for bad in (torch.zeros(2000), torch.zeros(1, 3, 2000), torch.zeros(0, 2000), torch.zeros(3, 0)):
        with pytest.raises(ValueError, match="rir: expected \\[B, L\\]"):
            check_rir_stats_args(CPU, bad)
    with pytest.raises(ValueError, match="rir: at most 65535 rows"):
        check_rir_stats_args(CPU, torch.zeros(1, 1).expand(65536, 1))
    with pytest.raises(ValueError, match="rir: rows of up to 65536 samples"):
        check_rir_stats_args(CPU, torch.zeros(1, 1).expand(1, 65537))
    with pytest.raises(ValueError, match="rir: rows must be contiguous"):
        check_rir_stats_args(CPU, torch.zeros(3, 4000)[:, ::2])
    with pytest.raises(TypeError, match="length: expected int32"):
        check_rir_stats_args(CPU, ok, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="length: expected \\[3\\]"):
        check_rir_stats_args(CPU, ok, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError, match="filters: expected float64"):
        check_rir_stats_args(CPU, ok, None, filt.float())
    for bad in (torch.zeros(511, dtype=torch.float64), torch.zeros(9, 511, dtype=torch.float64),
                torch.zeros(7, 510, dtype=torch.float64), torch.zeros(7, 1025, dtype=torch.float64),
                torch.zeros(0, 511, dtype=torch.float64)):
        with pytest.raises(ValueError, match="filters: expected \\[NB, NF\\]"):
            check_rir_stats_args(CPU, ok, None, bad)
    with pytest.raises(ValueError, match="filters: must be contiguous"):
        check_rir_stats_args(CPU, ok, None, torch.zeros(7, 1022, dtype=torch.float64)[:, ::2])
    for fs in (0, -16000, 16000.5, True, 2 ** 31):
        with pytest.raises(ValueError, match="fs must be a positive sample rate"):
            check_rir_stats_args(CPU, ok, None, None, fs)
    for ms in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="direct_ms must be finite"):
            check_rir_stats_args(CPU, ok, None, None, 16000, ms)


# ------------------------------------------------------------------ RirBank.where and DynamicMixer(room_stats=)
def _measured_bank(t30, drr, c50):
    """A bank of len(t30) two-tap responses with made-up stats in two columns (column 1 = column 0 + 1)."""
    R = len(t30)
    col = lambda v: torch.tensor([[x, x + 1.0] for x in v], dtype=torch.float64)
    filler = torch.zeros(R, 2, dtype=torch.float64)
    stats = RirStats(filler, filler, col(drr), col(c50), filler, filler, filler, filler, filler, col(t30),
                     torch.zeros(R, 2, dtype=torch.int32))
    data = torch.arange(R * 2, dtype=torch.float32).reshape(R, 2)
    rooms = torch.arange(R * 15, dtype=torch.float64).reshape(R, 15)
    return RirBank(data, torch.full((R,), 2, dtype=torch.int32), rooms, None, stats)


def test_where_selects_rows_in_closed_ranges_and_never_a_nan():
    bank = _measured_bank([0.2, 0.3, math.nan, 0.5, 0.6], [-3.0, 0.0, 5.0, 8.0, 12.0], [1.0, 2.0, 3.0, 4.0, 5.0])
    sub = bank.where(t30=(0.3, 0.5))
    assert len(sub) == 2 and sub.data.tolist() == [[2.0, 3.0], [6.0, 7.0]] and sub.stats.t30[:, 0].tolist() == [0.3, 0.5]
    assert sub.rooms[:, 0].tolist() == [15.0, 45.0] and sub.bands is None and sub.length.tolist() == [2, 2]
    assert sub.stats.status.dtype == torch.int32 and sub.data.is_contiguous()
    assert len(bank.where(drr_db=(-10.0, 20.0))) == 5             # the NaN is in t30, which was not asked
    assert len(bank.where(t30=(0.0, 10.0))) == 4
    assert bank.where(t30=(0.0, 10.0), drr_db=(0.0, 8.0), c50_db=(2.5, 10.0)).stats.drr_db[:, 0].tolist() == [8.0]
    assert bank.where(t30=(1.3, 1.5), band=1).stats.t30[:, 0].tolist() == [0.3, 0.5]
    with pytest.raises(ValueError, match="selects no row"):
        bank.where(t30=(2.0, 3.0))
    with pytest.raises(ValueError, match="t30 must be"):
        bank.where(t30=(0.5, 0.3))
    with pytest.raises(ValueError, match="t30 must be"):
        bank.where(t30=0.4)
    for band in (2, -1, True, 0.5):
        with pytest.raises(ValueError, match="band must be a column"):
            bank.where(t30=(0.0, 1.0), band=band)
    with pytest.raises(ValueError, match="needs a measured bank"):
        RirBank(bank.data, bank.length).where(t30=(0.0, 1.0))


def test_with_identity_keeps_a_measured_bank_measured():
    bank = _measured_bank([0.2, 0.3], [1.0, 2.0], [3.0, 4.0]).with_identity()
    assert len(bank) == 3 and tuple(bank.stats.t30.shape) == (3, 2)
    assert bank.stats.energy[2].tolist() == [1.0, 1.0] and bank.stats.drr_db[2].tolist() == [math.inf, math.inf]
    assert bool(torch.isnan(bank.stats.t30[2]).all()) and bank.stats.status[2].tolist() == [28, 28]
    assert RirBank(bank.data, bank.length).with_identity().stats is None


class _NoEngine:
    device = CPU


def test_mixer_room_stats_option():
    noise = NoiseBank.from_arrays([np.ones(100, dtype=np.float32)])
    plain = RirBank.from_arrays([np.ones(3, dtype=np.float32)])
    with pytest.raises(ValueError, match="room_stats=True needs rooms, or a rir_bank that has been measured"):
        DynamicMixer(_NoEngine(), noise, room_stats=True)
    with pytest.raises(ValueError, match="room_stats=True needs rooms, or a rir_bank that has been measured"):
        DynamicMixer(_NoEngine(), noise, plain, room_stats=True)
    with pytest.raises(TypeError, match="room_stats must be a bool"):
        DynamicMixer(_NoEngine(), noise, plain, room_stats=1)
    m = DynamicMixer(_NoEngine(), noise, plain)
    assert m.room_stats is False and m.last_room_stats is None
    measured = _measured_bank([0.2, 0.3, 0.4], [1.0, 2.0, 3.0], [3.0, 4.0, 5.0])
    gen = lambda: torch.Generator().manual_seed(3)
    m = DynamicMixer(_NoEngine(), noise, measured, room_stats=True, p_reverb=0.5, generator=gen())
    d = m.draw(8)
    got = m._room_stats(d, m.rir_bank, None)
    assert torch.equal(got.drr_db, m.rir_bank.stats.drr_db[d.rir_index.long()]) and tuple(got.t30.shape) == (8, 2)
    # the option draws nothing: the same draws as a mixer without it
    d0 = DynamicMixer(_NoEngine(), noise, measured, p_reverb=0.5, generator=gen()).draw(8)
    assert all(torch.equal(a, b) for a, b in zip(d[:6], d0[:6]))
