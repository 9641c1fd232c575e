"""CPU side of the speed perturbation (cmgan_amd/csrc/warp.hip; include/cmgan_hip.h, "Speed perturbation"): the numpy
model the GPU tests compare the kernel with (tests/warp_model.py) against facts that do not come from it, the condition
on E for every row the GPU tests judge, cmgan_warp_out_len against the model's count, and every argument error of
cmgan_warp, Engine.warp and DynamicMixer(speed=, p_speed=), all of which are judged before a handle or a GPU is needed."""
import math

import numpy as np
import pytest
import torch

import warp_model as M
from cmgan_amd import _lib
from cmgan_amd.engine import WARP_MAX_RATE, WARP_TILE, WARP_ZEROS, check_warp_args
from cmgan_amd.mixing import DynamicMixer, NoiseBank, warp_len

BADARG = -1
CPU = torch.device("cpu")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ the model against facts that are not its own
def test_sinpi_and_cospi_are_exact_where_they_should_be():
    for F in (np.float64, np.longdouble):
        z = np.arange(-8, 9).astype(F)
        assert not _any_nonzero(M.sinpi(z)) and np.array_equal(np.abs(M.cospi(z)), np.ones(17, dtype=F))
        assert not _any_nonzero(M.cospi(z + F(0.5))) and np.array_equal(np.abs(M.sinpi(z + F(0.5))), np.ones(17, dtype=F))
        v = np.linspace(-70.0, 70.0, 1001).astype(F)
        assert float(np.max(np.abs(M.sinpi(v) - np.sin(np.pi * v.astype(np.float64))))) < 1e-12
        assert float(np.max(np.abs(M.cospi(v) - np.cos(np.pi * v.astype(np.float64))))) < 1e-12


def _any_nonzero(a):
    return bool(np.any(a != 0))


@pytest.mark.parametrize("form", [M.direct, M.direct_ld, M.as_kernel])
def test_unit_rate_and_full_band_is_a_bitwise_copy(form):
    x = M.noise(1, 700)
    for zeros in (4, 24, 64):
        y = form(x, 700, 1.0, zeros, 1.0)
        assert len(y) == 700 and np.array_equal(_bits(y.astype(np.float32)), _bits(x))
    assert not np.array_equal(_bits(form(x, 700, 1.0, 24, 0.95).astype(np.float32)), _bits(x))     # filtered, not copied


@pytest.mark.parametrize("r", [0.9, 1.1])
def test_a_sine_comes_out_at_the_warped_frequency(r):
    """A unit 1 kHz sine at 16 kHz: 7.9e-6 (r = 0.9) and 3.1e-6 (r = 1.1) were measured on the model."""
    x = np.sin(2.0 * np.pi * 1000.0 * np.arange(8000) / 16000.0)
    ns = np.arange(200, 1801)
    want = np.sin(2.0 * np.pi * 1000.0 * ns * r / 16000.0)
    for form in (M.direct, M.as_kernel):
        err = float(np.max(np.abs(form(x, 8000, r, ns=ns) - want)))
        print(f"[warp] sine at r = {r}, {form.__name__}: {err:.2e}")
        assert err <= 2e-5


@pytest.mark.parametrize("r", [0.8, 1.0, 1.25, 3.0])
def test_a_constant_stays_a_constant(r):
    """At most 8.7e-6 above 1 was measured on the model (the taps are not normalised to unity at DC)."""
    x = np.ones(4000, dtype=np.float32)
    ns = np.arange(300, M.count(4000, r) - 300)
    for form in (M.direct, M.as_kernel):
        err = float(np.max(np.abs(form(x, 4000, r, ns=ns) - 1.0)))
        print(f"[warp] constant at r = {r}, {form.__name__}: {err:.2e}")
        assert err <= 1e-5


def test_long_double_form():
    x = M.noise(2, 700)
    for r in (0.25, 1.0371, 4.0):
        ld = M.direct_ld(x, 700, r)
        f64 = M.direct(x, 700, r)
        assert ld.dtype == np.longdouble and f64.dtype == np.float64 and len(ld) == len(f64) == M.count(700, r)
        assert float(np.max(np.abs(f64 - ld))) < 1e-13
        if np.finfo(np.longdouble).eps < 1e-18:                          # where long double is wider than double
            assert float(np.max(np.abs(f64 - ld))) > 0.0
            assert np.array_equal(f64.astype(np.float32), ld.astype(np.float32))


def test_ulp32():
    for w in (1.0, 0.75, 0.5, 1.9999, 3e-5, -0.3, 1e-42, 0.0):
        want = float(np.spacing(np.float32(abs(w)))) if abs(w) >= 2.0 ** -126 else 2.0 ** -149
        assert float(M.ulp32(w)) == want, w


def test_support_and_tap_counts():
    """51 - 203 taps for rates 0.25 .. 4 at the defaults, away from the row's ends."""
    for r, taps in ((0.25, 51), (1.0, 51), (1.1, 55), (4.0, 203)):
        fc, W = M.geometry(r, 24, 0.95)
        t = np.arange(300, 320, dtype=np.float64) * r
        k0, k1 = M.support(t, W, 10 ** 6)
        assert np.all(np.abs(t - k0) < W) and np.all(np.abs(t - k1) < W)
        assert np.all(np.abs(t - (k0 - 1)) >= W) and np.all(np.abs(t - (k1 + 1)) >= W)
        assert abs(int(np.max(k1 - k0 + 1)) - taps) <= 1, (r, int(np.max(k1 - k0 + 1)))
    k0, k1 = M.support(np.array([0.0, 5.5]), 4.0, 7)                      # |d| < W is strict; the clamp to the row
    assert k0.tolist() == [0, 2] and k1.tolist() == [3, 6]


def test_every_row_of_the_gpu_tests_respects_the_condition_on_E():
    """The rule |g - w| <= ulp32(w) / 2 + E may be used on a row only if E <= 2^-10 x ulp32(rms) / 2."""
    rows = M.build_rows(int(_lib.load().cmgan_warp_tile()))
    assert len(rows) > 100
    top, tight = 0.0, 0.0
    for key, row in rows.items():
        E, w, ns = M.case(key)
        bound = M.condition(E, w)
        assert len(w) == len(ns) > 0 and np.all(np.isfinite(w.astype(np.float64))), key
        assert E <= bound, f"{key}: E = {E:.3e} above {bound:.3e}"
        top, tight = max(top, E), max(tight, E / bound)
    print(f"[warp] {len(rows)} rows: largest E {top:.3e}, at most {tight:.2e} of the bound")


# ------------------------------------------------------------------ the library without a GPU
def test_symbols_tile_and_abi():
    lib = _lib.load()
    for name in ("cmgan_warp", "cmgan_warp_tile", "cmgan_warp_max_rate", "cmgan_warp_max_zeros", "cmgan_warp_out_len"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    T = lib.cmgan_warp_tile()
    assert T == WARP_TILE and T >= 64 and T % 64 == 0
    assert lib.cmgan_warp_max_rate() == WARP_MAX_RATE == M.MAX_RATE == 4.0 and 1.0 / WARP_MAX_RATE == M.MIN_RATE
    assert lib.cmgan_warp_max_zeros() == WARP_ZEROS[1] == 64
    assert lib.cmgan_abi_version() == _lib.ABI_VERSION >= 12


def test_out_len():
    lib = _lib.load()
    f = lambda n, r: int(lib.cmgan_warp_out_len(n, r))
    for (n, r), want in {(10, 1.0): 10, (10, 2.0): 5, (10, 3.0): 4, (7, 0.7): 10, (11, 1.1): 10, (1, 4.0): 1, (0, 1.0): 0,
                         (1, 0.25): 4, (32000, 1.0): 32000}.items():
        assert f(n, r) == M.count(n, r) == M.count_brute(n, r) == want, (n, r)
    rng = np.random.default_rng(14)
    for _ in range(1000):
        n = int(rng.integers(0, 3000))
        r = float(np.exp(rng.uniform(np.log(0.25), np.log(4.0)))) if rng.random() < 0.8 else float(rng.integers(1, 17)) / 4.0
        r = min(max(r, 0.25), 4.0)
        got = f(n, r)
        assert got == M.count(n, r) == M.count_brute(n, r), (n, r, got)
        assert got == 0 or float(got - 1) * r < n <= float(got) * r
    for n, r in ((2 ** 31 - 1, 0.25), (2 ** 40, 1.0001), (2 ** 50, 3.9)):
        assert f(n, r) == M.count(n, r)
    for n, r in ((-1, 1.0), (10, 0.0), (10, -1.0), (10, math.nan), (10, math.inf), (10, np.nextafter(4.0, 5.0)),
                 (10, np.nextafter(0.25, 0.0)), (2 ** 50 + 1, 1.0)):
        assert f(n, float(r)) == -1, (n, r)
    assert warp_len(32000, 1.1) == f(32000, 1.1) == 29091 and warp_len(0, 1.0) == 0
    for n, r in ((-1, 1.0), (100, 5.0), (100, math.nan)):
        with pytest.raises(ValueError, match="warp_len needs"):
            warp_len(n, r)


def test_library_rejects_bad_arguments_before_it_needs_a_handle():
    lib = _lib.load()
    x = np.zeros(8192, dtype=np.float32)
    y = np.zeros(8192, dtype=np.float32)
    lengths = np.zeros(8, dtype=np.int32)
    out_len = np.full(8, 7, dtype=np.int32)
    status = np.full(8, 7, dtype=np.int32)
    rate = np.ones(9, dtype=np.float64)
    px, py, pl, po, pt, pr = (a.ctypes.data for a in (x, y, lengths, out_len, status, rate))

    def call(x=px, B=2, L=1500, ldx=1500, lengths=pl, rate=pr, zeros=24, rolloff=0.95, y=py, N=1600, ldy=1600, out_len=po,
             status=pt):
        rc = lib.cmgan_warp(None, x, B, L, ldx, lengths, rate, zeros, rolloff, y, N, ldy, out_len, status, None)
        return rc, (lib.cmgan_last_error(None) or b"").decode()

    cases = {
        "null pointer": [dict(x=None), dict(rate=None), dict(y=None)],
        "4-byte aligned": [dict(x=px + 2), dict(y=py + 1), dict(lengths=pl + 1), dict(out_len=po + 2), dict(status=pt + 3)],
        "8-byte aligned": [dict(rate=pr + 4)],
        "need 1 <= B": [dict(B=0), dict(B=-3), dict(B=65536), dict(L=0), dict(L=-1), dict(N=0), dict(N=-2), dict(ldx=1499),
                        dict(ldy=1599)],
        "zeros must lie": [dict(zeros=3), dict(zeros=65), dict(zeros=0), dict(zeros=-24)],
        "rolloff must lie": [dict(rolloff=0.49), dict(rolloff=1.0 + 1e-12), dict(rolloff=0.0), dict(rolloff=math.nan),
                             dict(rolloff=math.inf), dict(rolloff=-0.95)],
        "overlap": [dict(y=px), dict(y=px + 4 * 1500), dict(y=px + 4 * 2999), dict(x=py + 4 * 100), dict(x=py + 4 * 3199)],
    }
    for text, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == BADARG and text in msg, (kw, rc, msg)
    # everything in order: only the handle is missing - nothing was enqueued, nothing was written
    for kw in (dict(), dict(lengths=None), dict(out_len=None), dict(status=None), dict(zeros=4), dict(zeros=64),
               dict(rolloff=0.5), dict(rolloff=1.0), dict(y=px + 4 * 3000), dict(x=py + 4 * 3200), dict(N=1, ldy=1),
               dict(B=1, L=1, ldx=1), dict(ldx=2000, ldy=2000)):
        rc, msg = call(**kw)
        assert rc == BADARG and "null handle" in msg, (kw, rc, msg)
    assert not y.any() and (status == 7).all() and (out_len == 7).all()


# ------------------------------------------------------------------ Engine.warp's argument rules
def test_check_warp_args():
    wav = torch.zeros(3, 2000)
    rate = torch.ones(3, dtype=torch.float64)
    i32 = lambda n=3: torch.zeros(n, dtype=torch.int32)
    assert check_warp_args(CPU, wav, rate) == (3, 2000, None)
    assert check_warp_args(CPU, wav, rate, 2200, i32(), 64, 1.0) == (3, 2000, 2200)
    assert check_warp_args(CPU, wav, rate, out=torch.zeros(3, 1800)) == (3, 2000, 1800)
    assert check_warp_args(CPU, wav, rate, 1800, out=torch.zeros(3, 2500)[:, :1800]) == (3, 2000, 1800)
    view = torch.zeros(3, 2500)[:, :2000]                                # a row stride larger than L
    assert check_warp_args(CPU, view, rate, 1) == (3, 2000, 1)
    assert check_warp_args(CPU, torch.zeros(1, 7), torch.ones(1, dtype=torch.float64), zeros=4, rolloff=0.5) == (1, 7, None)
    with pytest.raises(TypeError, match="wav: expected a torch.Tensor"):
        check_warp_args(CPU, np.zeros((3, 2000), dtype=np.float32), rate)
    with pytest.raises(TypeError, match="wav: expected float32"):
        check_warp_args(CPU, wav.double(), rate)
    with pytest.raises(RuntimeError, match="wav: tensor is on cpu"):
        check_warp_args(torch.device("cuda:0"), wav, rate)
    for bad in (torch.zeros(2000), torch.zeros(1, 3, 2000), torch.zeros(0, 2000), torch.zeros(3, 0)):
        with pytest.raises(ValueError, match="wav: expected \\[B, L\\]"):
            check_warp_args(CPU, bad, rate)
    with pytest.raises(ValueError, match="at most 65535 rows"):
        check_warp_args(CPU, torch.zeros(1, 1).expand(65536, 1), rate)
    for bad in (torch.zeros(3, 4000)[:, ::2], torch.zeros(2000, 3).t(), torch.zeros(1, 2000).expand(3, 2000)):
        with pytest.raises(ValueError, match="wav: rows must be contiguous"):
            check_warp_args(CPU, bad, rate)
    with pytest.raises(TypeError, match="rate: expected float64"):
        check_warp_args(CPU, wav, rate.float())
    with pytest.raises(TypeError, match="rate: expected a torch.Tensor"):
        check_warp_args(CPU, wav, 1.1)
    for bad in (torch.ones(2, dtype=torch.float64), torch.ones(3, 1, dtype=torch.float64)):
        with pytest.raises(ValueError, match="rate: expected \\[3\\]"):
            check_warp_args(CPU, wav, bad)
    with pytest.raises(ValueError, match="rate: must be contiguous"):
        check_warp_args(CPU, wav, torch.ones(6, dtype=torch.float64)[::2])
    with pytest.raises(TypeError, match="lengths: expected int32"):
        check_warp_args(CPU, wav, rate, None, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="lengths: expected \\[3\\]"):
        check_warp_args(CPU, wav, rate, None, i32(4))
    for bad in (0, -5, 2 ** 31, 100.5, True):
        with pytest.raises(ValueError, match="n_out must be"):
            check_warp_args(CPU, wav, rate, bad)
    for bad in (3, 65, 24.5, True):
        with pytest.raises(ValueError, match="zeros must be"):
            check_warp_args(CPU, wav, rate, zeros=bad)
    for bad in (0.49, 1.01, math.nan, True):
        with pytest.raises(ValueError, match="rolloff must lie"):
            check_warp_args(CPU, wav, rate, rolloff=bad)
    with pytest.raises(TypeError, match="out: expected float32"):
        check_warp_args(CPU, wav, rate, out=torch.zeros(3, 2000, dtype=torch.float64))
    with pytest.raises(ValueError, match="out: expected \\[3, 1800\\]"):
        check_warp_args(CPU, wav, rate, 1800, out=torch.zeros(3, 1801))
    with pytest.raises(ValueError, match="out: expected \\[3, N\\]"):
        check_warp_args(CPU, wav, rate, out=torch.zeros(2, 1800))
    with pytest.raises(ValueError, match="out: rows must be contiguous"):
        check_warp_args(CPU, wav, rate, out=torch.zeros(3, 4000)[:, ::2])


# ------------------------------------------------------------------ DynamicMixer's new arguments
class _NoEngine:
    device = CPU


def _bank():
    return NoiseBank.from_arrays([np.ones(100, dtype=np.float32), np.ones(50, dtype=np.float32)])


def test_mixer_rejects_bad_speed_options():
    bank = _bank()
    for bad in ((0.2, 1.0), (0.9, 4.5), (1.1, 0.9), (math.nan, 1.0), (0.9, math.inf)):
        with pytest.raises(ValueError, match="speed must be \\(low, high\\) with"):
            DynamicMixer(_NoEngine(), bank, speed=bad)
    for bad in (1.1, "fast", (0.9,), ("a", "b")):
        with pytest.raises(ValueError, match="speed must be None or \\(low, high\\)"):
            DynamicMixer(_NoEngine(), bank, speed=bad)
    for bad in (-0.1, 1.5, math.nan):
        with pytest.raises(ValueError, match="p_speed must lie in"):
            DynamicMixer(_NoEngine(), bank, speed=(0.9, 1.1), p_speed=bad)
    m = DynamicMixer(_NoEngine(), bank)
    assert m.speed is None and m.p_speed == 1.0
    m = DynamicMixer(_NoEngine(), bank, speed=(0.25, 4), p_speed=0.5)
    assert m.speed == (0.25, 4.0) and m.p_speed == 0.5


def test_speed_draw_comes_after_the_level_draw():
    bank = _bank()
    gen = lambda s=7: torch.Generator().manual_seed(s)
    g0, g1, g2 = gen(), gen(), gen()
    d0 = DynamicMixer(_NoEngine(), bank, generator=g0, level_db=(-35, -15)).draw(2000)
    d1 = DynamicMixer(_NoEngine(), bank, generator=g1, level_db=(-35, -15), speed=None).draw(2000)
    d2 = DynamicMixer(_NoEngine(), bank, generator=g2, level_db=(-35, -15), speed=(0.9, 1.1), p_speed=0.5).draw(2000)
    assert d0._fields[-1] == "speed" and d0.speed is None and d1.speed is None
    for a, b, c in zip(d0[:-1], d1[:-1], d2[:-1]):                      # every earlier draw is what it was
        assert (a is None and b is None and c is None) or (torch.equal(a, b) and torch.equal(a, c))
    assert torch.equal(g0.get_state(), g1.get_state()) and not torch.equal(g0.get_state(), g2.get_state())
    s = d2.speed
    assert s.dtype == torch.float64 and tuple(s.shape) == (2000,) and s.is_contiguous()
    assert bool(((s >= 0.9) & (s <= 1.1)).all())
    ones = int((s == 1.0).sum())
    assert 850 < ones < 1150                                             # exactly 1.0 with probability 1 - p_speed
    moved = s[s != 1.0]
    assert float(moved.min()) < 0.91 and float(moved.max()) > 1.09 and abs(float(moved.mean()) - 1.0) < 0.01
    every = DynamicMixer(_NoEngine(), bank, generator=gen(), speed=(1.05, 1.05)).draw(50).speed
    assert bool((every == 1.05).all())
    never = DynamicMixer(_NoEngine(), bank, generator=gen(), speed=(0.5, 2.0), p_speed=0.0).draw(50).speed
    assert bool((never == 1.0).all())
