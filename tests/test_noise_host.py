"""CPU side of the synthetic noise (cmgan_amd/csrc/noise.hip; include/cmgan_hip.h, "Synthetic noise"): the model the GPU
tests compare the kernels with (tests/noise_model.py) - whole against chunks, its noise against rir_tail_model's, E for
every row the GPU tests use - then the designs (noise_fir, power_law_magnitude), what a NoiseSampler draws, the workspace
formula, and every argument error of cmgan_noise, Engine.noise, NoiseSampler, NoiseBank.synthesize and DynamicMixer(noise=),
all of which are judged before a handle or a GPU is needed."""
import math

import numpy as np
import pytest
import torch

import noise_model as M
import rir_tail_model as T
from cmgan_amd import _lib
from cmgan_amd.engine import (NOISE_MAX_FILTER, NOISE_MAX_N, NOISE_MAX_POINTS, NOISE_MAX_TONES, NOISE_TILE, check_noise_args,
                              noise_workspace_bytes)
from cmgan_amd.mixing import DynamicMixer, NoiseBank, NoiseDraw, NoiseSampler, noise_fir, power_law_magnitude

BADARG = -1
CPU = torch.device("cpu")
FS = 16000


class _NoEngine:
    device = CPU


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ the model
def test_model_whole_is_the_model_in_chunks():
    c = M.get("whole")
    row = M.rows_of(c)[0]
    for real in (np.float64, np.longdouble):
        whole = M.row_model(row, c["H"], real)
        for cuts in ((0, 256, 1000), (0, 1, 255, 257, 999, 1000), (0, 700, 1000)):
            parts = [M.row_model(row, c["H"], real, a, b - a) for a, b in zip(cuts, cuts[1:])]
            assert np.array_equal(np.concatenate(parts), whole), (real, cuts)
        # a chunk is also the row of its own with start advanced
        moved = dict(row, start=row["start"] + 256, len=744)
        assert np.array_equal(M.row_model(moved, c["H"], real), whole[256:])
    assert np.abs(whole).max() > 1.0


def test_philox_and_noise_are_rir_tails_below_2_32():
    q = np.concatenate([np.arange(-5, 300), 2 ** 32 - 1 - np.arange(3)]).astype(np.int64)
    for seed in (0, 1, -1, 0x123456789abcdef, -2 ** 63):
        got, want = M.philox4x32_10((np.maximum(q, 0), 0, 0, 0), seed), T.philox4x32_10(np.maximum(q, 0), seed)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert np.array_equal(M.nu(seed, q), T.noise(seed, q))
    # the further counter words are counter words: another block, not the same one
    far = M.nu(5, np.array([7, 2 ** 32 + 7, 2 ** 33 + 7], dtype=np.int64))
    assert len(set(far.tolist())) == 3
    a, b = M.philox4x32_10((7, 0, 0, 0), 5), M.philox4x32_10((7, 0, 1, 0), 5)
    assert any(int(x) != int(y) for x, y in zip(a, b))
    # Philox4x32-10's known answer (Random123 kat_vectors: counter and key all ones)
    kat = M.philox4x32_10((0xffffffff,) * 4, 0xffffffffffffffff)
    assert [int(w) for w in kat] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    v = M.nu(9, np.arange(200000, dtype=np.int64))
    assert abs(v.mean()) < 0.01 and abs(v.var() - 1.0) < 0.01


def test_clicks_of_the_model():
    q = np.arange(-3, 100000, dtype=np.int64)
    plain = M.excitation(3, q)
    assert np.array_equal(M.excitation(3, q, (0.0, 9.0)), plain) and not plain[:3].any()
    for thr in (1.0, 2.0 ** 26, 2.0 ** 31, 2.0 ** 32 - 1.0):
        e = M.excitation(3, q, (thr, 8.0))
        hit = e != plain
        rate = hit[3:].mean()
        p = thr / 2.0 ** 32
        assert abs(rate - p) <= 5.0 * math.sqrt(p * (1.0 - p) / 1e5) + 1e-5, (thr, rate)
        assert np.all(np.abs(e - plain)[hit] <= 8.0) and not e[:3].any()


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_slack_of_every_gpu_row_is_far_below_a_float32_ulp(name):
    c = M.get(name)
    for r, (w, E, cap, status) in enumerate(M.case_model(name)):
        peak = float(np.max(np.abs(w), initial=0.0))
        print(f"[noise] {name} row {r}: status {status}, peak {peak:.3f}, E = {E:.3e}, cap = {cap:.3e}")
        assert status == 0 and w.shape == (c["K"],)
        if M.rows_of(c)[r]["len"] > 0:
            assert peak > 0.0 and E < 2.0 ** -20 * float(M.ulp32(peak)), (name, r, E)
            assert cap <= 2.0 ** -16 * float(M.ulp32(peak))       # the cap: sixteen binary orders under the ulp at the peak


# ------------------------------------------------------------------ the designs
@pytest.mark.parametrize("n_taps", [63, 255, 1023])
def test_noise_fir_follows_the_power_law(n_taps):
    slopes = torch.tensor([-6.0, -3.0, 0.0, 3.0], dtype=torch.float64)
    h = noise_fir(power_law_magnitude(slopes, FS), n_taps)
    assert h.dtype == torch.float64 and tuple(h.shape) == (4, n_taps) and h.is_contiguous()
    assert torch.allclose((h * h).sum(dim=1), torch.ones(4, dtype=torch.float64), rtol=0, atol=1e-14)
    H = np.abs(np.fft.rfft(h.numpy(), 1 << 16, axis=1))
    f = np.arange(H.shape[1]) * FS / float(1 << 16)
    band = (f >= 8.0 * FS / n_taps) & (f <= 7000.0)
    for k, slope in enumerate(slopes.tolist()):
        # the law up to the one gain the normalisation applies: the deviation from it, about its median over the band
        dev = 20.0 * np.log10(H[k, band]) - slope * np.log2(f[band] / 1000.0)
        worst = float(np.max(np.abs(dev - np.median(dev))))
        print(f"[noise] {n_taps} taps, {slope:+.0f} dB/oct: worst deviation {worst:.4f} dB")
        assert worst <= 0.25, (n_taps, slope, worst)


def test_power_law_magnitude_and_band():
    m = power_law_magnitude(torch.tensor([-3.0, 0.0]), FS)
    f = np.arange(2049) * FS / 4096.0
    assert tuple(m.shape) == (2, 2049) and m.dtype == torch.float64
    want = (np.maximum(f, 62.5) / 1000.0) ** (-3.0 / (20.0 * math.log10(2.0)))
    assert np.allclose(m[0].numpy(), want, rtol=1e-13) and np.array_equal(m[1].numpy(), np.ones(2049))
    assert m[0, 0] == m[0, 16] and 20.0 * math.log10(m[0, 256] / m[0, 512]) == pytest.approx(3.0, abs=1e-9)    # held below f_lo; 1 and 2 kHz
    assert tuple(power_law_magnitude(-3.0, FS).shape) == (2049,)
    b = power_law_magnitude(torch.zeros(1, dtype=torch.float64), FS, band=(200.0, 4000.0))[0].numpy()
    at = lambda hz: b[int(round(hz * 4096.0 / FS))]
    assert b[0] == 0.0 and at(200.0 * 2 ** -0.25) < 1e-3 and at(200.0) == pytest.approx(0.5, abs=0.02) and at(1000.0) == 1.0
    assert at(4000.0) == pytest.approx(0.5, abs=0.02) and at(4000.0 * 2 ** 0.26) == 0.0 and np.all((b >= 0.0) & (b <= 1.0))
    with pytest.raises(ValueError, match="fs and f_lo must be positive"):
        power_law_magnitude(0.0, 0)
    for bad in (torch.zeros(2049), torch.zeros(2, 2048, dtype=torch.float64), torch.zeros(2, 2049)):
        with pytest.raises(ValueError, match="magnitude must be a float64"):
            noise_fir(bad, 63)
    for bad in (0, 1024, 2.5, True):
        with pytest.raises(ValueError, match="n_taps must be a whole number"):
            noise_fir(torch.ones(1, 2049, dtype=torch.float64), bad)
    assert noise_fir(torch.zeros(1, 2049, dtype=torch.float64), 9).abs().sum() == 0.0      # a silent row stays finite
    assert tuple(noise_fir(torch.ones(2, 2049, dtype=torch.float64), 1).shape) == (2, 1)


# ------------------------------------------------------------------ the sampler
def test_sampler_ranges_and_determinism():
    N, n = 400, 32000
    kw = dict(slope_db=(-6.0, 0.0), band_hz=(100.0, 6000.0), mod_depth_db=(3.0, 9.0), p_hum=0.5, p_clicks=0.5, n_taps=63)
    d = NoiseSampler(generator=_gen(5), **kw).draw(N, n, FS)
    again = NoiseSampler(generator=_gen(5), **kw).draw(N, n, FS)
    other = NoiseSampler(generator=_gen(6), **kw).draw(N, n, FS)
    assert isinstance(d, NoiseDraw) and all(torch.equal(a, b) for a, b in zip(d, again))
    assert not torch.equal(d.seed, other.seed) and not torch.equal(d.fir, other.fir)
    s = NoiseSampler(**kw)
    H, P = s.hop(FS), s.points(n, FS)
    assert H == 320 and P == 2 + (n - 1) // H == 101
    assert d.seed.dtype == torch.int64 and tuple(d.seed.shape) == (N,) and d.seed.unique().numel() == N and int(d.seed.min()) >= 0
    assert d.fir.dtype == torch.float64 and tuple(d.fir.shape) == (N, 63) and d.fir.is_contiguous()
    assert torch.allclose((d.fir ** 2).sum(dim=1), torch.ones(N, dtype=torch.float64), rtol=0, atol=1e-13)
    assert d.env.dtype == torch.float64 and tuple(d.env.shape) == (N, P) and d.env.is_contiguous()
    depth = 20.0 * torch.log10(d.env).abs().amax(dim=1)
    assert float(depth.min()) >= 3.0 - 1e-9 and float(depth.max()) <= 9.0 + 1e-9 and float(depth.max() - depth.min()) > 3.0
    M_ = 5
    assert d.tones.dtype == torch.float64 and tuple(d.tones.shape) == (N, M_, 3) and d.n_tones.dtype == torch.int32
    assert int(d.n_tones.min()) == 0 and int(d.n_tones.max()) == 5 and 0.3 < float((d.n_tones > 0).double().mean()) < 0.7
    nu, amp, phi = d.tones.unbind(dim=2)
    f0 = nu[:, 0] * FS
    assert bool((((f0 - 50.0).abs() < 1e-9) | ((f0 - 60.0).abs() < 1e-9)).all()) and 0.3 < float((f0 < 55.0).double().mean()) < 0.7
    assert torch.allclose(nu, nu[:, :1] * torch.arange(1, 6, dtype=torch.float64)) and float(nu.max()) <= 0.5
    assert torch.allclose(amp[:, 1:] / amp[:, :-1], torch.full((N, 4), 0.5, dtype=torch.float64))
    level = 20.0 * torch.log10(amp[:, 0] / math.sqrt(2.0))
    assert float(level.min()) >= -30.0 - 1e-9 and float(level.max()) <= -10.0 + 1e-9
    assert float(phi.min()) >= 0.0 and float(phi.max()) < 1.0 and bool(torch.isfinite(d.tones).all())
    assert d.impulse.dtype == torch.float64 and tuple(d.impulse.shape) == (N, 2)
    thr, camp = d.impulse.unbind(dim=1)
    on = thr > 0
    assert 0.3 < float(on.double().mean()) < 0.7 and bool((thr == thr.floor()).all()) and float(thr.max()) < 2.0 ** 32
    rate = thr[on] / 2.0 ** 32 * FS
    assert float(rate.min()) >= 1.0 - 1e-3 and float(rate.max()) <= 20.0 + 1e-3
    assert float(camp.min()) >= 10.0 ** 0.5 - 1e-9 and float(camp.max()) <= 10.0 ** 1.5 + 1e-9
    # every row of a draw is one the kernels take
    c = M.case(d.seed.numpy(), 64, d.fir.numpy(), env=d.env.numpy(), H=H, tones=d.tones.numpy(), n_tones=d.n_tones.numpy(),
               imp=d.impulse.numpy())
    assert not any(M.invalid(row, 64, M_) for row in M.rows_of(c))
    # the spectrum: nothing is left at fs / 2, beyond the band's upper edge (63 taps cannot resolve the lower one)
    Hf = np.abs(np.fft.rfft(d.fir.numpy(), 4096, axis=1))
    assert np.all(Hf[:, -1] < 0.05 * Hf.max(axis=1))
    # hum above Nyquist is dropped; without hum and clicks the tables are None
    low = NoiseSampler(generator=_gen(1), p_hum=1.0, hum_hz=(300.0,), hum_harmonics=(8, 8)).draw(4, 100, 1000)
    assert low.n_tones.tolist() == [1] * 4 and tuple(low.tones.shape) == (4, 8, 3) and float(low.tones[..., 0].max()) <= 0.5
    bare = NoiseSampler(generator=_gen(1), p_hum=0.0, p_clicks=0.0).draw(3, 1, FS)
    assert bare.tones is None and bare.n_tones is None and bare.impulse is None and tuple(bare.env.shape) == (3, 2)


def test_sampler_rejects_bad_options():
    bad = [
        (dict(slope_db=3), "slope_db must be \\(low, high\\)"), (dict(slope_db=(1, 0)), "slope_db must be"),
        (dict(slope_db=(-math.inf, 0)), "slope_db must be"), (dict(band_hz=(0, 100)), "band_hz must be"),
        (dict(band_hz=5), "band_hz must be None or \\(low, high\\)"), (dict(mod_depth_db=(-1, 3)), "mod_depth_db must be"),
        (dict(mod_depth_db=(0, math.inf)), "mod_depth_db must be"), (dict(mod_rate_hz=(0, 1)), "mod_rate_hz must be"),
        (dict(p_hum=1.5), "p_hum must lie in \\[0, 1\\]"), (dict(p_clicks=-0.1), "p_clicks must lie in \\[0, 1\\]"),
        (dict(hum_hz=()), "hum_hz must be one or more"), (dict(hum_hz=(50, -1)), "hum_hz must be"), (dict(hum_hz=50), "hum_hz must be"),
        (dict(hum_db=(0, -10)), "hum_db must be"), (dict(hum_harmonics=(0, 3)), "hum_harmonics must be"),
        (dict(hum_harmonics=(1, 9)), "hum_harmonics must be"), (dict(hum_harmonics=(1.0, 2.0)), "hum_harmonics must be"),
        (dict(click_rate_hz=(0, 1)), "click_rate_hz must be"), (dict(click_db=(3, 1)), "click_db must be"),
        (dict(n_taps=0), "n_taps must be a whole number"), (dict(n_taps=1024), "n_taps must be"), (dict(n_taps=True), "n_taps must be"),
        (dict(env_hop_ms=0), "env_hop_ms must be"), (dict(env_hop_ms="20"), "env_hop_ms must be"),
    ]
    for kw, text in bad:
        with pytest.raises(ValueError, match=text):
            NoiseSampler(**kw)
    with pytest.raises(ValueError, match="need 4098 points"):
        NoiseSampler().draw(1, 4096 * 320 + 1, FS)
    with pytest.raises(ValueError, match="band_hz = .* must lie at or below fs / 2"):
        NoiseSampler(band_hz=(100, 5000)).draw(1, 10, 8000)


def test_bank_and_mixer_reject_bad_options():
    bank = NoiseBank.from_arrays([np.ones(9, np.float32)])
    with pytest.raises(TypeError, match="sampler must be a NoiseSampler"):
        NoiseBank.synthesize(_NoEngine(), "pink", 4, 1.0)
    for items in (0, 65536, 2.5, True):
        with pytest.raises(ValueError, match="items must be a whole number"):
            NoiseBank.synthesize(_NoEngine(), NoiseSampler(), items, 1.0)
    with pytest.raises(ValueError, match="seconds must give at least one sample"):
        NoiseBank.synthesize(_NoEngine(), NoiseSampler(), 4, 0.0)
    with pytest.raises(ValueError, match="out must be a contiguous float32 \\[4, 16000\\]"):
        NoiseBank.synthesize(_NoEngine(), NoiseSampler(), 4, 1.0, out=torch.zeros(4, 15999))
    assert bank.draw is None
    with pytest.raises(TypeError, match="noise must be a NoiseSampler or None"):
        DynamicMixer(_NoEngine(), bank, noise="pink")
    with pytest.raises(ValueError, match="either a noise_bank or noise=NoiseSampler"):
        DynamicMixer(_NoEngine(), bank, noise=NoiseSampler())
    with pytest.raises(ValueError, match="the mixer needs noise"):
        DynamicMixer(_NoEngine(), None)
    # judged after every other option: an earlier error is what it was
    with pytest.raises(ValueError, match="dynamics_on must be"):
        DynamicMixer(_NoEngine(), None, dynamics_on="x")
    with pytest.raises(ValueError, match="snr_db must be"):
        DynamicMixer(_NoEngine(), bank, noise=NoiseSampler(), snr_db=(5, 1))
    m = DynamicMixer(_NoEngine(), None, noise=NoiseSampler(), sources=(0, 2))
    assert m.noise_bank is None and m.source_bank is None and m.last_noise is None
    plain = DynamicMixer(_NoEngine(), bank)
    assert plain.noise is None and plain.noise_bank is bank and plain.last_noise is None
    # noise=None draws nothing: the draws and the generator's state are those of a mixer built without the argument
    g0, g1 = _gen(7), _gen(7)
    d0 = DynamicMixer(_NoEngine(), bank, generator=g0, level_db=(-35, -15)).draw(6)
    d1 = DynamicMixer(_NoEngine(), bank, generator=g1, level_db=(-35, -15), noise=None).draw(6)
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(d0, d1)) and torch.equal(g0.get_state(), g1.get_state())


# ------------------------------------------------------------------ the library without a GPU
def test_symbols_limits_and_abi():
    lib = _lib.load()
    for name in ("cmgan_noise", "cmgan_noise_workspace_bytes", "cmgan_noise_tile", "cmgan_noise_max_filter", "cmgan_noise_max_tones",
                 "cmgan_noise_max_points"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.cmgan_noise_tile() == NOISE_TILE == M.TILE == 256
    assert lib.cmgan_noise_max_filter() == NOISE_MAX_FILTER == M.MAX_FILTER == 1023
    assert lib.cmgan_noise_max_tones() == NOISE_MAX_TONES == M.MAX_TONES == 8
    assert lib.cmgan_noise_max_points() == NOISE_MAX_POINTS == M.MAX_POINTS == 4096
    assert lib.cmgan_abi_version() == _lib.ABI_VERSION >= 21


def test_workspace_formula():
    lib = _lib.load()
    ws = lambda N: int(lib.cmgan_noise_workspace_bytes(N))
    for N in (1, 2, 63, 64, 65, 32, 4096, 65535):
        assert ws(N) == noise_workspace_bytes(N) == ((4 * N + 255) & ~255) > 0
    assert ws(64) == 256 and ws(65) == 512
    for N in (0, -1, 65536):
        assert ws(N) == noise_workspace_bytes(N) == 0


def test_library_rejects_bad_arguments_before_it_needs_a_handle():
    lib = _lib.load()
    out = np.zeros(4096, dtype=np.float32)
    seed, start = np.zeros(9, dtype=np.int64), np.zeros(9, dtype=np.int64)
    length, n_tones, status = np.zeros(9, dtype=np.int32), np.zeros(9, dtype=np.int32), np.full(9, 7, dtype=np.int32)
    fir, env, tones, imp = (np.zeros(8 * 64 + 1, dtype=np.float64) for _ in range(4))
    raw = np.zeros(4096, dtype=np.uint8)
    base = (raw.ctypes.data + 255) & ~255
    po, ps, pa, pl, pn, pt, pf, pe, pq, pi = (a.ctypes.data for a in (out, seed, start, length, n_tones, status, fir, env, tones, imp))

    def call(out=po, N=2, K=1500, ld=1500, seed=ps, start=pa, length=pl, fir=pf, NF=9, env=pe, P=4, H=100, tones=pq, n_tones=pn,
             M=2, imp=pi, status=pt, ws=base, ws_bytes=256):
        rc = lib.cmgan_noise(None, out, N, K, ld, seed, start, length, fir, NF, env, P, H, tones, n_tones, M, imp, status, ws,
                             ws_bytes, None)
        return rc, (lib.cmgan_last_error(None) or b"").decode()

    cases = {
        "null pointer": [dict(out=None), dict(seed=None), dict(fir=None), dict(status=None)],
        "4-byte aligned": [dict(out=po + 2), dict(length=pl + 1), dict(n_tones=pn + 2), dict(status=pt + 3)],
        "8-byte aligned": [dict(seed=ps + 4), dict(start=pa + 4), dict(fir=pf + 4), dict(env=pe + 4), dict(tones=pq + 4), dict(imp=pi + 4)],
        "need 1 <= N": [dict(N=0), dict(N=-3), dict(N=65536), dict(K=-1), dict(ld=1499), dict(K=NOISE_MAX_N + 1, ld=2 ** 31 - 1)],
        "filter taps": [dict(NF=0), dict(NF=-1), dict(NF=1024)],
        "an envelope needs": [dict(P=0), dict(P=4097), dict(H=0), dict(H=-5), dict(env=None), dict(env=None, P=0), dict(env=None, H=0)],
        "tones": [dict(M=-1), dict(M=9), dict(M=0), dict(tones=None), dict(tones=None, M=0), dict(tones=None, n_tones=None)],
        "workspace": [dict(ws=None), dict(ws=base + 64), dict(ws_bytes=255), dict(ws_bytes=0), dict(N=65, ws_bytes=256)],
    }
    for text, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == BADARG and text in msg, (kw, rc, msg)
    # everything in order: only the handle is missing - nothing was enqueued, nothing was written
    for kw in (dict(), dict(start=None), dict(length=None), dict(env=None, P=0, H=0), dict(tones=None, n_tones=None, M=0),
               dict(n_tones=None), dict(imp=None), dict(K=0, out=None, ld=0), dict(ld=2000), dict(NF=1023), dict(P=4096, H=2 ** 31 - 1),
               dict(M=8), dict(N=1, K=1, ld=1)):
        rc, msg = call(**kw)
        assert rc == BADARG and "null handle" in msg, (kw, rc, msg)
    assert not out.any() and (status == 7).all()


# ------------------------------------------------------------------ Engine.noise's argument rules
def test_check_noise_args():
    i64, i32 = (lambda n=3: torch.zeros(n, dtype=torch.int64)), (lambda n=3: torch.zeros(n, dtype=torch.int32))
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)
    seed, fir = i64(), f64(3, 9)
    assert check_noise_args(CPU, seed, fir, 2000) == (3, 2000, 9, 0, 0, 0)
    assert check_noise_args(CPU, seed, fir, 0) == (3, 0, 9, 0, 0, 0)
    full = dict(lengths=i32(), start=i64(), env=f64(3, 5), env_hop=320, tones=f64(3, 8, 3), n_tones=i32(), impulse=f64(3, 2))
    assert check_noise_args(CPU, seed, fir, 2000, out=torch.zeros(3, 2000), **full) == (3, 2000, 9, 5, 320, 8)
    assert check_noise_args(CPU, seed, fir, 2000, out=torch.zeros(3, 2500)[:, :2000]) == (3, 2000, 9, 0, 0, 0)
    assert check_noise_args(CPU, seed, fir, 0, out=torch.zeros(3, 0)) == (3, 0, 9, 0, 0, 0)
    assert check_noise_args(CPU, seed, fir, 5, tones=f64(3, 0, 3)) == (3, 5, 9, 0, 0, 0)
    assert check_noise_args(CPU, i64(1), f64(1, 1023), NOISE_MAX_N, env=f64(1, 4096), env_hop=2 ** 31 - 1) == (1, NOISE_MAX_N, 1023, 4096,
                                                                                                                2 ** 31 - 1, 0)

    def bad(kind, text, **kw):
        args = dict(seed=seed, fir=fir, n=2000)
        args.update(kw)
        with pytest.raises(kind, match=text):
            check_noise_args(CPU, args.pop("seed"), args.pop("fir"), args.pop("n"), **args)

    bad(TypeError, "seed: expected a torch.Tensor", seed=np.zeros(3, dtype=np.int64))
    bad(TypeError, "seed: expected int64", seed=i32())
    with pytest.raises(RuntimeError, match="seed: tensor is on cpu"):
        check_noise_args(torch.device("cuda:0"), seed, fir, 2000)
    for t in (i64(0), torch.zeros(3, 1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64).expand(65536)):
        bad(ValueError, "seed: expected \\[N\\] with 1 <= N <= 65535", seed=t)
    bad(ValueError, "seed: must be contiguous", seed=i64(6)[::2])
    bad(TypeError, "fir: expected float64", fir=fir.float())
    for t in (f64(2, 9), f64(3, 0), f64(3, 1024), f64(27), f64(3, 9, 1)):
        bad(ValueError, "fir: expected \\[3, NF\\] with 1 <= NF <= 1023", fir=t)
    bad(ValueError, "fir: must be contiguous", fir=f64(3, 18)[:, ::2])
    for n in (-1, NOISE_MAX_N + 1, 2.5, True):
        bad(ValueError, "n must be a length in", n=n)
    bad(TypeError, "lengths: expected int32", lengths=i64())
    bad(ValueError, "lengths: expected \\[3\\]", lengths=i32(4))
    bad(ValueError, "lengths: must be contiguous", lengths=i32(6)[::2])
    bad(TypeError, "start: expected int64", start=i32())
    bad(ValueError, "start: expected \\[3\\]", start=i64(2))
    bad(TypeError, "env: expected float64", env=torch.zeros(3, 5), env_hop=10)
    for t in (f64(3, 0), f64(3, 4097), f64(2, 5), f64(15)):
        bad(ValueError, "env: expected \\[3, P\\] with 1 <= P <= 4096", env=t, env_hop=10)
    for hop in (None, 0, -3, 2.5, True, 2 ** 31):
        bad(ValueError, "env_hop must be the samples between two points", env=f64(3, 5), env_hop=hop)
    bad(ValueError, "env_hop given without env", env_hop=10)
    bad(TypeError, "tones: expected float64", tones=torch.zeros(3, 2, 3))
    for t in (f64(3, 9, 3), f64(3, 2, 2), f64(2, 2, 3), f64(3, 6)):
        bad(ValueError, "tones: expected \\[3, M, 3\\] with 0 <= M <= 8", tones=t)
    bad(ValueError, "tones: must be contiguous", tones=f64(3, 2, 6)[:, :, ::2])
    bad(TypeError, "n_tones: expected int32", tones=f64(3, 2, 3), n_tones=i64())
    bad(ValueError, "n_tones: expected \\[3\\]", tones=f64(3, 2, 3), n_tones=i32(1))
    bad(ValueError, "n_tones given without tones", n_tones=i32())
    bad(TypeError, "impulse: expected float64", impulse=torch.zeros(3, 2))
    for t in (f64(3, 3), f64(2, 2), f64(6)):
        bad(ValueError, "impulse: expected \\[3, 2\\]", impulse=t)
    bad(TypeError, "out: expected float32", out=f64(3, 2000))
    bad(ValueError, "out: expected \\[3, 2000\\]", out=torch.zeros(3, 2001))
    for t in (torch.zeros(3, 4000)[:, ::2], torch.zeros(2000, 3).t(), torch.zeros(1, 2000).expand(3, 2000)):
        bad(ValueError, "out: rows must be contiguous", out=t)
