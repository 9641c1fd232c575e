"""CPU side of the banded room simulator (cmgan_amd/csrc/rir.hip; include/cmgan_hip.h, "Room impulse responses in
frequency bands"): the float64 model the GPU tests compare the kernels with (tests/rir_bands_model.py) against its own
definition as a naive loop and against known answers, the octave filterbank, RoomSampler's band draws, the workspace
formula, and every argument error of cmgan_rir_bands and Engine.rir_bands, all judged before a handle or a GPU is needed."""
import math

import numpy as np
import pytest
import torch

import rir_bands_model as BM
import rir_model as M
from cmgan_amd import _lib
from cmgan_amd.engine import RIR_MAX_BANDS, RIR_MAX_FILTER, check_rir_bands_args
from cmgan_amd.mixing import Draw, DynamicMixer, NoiseBank, RirBank, RoomSampler, SceneDraw, octave_filterbank

BADARG, UNSUPPORTED = -1, -3
FS, C = 16000, 343.0


# ------------------------------------------------------------------ the model
def _naive(room, bands, n_taps, K, N, filt, fs, c, tw):
    NB, NF = filt.shape
    D = (NF - 1) // 2
    L, s, m = room[0:3], room[3:6], room[6:9]
    kr = min(max(n_taps, 1), K)
    hb = np.zeros((NB, K + D))
    for b in range(NB):
        beta, air = bands[b][0:6], bands[b][6]
        for nx in range(-N[0], N[0] + 1):
            for ny in range(-N[1], N[1] + 1):
                for nz in range(-N[2], N[2] + 1):
                    n = (nx, ny, nz)
                    for p in np.ndindex(2, 2, 2):
                        off = [(1 - 2 * p[i]) * s[i] + 2 * n[i] * L[i] - m[i] for i in range(3)]
                        d = math.sqrt(sum(o * o for o in off))
                        tau = d * fs / c
                        a = math.exp(-air * d) / (4 * math.pi * max(d, M.DMIN))
                        for i in range(3):
                            a *= beta[2 * i] ** abs(n[i] - p[i]) * beta[2 * i + 1] ** abs(n[i])
                        for q in range(kr + D):
                            t = q - tau
                            if abs(t) < tw:
                                sinc = 1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)
                                hb[b, q] += a * 0.5 * (1 + math.cos(math.pi * t / tw)) * sinc
    h = np.zeros(K)
    for k in range(kr):
        for b in range(NB):
            for j in range(NF):
                q = k + D - j
                if 0 <= q < kr + D:
                    h[k] += filt[b, j] * hb[b, q]
    return h, hb, kr


@pytest.mark.parametrize("N,n_taps,tw,NB,NF", [((1, 1, 1), 40, 5, 2, 5), ((1, 0, 1), 23, 3, 3, 1), ((0, 1, 0), 64, 8, 1, 7)])
def test_model_is_the_defining_loop(N, n_taps, tw, NB, NF):
    room = np.array([1.1, 0.9, 1.3, 0.3, 0.5, 0.4, 0.8, 0.2, 0.9, np.nan, np.nan, 7.0, -1.0, np.inf, 0.0])   # 9 - 14: never read
    rng = np.random.default_rng(NB * 10 + NF)
    bands = np.concatenate([rng.uniform(0.0, 1.0, (NB, 6)), rng.uniform(0.0, 0.2, (NB, 1))], axis=1)
    bands[0, 1] = 0.0                                            # an absorbing wall: 0^0 = 1 keeps the images that miss it
    filt = rng.standard_normal((NB, NF))
    K = 48
    h, bound, hb, Ab, kr = BM.rir_bands_row(room, bands, n_taps, K, N, filt, 8000, C, tw)
    hn, hbn, krn = _naive(room, bands, n_taps, K, N, filt, 8000, C, tw)
    assert kr == krn == min(n_taps, K)
    assert np.max(np.abs(hn)) > 0.01 and np.max(np.abs(hbn)) > 0.01
    assert np.allclose(hb, hbn, rtol=0, atol=1e-15 * np.max(Ab))
    assert np.allclose(h, hn, rtol=0, atol=1e-14 * np.max(Ab) * np.sum(np.abs(filt)))
    assert np.all(h[kr:] == 0.0) and np.all(bound[kr:] == 0.0) and np.all(hb[:, kr + (NF - 1) // 2:] == 0.0)
    assert np.all(bound >= 0.0) and np.all(bound[h != 0.0] > 0.0)


def test_model_anechoic_known_answer():
    """All coefficients are 0: only the direct image survives (0^0 = 1), 3.43 m = exactly 160 samples away, and band b is
    exp(-m_b d) / (4 pi d) times the windowed sinc - one tap."""
    room = [4, 5, 3, 0.5, 1, 1, 3.93, 1, 1] + [0.5] * 6
    m = np.array([0.0, 0.01, 0.3])
    bands = np.concatenate([np.zeros((3, 6)), m[:, None]], axis=1)
    filt = np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, -1.0]])      # D = 1: band b arrives at 160 + (j_b - 1)
    h, bound, hb, Ab, kr = BM.rir_bands_row(room, bands, 400, 400, (1, 1, 1), filt, FS, C, 40)
    assert kr == 400
    want = np.exp(-m * 3.43) / (4 * np.pi * 3.43)
    assert np.all(np.abs(hb[:, 160] / want - 1.0) <= 1e-15)
    assert np.max(np.abs(np.delete(hb, 160, axis=1))) < 1e-17
    assert np.all(np.abs(Ab[:, 160] / want - 1.0) <= 1e-15) and np.all(Ab[:, 160 + 40] == 0.0) and np.all(Ab[:, 160 + 39] > 0.0)
    assert abs(h[159] / want[0] - 1.0) <= 1e-14 and abs(h[160] / (2 * want[1]) - 1.0) <= 1e-14
    assert abs(h[161] / -want[2] - 1.0) <= 1e-14
    assert np.max(np.abs(np.delete(h, [159, 160, 161]))) < 1e-16


def test_flat_walls_without_air_are_the_single_band_model():
    """The same coefficients in every band, m = 0, octave_filterbank: the bank sums to a pure delay, which the join takes
    out, so the result is rir_model.rir_row's."""
    room = np.array([2.5, 2.0, 2.2, 0.7, 0.9, 1.1, 1.9, 0.6, 1.4, 0.9, 0.8, 0.85, 0.7, 0.6, 0.95])
    K, N, NB, NF = 300, (3, 3, 3), 5, 63
    filt = octave_filterbank(FS, NB, NF).numpy()
    bands = np.tile(np.concatenate([room[9:15], [0.0]]), (NB, 1))
    for n_taps in (K, 170):
        h, bound, hb, _, kr = BM.rir_bands_row(room, bands, n_taps, K, N, filt, FS, C, 40)
        want, _, kr1 = M.rir_row(room, n_taps, K, N, FS, C, 40)
        assert kr == kr1 == n_taps and np.max(np.abs(want)) > 0.01
        assert np.all(np.abs(h - want) <= bound)
        assert np.all(h[kr:] == 0.0)


def test_model_invalid_rows_and_length_clamp():
    good = np.array([2.5, 2.0, 2.2, 0.7, 0.9, 1.1, 1.9, 0.6, 1.4] + [np.nan] * 6)
    bands = np.array([[0.9, 0.8, 0.85, 0.7, 0.6, 0.95, 0.0], [0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.02]])
    filt = np.array([[1.0], [0.5]])
    args = (64, (1, 1, 1), filt)
    assert BM.rir_bands_row(good, bands, 50, *args)[4] == 50
    for at, v in [(0, np.nan), (4, np.inf), (1, -2.0), (2, 0.0)]:
        room = good.copy()
        room[at] = v
        h, bound, hb, Ab, kr = BM.rir_bands_row(room, bands, 50, *args)
        assert kr == 1 and not h.any() and not hb.any() and not bound.any()
    for at, v in [((0, 2), 1.5), ((1, 5), -0.1), ((1, 6), -1e-9), ((0, 6), np.nan), ((1, 0), np.inf)]:
        bad = bands.copy()
        bad[at] = v
        h, _, hb, _, kr = BM.rir_bands_row(good, bad, 50, *args)
        assert kr == 1 and not h.any() and not hb.any()
    assert BM.rir_bands_row(good, bands, 0, *args)[4] == 1 and BM.rir_bands_row(good, bands, 1000, *args)[4] == 64
    hs, bs, ls = BM.rir_bands(np.stack([good, good]), np.stack([bands, bands]), [64, 10], *args)
    assert hs.shape == bs.shape == (2, 64) and ls.dtype == np.int32 and ls.tolist() == [64, 10]


# ------------------------------------------------------------------ the filterbank
@pytest.mark.parametrize("fs,NB,NF", [(16000, 7, 511), (16000, 1, 1), (16000, 3, 9), (8000, 6, 255), (48000, 8, 1023), (16000, 2, 1)])
def test_filterbank_sums_to_a_pure_delay(fs, NB, NF):
    g = octave_filterbank(fs, NB, NF)
    assert isinstance(g, torch.Tensor) and g.dtype == torch.float64 and tuple(g.shape) == (NB, NF) and g.device.type == "cpu"
    assert bool(torch.isfinite(g).all())
    total = g.numpy().sum(axis=0)
    delta = np.zeros(NF)
    delta[(NF - 1) // 2] = 1.0
    assert np.max(np.abs(total - delta)) <= NB * 2.0 ** -52
    if NB == 1:
        assert np.array_equal(g.numpy()[0], delta)
    assert torch.equal(g, octave_filterbank(fs, NB, NF))


def test_filterbank_separates_the_octaves_at_16_khz():
    """7 bands of 511 taps at 16 kHz: a sinusoid at a band's centre passes its own band with gain >= 0.9 and any band two
    or more away with gain <= 0.01."""
    NB, NF = 7, 511
    g = octave_filterbank(16000, NB, NF).numpy()
    j = np.arange(NF)
    gain = np.array([[abs(np.sum(g[b] * np.exp(-2j * np.pi * 125.0 * 2 ** i / 16000 * j))) for b in range(NB)] for i in range(NB)])
    print("[rir_bands] gain of band b (column) at centre i (row):\n", np.array_str(gain, precision=4, suppress_small=True))
    for i in range(NB):
        assert gain[i, i] >= 0.9, (i, gain[i, i])
        for b in range(NB):
            if abs(b - i) >= 2:
                assert gain[i, b] <= 0.01, (i, b, gain[i, b])


def test_filterbank_argument_rules():
    for kw in (dict(n_bands=0), dict(n_bands=9), dict(n_bands=2.5), dict(n_bands=True), dict(n_taps=510), dict(n_taps=0),
               dict(n_taps=1025), dict(n_taps=7.5), dict(f0=0.0), dict(f0=float("nan"))):
        with pytest.raises(ValueError, match="n_bands|n_taps|f0"):
            octave_filterbank(16000, **kw)
    with pytest.raises(ValueError, match="fs"):
        octave_filterbank(0)
    with pytest.raises(ValueError, match="second-highest"):      # 125 * 2^6 = 8000 is not below 16000 / 2
        octave_filterbank(16000, n_bands=8)
    octave_filterbank(16000, n_bands=7)
    with pytest.raises(ValueError, match="second-highest"):
        octave_filterbank(8000, n_bands=7)
    octave_filterbank(16000.0, n_bands=2, n_taps=3, f0=7999.0)


# ------------------------------------------------------------------ the sampler
def _gen(seed=7):
    return torch.Generator().manual_seed(seed)


def test_sampler_without_bands_draws_exactly_what_it_drew():
    """bands=None: the sampler's draws are one rand(R, 10) and one rand(R, n, 3), the arithmetic of draw and draw_sources
    written out here; a banded sampler makes the same two draws and only then its own."""
    lo, hi, margin, R, K = (3.0, 3.0, 2.5), (10.0, 8.0, 4.0), 0.5, 9, 8000
    g = _gen()
    u = torch.rand(R, 10, dtype=torch.float64, generator=g)
    size = torch.tensor(lo, dtype=torch.float64) + (torch.tensor(hi, dtype=torch.float64) - torch.tensor(lo, dtype=torch.float64)) * u[:, 0:3]
    inner = size - 2.0 * margin
    rt = 0.2 + (0.8 - 0.2) * u[:, 9]
    V, S = size.prod(1), 2.0 * (size[:, 0] * size[:, 1] + size[:, 1] * size[:, 2] + size[:, 0] * size[:, 2])
    beta = torch.sqrt(1.0 - (0.161 * (size[:, 0] * size[:, 1] * size[:, 2]) / (S * rt)).clamp(0.0, 1.0))
    want = torch.cat([size, margin + inner * u[:, 3:6], margin + inner * u[:, 6:9], beta[:, None].expand(R, 6)], dim=1)
    us = torch.rand(R, 2, 3, dtype=torch.float64, generator=g)
    for kw in (dict(), dict(bands=None), dict(bands=5, tilt=(0.1, 0.4), air=[(0.0, 0.01)] * 5)):
        gen = _gen()
        s = RoomSampler(generator=gen, **kw)
        rooms, n_taps = s.draw(R, K, FS)
        assert torch.equal(rooms, want) and torch.equal(n_taps, torch.ceil(rt * FS).clamp(1, K).to(torch.int32))
        src = s.draw_sources(rooms, 2)
        assert torch.equal(src[:, :, 3:6], margin + inner[:, None, :] * us)
        assert torch.equal(gen.get_state(), g.get_state())
    plain = RoomSampler()
    assert plain.bands is None and plain.n_images(K, FS) == (30, 30, 36)
    with pytest.raises(ValueError, match="no bands"):
        plain.draw_bands(want)
    with pytest.raises(ValueError, match="no bands"):
        plain.filters(FS)


def test_draw_bands_shapes_determinism_and_the_reference_band():
    R, K = 40, 4000
    s = RoomSampler(generator=_gen(3), bands=7, tilt=(-0.3, 0.6), air=[(0.001 * b, 0.002 * b) for b in range(7)])
    assert s.band_ref == 3                                        # 125 * 2^3 = 1000 Hz
    rooms, _ = s.draw(R, K, FS)
    bands = s.draw_bands(rooms)
    assert tuple(bands.shape) == (R, 7, 7) and bands.dtype == torch.float64 and bands.is_contiguous() and bands.device == rooms.device
    beta, walls, m = rooms[:, 9:15], bands[:, :, 0:6], bands[:, :, 6]
    assert torch.equal(walls[:, 3], beta)                         # the band nearest 1 kHz is the room `draw` made, bit for bit
    assert bool(((walls >= 0) & (walls <= 1)).all()) and bool((walls == walls[:, :, :1]).all())
    for b in range(7):
        assert bool(((m[:, b] >= 0.001 * b) & (m[:, b] <= 0.002 * b)).all())
    assert float(m[:, 0].abs().max()) == 0.0 and float(m[:, 6].std()) > 0.0
    # alpha_b = alpha 2^(tilt (b - 3)) with ONE tilt per room in the range: recovered from two bands, it predicts the others
    alpha = 1.0 - walls[:, :, 0] ** 2
    tilt = torch.log2(alpha[:, 4] / alpha[:, 3])
    assert bool(((tilt > -0.3 - 1e-9) & (tilt < 0.6 + 1e-9)).all()) and float(tilt.std()) > 0.05
    for b in range(7):
        want = (alpha[:, 3] * torch.exp2(tilt * (b - 3))).clamp(0.0, 1.0)
        assert torch.allclose(alpha[:, b], want, rtol=1e-9, atol=1e-12)
    assert all(BM.row_is_valid(r, t) for r, t in zip(rooms.numpy(), bands.numpy()))
    # the same seed gives the same table, the next draw another
    s2 = RoomSampler(generator=_gen(3), bands=7, tilt=(-0.3, 0.6), air=[(0.001 * b, 0.002 * b) for b in range(7)])
    r2, _ = s2.draw(R, K, FS)
    assert torch.equal(s2.draw_bands(r2), bands) and not torch.equal(s2.draw_bands(r2), bands)
    # tilt = 0: the table's beta in every band, bit for bit; no air: m = 0
    flat = RoomSampler(generator=_gen(4), bands=4)
    assert flat.tilt == (0.0, 0.0) and flat.air is None and flat.band_ref == 3
    fb = flat.draw_bands(rooms)
    assert tuple(fb.shape) == (R, 4, 7) and torch.equal(fb[:, :, 0:6], beta[:, None, :].expand(R, 4, 6)) and not fb[:, :, 6].any()
    assert RoomSampler(bands=2).band_ref == 1 and RoomSampler(bands=1).band_ref == 0
    # a steep tilt saturates at a dead wall, never past it
    steep = RoomSampler(generator=_gen(5), bands=7, tilt=(3.0, 3.0)).draw_bands(rooms)
    assert float(steep[:, 6, 0].min()) == 0.0 and bool(torch.isfinite(steep).all())


def test_banded_sampler_image_ranges_filters_and_argument_rules():
    s = RoomSampler(dims=((3.0, 4.0, 2.5), (10.0, 8.0, 4.0)), bands=7, filter_taps=511)
    K, tw = 8000, 40
    reach = (K + 255 + tw) * 343.0 / 16000                        # the bands are simulated D = 255 taps past the row's end
    assert s.n_images(K, 16000) == tuple(math.ceil(reach / (2 * l)) + 1 for l in (3.0, 4.0, 2.5))
    assert s.n_images(K, 16000) != RoomSampler(dims=((3.0, 4.0, 2.5), (10.0, 8.0, 4.0))).n_images(K, 16000)
    f = s.filters(16000)
    assert torch.equal(f, octave_filterbank(16000, 7, 511)) and s.filters(16000) is f
    for kw, text in [(dict(bands=0), "bands"), (dict(bands=9), "bands"), (dict(bands=2.5), "bands"), (dict(bands=True), "bands"),
                     (dict(bands=3, filter_taps=510), "filter_taps"), (dict(bands=3, filter_taps=1025), "filter_taps"),
                     (dict(bands=3, tilt=(0.5, 0.1)), "tilt"), (dict(bands=3, tilt=(0.0, math.inf)), "tilt"),
                     (dict(bands=3, tilt=0.5), "tilt"),
                     (dict(bands=3, air=[(0.0, 0.1)] * 2), "air"), (dict(bands=3, air=[(0.1, 0.0)] * 3), "air"),
                     (dict(bands=3, air=[(-0.1, 0.0)] * 3), "air"), (dict(bands=3, air=0.1), "air"),
                     (dict(tilt=(0.1, 0.2)), "bands=n"), (dict(air=[(0.0, 0.1)]), "bands=n")]:
        with pytest.raises(ValueError, match=text):
            RoomSampler(**kw)
    with pytest.raises(ValueError, match=r"\[R, 15\]"):
        s.draw_bands(torch.ones(3, 15))
    with pytest.raises(ValueError, match=r"\[R, 15\]"):
        s.draw_bands(torch.ones(3, 14, dtype=torch.float64))


class _NoEngine:
    device = torch.device("cpu")


def test_dynamic_mixer_draws_bands_after_every_other_draw():
    noise = NoiseBank.from_arrays([np.ones(n, dtype=np.float32) for n in (10, 300)])
    fields = ("noise_start", "noise_len", "noise_off", "snr_db", "rir_index", "rir_len", "rooms", "level_db", "channel", "speed")
    assert Draw._fields == fields and SceneDraw._fields[:10] == fields
    for extra in (dict(), dict(sources=(0, 2))):
        draws = []
        for kw in (dict(), dict(bands=3, tilt=(0.0, 0.5), filter_taps=511)):
            m = DynamicMixer(_NoEngine(), noise, rooms=RoomSampler(generator=_gen(11), **kw), rir_seconds=0.1, p_reverb=0.5,
                             generator=_gen(12), **extra)
            d = m.draw(6)
            draws.append((m, d, m.draw_bands(d)))
        (m0, d0, b0), (m1, d1, b1) = draws
        assert type(d0) is type(d1) and b0 is None and tuple(b1.shape) == (6, 3, 7)
        for name in d0._fields:
            x, y = getattr(d0, name), getattr(d1, name)
            assert (x is None and y is None) or torch.equal(x, y), name
        assert m1.n_images == m1.rooms.n_images(1600, 16000) and m1.n_images > m0.n_images
        assert m0.last_bands is None and m1.last_bands is None     # (set by a call, not by draw)
        assert torch.equal(m0.generator.get_state(), m1.generator.get_state())
    assert DynamicMixer(_NoEngine(), noise).draw_bands(DynamicMixer(_NoEngine(), noise).draw(2)) is None
    assert RirBank.from_arrays([[1.0, 0.5]]).bands is None


# ------------------------------------------------------------------ the library
def test_exported_symbols_and_constants():
    lib = _lib.load()
    for name in ("cmgan_rir_bands", "cmgan_rir_bands_workspace_bytes", "cmgan_rir_max_bands", "cmgan_rir_max_filter"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.cmgan_rir_max_bands() == RIR_MAX_BANDS == 8 and lib.cmgan_rir_max_filter() == RIR_MAX_FILTER == 1023
    assert lib.cmgan_abi_version() == _lib.ABI_VERSION >= 15


def test_workspace_bytes_monotone_and_rejects_unsupported_shapes():
    lib = _lib.load()
    ws = lambda R=4, K=8000, tw=40, NB=7, NF=511: int(lib.cmgan_rir_bands_workspace_bytes(None, R, K, tw, NB, NF))
    base = ws(1, 1, 1, 1, 1)
    assert base > 0 and base % 256 == 0
    for name, values in (("R", (1, 2, 5, 32, 65535)), ("K", (1, 2, 255, 256, 257, 8000, 65536)), ("tw", (1, 4, 40, 64)),
                         ("NB", (1, 2, 3, 7, 8)), ("NF", (1, 3, 9, 511, 1023))):
        prev = 0
        for v in values:
            got = ws(**{name: v})
            assert got >= max(prev, 1) and got % 256 == 0, (name, v)
            prev = got
    # it holds at least the float64 band responses [R, NB, K + D]
    assert ws(32, 8000, 40, 7, 511) >= 32 * 7 * (8000 + 255) * 8
    for kw in (dict(R=0), dict(R=-1), dict(R=65536), dict(K=0), dict(K=-5), dict(K=65537), dict(tw=0), dict(tw=-1), dict(tw=65),
               dict(NB=0), dict(NB=-2), dict(NB=9), dict(NF=0), dict(NF=-1), dict(NF=2), dict(NF=510), dict(NF=1024), dict(NF=1025)):
        assert ws(**kw) == 0, kw


ORDER = ("h", "rooms", "bands", "n_taps", "R", "K", "NB", "filt", "NF", "fs", "c", "tw", "Nx", "Ny", "Nz", "rir", "ld", "len",
         "ws", "ws_bytes", "stream")


def _call(**over):
    """cmgan_rir_bands with plausible, aligned, never-dereferenced pointers: every error is raised before any is followed."""
    p = 0x10000
    a = dict(h=None, rooms=p, bands=p, n_taps=p, R=2, K=100, NB=3, filt=p, NF=9, fs=16000, c=343.0, tw=40, Nx=3, Ny=3, Nz=3,
             rir=p, ld=100, len=p, ws=p, ws_bytes=1 << 30, stream=None)
    a.update(over)
    lib = _lib.load()
    rc = lib.cmgan_rir_bands(*[a[k] for k in ORDER])
    return rc, lib.cmgan_last_error(None).decode()


@pytest.mark.parametrize("over,code,text", [
    (dict(rooms=None), BADARG, "null pointer"), (dict(bands=None), BADARG, "null pointer"), (dict(filt=None), BADARG, "null pointer"),
    (dict(n_taps=None), BADARG, "null pointer"), (dict(rir=None), BADARG, "null pointer"), (dict(len=None), BADARG, "null pointer"),
    (dict(rooms=0x10004), BADARG, "8-byte aligned"), (dict(bands=0x10004), BADARG, "8-byte aligned"),
    (dict(filt=0x10004), BADARG, "8-byte aligned"), (dict(n_taps=0x10002), BADARG, "4-byte aligned"),
    (dict(rir=0x10001), BADARG, "4-byte aligned"), (dict(len=0x10002), BADARG, "4-byte aligned"),
    (dict(R=0), BADARG, "R=0"), (dict(R=-3), BADARG, "R=-3"), (dict(R=65536), BADARG, "R=65536"),
    (dict(K=0), BADARG, "K=0"), (dict(ld=99), BADARG, "ld=99"),
    (dict(NB=0), BADARG, "NB=0"), (dict(NB=-1), BADARG, "NB=-1"), (dict(NB=9), BADARG, "NB=9"),
    (dict(NF=0), BADARG, "NF=0"), (dict(NF=-3), BADARG, "NF=-3"), (dict(NF=8), BADARG, "NF=8"), (dict(NF=1024), BADARG, "NF=1024"),
    (dict(NF=1025), UNSUPPORTED, "NF=1025"),
    (dict(fs=0), BADARG, "fs=0"), (dict(fs=-16000), BADARG, "fs=-16000"),
    (dict(c=0.0), BADARG, "speed of sound"), (dict(c=-343.0), BADARG, "speed of sound"),
    (dict(c=float("nan")), BADARG, "speed of sound"), (dict(c=float("inf")), BADARG, "speed of sound"),
    (dict(tw=0), BADARG, "tw=0"), (dict(tw=-1), BADARG, "tw=-1"), (dict(tw=65), UNSUPPORTED, "tw=65"),
    (dict(Nx=-1), BADARG, "Nx=-1"), (dict(Ny=-1), BADARG, "Ny=-1"), (dict(Nz=-1), BADARG, "Nz=-1"),
    (dict(Nx=256), UNSUPPORTED, "Nx=256"), (dict(Ny=256), UNSUPPORTED, "Ny=256"), (dict(Nz=256), UNSUPPORTED, "Nz=256"),
    (dict(K=65537, ld=65537), UNSUPPORTED, "65536 taps"),
    (dict(), BADARG, "null handle"),                              # everything valid: only now is the handle missed
    (dict(Nx=0, Ny=0, Nz=0, K=65536, ld=65536, R=65535, tw=64, NB=8, NF=1023), BADARG, "null handle"),
    (dict(Nx=255, Ny=255, Nz=255, NB=1, NF=1), BADARG, "null handle"),
])
def test_abi_argument_errors_without_gpu(over, code, text):
    rc, msg = _call(**over)
    assert rc == code, (rc, msg)
    assert "cmgan_rir_bands" in msg and text in msg, msg


# ------------------------------------------------------------------ argument errors of Engine.rir_bands, on CPU tensors
def _args(R=3, K=50, NB=4, NF=9):
    return dict(rooms=torch.ones(R, 15, dtype=torch.float64), bands=torch.ones(R, NB, 7, dtype=torch.float64),
                n_taps=torch.ones(R, dtype=torch.int32), K=K, filters=torch.ones(NB, NF, dtype=torch.float64), n_images=(2, 3, 4))


def test_engine_rir_bands_argument_rules_without_gpu():
    cpu = torch.device("cpu")
    assert check_rir_bands_args(cpu, **_args()) == (3, 50, (2, 3, 4), 4, 9)
    out = (torch.zeros(3, 50), torch.zeros(3, dtype=torch.int32))
    assert check_rir_bands_args(cpu, **_args(NB=8, NF=1023), out=out) == (3, 50, (2, 3, 4), 8, 1023)
    assert check_rir_bands_args(cpu, **_args(NB=1, NF=1)) == (3, 50, (2, 3, 4), 1, 1)
    f64 = dict(dtype=torch.float64)
    cases = [
        (dict(rooms=torch.ones(3, 15)), TypeError, "rooms"), (dict(rooms=torch.ones(3, 14, **f64)), ValueError, "rooms"),
        (dict(bands=torch.ones(3, 4, 7)), TypeError, "bands"), (dict(bands=np.ones((3, 4, 7))), TypeError, "bands"),
        (dict(bands=torch.ones(3, 4, 6, **f64)), ValueError, "bands"), (dict(bands=torch.ones(2, 4, 7, **f64)), ValueError, "bands"),
        (dict(bands=torch.ones(3, 28, **f64)), ValueError, "bands"), (dict(bands=torch.ones(3, 9, 7, **f64)), ValueError, "bands"),
        (dict(bands=torch.ones(3, 0, 7, **f64)), ValueError, "bands"),
        (dict(bands=torch.ones(3, 7, 4, **f64).transpose(1, 2)), ValueError, "contiguous"),
        (dict(filters=torch.ones(4, 9)), TypeError, "filters"), (dict(filters=torch.ones(3, 9, **f64)), ValueError, "filters"),
        (dict(filters=torch.ones(4, 8, **f64)), ValueError, "filters"), (dict(filters=torch.ones(4, 1025, **f64)), ValueError, "filters"),
        (dict(filters=torch.ones(36, **f64)), ValueError, "filters"), (dict(filters=torch.ones(4, 0, **f64)), ValueError, "filters"),
        (dict(filters=torch.ones(9, 4, **f64).t()), ValueError, "contiguous"),
        (dict(n_taps=torch.ones(3, dtype=torch.int64)), TypeError, "n_taps"), (dict(K=0), ValueError, "K"),
        (dict(n_images=(2, 3)), ValueError, "n_images"), (dict(fs=0), ValueError, "fs"), (dict(c=0.0), ValueError, "c must"),
        (dict(tw=65), ValueError, "tw"), (dict(out=torch.zeros(3, 50)), ValueError, "out"),
        (dict(out=(torch.zeros(3, 49), torch.zeros(3, dtype=torch.int32))), ValueError, r"out\[0\]"),
    ]
    for over, exc, text in cases:
        a = _args()
        a.update(over)
        with pytest.raises(exc, match=text):
            check_rir_bands_args(cpu, **a)
    with pytest.raises(RuntimeError, match="bound to"):
        check_rir_bands_args(torch.device("meta"), **_args())


# ------------------------------------------------------------------ the cases whose bits are recorded
def test_the_recorded_cases_are_not_trivial():
    """tests/rir_cases.py through the float64 model: what tests/golden/make_rir_bits.py asserts of the GPU's output."""
    import rir_cases as RC
    lib = _lib.load()
    T, cap = int(lib.cmgan_rir_tile()), int(lib.cmgan_rir_list_capacity())
    cases = RC.rir_bands_cases(T)
    assert tuple(cases) == RC.RIR_BANDS_NAMES
    for name, case in cases.items():
        h, length = RC.model(case)
        RC.nontrivial(name, case, h, length, T, cap)
