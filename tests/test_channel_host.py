"""CPU side of the recording channel (cmgan_amd/csrc/channel.hip; include/cmgan_hip.h, "Recording channel"): the float64
model the GPU tests compare the kernels with (tests/channel_model.py) against scipy.signal.sosfilt, the prescribed tiled
scan against the long-double loop, the filter designs of cmgan_amd.mixing against scipy's frequency responses, what a
ChannelSampler draws, the workspace formula, and every argument error of cmgan_channel, Engine.channel, ChannelSampler and
DynamicMixer(channel=, channel_on=), all of which are judged before a handle or a GPU is needed."""
import math

import numpy as np
import pytest
import torch
from scipy import signal

import channel_model as M
from cmgan_amd import _lib
from cmgan_amd.engine import (CHANNEL_MAX_L, CHANNEL_MAX_SECTIONS, CHANNEL_TILE, channel_workspace_bytes,
                              check_channel_args)
from cmgan_amd.mixing import (ChannelSampler, DynamicMixer, NoiseBank, biquad_high_shelf, biquad_highpass,
                              biquad_low_shelf, biquad_lowpass, biquad_peaking, butter_lowpass_sos)

BADARG = -1
CPU = torch.device("cpu")
FS = 16000


# ------------------------------------------------------------------ the model
def test_filt_is_sosfilt_bit_for_bit():
    sos = M.hard_cascade()
    x = M.noise(1, 6000)
    whole = signal.sosfilt(sos, x.astype(np.float64))
    assert np.array_equal(M.filt(x, 6000, sos, 8).view(np.uint64), whole.view(np.uint64))
    assert np.array_equal(M.filt(x, 4000, sos, 3), signal.sosfilt(sos[:3], x[:4000].astype(np.float64)))
    assert np.array_equal(M.filt(x, 100, sos, 0), x[:100].astype(np.float64))
    # ... which is the plain transposed-direct-form-II loop in float64
    y = x[:500].astype(np.float64)
    for s in range(8):
        b0, b1, b2, _, a1, a2 = sos[s].tolist()
        z1 = z2 = 0.0
        out = []
        for u in y.tolist():
            v = b0 * u + z1
            z1 = b1 * u - a1 * v + z2
            z2 = b2 * u - a2 * v
            out.append(v)
        y = np.array(out)
    assert np.array_equal(y.view(np.uint64), whole[:500].view(np.uint64))
    # the clip
    c = M.filt(x, 6000, sos, 8, 0.25)
    assert c.max() == 0.25 and c.min() == -0.25 and np.array_equal(c[np.abs(whole) < 0.25], whole[np.abs(whole) < 0.25])


def test_long_double_loop():
    sos = M.hard_cascade()
    x = M.noise(1, 3000)
    ld = M.filt_ld(x, 3000, sos, 8)
    assert ld.dtype == np.longdouble
    if np.finfo(np.longdouble).eps < 1e-18:                              # where long double is wider than double
        assert float(np.max(np.abs(M.loop_ld(x, 3000, sos, 8) - ld))) < 1e-14
        assert float(np.max(np.abs(M.filt(x, 3000, sos, 8) - ld))) > 0.0


@pytest.mark.parametrize("tile", [8 * 256, 4 * 256])
def test_tiled_scan_holds_on_the_hard_cascade(tile):
    """A condition on the METHOD: 1.7e-11 was measured before the kernels were written."""
    sos = M.hard_cascade()
    n = 50000
    x = M.noise(1, n)
    ref = M.filt_ld(x, n, sos, 8)
    err = float(np.max(np.abs(M.tiled(x, n, sos, 8, None, tile) - ref)))
    seq = float(np.max(np.abs(M.filt(x, n, sos, 8) - ref)))
    A = M.system_matrix(sos, 8)
    growth, P = 0.0, np.eye(16)
    for _ in range(4000):
        P = P @ A
        growth = max(growth, float(np.linalg.norm(P, 2)))
    print(f"[channel] hard cascade, tile {tile}: tiled vs long double {err:.2e}, sequential float64 {seq:.2e}, output peak "
          f"{float(np.max(np.abs(ref))):.2f}, max ||A^k|| {growth:.0f}, E = {M.slack(x, n, sos, 8, tile):.2e}")
    assert err <= 1e-9
    assert 100 < growth < 1000


@pytest.mark.parametrize("tile", [8 * 256, 4 * 256])
def test_tiled_scan_holds_on_sampler_draws(tile):
    gen = torch.Generator().manual_seed(5)
    sos, m, _, _ = ChannelSampler(p_highpass=0.7, p_bandlimit=0.5, generator=gen).draw(50, FS)
    sos, m = sos.numpy(), m.numpy()
    n = 2 * tile + 77
    worst = 0.0
    for b in range(50):
        x = M.noise(100 + b, n)
        worst = max(worst, float(np.max(np.abs(M.tiled(x, n, sos[b], int(m[b]), None, tile) - M.filt_ld(x, n, sos[b], int(m[b]))))))
    print(f"[channel] 50 sampler draws, tile {tile}: tiled vs long double {worst:.2e}")
    assert worst <= 1e-9 and int(m.max()) >= 5 and int(m.min()) <= 1


def test_ulp32():
    for w in (1.0, 0.75, 0.5, 1.9999, 3e-5, -0.3, 1e-42, 0.0):
        want = float(np.spacing(np.float32(abs(w)))) if abs(w) >= 2.0 ** -126 else 2.0 ** -149
        assert float(M.ulp32(w)) == want, w


# ------------------------------------------------------------------ the designs
def _gain_db(row, f, fs=FS):
    _, h = signal.sosfreqz(np.asarray(row, dtype=np.float64).reshape(-1, 6), worN=[f], fs=fs)
    return 20.0 * math.log10(abs(h[0]))


@pytest.mark.parametrize("f0,gain,q", [(1000.0, 6.0, 1.0), (50.0, -12.0, 4.0), (7000.0, 3.5, 0.5)])
def test_peaking(f0, gain, q):
    row = biquad_peaking(f0, gain, q, FS)
    assert row.dtype == torch.float64 and tuple(row.shape) == (6,) and float(row[3]) == 1.0
    assert abs(_gain_db(row, f0) - gain) < 1e-9
    assert abs(_gain_db(row, 0.0)) < 1e-9 and abs(_gain_db(row, FS / 2)) < 1e-9
    assert np.allclose(row.numpy(), M.peaking(f0, gain, q), rtol=1e-14, atol=0)


@pytest.mark.parametrize("f0,gain,q", [(300.0, 6.0, 0.7071), (2000.0, -9.0, 1.0)])
def test_shelves(f0, gain, q):
    lo, hi = biquad_low_shelf(f0, gain, q, FS), biquad_high_shelf(f0, gain, q, FS)
    assert float(lo[3]) == 1.0 and float(hi[3]) == 1.0
    assert abs(_gain_db(lo, 0.0) - gain) < 1e-9 and abs(_gain_db(lo, FS / 2)) < 1e-9
    assert abs(_gain_db(hi, FS / 2) - gain) < 1e-9 and abs(_gain_db(hi, 0.0)) < 1e-9
    assert abs(_gain_db(lo, f0) - gain / 2) < 1e-9 and abs(_gain_db(hi, f0) - gain / 2) < 1e-9


@pytest.mark.parametrize("fc", [100.0, 3800.0])
def test_lowpass_and_highpass(fc):
    lp, hp = biquad_lowpass(fc, math.sqrt(0.5), FS), biquad_highpass(fc, math.sqrt(0.5), FS)
    assert float(lp[3]) == 1.0 and float(hp[3]) == 1.0
    drop = 10.0 * math.log10(0.5)
    assert abs(_gain_db(lp, fc) - drop) < 1e-9 and abs(_gain_db(hp, fc) - drop) < 1e-9
    assert abs(_gain_db(lp, 0.0)) < 1e-9 and abs(_gain_db(hp, FS / 2)) < 1e-9
    assert np.allclose(hp.numpy(), M.highpass(fc, math.sqrt(0.5)), rtol=1e-14, atol=0)
    assert abs(_gain_db(biquad_lowpass(fc, 2.0, FS), fc) - 20.0 * math.log10(2.0)) < 1e-9


def test_designs_broadcast_over_tensors():
    f0 = torch.tensor([[100.0, 1000.0], [3000.0, 7000.0]], dtype=torch.float64)
    rows = biquad_peaking(f0, torch.tensor(3.0), 1.0, FS)
    assert tuple(rows.shape) == (2, 2, 6) and rows.dtype == torch.float64
    assert torch.equal(rows[1, 0], biquad_peaking(3000.0, 3.0, 1.0, FS))


@pytest.mark.parametrize("order", [2, 4, 6, 8])
def test_butterworth_matches_scipy(order):
    for fc in (3400.0, 3800.0, 500.0):
        ours = butter_lowpass_sos(order, fc, FS)
        assert tuple(ours.shape) == (order // 2, 6) and bool((ours[:, 3] == 1.0).all())
        w = np.linspace(0.0, FS / 2, 513)
        _, h1 = signal.sosfreqz(ours.numpy(), worN=w, fs=FS)
        _, h2 = signal.sosfreqz(signal.butter(order, fc, output="sos", fs=FS), worN=w, fs=FS)
        assert float(np.max(np.abs(h1 - h2))) <= 1e-12, (order, fc)
    assert tuple(butter_lowpass_sos(4, torch.tensor([3400.0, 3500.0, 3600.0], dtype=torch.float64), FS).shape) == (3, 2, 6)
    for bad in (0, 3, 10, 2.5, True):
        with pytest.raises(ValueError, match="order must be 2, 4, 6 or 8"):
            butter_lowpass_sos(bad, 1000.0, FS)


# ------------------------------------------------------------------ the sampler
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sampler_draws_are_stable_and_normalised(seed):
    gen = torch.Generator().manual_seed(seed)
    smp = ChannelSampler(p_highpass=0.5, p_bandlimit=0.5, p_clip=0.5, generator=gen)
    sos, m, shared, clip = smp.draw(1000, FS)
    S = sos.size(1)
    assert S == smp.sections == 8 and sos.dtype == torch.float64 and tuple(sos.shape) == (1000, 8, 6) and sos.is_contiguous()
    assert m.dtype == torch.int32 and shared.dtype == torch.int32 and clip.dtype == torch.float64
    assert torch.equal(m, shared) and int(m.min()) == 0 and int(m.max()) == 8
    a1, a2 = sos[..., 4], sos[..., 5]
    assert bool(torch.isfinite(sos).all()) and bool((sos[..., 3] == 1.0).all())
    assert bool((a2.abs() < 1.0).all()) and bool((a1.abs() < 1.0 + a2).all())
    used = torch.arange(S)[None, :] < m[:, None]
    ident = torch.tensor(M.IDENTITY)
    assert bool((sos[~used] == ident).all())                            # a row's own sections first, identity after them
    assert not bool((sos[used] == ident).all(dim=-1).any())
    on = torch.isfinite(clip)
    assert 350 < int(on.sum()) < 650 and bool((clip[on] >= 0.3).all()) and bool((clip[on] <= 0.9).all())
    assert bool(torch.isposinf(clip[~on]).all())


def test_sampler_options_fix_the_section_count():
    assert ChannelSampler().sections == 8
    assert ChannelSampler(p_highpass=0.0, max_eq=2, p_bandlimit=0.0).sections == 2
    assert ChannelSampler(max_eq=7, p_bandlimit=0.0).sections == 8
    s0 = ChannelSampler(p_highpass=0.0, max_eq=0, p_bandlimit=0.0, p_clip=1.0, generator=torch.Generator().manual_seed(1))
    sos, m, shared, clip = s0.draw(4, FS)
    assert tuple(sos.shape) == (4, 1, 6) and not m.any() and bool((sos == torch.tensor(M.IDENTITY)).all())
    assert bool(torch.isfinite(clip).all())
    one = ChannelSampler(p_highpass=1.0, max_eq=0, p_bandlimit=1.0, bandlimit_order=4, p_clip=0.0,
                         generator=torch.Generator().manual_seed(1))
    sos, m, _, clip = one.draw(6, FS)
    assert tuple(sos.shape) == (6, 3, 6) and bool((m == 3).all()) and bool(torch.isposinf(clip).all())
    # the same seed gives the same draw
    again = ChannelSampler(p_highpass=1.0, max_eq=0, p_bandlimit=1.0, bandlimit_order=4, p_clip=0.0,
                           generator=torch.Generator().manual_seed(1)).draw(6, FS)
    assert torch.equal(again[0], sos)
    # the band limit is a Butterworth low-pass at a cutoff inside the range (-3.01 dB there), after the high-pass
    f = np.linspace(3400.0, 3800.0, 401)
    for b in range(6):
        _, h = signal.sosfreqz(sos[b, 1:].numpy(), worN=f, fs=FS)
        assert np.min(np.abs(20 * np.log10(np.abs(h)) - 10 * math.log10(0.5))) < 0.05
        assert abs(_gain_db(sos[b, :1], 1000.0)) < 0.1 and _gain_db(sos[b, :1], 5.0) < -12.0


def test_sampler_rejects_bad_options():
    for kw, text in [(dict(p_highpass=1.5), "p_highpass must lie in"), (dict(p_bandlimit=-0.1), "p_bandlimit must lie in"),
                     (dict(p_clip=2.0), "p_clip must lie in"), (dict(highpass_hz=(120.0, 20.0)), "highpass_hz must be"),
                     (dict(highpass_hz=(0.0, 20.0)), "highpass_hz must be"), (dict(eq_hz=50.0), "eq_hz must be"),
                     (dict(eq_q=(0.0, 2.0)), "eq_q must be"), (dict(bandlimit_hz=(3800.0,)), "bandlimit_hz must be"),
                     (dict(clip_rel=(0.9, 0.3)), "clip_rel must be"), (dict(max_eq=-1), "max_eq must be"),
                     (dict(max_eq=1.5), "max_eq must be"), (dict(eq_db=-1.0), "eq_db must be"),
                     (dict(eq_db=math.inf), "eq_db must be"), (dict(bandlimit_order=5), "bandlimit_order must be"),
                     (dict(max_eq=4), "are 9 sections"), (dict(max_eq=8, p_highpass=0.0), "are 12 sections")]:
        with pytest.raises(ValueError, match=text):
            ChannelSampler(**kw)
    with pytest.raises(ValueError, match="must lie below fs / 2"):
        ChannelSampler().draw(4, 7000)                                   # a 3.8 kHz band limit in a 7 kHz file
    with pytest.raises(ValueError, match="eq_hz = .* must lie below fs / 2"):
        ChannelSampler(eq_hz=(50.0, 9000.0)).draw(4, FS)


# ------------------------------------------------------------------ DynamicMixer's new arguments
class _NoEngine:
    device = CPU


def test_mixer_rejects_bad_channel_options():
    bank = NoiseBank.from_arrays([np.ones(100, dtype=np.float32)])
    for bad in ("clean", "target", None, ""):
        with pytest.raises(ValueError, match="channel_on must be 'noisy' or 'both'"):
            DynamicMixer(_NoEngine(), bank, channel_on=bad)
    with pytest.raises(TypeError, match="channel must be a ChannelSampler"):
        DynamicMixer(_NoEngine(), bank, channel="telephone")
    m = DynamicMixer(_NoEngine(), bank)
    assert m.channel is None and m.channel_on == "noisy"
    m = DynamicMixer(_NoEngine(), bank, channel=ChannelSampler(), channel_on="both")
    assert m.channel_on == "both"


def test_channel_draw_comes_last_and_from_its_own_generator():
    bank = NoiseBank.from_arrays([np.ones(100, dtype=np.float32), np.ones(50, dtype=np.float32)])
    gen = lambda s=7: torch.Generator().manual_seed(s)
    g0, g1 = gen(), gen()
    smp = ChannelSampler(generator=gen(11))
    d0 = DynamicMixer(_NoEngine(), bank, generator=g0, level_db=(-35, -15)).draw(6)
    d1 = DynamicMixer(_NoEngine(), bank, generator=g1, level_db=(-35, -15), channel=smp).draw(6)
    assert d0.channel is None and len(d1.channel) == 4
    for a, b in zip(d0[:8], d1[:8]):
        assert (a is None and b is None) or torch.equal(a, b)
    assert torch.equal(g0.get_state(), g1.get_state())                   # the mixer's generator is not touched by the channel
    want = ChannelSampler(generator=gen(11)).draw(6, FS)
    assert all(torch.equal(a, b) for a, b in zip(d1.channel, want))


def test_channel_clip():
    noisy = torch.tensor([[0.5, -2.0, 1.0], [0.0, 0.0, 0.0], [0.25, 0.1, -0.1], [1.0, 1.0, 1.0]])
    rel = torch.tensor([0.5, 0.5, math.inf, 0.3], dtype=torch.float64)
    clip = DynamicMixer.channel_clip(rel, noisy)
    assert clip.dtype == torch.float64 and clip.tolist() == [1.0, math.inf, math.inf, 0.3]


# ------------------------------------------------------------------ the library without a GPU
def test_symbols_tile_and_abi():
    lib = _lib.load()
    for name in ("cmgan_channel", "cmgan_channel_workspace_bytes", "cmgan_channel_tile", "cmgan_channel_max_sections"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.cmgan_channel_max_sections() == CHANNEL_MAX_SECTIONS == 8
    T = lib.cmgan_channel_tile()
    assert T == CHANNEL_TILE and T % 256 == 0 and (T // 256) & (T // 256 - 1) == 0
    assert lib.cmgan_abi_version() == _lib.ABI_VERSION >= 11


def test_workspace_formula():
    lib = _lib.load()
    ws = lambda B, L, S: int(lib.cmgan_channel_workspace_bytes(B, L, S))
    T = CHANNEL_TILE
    for B in (1, 2, 5, 32, 65535):
        for L in (1, T - 1, T, T + 1, 32000, 160000, CHANNEL_MAX_L):
            for S in range(1, 9):
                assert ws(B, L, S) == channel_workspace_bytes(B, L, S) > 0 and ws(B, L, S) % 256 == 0, (B, L, S)
    assert ws(3, 32000, 3) <= ws(4, 32000, 3) <= ws(4, 32001 + T, 3) <= ws(4, 32001 + T, 5)
    assert ws(2, 5000, 3) == ws(2, 5000, 4) < ws(2, 5000, 5)             # padded to 1, 2, 4 or 8 sections
    for B, L, S in ((0, 100, 1), (-1, 100, 1), (65536, 100, 1), (1, 0, 1), (1, -5, 1), (1, CHANNEL_MAX_L + 1, 1), (1, 100, 0),
                    (1, 100, 9), (1, 100, -1)):
        assert ws(B, L, S) == channel_workspace_bytes(B, L, S) == 0, (B, L, S)


def test_library_rejects_bad_arguments_before_it_needs_a_handle():
    lib = _lib.load()
    x = np.zeros(8192, dtype=np.float32)
    y = np.zeros(8192, dtype=np.float32)
    lengths = np.zeros(8, dtype=np.int32)
    nsec = np.zeros(8, dtype=np.int32)
    status = np.full(8, 7, dtype=np.int32)
    sos = np.zeros(8 * 8 * 6 + 1, dtype=np.float64)
    clip = np.ones(9, dtype=np.float64)
    raw = np.zeros(1 << 20, dtype=np.uint8)
    base = (raw.ctypes.data + 255) & ~255
    px, py, pl, pn, pt, ps, pc = (a.ctypes.data for a in (x, y, lengths, nsec, status, sos, clip))

    def call(x=px, B=2, L=1500, ldx=1500, lengths=pl, sos=ps, nsec=pn, S=3, clip=pc, y=py, ldy=1500, status=pt, ws=base,
             ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = channel_workspace_bytes(B, L, S) if 1 <= B <= 8 and 1 <= L <= 4096 and 1 <= S <= 8 else 4096
        rc = lib.cmgan_channel(None, x, B, L, ldx, lengths, sos, nsec, S, clip, y, ldy, status, ws, ws_bytes, None)
        return rc, (lib.cmgan_last_error(None) or b"").decode()

    need = channel_workspace_bytes(2, 1500, 3)
    cases = {
        "null pointer": [dict(x=None), dict(sos=None), dict(y=None)],
        "4-byte aligned": [dict(x=px + 2), dict(y=py + 1), dict(lengths=pl + 1), dict(nsec=pn + 2), dict(status=pt + 3)],
        "8-byte aligned": [dict(sos=ps + 4), dict(clip=pc + 4)],
        "need 1 <= B": [dict(B=0), dict(B=-3), dict(B=65536), dict(L=0), dict(L=-1), dict(ldx=1499), dict(ldy=1499)],
        "rows of up to": [dict(L=CHANNEL_MAX_L + 1, ldx=2 ** 31 - 1, ldy=2 ** 31 - 1)],
        "S must lie": [dict(S=0), dict(S=9), dict(S=-1)],
        "overlap": [dict(y=px + 4), dict(y=px + 4 * 1500), dict(y=px, ldy=1501), dict(y=px + 4 * 2999), dict(x=py + 4 * 100)],
        "workspace": [dict(ws=None), dict(ws=base + 64), dict(ws_bytes=need - 1), dict(ws_bytes=0)],
    }
    for text, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == BADARG and text in msg, (kw, rc, msg)
    # everything in order: only the handle is missing - nothing was enqueued, nothing was written
    for kw in (dict(), dict(lengths=None), dict(nsec=None), dict(clip=None), dict(status=None), dict(S=1), dict(S=8),
               dict(y=px), dict(y=px, ldx=2000, ldy=2000), dict(y=px + 4 * 3000)):
        rc, msg = call(**kw)
        assert rc == BADARG and "null handle" in msg, (kw, rc, msg)
    assert not y.any() and (status == 7).all()


# ------------------------------------------------------------------ Engine.channel's argument rules
def test_check_channel_args():
    wav = torch.zeros(3, 2000)
    sos = torch.zeros(3, 4, 6, dtype=torch.float64)
    i32 = lambda n=3: torch.zeros(n, dtype=torch.int32)
    f64 = lambda n=3: torch.ones(n, dtype=torch.float64)
    assert check_channel_args(CPU, wav, sos) == (3, 2000, 4)
    assert check_channel_args(CPU, wav, sos, i32(), f64(), i32(), torch.zeros(3, 2000)) == (3, 2000, 4)
    assert check_channel_args(CPU, wav, sos, out=wav) == (3, 2000, 4)
    view = torch.zeros(3, 2500)[:, :2000]                                # a row stride larger than L
    assert check_channel_args(CPU, view, sos, out=view) == (3, 2000, 4)
    assert check_channel_args(CPU, torch.zeros(1, 7), torch.zeros(1, 8, 6, dtype=torch.float64)) == (1, 7, 8)
    with pytest.raises(TypeError, match="wav: expected a torch.Tensor"):
        check_channel_args(CPU, np.zeros((3, 2000), dtype=np.float32), sos)
    with pytest.raises(TypeError, match="wav: expected float32"):
        check_channel_args(CPU, wav.double(), sos)
    with pytest.raises(RuntimeError, match="wav: tensor is on cpu"):
        check_channel_args(torch.device("cuda:0"), wav, sos)
    for bad in (torch.zeros(2000), torch.zeros(1, 3, 2000), torch.zeros(0, 2000), torch.zeros(3, 0)):
        with pytest.raises(ValueError, match="wav: expected \\[B, L\\]"):
            check_channel_args(CPU, bad, sos)
    with pytest.raises(ValueError, match="at most 65535 rows"):
        check_channel_args(CPU, torch.zeros(1, 1).expand(65536, 1), sos)
    for bad in (torch.zeros(3, 4000)[:, ::2], torch.zeros(2000, 3).t(), torch.zeros(1, 2000).expand(3, 2000)):
        with pytest.raises(ValueError, match="wav: rows must be contiguous"):
            check_channel_args(CPU, bad, sos)
    with pytest.raises(TypeError, match="sos: expected float64"):
        check_channel_args(CPU, wav, sos.float())
    for bad in (torch.zeros(3, 6), torch.zeros(2, 4, 6), torch.zeros(3, 9, 6), torch.zeros(3, 0, 6), torch.zeros(3, 4, 5)):
        with pytest.raises(ValueError, match="sos: expected \\[3, S, 6\\]"):
            check_channel_args(CPU, wav, bad.double())
    with pytest.raises(ValueError, match="sos: must be contiguous"):
        check_channel_args(CPU, wav, torch.zeros(3, 8, 6, dtype=torch.float64)[:, ::2])
    with pytest.raises(TypeError, match="n_sections: expected int32"):
        check_channel_args(CPU, wav, sos, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="n_sections: expected \\[3\\]"):
        check_channel_args(CPU, wav, sos, i32(4))
    with pytest.raises(TypeError, match="clip: expected float64"):
        check_channel_args(CPU, wav, sos, None, torch.ones(3))
    with pytest.raises(TypeError, match="clip: expected a torch.Tensor"):
        check_channel_args(CPU, wav, sos, None, 0.5)
    with pytest.raises(ValueError, match="clip: expected \\[3\\]"):
        check_channel_args(CPU, wav, sos, None, f64(2))
    with pytest.raises(TypeError, match="lengths: expected int32"):
        check_channel_args(CPU, wav, sos, None, None, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="lengths: must be contiguous"):
        check_channel_args(CPU, wav, sos, None, None, torch.zeros(6, dtype=torch.int32)[::2])
    with pytest.raises(TypeError, match="out: expected float32"):
        check_channel_args(CPU, wav, sos, out=torch.zeros(3, 2000, dtype=torch.float64))
    with pytest.raises(ValueError, match="out: expected \\[3, 2000\\]"):
        check_channel_args(CPU, wav, sos, out=torch.zeros(3, 2001))
    with pytest.raises(ValueError, match="out: rows must be contiguous"):
        check_channel_args(CPU, wav, sos, out=torch.zeros(3, 4000)[:, ::2])
    both = torch.zeros(3, 4000)
    with pytest.raises(ValueError, match="out: in place needs the row stride of wav"):
        check_channel_args(CPU, both[:, :2000], sos, out=both.view(6, 2000)[:3])
