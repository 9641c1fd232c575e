"""CPU side of the diffuse reverberant tail (cmgan_amd/csrc/rir_tail.hip; include/cmgan_hip.h, "The diffuse reverberant
tail"): the long-double model the GPU tests compare the kernels with (tests/rir_tail_model.py) against a naive loop, literal
values and a closed form; the library's symbols and workspace formula; every argument error of cmgan_rir_tail, Engine.rir_tail
and RoomSampler(tail_ms=), all of which are judged before a handle or a GPU is needed; and one acoustic check of the model."""
import math

import numpy as np
import pytest
import torch

import rir_bands_model as BM
import rir_model as RM
import rir_stats_model as SM
import rir_tail_model as M
from cmgan_amd import _lib
from cmgan_amd.engine import RIR_MAX_BANDS, RIR_MAX_FILTER, RIR_TAIL_MAX_WINDOW, RirTail, check_rir_tail_args
from cmgan_amd.mixing import RoomSampler, TailDraw, octave_filterbank, sabine_beta

BADARG, UNSUPPORTED = -1, -3
CPU = torch.device("cpu")
LD = np.longdouble


# ------------------------------------------------------------------ the noise
def test_philox_known_answer_and_noise_literals():
    # Random123's known-answer vectors of Philox4x32-10
    assert [int(w[0]) for w in M.philox4x32_10(np.array([0]), 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ones = M.philox4x32_10(np.array([0xffffffff]), -1)
    assert all(0 <= int(w[0]) < 2 ** 32 for w in ones)
    assert M.NOISE_DIV == math.sqrt((2 ** 64 - 1) / 3) and M.THREE_LN10 == pytest.approx(3 * math.log(10), rel=1e-15)
    got = M.noise(1234, np.array([-1, 0, 1, 2, 65535]))
    assert got.tolist() == [0.0, 0.0734060714998014, -0.3631542958919652, 0.981177506700922, 1.4538400388965718]
    assert M.noise(-5, np.array([0, 7])).tolist() == [2.1067860083790757, 1.199404475099758]      # a negative seed is a key too
    # the numerator is the exact integer: nu NOISE_DIV is whole
    assert np.all(np.rint(got * M.NOISE_DIV) == np.round(got * M.NOISE_DIV, 3))


def test_noise_moments_seeds_and_negative_indices():
    q = np.arange(200000)
    v = M.noise(1234, q)
    assert abs(v.mean()) <= 0.01 and abs(v.var() - 1.0) <= 0.01                  # the standard errors are 0.002 and 0.003
    kurt = float(((v - v.mean()) ** 4).mean() / v.var() ** 2)
    assert 2.6 < kurt < 2.8                                                        # four uniforms: 3 - 6 / 20 = 2.7
    assert np.max(np.abs(v)) <= 2 * (2 ** 32 - 1) / M.NOISE_DIV
    other = M.noise(1235, q[:1000])
    assert np.count_nonzero(other == v[:1000]) == 0
    high = M.noise(1234 + 2 ** 32, q[:1000])                                       # the key's high word counts
    assert np.count_nonzero(high == v[:1000]) == 0
    assert not M.noise(1234, np.arange(-50, 0)).any()


# ------------------------------------------------------------------ the model against a naive loop and a closed form
def _naive_row(h, kx, kend, decay, seed, filt, W, fs):
    NB, NF = filt.shape
    D = (NF - 1) // 2
    hz = lambda i: float(h[i]) if 0 <= i < kx else 0.0
    A = []
    for b in range(NB):
        d = 3 * math.log(10) / (decay[b] * fs)
        E = S = 0.0
        for k in range(kx - D - W, kx - D):
            z = sum(filt[b][j] * hz(k + D - j) for j in range(NF))
            E += z * z
            S += math.exp(-2 * d * (k - kx))
        G = sum(filt[b][j] ** 2 for j in range(NF))
        A.append(math.sqrt(E / (G * S)) if E else 0.0)
    y = np.array(h, dtype=np.float64)
    for k in range(kx, kend):
        acc = 0.0
        for b in range(NB):
            d = 3 * math.log(10) / (decay[b] * fs)
            for j in range(NF):
                q = k + D - j
                acc += filt[b][j] * A[b] * math.exp(-d * (q - kx)) * float(M.noise(seed, np.array([q]))[0])
        y[k] = acc
    y[kend:] = 0.0
    return y, A


@pytest.mark.parametrize("NB,NF", [(0, 1), (2, 5)])
def test_model_equals_the_naive_double_loop(NB, NF):
    rng = np.random.default_rng(11)
    K, kx, n_taps, W, fs = 40, 17, 33, 9, 8000
    h = rng.standard_normal(K).astype(np.float32)
    filt = rng.standard_normal((NB, NF)) if NB else None
    decay = [0.004, 0.007][:max(NB, 1)]
    m = M.rir_tail_row(h, kx, n_taps, decay, 99, filt, W, fs)
    y, A = _naive_row(h, kx, n_taps, decay, 99, filt if NB else np.ones((1, 1)), W, fs)
    assert m["status"] == 0 and m["length"] == n_taps and (m["kx"], m["kend"]) == (kx, n_taps)
    assert np.allclose(m["gain"], A, rtol=1e-13, atol=0) and np.all(m["gain"] > 0)
    assert np.allclose(m["y"], y, rtol=1e-12, atol=1e-15)
    assert np.array_equal(m["y"][:kx], h[:kx].astype(np.float64)) and not m["y"][n_taps:].any() and m["y"][kx:n_taps].all()
    # the bound: positive on the tail and small beside the taps; zero where the device must give the bits themselves
    assert np.all(m["bound"][kx:n_taps] > 0) and not m["bound"][:kx].any() and not m["bound"][n_taps:].any()
    assert np.max(m["bound"][kx:n_taps]) < 1e-6 * np.max(np.abs(y[kx:n_taps]))
    assert np.all(m["gain_bound"] < 1e-12 * m["gain"])


def test_rows_left_untouched_and_the_clamps():
    h = SM.decaying_noise(3, 300, 0.2)
    row = lambda **kw: M.rir_tail_row(**{**dict(h=h, kx=100, n_taps=250, decay=[0.05], seed=1, W=64), **kw})
    ok = row()
    assert ok["status"] == 0 and ok["length"] == 250
    for kw, bits in ((dict(n_taps=100), M.NOTHING), (dict(n_taps=-4), M.NOTHING), (dict(kx=63), M.WINDOW), (dict(kx=0), M.WINDOW),
                     (dict(decay=[math.nan]), M.DECAY), (dict(decay=[0.0]), M.DECAY), (dict(decay=[-1.0]), M.DECAY),
                     (dict(decay=[math.inf]), M.DECAY), (dict(kx=20, n_taps=10, decay=[math.nan]), M.NOTHING | M.WINDOW | M.DECAY)):
        m = row(**kw)
        assert m["status"] == bits and m["length"] == kw.get("kx", 100) and not m["gain"].any(), kw
        assert np.array_equal(m["y"], h.astype(np.float64))
    bad = h.copy()
    bad[40] = np.inf
    assert row(h=bad)["status"] == M.NONFINITE and row(h=bad, W=59)["status"] == 0       # 100 - 59 = 41: beyond the fit's reach
    assert row(h=bad, kx=30, n_taps=20)["status"] == M.NOTHING | M.WINDOW                 # not judged where no window fits
    assert row(kx=64)["status"] == 0 and row(n_taps=10 ** 6)["length"] == 300
    # bands: the window moves D back and the fit reaches 2 D further
    delta3 = np.zeros((1, 7))
    delta3[0, 3] = 1.0
    assert row(filt=delta3, kx=66)["status"] == M.WINDOW and row(filt=delta3, kx=67)["status"] == 0
    assert row(h=bad, filt=delta3, kx=110)["status"] == M.NONFINITE                       # 110 - 64 - 6 = 40
    silent = row(filt=np.zeros((1, 7)))
    assert silent["status"] == 0 and silent["gain"][0] == 0 and not silent["y"][100:].any() and silent["length"] == 250


def test_geometric_input_gives_the_closed_form_level():
    """h[k] = a rho^k with rho = exp(-delta): E / S = a^2 rho^(2 k_x), so A = a rho^k_x, and under nu = 1 the tail goes on
    as the same geometric sequence."""
    fs, decay, a, K, kx, W = 16000, 0.25, 0.5, 3000, 1200, 480
    d = 3 * math.log(10) / (decay * fs)
    h = (a * np.exp(-d * np.arange(K))).astype(np.float32)
    ones = lambda seed, q: np.ones(len(q))
    m = M.rir_tail_row(h, kx, K, [decay], 0, None, W, fs, nu=ones)
    want = a * math.exp(-d * kx)
    assert m["gain"][0] == pytest.approx(want, rel=2.0 ** -23)                     # the input is rounded to float32
    k = np.arange(kx, K)
    assert np.allclose(m["y"][kx:], a * np.exp(-d * k), rtol=2.0 ** -22, atol=0)
    # through a filterbank that sums to a delay: the bands' levels are those of the filtered sequence
    filt = octave_filterbank(fs, 3, 31).numpy()
    mb = M.rir_tail_row(h, kx, K, [decay] * 3, 0, filt, W, fs, nu=ones)
    assert mb["status"] == 0 and np.all(mb["gain"] >= 0) and mb["gain"][0] > 10 * mb["gain"][2]   # a smooth decay is low-pass


# ------------------------------------------------------------------ the library without a GPU
def test_symbols_tile_and_abi():
    lib = _lib.load()
    for name in ("cmgan_rir_tail", "cmgan_rir_tail_workspace_bytes", "cmgan_rir_tail_tile", "cmgan_rir_tail_max_window"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.cmgan_rir_tail_tile() == 256
    assert lib.cmgan_rir_tail_max_window() == RIR_TAIL_MAX_WINDOW == 4096
    assert lib.cmgan_rir_max_bands() == RIR_MAX_BANDS and lib.cmgan_rir_max_filter() == RIR_MAX_FILTER
    assert lib.cmgan_abi_version() == _lib.ABI_VERSION >= 17
    assert RirTail._fields == ("gain", "status") and TailDraw._fields == ("n_full", "decay", "seed", "src_junction", "src_seed")
    assert (M.NOTHING, M.WINDOW, M.DECAY, M.NONFINITE) == (1, 2, 4, 8)


def test_workspace_formula():
    lib = _lib.load()
    ws = lambda R, K, NB, NF: int(lib.cmgan_rir_tail_workspace_bytes(None, R, K, NB, NF))
    for R in (1, 5, 64, 65, 65535):
        for K in (1, 255, 256, 257, 65536):
            for NB, NF in ((0, 1), (1, 3), (7, 511), (8, 1023)):
                assert ws(R, K, NB, NF) == ((4 * R + 255) & ~255) > 0, (R, K, NB, NF)
    base = (4, 3000, 3, 511)
    for i, more in enumerate((500, 6000, 4, 513)):
        grown = list(base)
        grown[i] = more
        assert ws(*base) <= ws(*grown), (i, more)
    for bad in ((0, 100, 0, 1), (-1, 100, 0, 1), (65536, 100, 0, 1), (1, 0, 0, 1), (1, 65537, 0, 1), (1, 100, -1, 1),
                (1, 100, 9, 1), (1, 100, 1, 0), (1, 100, 1, 4), (1, 100, 1, 1025), (1, 100, 1, -3)):
        assert ws(*bad) == 0, bad


def test_library_rejects_bad_arguments_before_it_needs_a_handle():
    lib = _lib.load()
    rir = np.zeros(8192, dtype=np.float32)
    length = np.full(8, 1000, dtype=np.int32)
    n_taps = np.full(8, 1500, dtype=np.int32)
    decay = np.ones(64, dtype=np.float64)
    seed = np.zeros(8, dtype=np.int64)
    filt = np.zeros(4096, dtype=np.float64)
    status = np.zeros(8, dtype=np.int32)
    gain = np.zeros(64, dtype=np.float64)
    raw = np.zeros(4096, dtype=np.uint8)
    base = (raw.ctypes.data + 255) & ~255
    pr, pl, pn, pd, ps, pf, pt, pg = (a.ctypes.data for a in (rir, length, n_taps, decay, seed, filt, status, gain))

    def call(rir=pr, R=2, K=1500, ld=1500, length=pl, n_taps=pn, decay=pd, seed=ps, filt=pf, NB=2, NF=511, window=480, fs=16000,
             status=pt, gain=pg, ws=base, ws_bytes=256):
        rc = lib.cmgan_rir_tail(None, rir, R, K, ld, length, n_taps, decay, seed, filt, NB, NF, window, fs, status, gain, ws,
                                ws_bytes, None)
        return rc, (lib.cmgan_last_error(None) or b"").decode()

    cases = {
        "null pointer": [dict(rir=None), dict(length=None), dict(n_taps=None), dict(decay=None), dict(seed=None), dict(status=None),
                         dict(gain=None)],
        "4-byte aligned": [dict(rir=pr + 2), dict(length=pl + 1), dict(n_taps=pn + 2), dict(status=pt + 2)],
        "8-byte aligned": [dict(decay=pd + 4), dict(seed=ps + 4), dict(filt=pf + 4), dict(gain=pg + 4)],
        "need 1 <= R": [dict(R=0), dict(R=-3), dict(R=65536), dict(K=0), dict(K=-1), dict(ld=1499)],
        "need 0 <= NB": [dict(NB=-1), dict(NB=9)],
        "must be null with NB = 0 and only then": [dict(filt=None), dict(NB=0)],
        "filter length must be odd": [dict(NF=0), dict(NF=-1), dict(NF=510), dict(NF=1024)],
        "window must have 1 .. 4096 samples": [dict(window=0), dict(window=-480), dict(window=4097)],
        "fs must be positive": [dict(fs=0), dict(fs=-16000)],
        "workspace": [dict(ws=None), dict(ws=base + 64), dict(ws_bytes=255), dict(ws_bytes=0), dict(R=65, ws_bytes=256)],
    }
    for text, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == BADARG and text in msg, (kw, rc, msg)
    for text, kw in (("responses of up to 65536 taps", dict(K=65537, ld=65537)), ("filters of up to 1023 taps", dict(NF=1025))):
        rc, msg = call(**kw)
        assert rc == UNSUPPORTED and text in msg, (kw, rc, msg)
    # everything in order: only the handle is missing - nothing was enqueued, nothing was written
    for kw in (dict(), dict(filt=None, NB=0, NF=1), dict(filt=None, NB=0, NF=511), dict(NF=1), dict(NF=1023), dict(NB=8, R=1),
               dict(ld=4096), dict(fs=1), dict(window=1), dict(window=4096), dict(R=64)):
        rc, msg = call(**kw)
        assert rc == BADARG and "null handle" in msg, (kw, rc, msg)
    assert not rir.any() and not status.any() and not gain.any() and np.all(length == 1000)


# ------------------------------------------------------------------ Engine.rir_tail's argument rules
def test_check_rir_tail_args():
    rir = torch.zeros(3, 2000)
    i32 = torch.zeros(3, dtype=torch.int32)
    one = torch.ones(3, 1, dtype=torch.float64)
    seed = torch.zeros(3, dtype=torch.int64)
    filt = torch.zeros(7, 511, dtype=torch.float64)
    seven = torch.ones(3, 7, dtype=torch.float64)
    assert check_rir_tail_args(CPU, rir, i32, i32, one, seed) == (3, 2000, 0, 1, 480)
    assert check_rir_tail_args(CPU, rir, i32, i32, seven, seed, filt, 8000, 12.5) == (3, 2000, 7, 511, 100)
    assert check_rir_tail_args(CPU, torch.zeros(3, 2500)[:, :2000], i32, i32, one, seed, window_ms=0.05) == (3, 2000, 0, 1, 1)
    assert check_rir_tail_args(CPU, rir, i32, i32, one, seed, window_ms=256.0)[4] == 4096
    with pytest.raises(TypeError, match="rir: expected float32"):
        check_rir_tail_args(CPU, rir.double(), i32, i32, one, seed)
    with pytest.raises(RuntimeError, match="rir: tensor is on cpu"):
        check_rir_tail_args(torch.device("cuda:0"), rir, i32, i32, one, seed)
    with pytest.raises(ValueError, match="rir: rows of up to 65536 samples"):
        check_rir_tail_args(CPU, torch.zeros(1, 1).expand(1, 65537), i32[:1], i32[:1], one[:1], seed[:1])
    with pytest.raises(ValueError, match="rir: rows must be contiguous"):
        check_rir_tail_args(CPU, torch.zeros(3, 4000)[:, ::2], i32, i32, one, seed)
    for name, args in (("length", (None, i32)), ("n_taps", (i32, None))):
        with pytest.raises(TypeError, match=f"{name}: expected a torch.Tensor"):
            check_rir_tail_args(CPU, rir, *args, one, seed)
    with pytest.raises(TypeError, match="length: expected int32"):
        check_rir_tail_args(CPU, rir, i32.long(), i32, one, seed)
    with pytest.raises(ValueError, match="n_taps: expected \\[3\\]"):
        check_rir_tail_args(CPU, rir, i32, torch.zeros(4, dtype=torch.int32), one, seed)
    with pytest.raises(TypeError, match="decay: expected float64"):
        check_rir_tail_args(CPU, rir, i32, i32, one.float(), seed)
    for bad in (torch.ones(3, dtype=torch.float64), seven, torch.ones(2, 1, dtype=torch.float64)):
        with pytest.raises(ValueError, match="decay: expected \\[3, 1\\]"):
            check_rir_tail_args(CPU, rir, i32, i32, bad, seed)
    with pytest.raises(ValueError, match="decay: expected \\[3, 7\\]"):
        check_rir_tail_args(CPU, rir, i32, i32, one, seed, filt)
    with pytest.raises(TypeError, match="seed: expected int64"):
        check_rir_tail_args(CPU, rir, i32, i32, one, i32)
    with pytest.raises(ValueError, match="seed: expected \\[3\\]"):
        check_rir_tail_args(CPU, rir, i32, i32, one, torch.zeros(3, 1, dtype=torch.int64))
    with pytest.raises(TypeError, match="filters: expected float64"):
        check_rir_tail_args(CPU, rir, i32, i32, seven, seed, filt.float())
    for bad in (torch.zeros(511, dtype=torch.float64), torch.zeros(9, 511, dtype=torch.float64),
                torch.zeros(7, 510, dtype=torch.float64), torch.zeros(7, 1025, dtype=torch.float64)):
        with pytest.raises(ValueError, match="filters: expected \\[NB, NF\\]"):
            check_rir_tail_args(CPU, rir, i32, i32, seven, seed, bad)
    for fs in (0, -16000, 16000.5, True, 2 ** 31):
        with pytest.raises(ValueError, match="fs must be a positive sample rate"):
            check_rir_tail_args(CPU, rir, i32, i32, one, seed, None, fs)
    for ms in (0.0, 0.03, -1.0, 256.1, math.inf, math.nan):
        with pytest.raises(ValueError, match="window_ms must give a window of 1 .. 4096 samples"):
            check_rir_tail_args(CPU, rir, i32, i32, one, seed, None, 16000, ms)


# ------------------------------------------------------------------ RoomSampler(tail_ms=)
def _old_draw(sampler, R, K, fs):
    """RoomSampler.draw as it was before tail_ms, from the sampler's generator."""
    u = torch.rand(R, 10, dtype=torch.float64, generator=sampler.generator)
    lo, hi = torch.tensor(sampler.lo, dtype=torch.float64), torch.tensor(sampler.hi, dtype=torch.float64)
    size = lo + (hi - lo) * u[:, 0:3]
    inner = size - 2.0 * sampler.margin
    source, receiver = sampler.margin + inner * u[:, 3:6], sampler.margin + inner * u[:, 6:9]
    rt = sampler.rt60[0] + (sampler.rt60[1] - sampler.rt60[0]) * u[:, 9]
    rooms = torch.cat([size, source, receiver, sabine_beta(rt, size)[:, None].expand(R, 6)], dim=1).contiguous()
    return rooms, torch.ceil(rt * fs).clamp(1, K).to(torch.int32), rt


def test_room_sampler_tail_arguments():
    for bad in (0.0, -60.0, math.inf, math.nan, True, "60"):
        with pytest.raises(ValueError, match="tail_ms must be None or a positive, finite number"):
            RoomSampler(tail_ms=bad)
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="tail_window_ms must be"):
            RoomSampler(tail_ms=60.0, tail_window_ms=bad)
    plain = RoomSampler(generator=torch.Generator().manual_seed(1))
    assert plain.tail_ms is None
    rooms, _ = plain.draw(2, 8000, 16000)
    with pytest.raises(ValueError, match="has no tail_ms"):
        plain.draw_tail(rooms, 16000)
    s = RoomSampler(tail_ms=60.0, generator=torch.Generator().manual_seed(1))
    with pytest.raises(ValueError, match="draw_tail follows draw"):
        s.draw_tail(rooms, 16000)
    rooms, _ = s.draw(2, 8000, 16000)
    with pytest.raises(ValueError, match="rooms must be a float64 \\[R, 15\\]"):
        s.draw_tail(rooms.float(), 16000)
    with pytest.raises(ValueError, match="draw_tail follows draw"):
        s.draw_tail(rooms[:1], 16000)
    with pytest.raises(ValueError, match="sources must be the float64 \\[2, n, 15\\]"):
        s.draw_tail(rooms, 16000, rooms)
    # the fit window (and with bands the filterbank's delay) must fit between the direct sound and the junction
    for kw in (dict(tail_ms=20.0), dict(tail_ms=45.0, bands=7), dict(tail_ms=60.0, tail_window_ms=300.0)):
        t = RoomSampler(generator=torch.Generator().manual_seed(1), **kw)
        r, _ = t.draw(2, 8000, 16000)
        if t.bands:
            t.draw_bands(r)
        with pytest.raises(ValueError, match="must leave room for the fit window"):
            t.draw_tail(r, 16000)
    banded = RoomSampler(tail_ms=60.0, bands=7, generator=torch.Generator().manual_seed(1))
    r, _ = banded.draw(2, 8000, 16000)
    with pytest.raises(ValueError, match="draw_tail follows draw"):
        banded.draw_tail(r, 16000)                                # draw_bands first


def test_sampler_without_a_tail_draws_what_it_did():
    R, K, fs = 6, 8000, 16000
    new, old = (RoomSampler(generator=torch.Generator().manual_seed(7)) for _ in range(2))
    rooms, n_taps = new.draw(R, K, fs)
    want_rooms, want_taps, _ = _old_draw(old, R, K, fs)
    assert torch.equal(rooms, want_rooms) and torch.equal(n_taps, want_taps)
    assert torch.equal(new.draw_sources(rooms, 2), old.draw_sources(want_rooms, 2))
    assert torch.equal(torch.rand(4, generator=new.generator), torch.rand(4, generator=old.generator))     # the same state
    assert new.n_images(K, fs) == tuple(int(math.ceil((K + 40) * 343.0 / fs / (2.0 * l))) + 1 for l in new.lo)
    assert new.max_junction(K, fs) == K


def test_sampler_with_a_tail_draws_junctions_decays_and_seeds():
    R, K, fs, ms = 6, 16000, 16000, 60.0
    s, old = (RoomSampler(generator=torch.Generator().manual_seed(7), **kw) for kw in (dict(tail_ms=ms), dict()))
    rooms, junction = s.draw(R, K, fs)
    want_rooms, n_full, rt = _old_draw(old, R, K, fs)
    assert torch.equal(rooms, want_rooms)                          # the same rooms; only n_taps differs
    direct = (rooms[:, 3:6] - rooms[:, 6:9]).square().sum(dim=1).sqrt() / 343.0
    want = torch.minimum(torch.ceil((direct + ms / 1000.0) * fs).to(torch.int32), n_full)
    assert torch.equal(junction, want) and bool((junction < n_full).all()) and bool((junction >= 960).all())
    assert int(junction.max()) <= s.max_junction(K, fs) < K
    src = s.draw_sources(rooms, 3)
    assert torch.equal(src, old.draw_sources(want_rooms, 3))
    t = s.draw_tail(rooms, fs, src)
    assert torch.equal(t.n_full, n_full) and torch.equal(t.decay, rt[:, None]) and t.decay.is_contiguous()
    assert t.seed.dtype == torch.int64 and tuple(t.seed.shape) == (R,) and tuple(t.src_seed.shape) == (R, 3)
    assert torch.unique(torch.cat([t.seed, t.src_seed.flatten()])).numel() == 4 * R
    far = (src[:, :, 3:6] - src[:, :, 6:9]).square().sum(dim=2).sqrt() / 343.0
    assert torch.equal(t.src_junction, torch.minimum(torch.ceil((far + ms / 1000.0) * fs).to(torch.int32), n_full[:, None]))
    # the seeds are the generator's next draws, after every other one
    g = old.generator
    assert torch.equal(t.seed, torch.randint(0, 2 ** 63 - 1, (R,), dtype=torch.int64, generator=g))
    assert torch.equal(t.src_seed, torch.randint(0, 2 ** 63 - 1, (R, 3), dtype=torch.int64, generator=g))
    plain = s.draw_tail(rooms, fs)
    assert plain.src_junction is None and plain.src_seed is None and not torch.equal(plain.seed, t.seed)


def test_n_images_shrinks_to_the_junction():
    fs, K = 16000, 32000
    full, hybrid = RoomSampler(), RoomSampler(tail_ms=80.0)
    d = math.sqrt(sum((l - 1.0) ** 2 for l in full.hi))
    kj = int(math.ceil((d / 343.0 + 0.08) * fs))
    assert hybrid.max_junction(K, fs) == kj < K // 10
    assert hybrid.n_images(K, fs) == full.n_images(kj, fs)
    assert all(a < b for a, b in zip(hybrid.n_images(K, fs), full.n_images(K, fs)))
    assert hybrid.n_images(1000, fs) == full.n_images(1000, fs)   # a response shorter than any junction: nothing to save
    banded = RoomSampler(tail_ms=80.0, bands=7)
    assert banded.n_images(K, fs) == full.n_images(kj + 255, fs)


def test_band_decay_table_is_walls_and_air():
    R, K, fs = 5, 16000, 16000
    air = [(0.0, 0.0), (0.0001, 0.0002), (0.0002, 0.0004), (0.0005, 0.001), (0.001, 0.002), (0.002, 0.004), (0.004, 0.008)]
    kw = dict(bands=7, tilt=(0.1, 0.4), air=air)
    s, old = (RoomSampler(generator=torch.Generator().manual_seed(3), **k) for k in (dict(tail_ms=70.0, **kw), kw))
    rooms, _ = s.draw(R, K, fs)
    _, _, rt = _old_draw(old, R, K, fs)
    table = s.draw_bands(rooms)
    u = torch.rand(R, 8, dtype=torch.float64, generator=old.generator)               # draw_bands' one rand
    tilt = 0.1 + 0.3 * u[:, 0]
    lo, hi = (torch.tensor([a[i] for a in air], dtype=torch.float64) for i in (0, 1))
    assert s.band_ref == 3 and torch.equal(table[:, :, 6], lo + (hi - lo) * u[:, 1:])
    t = s.draw_tail(rooms, fs)
    assert tuple(t.decay.shape) == (R, 7)
    for r in range(R):
        for b in range(7):
            walls = float(rt[r]) * 2.0 ** (-float(tilt[r]) * (b - 3))
            want = 1.0 / (1.0 / walls + float(table[r, b, 6]) * 343.0 / (3.0 * math.log(10.0)))
            assert float(t.decay[r, b]) == pytest.approx(want, rel=1e-12)
    assert bool((t.decay[:, 0] > t.decay[:, 6]).all())             # absorption grows with frequency
    flat = RoomSampler(tail_ms=70.0, bands=3, generator=torch.Generator().manual_seed(3))
    rooms, _ = flat.draw(R, K, fs)
    flat.draw_bands(rooms)
    assert torch.equal(flat.draw_tail(rooms, fs).decay, rt[:, None].expand(R, 3))      # no tilt, no air: the rt60 itself


# ------------------------------------------------------------------ one acoustic check, on the model alone
ROOM = (5.0, 4.0, 2.7)
SOURCE, RECEIVER = (1.1, 1.3, 1.2), (3.4, 2.9, 1.6)
FS, RT60, W_FIT, AFTER_MS = 16000, 0.3, 480, 80.0


def _t30(y, k0):
    n = len(y)
    val, _, status, *_ = SM.slice_stats(y, np.zeros(n), k0, n, FS, *SM.offsets(FS, 2.5))
    assert status & SM.NO_T30 == 0
    return val[SM.T30]


def _junction_and_images(K, after_ms=AFTER_MS):
    direct = math.dist(SOURCE, RECEIVER) / 343.0
    kx = int(math.ceil((direct + after_ms / 1000.0) * FS))
    N = tuple(int(math.ceil((K + 40) * 343.0 / FS / (2.0 * l))) + 1 for l in ROOM)
    return kx, N


def test_hybrid_response_decays_at_the_given_time_broad_band():
    n_full = int(0.45 * FS)                                       # 90 dB of decay: the curve's bend lies below the T30 range
    kx, N = _junction_and_images(1800)
    beta = float(sabine_beta(RT60, torch.tensor(ROOM, dtype=torch.float64)))
    h, _, kr = RM.rir_row(np.array(ROOM + SOURCE + RECEIVER + (beta,) * 6), kx, n_full, N, FS)
    assert kr == kx and not h[kx:].any()
    m = M.rir_tail_row(h.astype(np.float32), kx, n_full, [RT60], 2024, None, W_FIT, FS, real=np.float64)
    assert m["status"] == 0 and m["length"] == n_full and m["gain"][0] > 0
    t30 = _t30(m["y"], int(np.argmax(np.abs(m["y"]))))
    assert abs(t30 / RT60 - 1.0) <= 0.10, t30


def test_hybrid_response_decays_at_the_given_time_in_every_band():
    """Every band's T30 within 15 % of its given time, by rir_stats_model's T30 on the ENSEMBLE of eight noise keys (the
    band energies of seeds 0 .. 7 added before the backward integral, as ISO 3382 averages decays): one realisation of the
    250 Hz band - 180 Hz wide - scatters by +-8 % about the figures below, which are the model's own.  The junction is 40 ms
    after the direct sound and not 80: the bound stays, the junction moved.  Measured here, T30 / given per band:
        junction 40 ms   1.054 1.116 1.016 1.002 1.025 1.031 1.121
        junction 60 ms   1.046 1.185 0.995 0.972 1.001 1.013 1.130
        junction 80 ms   1.037 1.222 0.877 0.978 0.997 1.023 1.205
        all images       1.383 1.354 1.292 1.009 0.907 0.927 0.882   (no tail: the image-source method to the end)
    The image-source response of this room decays 1.35 times slower than Sabine's time in the 250 Hz band, so the later
    the junction, the more of the -5 .. -35 dB range lies in that early part; the tail itself follows the given time."""
    NB, NF = 7, 511
    D = (NF - 1) // 2
    filt = octave_filterbank(FS, NB, NF).numpy()
    decay = RT60 * 2.0 ** (-0.3 * (np.arange(NB) - 3))
    n_full = int(0.75 * FS)                                       # band 0 is given 0.56 s
    kx, N = _junction_and_images(1200 + D, after_ms=40.0)
    size = torch.tensor(ROOM, dtype=torch.float64)
    bands = np.zeros((NB, 7))
    for b in range(NB):
        bands[b, 0:6] = float(sabine_beta(float(decay[b]), size))
    h, _, _, _, kr = BM.rir_bands_row(np.array(ROOM + SOURCE + RECEIVER + (0.0,) * 6), bands, kx, n_full, N, filt, FS)
    assert kr == kx
    assert kx - D - W_FIT >= 0
    energy = np.zeros((NB, n_full))
    for seed in range(8):
        m = M.rir_tail_row(h.astype(np.float32), kx, n_full, decay, seed, filt, W_FIT, FS, real=np.float64)
        assert m["status"] == 0 and np.all(m["gain"] > 0)
        for b in range(NB):
            energy[b] += np.convolve(m["y"], filt[b])[D:D + n_full] ** 2
    k0 = int(np.argmax(np.abs(m["y"])))
    ratios = [_t30(np.sqrt(energy[b]), k0) / decay[b] for b in range(NB)]
    print("T30 / given per band:", np.round(ratios, 3))
    assert all(abs(r - 1.0) <= 0.15 for r in ratios), ratios
