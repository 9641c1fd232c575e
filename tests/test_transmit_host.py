"""CPU side of the transmission stage (cmgan_amd/csrc/transmit.hip; include/cmgan_hip.h, "Transmission"): the G.711 maps of
the numpy model the GPU tests compare the kernels with (tests/transmit_model.py) against Python's audioop on every int16
value, the model against the facts the definition promises, the two conditions on every row the GPU tests judge, the
sampler's closed form against a serial walk of the chain over the same uniforms, and every argument error of
cmgan_transmit, Engine.transmit, TransmissionSampler and DynamicMixer(transmission=...), all of which are judged before
a handle or a GPU is needed."""
import math

import numpy as np
import pytest
import torch

import transmit_model as M
from cmgan_amd import _lib
from cmgan_amd.engine import TRANSMIT_CODECS, TRANSMIT_FRAME, TRANSMIT_LAG, TRANSMIT_WINDOW, check_transmit_args, transmit_scalars
from cmgan_amd.mixing import DynamicMixer, NoiseBank, TransmissionSampler, TransmitDraw

BADARG = -1
CPU = torch.device("cpu")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ G.711 against an independent implementation
def test_g711_maps_agree_with_audioop_on_every_int16_value():
    audioop = pytest.importorskip("audioop")
    q = np.arange(-32768, 32768, dtype=np.int16)
    raw = q.tobytes()
    assert np.array_equal(M.ulaw_encode(q), np.frombuffer(audioop.lin2ulaw(raw, 2), dtype=np.uint8))
    assert np.array_equal(M.alaw_encode(q), np.frombuffer(audioop.lin2alaw(raw, 2), dtype=np.uint8))
    codes = np.arange(256, dtype=np.uint8)
    assert np.array_equal(M.ulaw_decode(codes), np.frombuffer(audioop.ulaw2lin(codes.tobytes(), 2), dtype=np.int16))
    assert np.array_equal(M.alaw_decode(codes), np.frombuffer(audioop.alaw2lin(codes.tobytes(), 2), dtype=np.int16))
    x = (q.astype(np.float64) / 32768.0).astype(np.float32)
    for kind, there, back in ((M.ULAW, audioop.lin2ulaw, audioop.ulaw2lin), (M.ALAW, audioop.lin2alaw, audioop.alaw2lin)):
        want = np.frombuffer(back(there(raw, 2), 2), dtype=np.int16).astype(np.float64) / 32768.0
        assert np.array_equal(M.codec(x, kind).astype(np.float64), want)


def test_quantiser_rounds_half_to_even_and_saturates():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 32766.5, 32767.5, -32768.5, 1e9, -1e9], dtype=np.float64) / 32768.0
    assert M.quantise(x.astype(np.float32)).tolist() == [0, 2, 2, 0, -2, -2, 32766, 32767, -32768, 32767, -32768]
    assert M.quantise(np.array([np.nan, np.inf, -np.inf], dtype=np.float32)).tolist() == [0, 32767, -32768]
    nan = np.array([0x7FC12345], dtype=np.uint32).view(np.float32)
    assert np.array_equal(_bits(M.codec(nan, M.NONE)), _bits(nan)) and M.codec(nan, M.PCM16)[0] == 0.0
    x = M.speech(1, 500)
    assert np.array_equal(M.codec(x, M.PCM16), (np.rint(x.astype(np.float64) * 32768.0) / 32768.0).astype(np.float32))
    for kind in (M.ULAW, M.ALAW):                                        # companding: the error follows the signal
        err = np.abs(M.codec(x, kind).astype(np.float64) - x)
        assert err.max() < 0.04 * np.abs(x).max() and err.max() > 2.0 ** -15


# ------------------------------------------------------------------ the model against the definition's promises
def test_no_loss_and_no_codec_is_a_bit_copy():
    x = M.speech(2, 3000)
    res = M.transmit(x, 3000, np.zeros(10, dtype=np.uint8), M.NONE, 1)
    assert np.array_equal(_bits(res.y), _bits(x)) and not res.lag.any() and not res.runs and M.slack(res) == 0.0


def test_model_agrees_with_a_loop_over_single_samples():
    """The lag by plain Python sums, and the samples one at a time in Python floats (float64)."""
    F, pmin, pmax, W, A = 32, 16, 40, 24, 20
    x = M.speech(3, 400, f0=500.0)
    lost = M.table(13, 0, 4, 5, 9, 12)
    res = M.transmit(x, 400, lost, M.NONE, 1, F, pmin, pmax, W, A)
    y = [float(v) for v in x]
    h = lambda i: y[i] if i >= 0 else 0.0
    for k0, k1 in M.runs(lost, 13):
        s, e = k0 * F, min(k1 * F, 400)
        best, P = -math.inf, pmin
        for p in range(pmin, pmax + 1):
            C = E = 0.0
            for i in range(W):
                C += h(s - W + i) * h(s - W - p + i)
                E += h(s - W - p + i) ** 2
            sc = 2.0 * C - E
            if sc > best:
                best, P = sc, p
        assert res.lag[k0] == P
        Q = P // 4
        v = [h(s - P + i) for i in range(P)]
        for i in range(P - Q, P):
            t = (i - (P - Q) + 1) / (Q + 1)
            v[i] = (1.0 - t) * h(s - P + i) + t * h(s - 2 * P + i)
        g = lambda j: min(1.0, max(0.0, (6 * A - j) / (5 * A)))
        M_ = e - s
        R = min(Q, F, 400 - e) if e < 400 else 0
        new = [g(j) * v[j % P] for j in range(M_)]
        for i in range(R):
            t = (i + 1) / (R + 1)
            new.append((1.0 - t) * (g(M_ + i) * v[(M_ + i) % P]) + t * y[e + i])
        for j, val in enumerate(new):
            assert val == res.d[s + j], (k0, j)
            y[s + j] = float(np.float32(res.w[s + j]))
    assert np.array_equal(np.array(y, dtype=np.float32), res.y)
    assert res.lag[0] == pmin and not res.y[:F].any()                    # a run at the start of the row: zeros
    assert (res.lag[[1, 2, 3, 5, 6, 7, 8, 10, 11]] == 0).all() and res.lag[4] > 0 and res.lag[9] > 0 and res.lag[12] > 0


def test_concealment_repeats_the_pitch_period_and_fades():
    x = M.periodic(4, 4000, 100)
    res = M.transmit(x, 4000, M.table(13, 4, 5, 6, 7, 8), M.NONE, 1)
    s = 4 * 320
    assert res.lag[4] == 100                                             # the smallest of the equal maxima 100, 200
    assert np.array_equal(_bits(res.y[s:s + 160]), _bits(x[s:s + 160]))  # an exact period continues bit for bit while g = 1
    assert np.abs(res.y[s + 160:s + 960]).max() < np.abs(x).max() and not res.y[s + 960:s + 1600].any()
    env = np.abs(res.y[s:s + 1000].astype(np.float64)).reshape(10, 100).max(axis=1)
    assert np.all(np.diff(env[1:]) < 0)
    gap = M.transmit(x, 4000, M.table(13, 4, 5, 6, 7, 8), M.NONE, 0)
    assert not gap.y[s:s + 1600].any() and np.array_equal(gap.y[:s], x[:s]) and np.array_equal(gap.y[s + 1600:], x[s + 1600:])
    assert np.array_equal(res.y[s + 1600 + 320:], x[s + 1600 + 320:])    # the fade back stays inside the next frame
    assert M.gain(np.array([0, 160, 161, 320, 959, 960, 5000]), 160).tolist() == [1.0, 1.0, 799 / 800, 0.8, 1 / 800, 0.0, 0.0]


def test_every_row_of_the_gpu_tests_respects_both_conditions():
    """The rule |g - w| <= ulp32(w) / 2 + E may be used on a row only if E <= 2^-10 x ulp32(rms) / 2, and only if every
    searched run is a tie by construction or is decided by at least 2^-12 of its window's energy."""
    rows = M.build_rows()
    assert len(rows) > 40
    top, tight, thin, n_runs = 0.0, 0.0, math.inf, 0
    for key, row in rows.items():
        res, E = M.case(key)
        bound = M.condition(res)
        assert len(res.w) == row.n and len(res.lag) == -(-row.n // row.F), key
        assert E <= bound, f"{key}: E = {E:.3e} above {bound:.3e}"
        assert M.margins_ok(res, row.tie), f"{key}: {[(r.lag, r.margin, M.MARGIN * r.energy) for r in res.runs]}"
        top, tight = max(top, E), max(tight, E / bound)
        for r in res.runs:
            if r.lag and not row.tie and r.energy > 0 and math.isfinite(r.margin):
                thin, n_runs = min(thin, r.margin / (M.MARGIN * r.energy)), n_runs + 1
    print(f"[transmit] {len(rows)} rows: largest E {top:.3e}, at most {tight:.2e} of the bound; {n_runs} searched runs, the "
          f"thinnest margin {thin:.1f} x the bound")
    res = M.case("tie-period")[0]
    assert res.runs[0].lag == 100 and res.runs[0].margin == 0.0         # the tie is exact
    assert [r.lag for r in M.case("bench-pattern")[0].runs] == [125, 115, 155, 112, 143]


# ------------------------------------------------------------------ the sampler
def _serial(u, p_gb, q):
    lost = np.zeros(u.shape, dtype=np.uint8)
    for b in range(u.shape[0]):
        bad = False
        for k in range(u.shape[1]):
            if u[b, k] < p_gb[b]:
                bad = True
            elif u[b, k] >= 1.0 - q[b]:
                bad = False
            lost[b, k] = bad
    return lost


@pytest.mark.parametrize("kw", [dict(p=1.0, loss=(0.01, 0.3), burst=(1.0, 6.0)), dict(p=1.0, loss=(0.3, 0.6), burst=(1.0, 1.2)),
                                dict(p=1.0, loss=(0.0, 0.0), burst=(2.0, 2.0)), dict(p=0.0), dict(p=0.5)])
def test_sampler_pattern_is_the_serial_chain(kw):
    B, n = 24, 300
    gen = torch.Generator().manual_seed(11)
    d = TransmissionSampler(generator=gen, **kw).draw(B, n)
    assert isinstance(d, TransmitDraw) and d.lost.dtype == torch.uint8 and tuple(d.lost.shape) == (B, n) and d.lost.is_contiguous()
    assert d.codec.dtype == torch.int32 and d.plc.dtype == torch.int32 and d.rate.dtype == torch.float64 and d.burst.dtype == torch.float64
    u = torch.rand(B, 5 + n, dtype=torch.float64, generator=torch.Generator().manual_seed(11)).numpy()
    rate, burst = d.rate.numpy(), d.burst.numpy()
    q = 1.0 / burst
    p_gb = rate * q / (1.0 - rate)
    assert np.array_equal(d.lost.numpy(), _serial(u[:, 5:], p_gb, q))
    chosen = u[:, 0] < kw.get("p", 0.5)
    assert (rate[~chosen] == 0).all() and not d.lost.numpy()[~chosen].any() and not d.codec.numpy()[~chosen].any()
    assert (burst >= 1.0 / (1.0 - rate)).all() and (p_gb <= 1.0 - q + 1e-15).all()
    if kw.get("loss") == (0.3, 0.6):                                     # the burst was raised: independent loss
        assert np.allclose(burst, 1.0 / (1.0 - rate)) and np.array_equal(d.lost.numpy(), (u[:, 5:] < rate[:, None]).astype(np.uint8))
    if kw.get("loss") == (0.0, 0.0) or kw.get("p") == 0.0:
        assert not d.lost.any()
    assert set(d.codec.tolist()) <= {0, 1, 2, 3} and set(d.plc.tolist()) <= {0, 1}


def test_sampler_statistics_and_options():
    gen = torch.Generator().manual_seed(5)
    d = TransmissionSampler(p=1.0, loss=(0.1, 0.1), burst=(3.0, 3.0), p_conceal=1.0, p_pcm16=0.0, p_ulaw=1.0, p_alaw=0.0,
                            generator=gen).draw(64, 4000)
    lost = d.lost.numpy()
    assert abs(lost.mean() - 0.1) < 0.01 and (d.codec == 2).all() and (d.plc == 1).all()
    starts = (np.diff(np.concatenate([np.zeros((64, 1), dtype=np.int8), lost.astype(np.int8)], axis=1), axis=1) == 1).sum()
    assert abs(lost.sum() / starts - 3.0) < 0.15                         # the mean burst length
    assert not lost[:, 0].all()                                          # the chain starts in the good state
    assert TransmissionSampler().frame(16000) == 320 and TransmissionSampler(frame_ms=10.0).frame(8000) == 80
    assert tuple(TransmissionSampler().draw(3, 0).lost.shape) == (3, 0)
    for bad in (-0.1, 1.5, math.nan):
        for name in ("p", "p_conceal", "p_pcm16", "p_ulaw", "p_alaw"):
            with pytest.raises(ValueError, match=f"{name} must lie in"):
                TransmissionSampler(**{name: bad})
    with pytest.raises(ValueError, match="p_pcm16 \\+ p_ulaw \\+ p_alaw must not exceed 1"):
        TransmissionSampler(p_pcm16=0.5, p_ulaw=0.4, p_alaw=0.2)
    for bad in ((0.1, 1.0), (-0.1, 0.2), (0.3, 0.2), (math.nan, 0.5), 0.1, (0.1,)):
        with pytest.raises(ValueError, match="loss must be"):
            TransmissionSampler(loss=bad)
    for bad in ((0.5, 2.0), (3.0, 2.0), (1.0, math.inf), (math.nan, 2.0), 2.0):
        with pytest.raises(ValueError, match="burst must be"):
            TransmissionSampler(burst=bad)
    for bad in (0.0, -20.0, math.inf, math.nan, True, "20"):
        with pytest.raises(ValueError, match="frame_ms must be"):
            TransmissionSampler(frame_ms=bad)


# ------------------------------------------------------------------ the library without a GPU
def test_symbols_and_constants():
    lib = _lib.load()
    for name in ("cmgan_transmit", "cmgan_transmit_max_lag", "cmgan_transmit_max_window"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.cmgan_transmit_max_lag() == TRANSMIT_LAG[1] == 1024 and TRANSMIT_LAG[0] == 16
    assert lib.cmgan_transmit_max_window() == TRANSMIT_WINDOW[1] == 1024 and TRANSMIT_WINDOW[0] == 16
    assert TRANSMIT_FRAME == (16, 4096) and TRANSMIT_CODECS == {"none": M.NONE, "pcm16": M.PCM16, "ulaw": M.ULAW, "alaw": M.ALAW}
    assert lib.cmgan_abi_version() == _lib.ABI_VERSION >= 22
    assert transmit_scalars(16000) == (M.F_D, M.PMIN_D, M.PMAX_D, M.W_D, M.A_D) == (320, 80, 240, 320, 160)
    assert transmit_scalars(8000) == (160, 40, 120, 160, 80) and transmit_scalars(48000, pmax=1000) == (960, 240, 1000, 960, 480)
    import cmgan_amd.mixing as mixing
    assert {"TransmissionSampler", "TransmitDraw", "TransmitInfo"} <= set(mixing.__all__)


def test_library_rejects_bad_arguments_before_it_needs_a_handle():
    lib = _lib.load()
    x = np.zeros(8192, dtype=np.float32)
    y = np.zeros(8192, dtype=np.float32)
    lengths, codec, plc = (np.zeros(8, dtype=np.int32) for _ in range(3))
    status = np.full(8, 7, dtype=np.int32)
    lag = np.full(64, 7, dtype=np.int32)
    lost = np.zeros(64, dtype=np.uint8)
    px, py, pl, pc, pp, pt, pg, po = (a.ctypes.data for a in (x, y, lengths, codec, plc, status, lag, lost))

    def call(x=px, B=2, L=1500, ldx=1500, lengths=pl, lost=po, ldl=5, codec=pc, plc=pp, frame=320, pmin=80, pmax=240, window=320,
             fade=160, y=py, ldy=1600, status=pt, lag=pg):
        rc = lib.cmgan_transmit(None, x, B, L, ldx, lengths, lost, ldl, codec, plc, frame, pmin, pmax, window, fade, y, ldy, status,
                                lag, None)
        return rc, (lib.cmgan_last_error(None) or b"").decode()

    cases = {
        "null pointer": [dict(x=None), dict(lost=None), dict(codec=None), dict(plc=None), dict(y=None)],
        "4-byte aligned": [dict(x=px + 2), dict(y=py + 1), dict(lengths=pl + 1), dict(codec=pc + 2), dict(plc=pp + 3),
                           dict(status=pt + 2), dict(lag=pg + 1)],
        "need 1 <= B": [dict(B=0), dict(B=-3), dict(B=65536), dict(L=0), dict(L=-1), dict(ldx=1499), dict(ldy=1499)],
        "frame must lie": [dict(frame=15), dict(frame=4097), dict(frame=0), dict(frame=-320)],
        "<= pmin <= pmax <=": [dict(pmin=15), dict(pmax=1025), dict(pmin=241), dict(pmin=0, pmax=0), dict(pmin=-80)],
        "window must lie": [dict(window=15), dict(window=1025), dict(window=0)],
        "fade must be": [dict(fade=0), dict(fade=-160)],
        "ldl must be at least": [dict(ldl=4), dict(ldl=0), dict(ldl=-1), dict(frame=16, ldl=93)],
        "overlap": [dict(y=px + 4), dict(y=px + 4 * 1500), dict(y=px + 4 * 2999), dict(x=py + 4 * 100), dict(x=py + 4 * 3099),
                    dict(y=px, ldy=1500, ldx=1501), dict(y=px, ldy=1600)],
    }
    for text, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == BADARG and "cmgan_transmit" in msg and text in msg, (kw, rc, msg)
    # everything in order: only the handle is missing - nothing was enqueued, nothing was written
    for kw in (dict(), dict(lengths=None), dict(status=None), dict(lag=None), dict(y=px, ldy=1500), dict(lost=po + 1),
               dict(frame=16, ldl=94), dict(frame=4096, ldl=1), dict(pmin=16, pmax=16), dict(pmin=1024, pmax=1024),
               dict(window=16), dict(window=1024), dict(fade=1), dict(fade=2 ** 31 - 1), dict(y=px + 4 * 3000),
               dict(x=py + 4 * 3100), dict(B=1, L=1, ldx=1, ldy=1, ldl=1), dict(ldx=2000, ldy=2000)):
        rc, msg = call(**kw)
        assert rc == BADARG and "null handle" in msg, (kw, rc, msg)
    assert not y.any() and (status == 7).all() and (lag == 7).all()


# ------------------------------------------------------------------ Engine.transmit's argument rules
def test_check_transmit_args():
    wav = torch.zeros(3, 2000)
    u8 = lambda n=7: torch.zeros(3, n, dtype=torch.uint8)
    i32 = lambda n=3: torch.zeros(n, dtype=torch.int32)
    assert check_transmit_args(CPU, wav, u8()) == (3, 2000, 320, 80, 240, 320, 160)
    assert check_transmit_args(CPU, wav, u8(9), None, i32(), i32(), i32()) == (3, 2000, 320, 80, 240, 320, 160)
    assert check_transmit_args(CPU, wav, u8(13), 160, fs=8000) == (3, 2000, 160, 40, 120, 160, 80)
    assert check_transmit_args(CPU, wav, u8(125), 16, pmin=16, pmax=64, window=64, fade=8) == (3, 2000, 16, 16, 64, 64, 8)
    assert check_transmit_args(CPU, wav, torch.zeros(3, 20, dtype=torch.uint8)[:, :7], out=wav)[0] == 3
    assert check_transmit_args(CPU, wav, u8(), out=torch.zeros(3, 2500)[:, :2000])[1] == 2000
    assert check_transmit_args(CPU, torch.zeros(3, 2500)[:, :2000], u8())[1] == 2000
    raises = lambda text: pytest.raises(ValueError, match=text)
    with raises("wav: expected a torch.Tensor"):
        check_transmit_args(CPU, np.zeros((3, 2000), dtype=np.float32), u8())
    with raises("wav: expected float32"):
        check_transmit_args(CPU, wav.double(), u8())
    with raises("wav: tensor is on cpu"):
        check_transmit_args(torch.device("cuda:0"), wav, u8())
    for bad in (torch.zeros(2000), torch.zeros(1, 3, 2000), torch.zeros(0, 2000), torch.zeros(3, 0)):
        with raises("wav: expected \\[B, L\\]"):
            check_transmit_args(CPU, bad, u8())
    with raises("at most 65535 rows"):
        check_transmit_args(CPU, torch.zeros(1, 1).expand(65536, 1), u8())
    for bad in (torch.zeros(3, 4000)[:, ::2], torch.zeros(2000, 3).t()):
        with raises("wav: rows must be contiguous"):
            check_transmit_args(CPU, bad, u8())
    with raises("lost: expected a torch.Tensor"):
        check_transmit_args(CPU, wav, None)
    for bad in (torch.zeros(3, 7, dtype=torch.bool), torch.zeros(3, 7, dtype=torch.int32), torch.zeros(3, 7)):
        with raises("lost: expected uint8"):
            check_transmit_args(CPU, wav, bad)
    for bad in (u8(6), torch.zeros(2, 7, dtype=torch.uint8), torch.zeros(21, dtype=torch.uint8)):
        with raises("lost: expected \\[3, n_frames\\] with n_frames >= ceil\\(L / frame\\) = 7"):
            check_transmit_args(CPU, wav, bad)
    with raises("lost: expected .* = 13"):
        check_transmit_args(CPU, wav, u8(12), 160)
    for bad in (torch.zeros(3, 14, dtype=torch.uint8)[:, ::2], torch.zeros(7, 3, dtype=torch.uint8).t()):
        with raises("lost: rows must be contiguous"):
            check_transmit_args(CPU, wav, bad)
    for name, pos in (("codec", 0), ("plc", 1), ("lengths", 2)):
        args = [None, None, None]
        for bad, text in ((torch.zeros(3, dtype=torch.int64), "expected int32"), (2, "expected a torch.Tensor"),
                          (i32(4), "expected \\[3\\]"), (torch.zeros(6, dtype=torch.int32)[::2], "must be contiguous")):
            args[pos] = bad
            with raises(f"{name}: {text}"):
                check_transmit_args(CPU, wav, u8(), None, *args)
    for bad in (0, -16000, 16000.5, True):
        with raises("fs must be"):
            check_transmit_args(CPU, wav, u8(), fs=bad)
    for name, values in (("frame", (15, 4097, 320.5, True)), ("pmin", (15, 1025, 80.5, True)), ("pmax", (15, 1025, True)),
                         ("window", (15, 1025, True)), ("fade", (0, -1, 0.5, True))):
        for bad in values:
            with raises(f"{name} must be a whole number"):
                check_transmit_args(CPU, wav, torch.zeros(3, 200, dtype=torch.uint8), **{name: bad})
    with raises("pmin must not exceed pmax"):
        check_transmit_args(CPU, wav, u8(), pmin=200, pmax=100)
    with raises("pmax must be a whole number in \\[16, 1024\\], got 1440 \\(the default at fs = 96000\\)"):
        check_transmit_args(CPU, wav, u8(), fs=96000)
    with raises("frame must be a whole number .* \\(the default at fs = 500\\)"):
        check_transmit_args(CPU, wav, torch.zeros(3, 200, dtype=torch.uint8), fs=500)
    with raises("out: expected float32"):
        check_transmit_args(CPU, wav, u8(), out=torch.zeros(3, 2000, dtype=torch.float64))
    with raises("out: expected \\[3, 2000\\]"):
        check_transmit_args(CPU, wav, u8(), out=torch.zeros(3, 2001))
    with raises("out: rows must be contiguous"):
        check_transmit_args(CPU, wav, u8(), out=torch.zeros(3, 4000)[:, ::2])
    big = torch.zeros(3, 2600)
    with raises("out: overlaps wav"):
        check_transmit_args(CPU, big[:, :2000], u8(), out=big[:, 500:2500])
    with raises("out: overlaps wav"):
        check_transmit_args(CPU, big[:, :2000], u8(), out=big.view(-1)[:6000].view(3, 2000))


# ------------------------------------------------------------------ DynamicMixer's new arguments
class _NoEngine:
    device = CPU


def _bank():
    return NoiseBank.from_arrays([np.ones(100, dtype=np.float32), np.ones(50, dtype=np.float32)])


def test_mixer_rejects_bad_transmission_options():
    bank = _bank()
    mk = lambda **kw: DynamicMixer(_NoEngine(), bank, **kw)
    for bad in ("clean", "target", None, True):
        with pytest.raises(ValueError, match="transmission_on must be 'noisy' or 'both'"):
            mk(transmission_on=bad)
    for bad in (0.5, "gsm", (0.01, 0.2), TransmissionSampler):
        with pytest.raises(TypeError, match="transmission must be a TransmissionSampler or None"):
            mk(transmission=bad)
    with pytest.raises(ValueError, match="transmission at sample_rate = 16000: frame must be"):
        mk(transmission=TransmissionSampler(frame_ms=0.5))
    with pytest.raises(ValueError, match="transmission at sample_rate = 96000: pmax must be"):
        mk(transmission=TransmissionSampler(), sample_rate=96000)
    m = mk()
    assert m.transmission is None and m.transmission_on == "noisy" and m.last_transmission is None
    s = TransmissionSampler()
    m = mk(transmission=s, transmission_on="both")
    assert m.transmission is s and m.transmission_on == "both" and m.last_transmission is None
