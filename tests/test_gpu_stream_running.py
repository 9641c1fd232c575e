"""Carried-state streaming with RUNNING InstanceNorm statistics (stats_mode="running"; include/cmgan_hip.h, "Streaming";
cmgan_amd/csrc/in_running.hip) on the GPU: against the CPU model of the contract (tests/stream_running_model.py), graph
replay / eager / pipelined runs bit for bit, the sums reset per stream, frozen and running streams side by side on one
engine, one window = the plain forward, the live front end, lock-step rows and the 48 kHz configuration."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import GOLDEN, assert_close, rel_err
from oracle.weights import make_state_dict, synthetic_clips

import stream_running_model as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STAGE = 2e-4
MODES = ["f16x3", "f32"]
_CPU = {}


def _report(name, err):
    print(f"[running] {name}: rel_err = {err:.3e}")
    return err


def _check(name, got, want, gate=STAGE, rtol=1e-3, atol_rel=2e-5):
    """test_gpu_parity._check: max-norm relative error under `gate` AND the elementwise bound."""
    assert _report(name, rel_err(got, want)) < gate, name
    assert_close(got, want, rtol=rtol, atol_rel=atol_rel, name=name)


def _once(key, fn):
    if key not in _CPU:
        _CPU[key] = fn()
    return _CPU[key]


@pytest.fixture(scope="module")
def sd():
    return make_state_dict(seed=0, num_features=201)


@pytest.fixture(scope="module", params=MODES)
def model(request, sd):
    from cmgan_amd import TSCNet
    return TSCNet(num_channel=64, num_features=201, mfma_mode=request.param).cuda().load_state_dict(sd).eval()


def _silence_track():
    z = np.load(f"{GOLDEN}/tracks.npz")
    pcm = torch.from_numpy(z["pcm_silence"].astype(np.float32) / 32768.0)[None]
    return pcm[:, :pcm.size(1) // 100 * 100].contiguous()


@pytest.mark.parametrize("la", [8, 0])
def test_enhance_stream_running_matches_the_model_and_every_run_form_gives_the_same_bits(model, sd, la):
    """1.6 s in 40-frame windows, context 12: five steps of three shapes.  The pipelined graphs (the default), one
    graph per step, eager launches and a second pipelined run of the same clip give the same bits - the sums are
    reduced in a fixed order and reset when a stream claims its slot."""
    from cmgan_amd.streaming import enhance_stream
    wav = synthetic_clips(1, 16000, seed=33)
    want = _once(("syn", la), lambda: R.enhance_stream(sd, wav, window=40, context=12, lookahead=la)[0])
    kw = dict(window=40, context=12, lookahead=la, stats_mode="running")
    got = enhance_stream(model, wav.to(DEV), **kw)
    _check(f"enhance_stream running la={la} [{model.engine.mfma_mode}] vs model", got, want)
    again = enhance_stream(model, wav.to(DEV), **kw)
    stepped = enhance_stream(model, wav.to(DEV), pipeline=False, **kw)
    eager = enhance_stream(model, wav.to(DEV), graph=False, **kw)
    assert torch.equal(again, got) and torch.equal(stepped, got) and torch.equal(eager, got)
    # and it is not the frozen stream
    assert not torch.equal(enhance_stream(model, wav.to(DEV), window=40, context=12, lookahead=la), got)


def test_a_recording_that_starts_in_silence(model):
    """tracks.npz `silence` (3.5 s, digital silence first) in 100-frame windows: where a frozen blob calibrated on the
    first window is furthest off (tests/golden/stream_running_cost.json)."""
    from cmgan_amd.streaming import enhance_stream
    sd0, la = make_state_dict(seed=0), 0
    pcm = _silence_track()
    want = _once(("silence", la), lambda: R.enhance_stream(sd0, pcm, window=100, context=40, lookahead=la)[0])
    got = enhance_stream(model, pcm.to(DEV), window=100, context=40, lookahead=la, stats_mode="running")
    _check(f"track_silence w100 l{la} [{model.engine.mfma_mode}] vs model", got, want)


def _drive(model, spec, states, W, La):
    """Step every StreamState of `states` through spec [B,2,T,F] in turn (interleaved on one engine)."""
    eng = model.engine
    T = spec.size(2)
    outs = [(torch.empty(spec.size(0), 1, T, eng.F, device=DEV), torch.empty(spec.size(0), 1, T, eng.F, device=DEV))
            for _ in states]
    k, fed = 0, 0
    while fed < T:
        upto = min((k + 1) * W + La, T)
        for st, (r, i) in zip(states, outs):
            st.step(spec[:, :, fed:upto].contiguous(), last=upto == T, out=(r[:, :, k * W:], i[:, :, k * W:]))
        fed, k = upto, k + 1
    return outs


def test_frozen_and_running_streams_interleaved_on_one_engine(model):
    """Two live streams of the same shape, one per statistics mode, stepped alternately: each gives the bits of its
    own stream run alone (enhance_stream, one graph per step)."""
    from cmgan_amd.streaming import StreamState, enhance_stream
    eng = model.engine
    wav = synthetic_clips(1, 16000, seed=41).to(DEV)
    kw = dict(window=40, context=12, lookahead=8)
    c = eng.rms_scale(wav)
    spec = eng.stft_compress(wav, c)
    stats = eng.tscnet_forward_stats(spec[:, :, :48].contiguous())[2]
    want_f = enhance_stream(model, wav, stats=stats, pipeline=False, **kw)
    want_r = enhance_stream(model, wav, stats_mode="running", pipeline=False, **kw)
    st_f = StreamState(model, stats, 1, 40, 12, 8)
    st_r = StreamState(model, None, 1, 40, 12, 8, stats_mode="running")
    (rf, jf), (rr, jr) = _drive(model, spec, [st_f, st_r], 40, 8)
    got_f = (eng.uncompress_istft(rf, jf) / c[:, None]).reshape(-1)
    got_r = (eng.uncompress_istft(rr, jr) / c[:, None]).reshape(-1)
    assert torch.equal(got_f, want_f) and torch.equal(got_r, want_r)


def test_one_window_covering_the_clip_is_the_plain_forward(model):
    """window >= T on fresh sums: the reference arithmetic on the clip, up to the fp64 summation order (in_running's
    chunks vs in_finalize's tiles); the blobs the two halves report are the forward's own statistics."""
    from cmgan_amd.streaming import enhance_stream
    eng = model.engine
    wav = synthetic_clips(1, 6000, seed=35).to(DEV)
    want = eng.enhance(wav)[0]
    for graph in (False, True):
        got = enhance_stream(model, wav, window=64, context=8, lookahead=8, graph=graph, stats_mode="running")
        assert _report(f"one window, graph={graph} [{eng.mfma_mode}] vs enhance()", rel_err(got, want)) < 1e-5
    spec = eng.stft_compress(wav)
    _, _, blob = eng.tscnet_forward_stats(spec)
    sums = torch.zeros(eng.stream_sums_doubles(1), dtype=torch.float64, device=DEV)
    used = torch.full((eng.stats_floats(1),), float("nan"), device=DEV)
    x = eng.stream_encoder_running(spec, 0, sums, stats_out=used)
    eng.stream_tscb(x)
    eng.stream_decoder_running(x, spec, 0, sums, stats_out=used)
    assert torch.isfinite(used).all()
    assert _report("stats_out of one running step vs the forward's blob", rel_err(used, blob)) < 1e-5
    counts = sums.view(-1, 3)[:, 0]                          # n of every (norm, channel): T x (bins of that norm)
    T, F, F2 = spec.size(2), eng.F, (eng.F + 1) // 2
    per_norm = [T * F] * 5 + [T * F2] * 9 + [T * 2 * F2]
    want_n = torch.tensor([n for n in per_norm for _ in range(64)] + [T * F], dtype=torch.float64, device=DEV)
    assert torch.equal(counts, want_n)


def test_streaming_enhancer_running_on_ragged_chunks_equals_enhance_stream(model):
    """The live front end needs no statistics blob in running mode; fed ragged chunks it returns enhance_stream's
    samples to rounding (the 1.5e-6 tile effect of the split-f16 transforms, see StreamingEnhancer)."""
    from cmgan_amd.streaming import StreamingEnhancer, enhance_stream
    eng = model.engine
    wav = synthetic_clips(1, 16000, seed=37).to(DEV)
    c = eng.rms_scale(wav)
    want = enhance_stream(model, wav, window=40, context=12, lookahead=8, graph=False, stats_mode="running")
    for sizes in ((1600,) * 10, (137, 3333, 50, 4000, 1, 2479, 6000)):
        live = StreamingEnhancer(model, window=40, context=12, lookahead=8, scale=c, stats_mode="running")
        out, pos = [], 0
        for n in sizes:
            out.append(live.push(wav[0, pos:pos + n]))
            pos += n
        out.append(live.flush())
        got = torch.cat(out)
        assert got.shape == want.shape
        assert _report(f"StreamingEnhancer running in {len(sizes)} chunks", rel_err(got, want)) < 1e-5, sizes
    with pytest.raises(ValueError):
        StreamingEnhancer(model, window=40, context=12, lookahead=8)            # frozen mode still needs its blob


def test_lock_step_rows_equal_their_single_streams(model):
    """B = 2 streams in lock-step: each row carries its own sums and gives the bits of its B = 1 stream."""
    from cmgan_amd.streaming import StreamState
    eng = model.engine
    wav = synthetic_clips(2, 12000, seed=43).to(DEV)
    spec = eng.stft_compress(wav, eng.rms_scale(wav))
    for graph in (True, False):
        (r2, i2), = _drive(model, spec, [StreamState(model, None, 2, 30, 10, 6, graph=graph, stats_mode="running")], 30, 6)
        for b in range(2):
            (r1, i1), = _drive(model, spec[b:b + 1].contiguous(),
                               [StreamState(model, None, 1, 30, 10, 6, graph=graph, stats_mode="running")], 30, 6)
            assert torch.equal(r2[b:b + 1], r1) and torch.equal(i2[b:b + 1], i1), (graph, b)


@pytest.mark.parametrize("mode", MODES)
def test_48k_running_stream_matches_the_model(mode):
    """n_fft 1200 / hop 300 (F = 601): 0.5 s in 30-frame windows."""
    from cmgan_amd import TSCNet
    from cmgan_amd.streaming import enhance_stream
    sd48 = make_state_dict(seed=5, num_features=601)
    m48 = TSCNet(64, 601, mfma_mode=mode).load_state_dict(sd48).eval()
    wav = synthetic_clips(1, 24000, seed=47)
    want = _once("48k", lambda: R.enhance_stream(sd48, wav, window=30, context=8, lookahead=6, n_fft=1200, hop=300)[0])
    got = enhance_stream(m48, wav.to(DEV), window=30, context=8, lookahead=6, stats_mode="running")
    _check(f"48k running stream [{mode}] vs model", got, want)


def test_running_arguments_are_checked_before_anything_runs(model):
    from cmgan_amd.streaming import enhance_stream
    eng = model.engine
    wav = synthetic_clips(1, 6000, seed=35).to(DEV)
    with pytest.raises(ValueError):
        enhance_stream(model, wav, window=40, stats=torch.zeros(eng.stats_floats(1), device=DEV), stats_mode="running")
    with pytest.raises(ValueError):
        enhance_stream(model, wav, window=40, calib_frames=20, stats_mode="running")
    with pytest.raises(ValueError):
        enhance_stream(model, wav, window=40, stats_mode="adaptive")
    spec = eng.stft_compress(wav)
    T = spec.size(2)
    sums = torch.zeros(eng.stream_sums_doubles(1), dtype=torch.float64, device=DEV)
    x = torch.zeros(1, T, (eng.F + 1) // 2, 64, device=DEV)
    out = torch.zeros(1, 1, T, eng.F, device=DEV)
    ws = eng._workspace(1, T)
    lib, h, s = eng.lib, eng._h, eng._stream()
    BADARG = -1
    for hist in (-1, T, T + 5):
        assert lib.cmgan_stream_encoder_running(h, spec.data_ptr(), 1, T, hist, sums.data_ptr(), None, x.data_ptr(),
                                                ws.data_ptr(), ws.numel(), s) == BADARG
        assert lib.cmgan_stream_decoder_running(h, x.data_ptr(), spec.data_ptr(), 1, T, hist, sums.data_ptr(), None,
                                                out.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), s) == BADARG
    assert lib.cmgan_stream_encoder_running(h, spec.data_ptr(), 1, T, 0, None, None, x.data_ptr(), ws.data_ptr(),
                                            ws.numel(), s) == BADARG
    assert lib.cmgan_stream_decoder_running(h, x.data_ptr(), None, 1, T, 0, sums.data_ptr(), None, out.data_ptr(),
                                            out.data_ptr(), ws.data_ptr(), ws.numel(), s) == BADARG
    assert lib.cmgan_stream_sums_doubles(h, 0) == 0 and lib.cmgan_stream_sums_doubles(h, 3) == (15 * 64 + 1) * 9
    torch.cuda.synchronize()
    assert not sums.any() and not x.any() and not out.any()  # nothing ran
    with pytest.raises(ValueError):
        eng.stream_encoder_running(spec, 0, sums.float())                   # sums must be float64
