"""The GPU resampler (cmgan_amd/csrc/resample.hip; include/cmgan_hip.h, "Sample-rate conversion") and what is built on
it: the kernel against scipy.signal.resample_poly on the float64 copy of the same float32 samples, chunked calls and the
incremental Resampler bit for bit against the one-call result, hipGraph replay, and the three front ends that take a
sample rate - enhance_one_track, evaluation(resample=True) and StreamingEnhancer - against the same composition built
on the CPU (scipy's resampling around the oracle)."""
import numpy as np
import pytest
import torch
from scipy import signal as sig

import resample_model as RM
import stream_running_model as R
from conftest import assert_close, rel_err
from oracle import cmgan_oracle as O
from oracle import stream_oracle as S
from oracle.weights import make_state_dict, synthetic_clips

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GATE = 1e-3          # tests/test_gpu_parity.py
STAGE = 2e-4         # tests/test_gpu_stream_running.py, tests/test_gpu_stream_config5.py
MODES = ["f16x3", "f32"]
TILE = 256           # outputs per block of resample_poly
_CPU = {}


def _once(key, fn):
    if key not in _CPU:
        _CPU[key] = fn()
    return _CPU[key]


def _report(name, err):
    print(f"[resample] {name}: rel_err = {err:.3e}")
    return err


def _check(name, got, want, gate=GATE, rtol=1e-3, atol_rel=2e-5):
    """tests/test_gpu_parity.py::_check: max-norm relative error under `gate` AND the elementwise bound."""
    assert _report(name, rel_err(got, want)) < gate, name
    assert_close(got, want, rtol=rtol, atol_rel=atol_rel, name=name)


def _poly(x, fs_in, fs_out):
    """scipy.signal.resample_poly on the float64 copy of the samples, along the last axis."""
    up, down, _, _ = RM.geometry(fs_in, fs_out)
    return sig.resample_poly(np.asarray(x, dtype=np.float64), up, down, axis=-1)


def _poly32(x, fs_in, fs_out):
    """... rounded to float32 once, as the device stores it: a [.., N] float32 torch tensor."""
    return torch.from_numpy(_poly(x.numpy() if isinstance(x, torch.Tensor) else x, fs_in, fs_out).astype(np.float32))


@pytest.fixture(scope="module")
def eng():
    from cmgan_amd.engine import Engine
    return Engine(device=DEV)


@pytest.fixture(scope="module")
def sd():
    return make_state_dict(seed=0, num_features=201)


@pytest.fixture(scope="module", params=MODES)
def model(request, sd):
    from cmgan_amd import TSCNet
    return TSCNet(num_channel=64, num_features=201, mfma_mode=request.param).cuda().load_state_dict(sd).eval()


# ------------------------------------------------------------------ 4. the kernel against scipy
def _inputs(kind, B, L, rng):
    if kind == "noise":
        return rng.standard_normal((B, L)).astype(np.float32)
    if kind == "zeros":                                         # a leading and a trailing stretch of exact zeros
        x = rng.standard_normal((B, L)).astype(np.float32)
        x[:, :L // 4] = 0.0
        x[:, L - L // 3:] = 0.0
        return x
    x = np.zeros((B, L), dtype=np.float32)                      # a full-scale step
    x[:, L // 2:] = 1.0
    return x


@pytest.mark.parametrize("fs_in,fs_out", RM.PAIRS)
def test_kernel_matches_scipy_resample_poly(eng, fs_in, fs_out):
    """Elementwise |got - want| <= 2^-24 |want| + 1e-12 max|want|: the one rounding to float32, plus the float64
    summation order (about 60 terms of 1.1e-16)."""
    up, down, _, _ = RM.geometry(fs_in, fs_out)
    rng = np.random.default_rng(fs_in * 3 + fs_out)
    lengths = sorted({1, 255, 257, (TILE - 1) * down // up, (TILE + 1) * down // up + 1, 2 * fs_in})
    worst = 0.0
    for B in (1, 5, 32):
        for L in lengths:
            for kind in ("noise", "zeros", "step"):
                x = _inputs(kind, B, L, rng)
                want = _poly(x, fs_in, fs_out)
                got = eng.resample(torch.from_numpy(x).to(DEV), fs_in, fs_out)
                assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (B, RM.out_len(fs_in, fs_out, L))
                got = got.cpu().numpy().astype(np.float64)
                peak = np.max(np.abs(want))
                excess = np.abs(got - want) - (2.0 ** -24 * np.abs(want) + 1e-12 * peak)
                worst = max(worst, float(np.max(np.abs(got - want)) / max(peak, 1e-300)))
                assert np.max(excess) <= 0.0, (f"{fs_in}->{fs_out} B={B} L={L} {kind}: {int((excess > 0).sum())} of "
                                               f"{got.size} outside the bound, worst excess {np.max(excess):.3e}")
    print(f"[resample] {fs_in}->{fs_out}: worst |got - scipy| / peak = {worst:.3e}")


@pytest.mark.parametrize("fs_in,fs_out", [(48000, 300), (64000, 100), (100, 64000)])
def test_extreme_ratios_take_the_small_tile_and_the_unstaged_paths(eng, fs_in, fs_out):
    """Decimation by 160 (one phase of 3362 taps: tiles of 31 outputs), by 640 (13442 taps, longer than the LDS span: the
    kernel reads global memory directly) and interpolation by 640.  The sums are up to 13441 terms long, so in place of
    the 1e-12 max|want| that stands for about 60 terms the bound carries the textbook term for two float64 sums of T terms,
    2 T 2^-53 max_p sum_j |h[p + j up]| max|x|, plus T taps that may each be 1e-13 off scipy's (the tolerance
    tests/test_resample_host.py holds the table to), T 1e-13 max|x|."""
    up, down, n_taps, _ = RM.geometry(fs_in, fs_out)
    h = RM.taps(fs_in, fs_out)
    T = -(-n_taps // up)
    habs = max(float(np.sum(np.abs(h[p::up]))) for p in range(up))
    rng = np.random.default_rng(fs_in + fs_out)
    for B, L in ((2, 3 * max(down, 1) * 40 + 17), (1, 1)):
        x = rng.standard_normal((B, L)).astype(np.float32)
        want = _poly(x, fs_in, fs_out)
        got = eng.resample(torch.from_numpy(x).to(DEV), fs_in, fs_out).cpu().numpy().astype(np.float64)
        assert got.shape == want.shape
        bound = 2.0 ** -24 * np.abs(want) + (2 * T * 2.0 ** -53 * habs + T * 1e-13) * float(np.max(np.abs(x)))
        print(f"[resample] {fs_in}->{fs_out} [{B}, {L}]: worst |got - scipy| / peak = "
              f"{np.max(np.abs(got - want)) / np.max(np.abs(want)):.3e}")
        assert np.max(np.abs(got - want) - bound) <= 0.0


def test_equal_rates_copy_and_unsupported_pairs_raise(eng):
    from cmgan_amd._lib import CmganError
    x = torch.randn(3, 1001, device=DEV)
    assert torch.equal(eng.resample(x, 16000, 16000), x)
    assert torch.equal(eng.resample(x[0], 48000, 48000), x[0])
    with pytest.raises(CmganError) as e:
        eng.resample(x, 16000, 44101)
    assert e.value.code == -3                                   # CMGAN_E_UNSUPPORTED
    y = eng.resample(x[0], 48000, 16000)                        # a 1-D signal keeps its rank
    assert tuple(y.shape) == (334,)


# ------------------------------------------------------------------ 5. chunk invariance
@pytest.mark.parametrize("fs_in,fs_out", [(44100, 16000), (16000, 44100)])
def test_chunked_calls_and_resampler_pushes_equal_the_one_call_result(eng, fs_in, fs_out):
    from cmgan_amd.resample import ResamplePlan, Resampler
    B, L = 2, 30011
    geom = RM.geometry(fs_in, fs_out)
    rng = np.random.default_rng(fs_in)
    x = torch.from_numpy(rng.standard_normal((B, L)).astype(np.float32)).to(DEV)
    whole = eng.resample(x, fs_in, fs_out)
    N = whole.size(1)
    # the C ABI in pieces: outputs [n0, n0 + n) from the rows of x themselves (ld_in = L), the window advancing with n0
    plan = ResamplePlan(*geom)
    ws = eng._resample_ws(fs_in, fs_out)
    parts, n0 = [], 0
    while n0 < N:
        n = int(min(N - n0, rng.choice([1, 7, 255, 256, 257, 1000, 4099])))
        lo, hi = plan.first_input(n0), min(plan.last_input(n0 + n - 1), L - 1)
        out = torch.full((B, n + 3), float("nan"), device=DEV)
        rc = eng.lib.cmgan_resample(eng._h, x.data_ptr() + 4 * lo, B, hi - lo + 1, L, lo, fs_in, fs_out, n0, n,
                                    out.data_ptr(), n + 3, ws.data_ptr(), ws.numel(),
                                    torch.cuda.current_stream().cuda_stream)
        assert rc == 0, eng.lib.cmgan_last_error(eng._h)
        assert torch.isnan(out[:, n:]).all()                    # nothing written past the chunk
        parts.append(out[:, :n])
        n0 += n
    assert torch.equal(torch.cat(parts, dim=1), whole)
    # Resampler.push / flush on random chunk sizes, chunks of 1 sample and chunks longer than the table included
    for trial in range(3):
        rs = Resampler(eng, fs_in, fs_out, B=B)
        outs, pos, held = [], 0, 0
        while pos < L:
            n = int(min(L - pos, rng.choice([1, 2, 160, 441, 3000, geom[2] + 100])))
            outs.append(rs.push(x[:, pos:pos + n]))
            pos += n
            held = max(held, rs.buf.size(1))
        outs.append(rs.flush())
        assert torch.equal(torch.cat(outs, dim=1), whole), trial
        assert rs.n_out == N and rs.flush().size(1) == 0
        assert held <= geom[2] // geom[0] + 2                   # what one output reaches, not the chunks pushed


# ------------------------------------------------------------------ 6. hipGraph
def test_captured_resample_replays_to_the_eager_bits(eng):
    fs_in, fs_out = 44100, 16000
    x = torch.randn(4, 22050, device=DEV)
    eager = eng.resample(x, fs_in, fs_out)                      # the warm-up call (allocates the pair's workspace)
    torch.cuda.synchronize()
    g_in = x.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out = eng.resample(g_in, fs_in, fs_out)
    graph.replay()
    assert torch.equal(g_out, eager)
    x2 = torch.randn(4, 22050, device=DEV)
    g_in.copy_(x2)
    graph.replay()
    assert torch.equal(g_out, eng.resample(x2, fs_in, fs_out))


# ------------------------------------------------------------------ 7. enhance_one_track(sample_rate=...)
@pytest.mark.parametrize("fs,L", [(44100, 30011), (8000, 6001)])
def test_enhance_one_track_at_a_foreign_rate(model, sd, fs, L):
    """scipy resample -> oracle enhance -> scipy resample back -> [:L], on the CPU."""
    from cmgan_amd.evaluation import enhance_one_track
    x = synthetic_clips(1, L, seed=fs % 97)

    def cpu():
        est = O.enhance(sd, _poly32(x, fs, 16000))
        return _poly32(est.reshape(1, -1), 16000, fs)[0, :L]
    want = _once(("track", fs), cpu)
    got = enhance_one_track(model, x.to(DEV), sample_rate=fs)
    assert got.shape == (L,)
    _check(f"enhance_one_track at {fs} Hz [{model.engine.mfma_mode}]", got, want)


def test_enhance_one_track_without_a_rate_is_todays_call(model):
    from cmgan_amd.evaluation import enhance_one_track
    x = synthetic_clips(1, 9050, seed=5).to(DEV)
    today = enhance_one_track(model, x)
    assert torch.equal(enhance_one_track(model, x, sample_rate=None), today)
    assert torch.equal(enhance_one_track(model, x, sample_rate=16000), today)
    assert torch.equal(enhance_one_track(model, x, 16000 * 16, 400, 100, None, 16000), today)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [4000, 4001])
def test_48k_model_enhances_a_16k_track(mode, L):
    """BASELINE configs[3] (n_fft 1200 / hop 300, the weights' shape of tests/golden/pipeline48.npz) behind the resampler.
    L = 4001 is 12003 samples at 48 kHz: the reference's glue wrap-pads to a multiple of 100 (12100) and its ISTFT
    returns hop (T - 1) = 12000 of them (tests/golden/pipeline48.npz holds such a ragged case), so the composition comes
    back one sample short there, on the CPU and on the GPU alike."""
    from cmgan_amd import TSCNet
    from cmgan_amd.evaluation import enhance_one_track
    sd48 = make_state_dict(seed=5, num_features=601)
    m48 = TSCNet(64, 601, mfma_mode=mode).load_state_dict(sd48).eval()
    x = synthetic_clips(1, L, seed=48)

    def cpu():
        est = O.enhance(sd48, _poly32(x, 16000, 48000), cut_len=48000 * 16, n_fft=1200, hop=300)
        return _poly32(est.reshape(1, -1), 48000, 16000)[0, :L]
    want = _once(("track48", L), cpu)
    got = enhance_one_track(m48, x.to(DEV), 48000 * 16, 1200, 300, sample_rate=16000, model_rate=48000)
    assert got.shape == want.shape == (4000,)
    _check(f"48 kHz model on a 16 kHz track of {L} samples [{mode}]", got, want)


# ------------------------------------------------------------------ 8. evaluation(resample=True)
def _pcm(x):
    return np.round(x * 32767).astype(np.int16)


def _write_pairs(tmp_path, fs, n0, names):
    from scipy.io import wavfile
    noisy_dir, clean_dir = tmp_path / "noisy", tmp_path / "clean"
    noisy_dir.mkdir(); clean_dir.mkdir()
    pairs = []
    for i, name in enumerate(names):
        clean = synthetic_clips(1, n0 + 700 * i, seed=30 + i)[0].numpy() * 0.2
        noisy = clean + 0.05 * synthetic_clips(1, clean.size, seed=40 + i)[0].numpy()
        wavfile.write(str(noisy_dir / name), fs, _pcm(noisy))
        wavfile.write(str(clean_dir / name), fs, _pcm(clean))
        pairs.append((_pcm(noisy).astype(np.float64) / 32768.0, _pcm(clean).astype(np.float64) / 32768.0))
    return noisy_dir, clean_dir, pairs


def test_evaluation_resamples_44100_files(model, sd, tmp_path):
    """The six averages against the same composition on the CPU, under the 1e-3 of
    test_evaluation_directory_driver_scores_like_the_oracle_path; saved tracks keep the input's rate and length."""
    from scipy.io import wavfile
    from cmgan_amd import metrics
    from cmgan_amd.evaluation import evaluation
    names = ["p1_10.wav", "p1_2.wav"]
    noisy_dir, clean_dir, pairs = _write_pairs(tmp_path, 44100, 44100, names)

    def cpu():
        want = np.zeros(6)
        for nz, cl in pairs:
            nz32 = torch.from_numpy(nz).float()[None, :]
            est = O.enhance(sd, _poly32(nz32, 44100, 16000))
            est44 = _poly32(est.reshape(1, -1), 16000, 44100)[:, :nz.size]
            est16 = _poly32(est44, 44100, 16000)[0].numpy().astype(np.float64)
            cl16 = _poly32(torch.from_numpy(cl).float()[None, :], 44100, 16000)[0].numpy().astype(np.float64)
            want += np.array(metrics.compute_metrics(cl16, est16, 16000, 0, pesq_mos=2.0))
        return want / len(pairs)
    want = _once("eval44", cpu)
    out_dir = tmp_path / "enh"
    got = evaluation(model, str(noisy_dir), str(clean_dir), True, str(out_dir), pesq_fn=lambda fs, a, b: 2.0,
                     verbose=False, resample=True)
    assert _report("evaluation(resample=True) averages vs the CPU composition",
                   rel_err(torch.tensor(got), torch.tensor(want))) < 1e-3
    assert sorted(p.name for p in out_dir.iterdir()) == sorted(names)
    for name, (nz, _) in zip(names, pairs):
        sr, data = wavfile.read(str(out_dir / name))
        assert sr == 44100 and data.shape == nz.shape
    with pytest.raises(ValueError, match="expected 16 kHz audio, got 44100"):
        evaluation(model, str(noisy_dir), str(clean_dir), pesq_fn=lambda fs, a, b: 2.0, verbose=False)


def test_evaluation_scores_the_48k_model(tmp_path):
    """48 kHz files through the 48 kHz model, scored at 16 kHz: BASELINE configs[3]'s first scores."""
    from cmgan_amd import TSCNet, metrics
    from cmgan_amd.evaluation import evaluation
    sd48 = make_state_dict(seed=5, num_features=601)
    m48 = TSCNet(64, 601).load_state_dict(sd48).eval()
    noisy_dir, clean_dir, pairs = _write_pairs(tmp_path, 48000, 24000, ["a.wav"])
    nz, cl = pairs[0]
    est = O.enhance(sd48, torch.from_numpy(nz).float()[None, :], cut_len=48000 * 16, n_fft=1200, hop=300)
    est16 = _poly32(est.reshape(1, -1), 48000, 16000)[0].numpy().astype(np.float64)
    cl16 = _poly32(torch.from_numpy(cl).float()[None, :], 48000, 16000)[0].numpy().astype(np.float64)
    want = np.array(metrics.compute_metrics(cl16, est16, 16000, 0, pesq_mos=2.0))
    got = evaluation(m48, str(noisy_dir), str(clean_dir), pesq_fn=lambda fs, a, b: 2.0, verbose=False, resample=True,
                     model_rate=48000)
    print("[resample] 48 kHz model, scored at 16 kHz:", got)
    assert _report("evaluation(48 kHz model) vs the CPU composition", rel_err(torch.tensor(got), torch.tensor(want))) < 1e-3


# ------------------------------------------------------------------ 9. StreamingEnhancer(sample_rate=...)
W, CA, LA = 40, 12, 8


@pytest.mark.parametrize("stats_mode", ["frozen", "running"])
def test_streaming_enhancer_at_44100(model, sd, stats_mode):
    """Uneven pushes at 44.1 kHz against scipy -> the CPU stream (oracle/stream_oracle.py for frozen statistics,
    tests/stream_running_model.py for running ones) on the zero-padded 16 kHz signal -> scipy back -> [:L]."""
    from cmgan_amd.streaming import StreamingEnhancer
    eng = model.engine
    fs, L = 44100, 44100 + 333
    x = synthetic_clips(1, L, seed=71)

    def cpu():
        x16 = _poly32(x, fs, 16000)
        x16 = torch.cat([x16, x16.new_zeros(1, -x16.size(1) % 100)], dim=1)
        y16 = (R.enhance_stream(sd, x16, W, CA, LA)[0] if stats_mode == "running" else S.enhance_stream(sd, x16, W, CA, LA))
        return _poly32(y16.reshape(1, -1), 16000, fs)[0, :L]
    want = _once(("live", stats_mode), cpu)
    xd = x.to(DEV)
    x16 = eng.resample(xd, fs, 16000)
    x16 = torch.cat([x16, x16.new_zeros(1, -x16.size(1) % 100)], dim=1)
    c = eng.rms_scale(x16)
    stats = None
    if stats_mode == "frozen":
        stats = eng.tscnet_forward_stats(eng.stft_compress(x16, c)[:, :, :W + LA].contiguous())[2]
    live = StreamingEnhancer(model, stats, window=W, context=CA, lookahead=LA, scale=c, stats_mode=stats_mode,
                             sample_rate=fs)
    out, pos = [], 0
    for n in (137, 9001, 50, 12000, 1, 2479, 15000, L - 38668):
        out.append(live.push(xd[0, pos:pos + n]))
        pos += n
    assert pos == L
    out.append(live.flush())
    got = torch.cat(out)
    assert got.shape == (L,) and live.flush().numel() == 0
    assert sum(o.numel() for o in out[:-1]) > 0                 # samples came out while the stream was running
    _check(f"StreamingEnhancer at 44.1 kHz, {stats_mode} [{eng.mfma_mode}]", got, want, gate=STAGE)


def test_streaming_enhancer_without_a_rate_is_unchanged(model):
    from cmgan_amd.streaming import StreamingEnhancer
    eng = model.engine
    wav = synthetic_clips(1, 16000, seed=37).to(DEV)
    c = eng.rms_scale(wav)
    runs = []
    for kw in ({}, {"sample_rate": None}, {"sample_rate": 16000}):
        live = StreamingEnhancer(model, window=W, context=CA, lookahead=LA, scale=c, stats_mode="running", **kw)
        assert live.rs_in is None and live.rs_out is None
        out, pos = [], 0
        for n in (137, 3333, 50, 4000, 1, 2479, 6000):
            out.append(live.push(wav[0, pos:pos + n]))
            pos += n
        out.append(live.flush())
        runs.append(out)
    for other in runs[1:]:
        assert len(other) == len(runs[0]) and all(torch.equal(a, b) for a, b in zip(other, runs[0]))
