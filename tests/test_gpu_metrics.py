"""Engine.metrics / cmgan_metrics (cmgan_amd/csrc/metrics.hip) against the host module cmgan_amd.metrics (itself pinned
to the reference tool at 1e-9, tests/test_metrics.py) and against the reference tool's own logged scores.  Inputs are
float32 on both sides (the library's audio dtype), so the bar is float64 round-off."""
import math
import os

import numpy as np
import pytest
import torch

from cmgan_amd import metrics as M
from metrics_signals import CASES, pair, speechlike

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "metrics.npz"))
KA = np.load(os.path.join(os.path.dirname(__file__), "golden", "metrics_known_answers.npz"))
PESQ = float(G["pesq_stub"])


def close(a, b, tol=1e-9):          # tests/test_metrics.py's bar
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b) / (1.0 + np.abs(b)))) < tol


@pytest.fixture(scope="module")
def eng():
    from cmgan_amd.engine import Engine
    return Engine()                 # no weights: scoring needs none


def f32(x):
    return np.asarray(x, dtype=np.float32)


def dev(x):
    return torch.from_numpy(f32(x)).to(DEV)


def host_scores(clean, enh, fs, pesq_mos=PESQ):
    """compute_metrics plus the trimmed WSS / LLR and the overall SNR it computes on the way."""
    a, b = np.asarray(clean, np.float64), np.asarray(enh, np.float64)
    s = M.compute_metrics(a, b, fs, 0, pesq_mos=pesq_mos)
    if a.size != b.size:
        n = min(a.size, b.size)
        a, b = a[:n] + M._EPS, b[:n] + M._EPS

    def trimmed(v):
        return float(np.mean(np.sort(v)[: round(v.size * 0.95)]))
    return s, trimmed(M.wss(a, b, fs)), trimmed(M.llr(a, b, fs)), M.segmental_snr(a, b, fs)[0]


@pytest.mark.parametrize("fs,n,seed", CASES)
def test_per_frame_values_match_the_host_module(eng, fs, n, seed):
    clean, enh = (f32(v) for v in pair(fs, n, seed))
    _, fr = eng.metrics(dev(clean)[None], dev(enh)[None], fs, per_frame=True)
    assert close(fr.wss[0].cpu().numpy(), M.wss(clean, enh, fs))
    assert close(fr.llr[0].cpu().numpy(), M.llr(clean, enh, fs))
    assert close(fr.segsnr[0].cpu().numpy(), M.segmental_snr(clean, enh, fs)[1])


@pytest.mark.parametrize("fs,n,seed", CASES)
def test_per_clip_values_match_compute_metrics(eng, fs, n, seed):
    clean, enh = (f32(v) for v in pair(fs, n, seed))
    got = eng.metrics(dev(clean)[None], dev(enh)[None], fs, pesq_mos=PESQ)
    s, wss, llr, snr = host_scores(clean, enh, fs)
    got = [float(t[0]) for t in got]
    assert close(got[:6], list(s), 1e-8), (got, s)
    assert close(got[6:], [wss, llr, snr], 1e-8)


@pytest.mark.parametrize("name", [str(n) for n in KA["names"]])
def test_logged_scores_of_the_reference_tool(eng, name):
    """The reference tool's python_noisy_metrics.log values on three VoiceBank tracks (int16 PCM, clean vs noisy),
    with the logged PESQ as input: CSIG, CBAK, COVL, SSNR and STOI."""
    pesq_mos, *want = [float(v) for v in KA[f"log_{name}"]]
    clean, noisy = KA[f"clean_{name}"], KA[f"noisy_{name}"]
    got = eng.metrics(dev(clean)[None], dev(noisy)[None], 16000, pesq_mos=pesq_mos)
    got = [float(t[0]) for t in got[1:6]]
    assert max(abs(a - b) for a, b in zip(got, want)) < 1e-6, (got, want)


def _batch(B, n=32000, fs=16000):
    rows = [pair(fs, n, 10 + i) for i in range(B)]
    return dev(np.stack([r[0] for r in rows])), dev(np.stack([r[1] for r in rows]))


def test_batch_rows_equal_single_calls_bit_for_bit(eng):
    clean, enh = _batch(5)
    mos = torch.linspace(1.5, 3.5, 5, dtype=torch.float64, device=DEV)
    s, fr = eng.metrics(clean, enh, 16000, pesq_mos=mos, per_frame=True)
    s, fr = torch.stack(tuple(s), 1), torch.stack(tuple(fr), 1)
    for b in range(5):
        one, fr1 = eng.metrics(clean[b:b + 1], enh[b:b + 1], 16000, pesq_mos=mos[b:b + 1], per_frame=True)
        assert torch.equal(torch.stack(tuple(one), 1)[0], s[b])
        assert torch.equal(torch.stack(tuple(fr1), 1)[0], fr[b])
    again, _ = eng.metrics(clean, enh, 16000, pesq_mos=mos, per_frame=True)
    assert torch.equal(torch.stack(tuple(again), 1), s)
    assert torch.isfinite(s).all()


def test_graph_replay_equals_the_eager_call(eng):
    clean, enh = _batch(3)
    eager = torch.stack(tuple(eng.metrics(clean, enh, 16000, pesq_mos=2.5)), 1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = eng.metrics(clean, enh, 16000, pesq_mos=2.5)
    torch.cuda.current_stream().wait_stream(s)
    clean.mul_(0.5)                    # replay reads the live inputs
    enh.mul_(0.75)
    g.replay()
    torch.cuda.synchronize()
    want = torch.stack(tuple(eng.metrics(clean, enh, 16000, pesq_mos=2.5)), 1)
    assert torch.equal(torch.stack(tuple(out), 1), want)
    assert not torch.equal(want, eager)


def test_edge_rows(eng):
    fs, n = 16000, 32000
    clean, enh = pair(fs, n, 3)
    # mostly silence: a 0.15 s burst 100 dB above the floor keeps ~ 15 STOI frames (< 30); the host raises there
    quiet = np.random.default_rng(5).standard_normal(n) * 1e-2
    quiet[8000:10400] += speechlike(2400, fs, 7)
    with pytest.raises(Exception):
        M.stoi(f32(quiet), f32(quiet * 0.9), fs)
    rows_c, rows_e = dev(np.stack([clean, quiet])), dev(np.stack([enh, quiet * 0.9]))
    s = eng.metrics(rows_c, rows_e, fs, pesq_mos=PESQ)
    assert math.isnan(float(s.stoi[1])) and math.isfinite(float(s.stoi[0]))
    for field in ("csig", "cbak", "covl", "ssnr", "wss", "llr", "snr"):
        assert torch.isfinite(getattr(s, field)).all(), field
    # no PESQ: NaN composites (like the host's lim()), the rest unchanged
    bare = eng.metrics(rows_c, rows_e, fs)
    for field in ("pesq", "csig", "cbak", "covl"):
        assert torch.isnan(getattr(bare, field)).all(), field
    for field in ("ssnr", "wss", "llr", "snr"):
        assert torch.equal(getattr(bare, field), getattr(s, field)), field
    # unequal lengths: trimmed, eps added to both (compute_metrics.py:41-44)
    c32, e32 = f32(clean), f32(enh)[:-123]
    got = eng.metrics(dev(c32)[None], dev(e32)[None], fs, pesq_mos=PESQ)
    hs, wss, llr, snr = host_scores(c32, e32, fs)
    assert close([float(t[0]) for t in got[:6]], list(hs), 1e-8)
    assert close([float(got.wss[0]), float(got.llr[0]), float(got.snr[0])], [wss, llr, snr], 1e-8)


def test_evaluation_driver_scores_on_the_gpu_like_the_host(tmp_path):
    from scipy.io import wavfile

    from cmgan_amd import TSCNet
    from cmgan_amd.evaluation import _read_wav, enhance_one_track, evaluation
    from cmgan_amd.synth import make_state_dict
    model = TSCNet(64, 201).cuda().load_state_dict(make_state_dict(seed=0)).eval()
    noisy_dir, clean_dir = tmp_path / "noisy", tmp_path / "clean"
    noisy_dir.mkdir()
    clean_dir.mkdir()
    names, lengths = ["t_1.wav", "t_2.wav", "t_10.wav"], [(20000, 20000), (23017, 23017), (21000, 20400)]
    for i, (name, (ln, lc)) in enumerate(zip(names, lengths)):
        c = speechlike(max(ln, lc), 16000, 40 + i) / 3.0
        nz = c + np.random.default_rng(i).standard_normal(c.size) * 600.0
        wavfile.write(str(noisy_dir / name), 16000, np.round(nz[:ln]).astype(np.int16))
        wavfile.write(str(clean_dir / name), 16000, np.round(c[:lc]).astype(np.int16))

    def stub(fs, a, b):
        return 2.0 + 1e-5 * (len(b) % 1000)
    want = np.zeros(6)
    for name in names:
        noisy, _ = _read_wav(str(noisy_dir / name))
        clean, _ = _read_wav(str(clean_dir / name))
        est = enhance_one_track(model, torch.from_numpy(noisy).to(DEV, torch.float32)[None, :]).cpu().numpy()
        est = est.astype(np.float64)
        want += np.array(M.compute_metrics(clean, est, 16000, 0, pesq_mos=stub(16000, clean, est)))
    want /= len(names)
    got = evaluation(model, str(noisy_dir), str(clean_dir), pesq_fn=stub, verbose=False)
    assert close(np.array(got), want, 1e-9), (got, want)
