"""The active speech level on the GPU (cmgan_amd/csrc/level.hip; include/cmgan_hip.h, "Active speech level"):
Engine.speech_level against the float64 model of tests/level_model.py at the kernel's tile and hangover edges, per-row
lengths with NaN tails, special rows, bit-reproducibility and row independence, hipGraph replay with the input changed in
place, one real track, and the two consumers in DynamicMixer (snr_on="active", level_db=).

Every comparison first asserts level_model.guard_hits == 0 on the model: no threshold decision of the input is within
reach of rounding (the guard and its derivation are in level_model's docstring), which is a condition on the inputs,
not a tolerance.  Under it the counts must equal the model's integers exactly, and ms, active_ms and activity agree to a
relative (n + 64) 2^-53: n roundings of the sum of squares plus 64 ulps for the device's log10 / pow."""
import functools

import numpy as np
import pytest
import torch

import level_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    from cmgan_amd.engine import Engine
    return Engine(device=DEV)


@pytest.fixture(scope="module")
def T():
    from cmgan_amd import _lib
    return int(_lib.load().cmgan_speech_level_tile())


@functools.lru_cache(maxsize=None)
def _model(key, n, fs):
    """The model's answer for the first n samples of the registered signal `key`: computed once, shared, read-only."""
    x = _SIGNALS[key]
    ms, active, frac, counts, q = M.level(x, n, fs)
    hits = M.guard_hits(q, x, counts, fs)
    counts.setflags(write=False)
    return ms, active, frac, counts, hits


_SIGNALS = {}


def _register(key, x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    _SIGNALS.setdefault(key, x)
    return _SIGNALS[key]


def _run(eng, rows, lengths=None, fs=16000, pad=0, fill=0.0):
    """rows: equally long float32 arrays -> (level float64 [B, 3], counts int64 [B, 16]) as numpy; pad > 0 makes the row
    stride larger than L, with `fill` between the rows."""
    B, L = len(rows), len(rows[0])
    buf = torch.full((B, L + pad), fill, dtype=torch.float32, device=DEV)
    wav = buf[:, :L]
    wav.copy_(torch.from_numpy(np.stack(rows)))
    ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
    lv, cnt = eng.speech_level(wav, ld, fs=fs, counts=True)
    assert all(v.dtype == torch.float64 and tuple(v.shape) == (B,) for v in lv)
    assert cnt.dtype == torch.int64 and tuple(cnt.shape) == (B, 16)
    return torch.stack(list(lv), dim=1).cpu().numpy(), cnt.cpu().numpy()


def _check(tag, got, keys, lengths, fs):
    """Every row against the model: guard off, counts exact, levels within the bound.  Returns the worst error / bound."""
    level, cnt = got
    worst = 0.0
    for b, (key, n) in enumerate(zip(keys, lengths)):
        ms, active, frac, counts, hits = _model(key, n, fs)
        assert hits == 0, f"{tag} row {b}: {hits} threshold decisions of the INPUT are within the guard - change the seed"
        assert cnt[b].tolist() == counts.tolist(), f"{tag} row {b}: counts {cnt[b].tolist()}, model {counts.tolist()}"
        for name, g, w in zip(("ms", "active_ms", "activity"), level[b], (ms, active, frac)):
            tol = M.tolerance(n) * abs(w)
            print(f"[level] {tag} row {b} {name}: gpu {g!r} model {w!r} |diff| {abs(g - w):.3e} bound {tol:.3e}")
            assert abs(g - w) <= tol, f"{tag} row {b} {name}: {g!r} vs {w!r}, bound {tol:.3e}"
            if tol > 0:
                worst = max(worst, abs(g - w) / tol)
    return worst


# ------------------------------------------------------------------ 1. tile and hangover edges
_EDGES = {"1": lambda T, I: 1, "T-1": lambda T, I: T - 1, "T": lambda T, I: T, "T+1": lambda T, I: T + 1,
          "2T+1": lambda T, I: 2 * T + 1, "I": lambda T, I: I, "I+1": lambda T, I: I + 1, "I+T+1": lambda T, I: I + T + 1,
          "3I+5": lambda T, I: 3 * I + 5}


@pytest.mark.parametrize("fs", [16000, 8000])
@pytest.mark.parametrize("edge", list(_EDGES))
def test_tile_and_hangover_edges(eng, T, edge, fs):
    I = M.constants(fs)[1]
    assert I == {16000: 3200, 8000: 1600}[fs] and T <= I + 1
    L = _EDGES[edge](T, I)
    keys = [f"edge-{fs}-{edge}-{r}" for r in range(3)]
    rows = [_register(k, M.bursts(100 * (fs // 8000) + 7 * r + len(edge), L, fs=fs)) for r, k in enumerate(keys)]
    got = _run(eng, rows, fs=fs, pad=37, fill=float("nan"))            # B = 3 with a row stride larger than L
    worst = _check(f"fs={fs} L={edge}", got, keys, [L] * 3, fs)
    if L > T:
        assert any(_model(k, L, fs)[3][0] > 0 for k in keys)
    print(f"[level] fs={fs} L={edge}={L}: worst error / bound {worst:.3f}")


def test_more_tiles_than_one_chunk_of_the_folds(eng, T):
    """level_fold and level_select take the tiles 256 at a time: a row of 257 tiles and a bit crosses a chunk, and a
    burst that ends just before tile 256 leaves a hangover that reaches into the second chunk."""
    fs = 16000
    L = 257 * T + 5
    keys = ["chunk-0", "chunk-1"]
    rows = [_register(k, M.bursts(500 + r, L, fs=fs)).copy() for r, k in enumerate(keys)]
    rng = np.random.default_rng(501)
    rows[1][255 * T:256 * T - 40] = (0.2 * rng.standard_normal(T - 40)).astype(np.float32)
    rows[1][256 * T - 40:] = 0.0
    _SIGNALS.pop("chunk-1")
    rows[1] = _register("chunk-1", rows[1])
    got = _run(eng, rows, fs=fs)
    _check("257 tiles", got, keys, [L] * 2, fs)
    assert got[1][1, 5] > 0


def test_higher_rate_longer_hangover(eng, T):
    """48 kHz: I = 9600 samples is ten tiles of hangover, and the guard is the derived one (wider than 2^-40)."""
    fs = 48000
    I = M.constants(fs)[1]
    assert I == 9600 and M.guard_delta(fs) > 2.0 ** -40
    L = I + 2 * T + 7
    keys = [f"48k-{r}" for r in range(2)]
    rows = [_register(k, M.bursts(700 + r, L, fs=fs)) for r, k in enumerate(keys)]
    got = _run(eng, rows, fs=fs)
    _check("48 kHz", got, keys, [L] * 2, fs)
    assert got[1][:, 0].max() > 0


# ------------------------------------------------------------------ 2. hangover placement
def _loud_then_silent(shift, total):
    rng = np.random.default_rng(21)
    x = np.zeros(total)
    x[shift:shift + 1500] = 0.3 * np.clip(rng.standard_normal(1500), -3.0, 3.0)
    return x.astype(np.float32)


@pytest.mark.parametrize("place", ["as it falls", "last sample of a tile", "first sample of a tile"])
def test_hangover_placement(eng, T, place):
    """One loud stretch, then silence: for a mid threshold the activity ends exactly I samples after its last crossing i'.
    Rows of i' + I, i' + I + 1 and i' + I + 2 samples sit around that end; zeros in front move i' onto a tile's edges."""
    fs, j = 16000, 8
    I = M.constants(fs)[1]
    base = _loud_then_silent(0, 1500 + 3 * T)
    last0 = int(np.nonzero(M.envelope(base, fs) >= M.THRESHOLDS[j])[0][-1])
    assert 1500 < last0 < 1500 + 3 * T - 1
    shift = {"as it falls": 0, "last sample of a tile": (T - 1 - last0) % T, "first sample of a tile": (-last0) % T}[place]
    last = last0 + shift
    if place != "as it falls":
        assert last % T == (T - 1 if place.startswith("last") else 0)
    L = last + I + 2
    key = f"hang-{place}"
    x = _register(key, _loud_then_silent(shift, L))
    q = M.envelope(x, fs)
    assert int(np.nonzero(q >= M.THRESHOLDS[j])[0][-1]) == last          # zeros in front shift the envelope, nothing else
    lengths = [last + I, last + I + 1, last + I + 2]
    got = _run(eng, [x, x, x], lengths, fs=fs, pad=5, fill=float("nan"))
    _check(place, got, [key] * 3, lengths, fs)
    a = got[1][:, j]
    assert a[1] == a[0] + 1 and a[2] == a[1], a                            # sample i' + I is the last active one


# ------------------------------------------------------------------ 3. per-row lengths
def test_per_row_lengths_with_nan_tails(eng, T):
    fs, L = 16000, 2 * T + 301
    lengths = [0, 1, T, L]
    keys = [f"len-{r}" for r in range(4)]
    rows = [_register(k, M.bursts(40 + r, L, fs=fs)).copy() for r, k in enumerate(keys)]
    for r, n in zip(rows, lengths):
        r[n:] = np.nan                                                   # samples from a row's length on are never read
    level, cnt = _run(eng, rows, lengths, fs=fs, pad=3, fill=float("nan"))
    assert np.isfinite(level).all()
    assert not level[0].any() and cnt[0].tolist() == [0] * 16
    _check("lengths", (level, cnt), keys, lengths, fs)
    for b, n in enumerate(lengths[1:], start=1):                          # the same row alone, at its own length as L
        alone_level, alone_cnt = _run(eng, [rows[b][:n]], None, fs=fs)
        assert np.array_equal(alone_level[0].view(np.uint64), level[b].view(np.uint64)), (b, alone_level, level[b])
        assert np.array_equal(alone_cnt[0], cnt[b])
        same_level, same_cnt = _run(eng, [rows[b]], [n], fs=fs)             # and alone in the batch's width
        assert np.array_equal(same_level[0].view(np.uint64), level[b].view(np.uint64)) and np.array_equal(same_cnt[0], cnt[b])
    # lengths outside [0, L] are clamped
    clamp_level, clamp_cnt = _run(eng, [rows[3], rows[3]], [-5, L + 1000], fs=fs)
    assert not clamp_level[0].any() and clamp_cnt[0].tolist() == [0] * 16
    assert np.array_equal(clamp_level[1].view(np.uint64), level[3].view(np.uint64)) and clamp_cnt[1, 15] == L


# ------------------------------------------------------------------ 4. special rows
def test_special_rows(eng, T):
    fs, L = 16000, 3 * T + 11
    alt = np.where(np.arange(L) % 2 == 0, 1.0, -1.0)
    named = {"silent": np.zeros(L), "sub-threshold": np.full(L, 0.99 * 2.0 ** -16), "plus one": np.ones(L),
             "minus one": -np.ones(L), "alternating": alt, "bursts": M.bursts(77, L, fs=fs)}
    keys = [f"special-{k}" for k in named]
    rows = [_register(k, v) for k, v in zip(keys, named.values())]
    level, cnt = _run(eng, rows, fs=fs)
    _check("special", (level, cnt), keys, [L] * len(rows), fs)
    for b in (0, 1):
        assert not level[b].any() and cnt[b].tolist() == [0] * 15 + [L]
    for b in (2, 3, 4):
        assert level[b, 0] == 1.0 and cnt[b, 0] > L - 200 and 0.8 < level[b, 2] <= 1.0
    # one Inf sample: that row is three NaNs, the others keep their bits
    bad = rows[5].copy()
    bad[T + 5] = np.inf
    level2, cnt2 = _run(eng, rows[:5] + [bad] + [rows[5]], fs=fs)
    assert np.isnan(level2[5]).all()
    keep = [0, 1, 2, 3, 4, 6]
    assert np.array_equal(level2[keep].view(np.uint64), level[[0, 1, 2, 3, 4, 5]].view(np.uint64))
    assert np.array_equal(cnt2[keep], cnt)
    nan_row = rows[5].copy()
    nan_row[7] = np.nan
    assert np.isnan(_run(eng, [nan_row], fs=fs)[0]).all()


# ------------------------------------------------------------------ 5. determinism and row independence
def test_bit_reproducible_and_row_independent(eng, T):
    fs, L = 16000, 3 * T + 5
    rows = [M.bursts(60 + r, L, fs=fs) for r in range(5)]
    a = _run(eng, rows, fs=fs)
    b = _run(eng, rows, fs=fs)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])
    assert a[1][:, 0].min() > 0
    for k in range(5):
        one = _run(eng, [rows[k]], fs=fs)
        assert np.array_equal(one[0][0].view(np.uint64), a[0][k].view(np.uint64)), k
        assert np.array_equal(one[1][0], a[1][k])


# ------------------------------------------------------------------ 6. graph replay
def test_captured_call_replays_with_new_input_and_lengths(eng, T):
    fs, L = 16000, 2 * T + 9
    keys = ["graph-0", "graph-1"]
    new = [_register(k, M.bursts(90 + r, L, fs=fs)) for r, k in enumerate(keys)]
    wav = torch.from_numpy(np.stack([M.bursts(80 + r, L, fs=fs) for r in range(2)])).to(DEV)
    lengths = torch.tensor([L, L - 100], dtype=torch.int32, device=DEV)
    eager, eager_cnt = eng.speech_level(wav, lengths, fs=fs, counts=True)      # the warm-up call (grows the workspace)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_level, g_cnt = eng.speech_level(wav, lengths, fs=fs, counts=True)
    graph.replay()
    assert all(torch.equal(a, b) for a, b in zip(g_level, eager)) and torch.equal(g_cnt, eager_cnt)
    wav.copy_(torch.from_numpy(np.stack(new)).to(DEV))
    lengths.copy_(torch.tensor([T + 1, L], dtype=torch.int32, device=DEV))
    graph.replay()
    again, again_cnt = eng.speech_level(wav, lengths, fs=fs, counts=True)
    assert not torch.equal(again_cnt, eager_cnt)
    assert all(torch.equal(a, b) for a, b in zip(g_level, again)) and torch.equal(g_cnt, again_cnt)
    _check("replayed", (torch.stack(list(g_level), dim=1).cpu().numpy(), g_cnt.cpu().numpy()), keys, [T + 1, L], fs)


# ------------------------------------------------------------------ 7. one real track
def test_real_track(eng):
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_known_answers.npz"))
    name = str(z["names"][0])
    x = _register("real", z["clean_" + name].astype(np.float32) / 32768.0)
    got = _run(eng, [x], fs=16000)
    _check(name, got, ["real"], [len(x)], 16000)
    ms, active, frac, counts, _ = _model("real", len(x), 16000)
    assert 0.5 < frac < 1.0 and active > ms > 0 and counts[0] > 0
    print(f"[level] {name}: {len(x)} samples, activity {frac:.4f}, active level {10 * np.log10(active):.2f} dBFS, "
          f"{10 * np.log10(active / ms):.2f} dB above the RMS level")


# ------------------------------------------------------------------ 8, 9. the mixer
def _speechlike(B, L, fs=16000):
    """Rows of seeded bursts whose pauses make activity clearly smaller than 1."""
    return np.stack([M.bursts(300 + b, L, peak=0.3, fs=fs) for b in range(B)])


def _mixer(eng, seed, **kw):
    from cmgan_amd.mixing import DynamicMixer, NoiseBank
    rng = np.random.default_rng(5)
    nb = NoiseBank.from_arrays([0.1 * rng.standard_normal(5000), 0.05 * rng.standard_normal(1234)], device=DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    # peak = 100: the peak guard stays off, so noisy - target is the scaled noise alone
    return DynamicMixer(eng, nb, None, snr_db=(0.0, 15.0), early_ms=None, peak=100.0, generator=gen, **kw), nb


def test_mixer_snr_on_active_speech_level(eng, T):
    B, L = 4, 4 * T + 123
    clean = torch.from_numpy(_speechlike(B, L)).to(DEV)
    mixer, nb = _mixer(eng, 9, snr_on="active")
    target, noisy, info = mixer(clean)
    assert torch.equal(target, clean) and bool((info.scale == 1.0).all())
    lv = mixer.last_level
    ref = eng.speech_level(clean)
    assert all(torch.equal(a, b) for a, b in zip(lv, ref))
    activity = lv.activity.cpu().numpy()
    assert np.all(activity > 0.2) and np.all(activity < 0.97)            # pauses: active and RMS levels differ visibly
    gn = noisy.double() - target.double()                                # = g n, up to the float32 rounding of noisy
    achieved = 10.0 * torch.log10(lv.active_ms / (gn * gn).mean(dim=1))
    drawn = mixer.last_draw.snr_db.double()
    err = (achieved - drawn).abs().cpu().numpy()
    print(f"[level] snr_on=active: drawn {drawn.cpu().numpy()}, achieved - drawn {err}")
    assert np.all(err <= 1e-3)
    rms_snr = 10.0 * torch.log10(info.Ps / (info.g ** 2 * info.Pn))
    assert torch.allclose(rms_snr - drawn, 10.0 * torch.log10(lv.activity), atol=1e-5, rtol=0)
    # the same seed with snr_on="rms" is Engine.mix on last_draw, bit for bit, and measures nothing
    plain, _ = _mixer(eng, 9, snr_on="rms")
    t2, n2, i2 = plain(clean)
    d = plain.last_draw
    assert plain.last_level is None and torch.equal(d.snr_db, mixer.last_draw.snr_db)
    n3, t3, i3 = eng.mix(clean, nb.data, d.noise_start, d.noise_len, d.noise_off, d.snr_db, peak=100.0, early=-1)
    assert torch.equal(n2, n3) and torch.equal(t2, t3) and all(torch.equal(a, b) for a, b in zip(i2, i3))
    assert not torch.equal(n2, noisy)


def test_mixer_level_db(eng, T):
    from cmgan_amd.mixing import DynamicMixer
    B, L = 4, 3 * T + 50
    x = _speechlike(B, L)
    x[2] = 0.0                                                           # a row with no speech keeps its samples
    clean = torch.from_numpy(x).to(DEV)
    mixer, nb = _mixer(eng, 4, level_db=(-35.0, -15.0))
    target, noisy, info = mixer(clean)
    d, lv = mixer.last_draw, mixer.last_level
    level = d.level_db
    assert level.dtype == torch.float64 and bool(((level >= -35.0) & (level <= -15.0)).all())
    ok = torch.isfinite(lv.active_ms) & (lv.active_ms > 0)
    assert ok.tolist() == [True, True, False, True]
    gain = torch.where(ok, torch.sqrt(10.0 ** (level / 10.0) / torch.where(ok, lv.active_ms, torch.ones_like(level))),
                       torch.ones_like(level)).to(torch.float32)
    assert torch.equal(gain, DynamicMixer.level_gain(lv, level)) and float(gain[2]) == 1.0
    assert torch.equal(target, clean * gain[:, None])
    assert bool((info.scale == 1.0).all())
    # one measurement, one gain: the scaled rows measure close to the drawn level (absolute thresholds: not exactly)
    after = eng.speech_level(target)
    off = (10.0 * torch.log10(after.active_ms[ok]) - level[ok]).abs()
    print(f"[level] level_db: drawn {level.cpu().numpy()}, re-measured - drawn {off.cpu().numpy()} dB")
    # the draws that existed before come first and are unchanged
    plain, _ = _mixer(eng, 4)
    for a, b in zip(plain.draw(B)[:4], d[:4]):
        assert torch.equal(a, b)


def test_mixer_defaults_change_nothing(eng, T):
    B, L = 3, 2 * T + 17
    clean = torch.from_numpy(_speechlike(B, L)).to(DEV)
    a, _ = _mixer(eng, 12)
    b, _ = _mixer(eng, 12, snr_on="rms", level_db=None)
    ta, na, ia = a(clean)
    tb, nb_, ib = b(clean)
    assert torch.equal(ta, tb) and torch.equal(na, nb_) and all(torch.equal(p, q) for p, q in zip(ia, ib))
    assert a.last_level is None and b.last_level is None
    for p, q in zip(a.last_draw, b.last_draw):
        assert (p is None and q is None) or torch.equal(p, q)
    assert a.last_draw.level_db is None
