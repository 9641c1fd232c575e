"""Dynamic mixing on the GPU (cmgan_amd/csrc/scene.hip; include/cmgan_hip.h, "Dynamic mixing"): Engine.mix against the
float64 numpy model of tests/mix_model.py over the kernels' tile, chunk and length edges, the edge semantics of gain and
peak guard, bit-reproducibility and row independence, hipGraph replay with the device-side draws changed in place, and
the front end (DynamicMixer, MixingLoader) against the model fed with the same draws."""
import numpy as np
import pytest
import torch

import mix_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U32, U64 = 2.0 ** -24, 2.0 ** -53
PEAK = 0.99


@pytest.fixture(scope="module")
def eng():
    from cmgan_amd.engine import Engine
    return Engine(device=DEV)


@pytest.fixture(scope="module")
def TILE():
    from cmgan_amd.mixing import tile
    return tile()


def _clean(kind, B, L, rng):
    if kind == "noise":
        return (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    if kind == "zeros":                                         # a leading and a trailing stretch of exact zeros
        x = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
        x[:, :L // 4] = 0.0
        x[:, L - L // 3:] = 0.0
        return x
    x = np.zeros((B, L), dtype=np.float32)                      # a full-scale step
    x[:, L // 2:] = 1.0
    return x


def _rirs(R, K, rng):
    """R decaying-noise responses of exactly K taps whose largest tap sits at the front, inside and at the very end."""
    h = rng.standard_normal((R, K)) * np.exp(-np.arange(K) / (0.15 * K + 1.0))
    for r in range(R):
        h[r, [0, K // 3, K - 1][r % 3]] = 1.5 * (-1) ** r
    return h.astype(np.float32)


def _tables(B, bank_items, rng, L):
    """Per-row noise draws over a bank whose items are 1 sample, shorter than L and longer than L."""
    lens = np.array([it.size for it in bank_items], dtype=np.int64)
    starts = np.cumsum(lens) - lens
    item = rng.integers(0, len(lens), B)
    item[0] = min(1, len(lens) - 1)
    off = rng.integers(0, 10 ** 6, B).astype(np.int64)          # far beyond the item: the offset wraps too
    return starts[item], lens[item], off


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _mix(eng, clean, bank, start, length, off, snr, rir=None, idx=None, rlen=None, peak=PEAK, early=-1):
    noisy, target, info = eng.mix(_t(clean), _t(bank), _t(start), _t(length), _t(off), _t(snr),
                                  None if rir is None else _t(rir), None if rir is None else _t(idx),
                                  None if rir is None else _t(rlen), peak=peak, early=early)
    return noisy.cpu().numpy(), target.cpu().numpy(), [v.cpu().numpy() for v in info]


def _check_rows(tag, got, rows, clean, h_rows, L, early):
    """The bound of test_kernel_matches_the_float64_model, row by row.  Returns the worst error / bound ratio."""
    noisy, target, (g, scale, ps, pn) = got
    worst = 0.0
    for b, r in enumerate(rows):
        h = h_rows[b]
        K = 1 if h is None else h.size
        e_conv = 2.0 * K * U64 * (1.0 if h is None else float(np.sum(np.abs(h.astype(np.float64))))) * float(np.max(np.abs(clean[b])))
        s = r["scale"]
        bound_n = U32 * np.abs(r["noisy"]) + s * (e_conv + 2.0 * L * U64 * r["g"] * np.abs(r["noise"]))
        bound_t = U32 * np.abs(r["target"]) + s * e_conv
        for name, a, w, bd in (("noisy", noisy[b], r["noisy"], bound_n), ("target", target[b], r["target"], bound_t)):
            err = np.abs(a.astype(np.float64) - w)
            bad = err > bd
            assert not bad.any(), (f"{tag} row {b} {name}: {int(bad.sum())} of {L} outside the bound, worst "
                                   f"err {err[bad].max():.3e} at bound {bd[bad][np.argmax(err[bad])]:.3e}")
            worst = max(worst, float(np.max(err / np.maximum(bd, 1e-300))))
        for name, a, w in (("g", g[b], r["g"]), ("scale", scale[b], r["scale"]), ("Ps", ps[b], r["Ps"]), ("Pn", pn[b], r["Pn"])):
            assert abs(a - w) <= 1e-12 * abs(w), f"{tag} row {b} info.{name}: got {a!r}, model {w!r}"
        if early < 0 and s == 1.0:
            assert np.array_equal(target[b].view(np.uint32), clean[b].view(np.uint32)), f"{tag} row {b}: target is not clean's bits"
    return worst


# ------------------------------------------------------------------ 1. the kernels against the model
def test_kernel_matches_the_float64_model(eng, TILE):
    """Elementwise, against the model's float64 value `want` BEFORE its rounding to float32:

        |noisy - want|  <= 2^-24 |want| + s (E_conv + 2 L 2^-53 g |n|)
        |target - want| <= 2^-24 |want| + s E_conv,        E_conv = 2 K 2^-53 sum|h| max|clean|

    2^-24 |want| is the one rounding to float32 (round to nearest, half an ulp).  The rest is float64 summation in an
    order that differs between the kernels and numpy: a K-term sum of products carries at most K 2^-53 sum|h_k x_k| <=
    K 2^-53 sum|h| max|clean| in either order (Higham, gamma_K to first order), hence 2 K for the pair; Ps and Pn are
    L-term sums of non-negative terms, each within L 2^-53 relative in either order, and g = sqrt(Ps / (Pn c)) takes half
    of the relative error of each, so the two orders differ by at most 2 L 2^-53 relative in g, which reaches the output
    through g |n|.  The peak scale s (<= 1) multiplies both.  info is held to 1e-12 relative; with s == 1 and early == -1
    the target must be clean's bits."""
    rng = np.random.default_rng(2024)
    B = 5
    lengths = [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 4000]
    cases = [(L, K) for L in lengths for K in (None, 1, 2, 63, 65, 1000)] + [(300, 20000)]
    worst = 0.0
    for L, K in cases:
        bank_items = [rng.standard_normal(n).astype(np.float32) for n in (1, max(L // 3, 1), L + 17)]
        bank = np.concatenate(bank_items)
        start, length, off = _tables(B, bank_items, rng, L)
        snr = rng.uniform(0.0, 20.0, B).astype(np.float32)
        rir = idx = rlen = None
        if K is not None:
            rir = np.zeros((4, K + 5), dtype=np.float32)        # rows padded with zeros beyond their own length
            rir[:3, :K] = _rirs(3, K, rng)
            rir[3, :max(K // 2, 1)] = _rirs(1, max(K // 2, 1), rng)[0]
            idx = np.array([0, 1, 2, 3, 1], dtype=np.int32)
            rlen = np.array([K, K, K, max(K // 2, 1), K], dtype=np.int32)
        for kind in ("noise", "zeros", "step"):
            clean = _clean(kind, B, L, rng)
            for early in (-1, 0, 40, (K or 1) + 3):
                h_rows = [None if rir is None else rir[idx[b], :rlen[b]] for b in range(B)]
                rows = M.mix_batch(clean, bank, start, length, off, snr, rir, idx, rlen, PEAK, early)
                tag = f"L={L} K={K} {kind} early={early}"
                got = _mix(eng, clean, bank, start, length, off, snr, rir, idx, rlen, PEAK, early)
                worst = max(worst, _check_rows(tag + " B=5", got, rows, clean, h_rows, L, early))
                got1 = _mix(eng, clean[:1], bank, start[:1], length[:1], off[:1], snr[:1], rir,
                            None if rir is None else idx[:1], None if rir is None else rlen[:1], PEAK, early)
                worst = max(worst, _check_rows(tag + " B=1", got1, rows[:1], clean[:1], h_rows[:1], L, early))
    print(f"[mix] worst error / bound over the sweep: {worst:.3f}")


# ------------------------------------------------------------------ 2. edge semantics
def _small(rng, B=3, L=1500, K=40):
    clean = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    bank = rng.standard_normal(2000).astype(np.float32)
    start = np.array([0, 100, 700], dtype=np.int64)[:B]
    length = np.array([2000, 333, 1300], dtype=np.int64)[:B]
    off = np.array([5, 4000, 77], dtype=np.int64)[:B]
    rir = _rirs(3, K, rng)
    idx = np.array([0, 1, 2], dtype=np.int32)[:B]
    rlen = np.full(B, K, dtype=np.int32)
    return clean, bank, start, length, off, rir, idx, rlen


def test_silent_noise_and_silent_clean_give_zero_gain(eng):
    rng = np.random.default_rng(7)
    clean, bank, start, length, off, rir, idx, rlen = _small(rng)
    snr = np.full(3, 5.0, dtype=np.float32)
    rows = M.mix_batch(clean, bank * 0, start, length, off, snr, rir, idx, rlen, 100.0, -1)
    noisy, target, (g, scale, ps, pn) = _mix(eng, clean, bank * 0, start, length, off, snr, rir, idx, rlen, 100.0, -1)
    assert np.all(g == 0.0) and np.all(pn == 0.0) and np.all(scale == 1.0)
    # noisy is the reverberant speech alone: its float64 value rounded once - bitwise what the early >= K target is
    _, speech, _ = _mix(eng, clean, bank, start, length, off, snr, rir, idx, rlen, 100.0, 10 ** 6)
    assert np.array_equal(noisy, speech)
    for b in range(3):
        assert np.max(np.abs(noisy[b] - rows[b]["speech"])) <= U32 * np.max(np.abs(rows[b]["speech"])) * 1.0001
    noisy, target, (g, scale, ps, pn) = _mix(eng, clean * 0, bank, start, length, off, snr, rir, idx, rlen, PEAK, 0)
    assert np.all(g == 0.0) and np.all(ps == 0.0) and np.all(pn > 0.0)
    assert np.all(noisy == 0.0) and np.all(target == 0.0)


def test_peak_guard_and_achieved_snr(eng):
    rng = np.random.default_rng(8)
    clean, bank, start, length, off, rir, idx, rlen = _small(rng)
    snr = np.array([20.0, 12.5, 3.0], dtype=np.float32)
    # not triggered: scale is exactly 1 and the dry target is clean's bits
    noisy, target, (g, scale, ps, pn) = _mix(eng, clean, bank, start, length, off, snr, rir, idx, rlen, 50.0, -1)
    assert np.all(scale == 1.0)
    assert np.array_equal(target.view(np.uint32), clean.view(np.uint32))
    got_snr = 10.0 * np.log10(ps / (g * g * pn))
    assert np.max(np.abs(got_snr - snr.astype(np.float64))) < 1e-9, got_snr
    # triggered at -30 dB: the peak holds, and the target carries the same scale
    low = np.full(3, -30.0, dtype=np.float32)
    pk = float(np.float32(PEAK))
    for early in (-1, 15):
        noisy, target, (g, scale, ps, pn) = _mix(eng, clean, bank, start, length, off, low, rir, idx, rlen, PEAK, early)
        rows = M.mix_batch(clean, bank, start, length, off, low, rir, idx, rlen, PEAK, early)
        assert np.all(scale < 1.0)
        assert np.max(np.abs(noisy)) <= pk
        assert np.all(np.max(np.abs(noisy), axis=1) >= pk * (1 - 1e-6))           # the guard scales TO the peak
        got_snr = 10.0 * np.log10(ps / (g * g * pn))
        assert np.max(np.abs(got_snr + 30.0)) < 1e-9
        for b in range(3):
            assert abs(scale[b] - rows[b]["scale"]) <= 1e-12 * rows[b]["scale"]
            unscaled = rows[b]["target"] / rows[b]["scale"]
            want = (unscaled * scale[b]).astype(np.float32)                          # the SAME s as noisy got
            assert np.max(np.abs(target[b] - want)) <= np.spacing(np.max(np.abs(want)))


# ------------------------------------------------------------------ 3. determinism
def test_bit_identical_between_calls_and_row_independent(eng, TILE):
    rng = np.random.default_rng(9)
    B, L, K = 5, 2 * TILE + 77, 1500
    clean = (0.2 * rng.standard_normal((B, L))).astype(np.float32)
    bank = rng.standard_normal(5000).astype(np.float32)
    start = rng.integers(0, 1000, B).astype(np.int64)
    length = rng.integers(1, 4000, B).astype(np.int64)
    off = rng.integers(0, 10 ** 5, B).astype(np.int64)
    snr = rng.uniform(-30, 10, B).astype(np.float32)
    rir = _rirs(3, K, rng)
    idx = np.array([2, 0, 1, 2, 0], dtype=np.int32)
    rlen = np.array([K, K - 1, 700, 1025, 1], dtype=np.int32)
    a = _mix(eng, clean, bank, start, length, off, snr, rir, idx, rlen, PEAK, 80)
    b = _mix(eng, clean, bank, start, length, off, snr, rir, idx, rlen, PEAK, 80)
    for x, y in zip([a[0], a[1], *a[2]], [b[0], b[1], *b[2]]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    r = slice(3, 4)
    one = _mix(eng, clean[r], bank, start[r], length[r], off[r], snr[r], rir, idx[r], rlen[r], PEAK, 80)
    assert np.array_equal(one[0][0].view(np.uint32), a[0][3].view(np.uint32))
    assert np.array_equal(one[1][0].view(np.uint32), a[1][3].view(np.uint32))
    for x, y in zip(one[2], a[2]):
        assert x[0].tobytes() == y[3].tobytes()


# ------------------------------------------------------------------ 4. hipGraph
def test_captured_mix_replays_with_new_device_side_draws(eng):
    rng = np.random.default_rng(10)
    clean, bank, start, length, off, rir, idx, rlen = _small(rng)
    snr = np.array([10.0, 0.0, 5.0], dtype=np.float32)
    dev = [_t(v) for v in (clean, bank, start, length, off, snr, rir, idx, rlen)]
    call = lambda: eng.mix(dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6], dev[7], dev[8], peak=PEAK, early=20)
    eager = call()                                              # the warm-up call (grows the workspace)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_noisy, g_target, g_info = call()
    graph.replay()
    assert torch.equal(g_noisy, eager[0]) and torch.equal(g_target, eager[1])
    # new draws, written in place into the tensors the graph reads
    dev[5].copy_(_t(np.array([-30.0, 7.5, 19.0], dtype=np.float32)))
    dev[4].copy_(_t(np.array([1234, 0, 999999], dtype=np.int64)))
    dev[2].copy_(_t(np.array([0, 40, 600], dtype=np.int64)))
    dev[7].copy_(_t(np.array([2, 2, 0], dtype=np.int32)))
    dev[8].copy_(_t(np.array([17, 40, 1], dtype=np.int32)))
    graph.replay()
    again = call()
    assert not torch.equal(again[0], eager[0])
    assert torch.equal(g_noisy, again[0]) and torch.equal(g_target, again[1])
    for x, y in zip(g_info, again[2]):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ 5. the front end
def _banks(rng):
    from cmgan_amd.mixing import NoiseBank, RirBank
    noise = [rng.standard_normal(n).astype(np.float32) for n in (1, 300, 5000, 1234)]
    rirs = [_rirs(1, k, rng)[0] for k in (1, 30, 200)]
    return noise, rirs, NoiseBank.from_arrays(noise, device=DEV), RirBank.from_arrays(rirs, device=DEV)


def _model_of_draw(clean, nb, rb, d, peak, early):
    """The model fed with a mixer's draws, read back here once."""
    bank = nb.data.cpu().numpy()
    rir = rb.data.cpu().numpy() if rb is not None else None
    g = lambda t: None if t is None else t.cpu().numpy()
    return M.mix_batch(clean, bank, g(d.noise_start), g(d.noise_len), g(d.noise_off), g(d.snr_db), rir,
                       g(d.rir_index), g(d.rir_len), peak, early if rb is not None else -1)


def _assert_rows32(tag, got, rows, key):
    """Against the model's value rounded to float32: the kernel's float64 value may round the other way where the two
    float64 sums straddle a tie, so up to one float32 ulp of the row's peak, 2 * 2^-24 max|want|."""
    for b, r in enumerate(rows):
        want = r[key].astype(np.float32).astype(np.float64)
        err = np.max(np.abs(got[b].astype(np.float64) - want))
        assert err <= 2.0 * U32 * np.max(np.abs(want)) + 1e-30, f"{tag} row {b} {key}: {err:.3e}"


def test_dynamic_mixer_reproduces_the_model_and_its_seed(eng):
    from cmgan_amd.mixing import DynamicMixer
    rng = np.random.default_rng(11)
    noise, rirs, nb, rb = _banks(rng)
    B, L = 6, 1700
    clean = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    cd = _t(clean)

    def mixer(seed, **kw):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(seed)
        return DynamicMixer(eng, nb, rb, snr_db=(-5.0, 15.0), early_ms=2.0, p_reverb=0.5, generator=gen, **kw)

    m1, m2 = mixer(5), mixer(5)
    assert m1.early == 32 and len(m1.rir_bank) == len(rb) + 1
    t1, n1, i1 = m1(cd)
    t2, n2, i2 = m2(cd)
    assert torch.equal(t1, t2) and torch.equal(n1, n2) and all(torch.equal(a, b) for a, b in zip(i1, i2))
    d = m1.last_draw
    start, length, off = d.noise_start.cpu().numpy(), d.noise_len.cpu().numpy(), d.noise_off.cpu().numpy()
    item_starts = nb.start.cpu().tolist()
    assert all(s in item_starts for s in start.tolist()) and np.all(off >= 0) and np.all(off < length)
    snr = d.snr_db.cpu().numpy()
    assert np.all(snr >= -5.0) and np.all(snr <= 15.0)
    idx = d.rir_index.cpu().numpy()
    assert np.all(idx >= 0) and np.all(idx <= len(rb))           # len(rb) = the identity row of the dry rows
    rows = _model_of_draw(clean, nb, m1.rir_bank, d, m1.peak, m1.early)
    _assert_rows32("mixer", n1.cpu().numpy(), rows, "noisy")
    _assert_rows32("mixer", t1.cpu().numpy(), rows, "target")
    for b, r in enumerate(rows):
        assert abs(float(i1.g[b]) - r["g"]) <= 1e-12 * r["g"]
    # the stream of draws advances: a second call mixes differently, and the same way for both mixers
    t1b, n1b, _ = m1(cd)
    t2b, n2b, _ = m2(cd)
    assert torch.equal(n1b, n2b) and not torch.equal(n1b, n1)
    # no RIR bank: the target is the clean batch itself
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    dry = DynamicMixer(eng, nb, None, snr_db=(10.0, 10.0), generator=gen, peak=100.0)
    t, n, info = dry(cd)
    assert torch.equal(t, cd) and torch.all(info.scale == 1.0)


def test_mixing_loader_feeds_a_generator_train_step(eng):
    """An in-memory clean set through MixingLoader and the DevicePrefetcher that Trainer wraps its loaders in, at the
    shape of test_generator_train_step_matches_the_reference_trainer (2 x 800 samples = 9 frames): every batch the
    prefetcher hands out is the model's mix of that batch, and one generator step on the first has finite losses."""
    from cmgan_amd.data import DevicePrefetcher
    from cmgan_amd.mixing import DynamicMixer, MixingLoader
    from cmgan_amd.training import AdamW, GeneratorTrain, generator_train_step
    from oracle.weights import make_state_dict
    rng = np.random.default_rng(12)
    noise, rirs, nb, rb = _banks(rng)
    B, L, batches = 2, 800, 4
    clips = (0.1 * rng.standard_normal((batches * B, L))).astype(np.float32)
    ds = [(torch.from_numpy(clips[i]), L) for i in range(len(clips))]
    loader = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=False)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    mixer = DynamicMixer(eng, nb, rb, snr_db=(0.0, 20.0), early_ms=1.0, generator=gen)
    draws = []
    mixer_call = mixer.draw
    mixer.draw = lambda n: draws.append(mixer_call(n)) or draws[-1]            # keep every batch's draws for the model
    ml = MixingLoader(loader, mixer)
    assert len(ml) == batches
    net = GeneratorTrain(make_state_dict(seed=0), engine=eng)
    opt = AdamW(eng, net.param_bucket, net.grad_bucket, lr=5e-4)
    seen = []
    for k, (target, noisy, length) in enumerate(DevicePrefetcher(ml, torch.device(DEV))):
        assert target.is_cuda and noisy.is_cuda and tuple(noisy.shape) == (B, L) and length.tolist() == [L] * B
        if k == 0:
            loss, terms = generator_train_step(net, opt, target, noisy)
            assert np.isfinite(float(loss)) and bool(torch.isfinite(terms).all())
        seen.append((target.clone(), noisy.clone()))
    assert len(seen) == len(draws) == batches
    for k, (target, noisy) in enumerate(seen):
        rows = _model_of_draw(clips[k * B:(k + 1) * B], nb, mixer.rir_bank, draws[k], mixer.peak, mixer.early)
        _assert_rows32(f"batch {k}", noisy.cpu().numpy(), rows, "noisy")
        _assert_rows32(f"batch {k}", target.cpu().numpy(), rows, "target")


# ------------------------------------------------------------------ 6. the mixer's stages, against the recorded bits
def test_mixer_gives_the_recorded_bits(eng):
    """The 12 configurations of tests/mixer_cases.py - every stage alone, the usual pairs and everything at once, B = 3,
    L = 1536 - give the bits DynamicMixer gave at the commit before its constructor, draws and call were taken apart into
    helpers and stages (tests/golden/make_mixer_bits.py): target, noisy, every info vector, and every tensor of last_draw,
    last_stretch and last_level; a field that was None is None."""
    import os
    import mixer_cases as C
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixer_parent_bits.npz"))
    names = []
    for name, mixer, clean in C.bits_configs(eng):
        fields = C.mixed_fields(mixer, clean)
        assert sorted(f"{name}/{k}" for k, _ in fields) == sorted(k for k in want.files if k.startswith(name + "/")), name
        for key, t in fields:
            if want[f"{name}/{key}"].dtype.kind == "U":
                assert t is None and str(want[f"{name}/{key}"]) == "None", f"{name} {key}: recorded as None, got {t}"
            else:
                assert t is not None, f"{name} {key}: None, recorded as a tensor"
                C.assert_recorded_bits(name, {key: t}, want)
        names.append(name)
    assert len(names) == 12
