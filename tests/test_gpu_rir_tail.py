"""cmgan_rir_tail / Engine.rir_tail on the GPU against the long-double model of tests/rir_tail_model.py, within the bounds
that model derives (its docstring): every tail sample and every fitted level; exactly - the taps below the junction, the
zeros beyond the end, the lengths and the status words; junctions and ends inside a tile and on its edges, the rows that are
left untouched, filterbanks from one tap to the longest, bit reproducibility and row independence, hipGraph replay, and the
front end (RirBank.simulate and DynamicMixer with RoomSampler(tail_ms=)).

The banks are exponentially decaying seeded noise behind a direct spike (rir_stats_model.decaying_noise): no image-source
call is needed to test these kernels.  Each case also asserts what keeps it from passing empty-handed: more than half of the
tail samples are non-zero, and the tail's peak lies above 1e-4 of the row's."""
import functools

import numpy as np
import pytest
import torch

import rir_stats_model as SM
import rir_tail_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS = 16000
W = 64
W_MS = 1000.0 * W / FS


@pytest.fixture(scope="module")
def eng():
    from cmgan_amd.engine import Engine
    return Engine(device=DEV)


@pytest.fixture(scope="module")
def T():
    from cmgan_amd import _lib
    return int(_lib.load().cmgan_rir_tail_tile())


# ------------------------------------------------------------------ inputs (pure numpy: importable without a GPU)
@functools.lru_cache(maxsize=None)
def filters(NB, NF):
    """The test filterbanks: octave bands where the length allows a design (band 5 of the longest silenced), seeded noise
    for the short one, {1} for NF = 1."""
    from cmgan_amd.mixing import octave_filterbank
    if NB == 0:
        return None
    if NF == 1:
        return np.ones((NB, 1))
    if NF >= 63:
        bank = octave_filterbank(FS, NB, NF, f0=62.5).numpy().copy()
        bank[5] = 0.0
        return bank
    return np.random.default_rng(100 * NB + NF).standard_normal((NB, NF)) / np.sqrt(NF)


def noise_bank(R, K, seed, db_per_sample=0.05):
    return np.stack([SM.decaying_noise(seed + r, K, db_per_sample, k0=3 * r) for r in range(R)])


def decays(R, NB, seed):
    """60 dB times of 0.04 .. 0.1 s: 640 .. 1600 samples, so a tail of a few tiles falls by tens of dB and stays normal."""
    return np.random.default_rng(seed).uniform(0.04, 0.1, (R, max(NB, 1)))


def run(eng, bank, length, n_taps, decay, seed, filt, ld=None):
    """Engine.rir_tail on copies of the inputs: (rows, length, gain, status) as numpy."""
    R, K = bank.shape
    store = torch.zeros(R, ld or K, dtype=torch.float32, device=DEV)
    store[:, :K] = torch.from_numpy(bank)
    rir = store[:, :K]
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
    ln = dev(length, torch.int32)
    out, ln2, tail = eng.rir_tail(rir, ln, dev(n_taps, torch.int32), dev(decay, torch.float64), dev(seed, torch.int64),
                                  None if filt is None else dev(filt, torch.float64), fs=FS, window_ms=W_MS)
    assert out is rir and ln2 is ln
    if ld:
        assert not store[:, K:].any()                              # the padding between rows is never written
    return rir.cpu().numpy(), ln.cpu().numpy(), tail.gain.cpu().numpy(), tail.status.cpu().numpy()


def compare(got, bank, length, n_taps, decay, seed, filt, want_status):
    """Every row against the model; returns the models."""
    rows, ln, gain, status = got
    models = M.rir_tail(bank, length, n_taps, decay, seed, filt, W, FS)
    assert status.tolist() == [m["status"] for m in models] == list(want_status)
    assert ln.tolist() == [m["length"] for m in models]
    for r, m in enumerate(models):
        kx, kend = m["kx"], m["kend"]
        if m["status"]:
            assert np.array_equal(rows[r].view(np.int32), bank[r].view(np.int32)) and not gain[r].any(), r
            continue
        assert np.array_equal(rows[r, :kx].view(np.int32), bank[r, :kx].view(np.int32)), r
        assert not rows[r, kend:].any() and np.array_equal(rows[r, kend:].view(np.int32), np.zeros(len(rows[r]) - kend, np.int32)), r
        err = np.abs(rows[r, kx:kend].astype(np.float64) - m["y"][kx:kend])
        assert np.all(np.isfinite(m["bound"])) and np.all(err <= m["bound"][kx:kend]), (r, float(np.max(err / m["bound"][kx:kend])))
        assert np.all(np.abs(gain[r] - m["gain"]) <= m["gain_bound"]), (r, gain[r], m["gain"], m["gain_bound"])
        # not empty-handed, and a bound that would catch a wrong index: far below the samples it guards
        tail = rows[r, kx:kend]
        assert np.count_nonzero(tail) > 0.5 * tail.size and np.max(np.abs(tail)) > 1e-4 * np.nanmax(np.abs(rows[r])), r
        assert np.median(m["bound"][kx:kend]) < 1e-5 * np.median(np.abs(m["y"][kx:kend])), r
    return models


# ------------------------------------------------------------------ 1. values
def test_broad_band_rows_junctions_and_ends_at_the_tile_edges(eng, T):
    K = 2 * T + 3
    bank = noise_bank(4, K, 10)
    length = np.array([T - 5, T, T + 40, T + 9], dtype=np.int32)
    n_taps = np.array([K + 100, K - 17, T + 39, K], dtype=np.int32)
    decay = decays(4, 0, 1)
    decay[3, 0] = np.nan
    seed = np.array([5, -6, 7, 8], dtype=np.int64)
    got = run(eng, bank, length, n_taps, decay, seed, None)
    models = compare(got, bank, length, n_taps, decay, seed, None, [0, 0, M.NOTHING, M.DECAY])
    assert got[1].tolist() == [K, K - 17, T + 40, T + 9] and models[0]["kend"] == K


def test_one_band_of_one_tap_is_the_broad_band_tail(eng, T):
    K = 2 * T + 3
    bank = noise_bank(2, K, 20)
    length = np.array([T - 5, T + 1], dtype=np.int32)
    n_taps = np.array([K, K - 1], dtype=np.int32)
    decay, seed = decays(2, 1, 2), np.array([11, 12], dtype=np.int64)
    banded = run(eng, bank, length, n_taps, decay, seed, filters(1, 1))
    compare(banded, bank, length, n_taps, decay, seed, filters(1, 1), [0, 0])
    broad = run(eng, bank, length, n_taps, decay, seed, None)
    models = compare(broad, bank, length, n_taps, decay, seed, None, [0, 0])
    for r, m in enumerate(models):                                 # both within the bound of the one model: of each other
        assert np.all(np.abs(banded[0][r].astype(np.float64) - broad[0][r]) <= 2 * m["bound"] + 2.0 ** -149)


def test_three_bands_of_nine_taps(eng, T):
    K, NB, NF = 2 * T + 3, 3, 9
    bank = noise_bank(3, K, 30)
    length = np.array([T + 11, W + 4, W + 3], dtype=np.int32)      # the last window starts one sample before the row
    n_taps = np.array([K, 2 * T, K], dtype=np.int32)
    decay, seed = decays(3, NB, 3), np.array([21, 22, 23], dtype=np.int64)
    got = run(eng, bank, length, n_taps, decay, seed, filters(NB, NF))
    compare(got, bank, length, n_taps, decay, seed, filters(NB, NF), [0, 0, M.WINDOW])


def test_eight_bands_of_the_longest_filter(eng, T):
    K, NB, NF = 4 * T + 3, 8, 1023
    kx = 511 + W + 1                                               # the window starts at sample 1; the span outgrows a tile
    bank = noise_bank(3, K, 40, db_per_sample=0.03)
    # one smaller: the window starts at sample 0 and still fits (k_x - D - W = 0); two smaller: it does not
    length = np.array([kx, kx - 1, kx - 2], dtype=np.int32)
    n_taps = np.array([K, K, K], dtype=np.int32)
    decay, seed = decays(3, NB, 4), np.array([31, 32, 33], dtype=np.int64)
    filt = filters(NB, NF)
    got = run(eng, bank, length, n_taps, decay, seed, filt)
    models = compare(got, bank, length, n_taps, decay, seed, filt, [0, 0, M.WINDOW])
    assert got[2][0, 5] == 0.0 and models[0]["gain"][5] == 0.0 and np.all(np.delete(got[2][0], 5) > 0)   # the silent band
    # it contributes nothing: the same taps without it, where the other bands keep their order
    keep = [0, 1, 2, 3, 4, 6, 7]
    less = run(eng, bank[:1], length[:1], n_taps[:1], decay[:1, keep], seed[:1], filt[keep])
    assert np.array_equal(less[0][0].view(np.int32), got[0][0].view(np.int32))


def test_non_finite_sample_in_the_fits_reach_leaves_the_row(eng, T):
    K = 2 * T + 3
    bank = noise_bank(3, K, 50)
    kx = T + 30
    bank[0, kx - W] = np.inf                                       # the fit's first sample
    bank[1, kx - W - 1] = np.nan                                   # one before it: not read
    bank[2, kx] = np.nan                                           # at the junction: overwritten, not read
    length, n_taps = np.full(3, kx, dtype=np.int32), np.full(3, K, dtype=np.int32)
    decay, seed = decays(3, 0, 5), np.array([41, 42, 43], dtype=np.int64)
    got = run(eng, bank, length, n_taps, decay, seed, None)
    assert got[3].tolist() == [M.NONFINITE, 0, 0] and got[1].tolist() == [kx, K, K]
    assert np.array_equal(got[0][0].view(np.int32), bank[0].view(np.int32)) and np.all(np.isfinite(got[0][1:, kx:]))
    compare((got[0][1:], got[1][1:], got[2][1:], got[3][1:]), bank[1:], length[1:], n_taps[1:], decay[1:], seed[1:], None, [0, 0])


# ------------------------------------------------------------------ 2. bits
@pytest.mark.parametrize("NB,NF", [(0, 1), (3, 9)])
def test_bits_do_not_depend_on_the_run_the_batch_the_stride_or_the_padding(eng, T, NB, NF):
    K = 2 * T + 3
    filt = filters(NB, NF)
    bank = noise_bank(4, K, 60)
    bank[2] = bank[0]                                              # rows 0 and 2: equal inputs
    length = np.array([T - 5, T + 11, T - 5, T + 70], dtype=np.int32)
    n_taps = np.array([K - 9, K, K - 9, K - 1], dtype=np.int32)
    decay = decays(4, NB, 6)
    decay[2] = decay[0]
    seed = np.array([51, 52, 51, 53], dtype=np.int64)
    first = run(eng, bank, length, n_taps, decay, seed, filt)
    again = run(eng, bank, length, n_taps, decay, seed, filt)
    bits = lambda a: a.view(np.int32) if a.dtype == np.float32 else a.view(np.int64) if a.dtype == np.float64 else a
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, again)) and not first[3].any()
    rows, _, gain, _ = first
    assert np.array_equal(bits(rows[0]), bits(rows[2])) and np.array_equal(bits(gain[0]), bits(gain[2]))      # the same seed
    for r in range(4):                                             # a row alone
        alone = run(eng, bank[r:r + 1], length[r:r + 1], n_taps[r:r + 1], decay[r:r + 1], seed[r:r + 1], filt)
        assert np.array_equal(bits(alone[0][0]), bits(rows[r])) and np.array_equal(bits(alone[2][0]), bits(gain[r])), r
    # a wider bank with padding between the rows: equal bits below k_end (n_taps is what ends the row, not K)
    wide = np.concatenate([bank, noise_bank(4, T, 70)], axis=1)
    spaced = run(eng, wide, length, n_taps, decay, seed, filt, ld=K + T + 13)
    for r in range(4):
        assert np.array_equal(bits(spaced[0][r, :n_taps[r]]), bits(rows[r, :n_taps[r]])) and not spaced[0][r, n_taps[r]:].any(), r
    assert np.array_equal(bits(spaced[2]), bits(gain)) and spaced[1].tolist() == first[1].tolist()
    # another seed: another tail from the same level
    other = run(eng, bank, length, n_taps, decay, seed + 1000, filt)
    assert np.array_equal(bits(other[2]), bits(gain))
    for r in range(4):
        tail = slice(length[r], n_taps[r])
        assert np.count_nonzero(other[0][r, tail] == rows[r, tail]) < 0.01 * (n_taps[r] - length[r]), r


# ------------------------------------------------------------------ 3. hipGraph
def test_captured_call_replays_the_eager_one(eng, T):
    K, NB, NF = 2 * T + 3, 3, 9
    bank, filt = noise_bank(3, K, 80), filters(NB, NF)
    length = np.array([T - 5, T + 11, 20], dtype=np.int32)         # row 2: no window fits
    n_taps = np.array([K, K - 30, K], dtype=np.int32)
    decay, seed = decays(3, NB, 7), np.array([61, 62, 63], dtype=np.int64)
    eager = run(eng, bank, length, n_taps, decay, seed, filt)      # (also grows the workspace before the capture)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
    rir, ln = dev(bank, torch.float32), dev(length, torch.int32)
    args = (dev(n_taps, torch.int32), dev(decay, torch.float64), dev(seed, torch.int64), dev(filt, torch.float64))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, _, tail = eng.rir_tail(rir, ln, *args, fs=FS, window_ms=W_MS)
    for _ in range(2):                                             # the call works in place: its inputs are put back first
        rir.copy_(dev(bank, torch.float32))
        ln.copy_(dev(length, torch.int32))
        graph.replay()
        got = (rir.cpu().numpy(), ln.cpu().numpy(), tail.gain.cpu().numpy(), tail.status.cpu().numpy())
        assert np.array_equal(got[0].view(np.int32), eager[0].view(np.int32)) and got[1].tolist() == eager[1].tolist()
        assert np.array_equal(got[2].view(np.int64), eager[2].view(np.int64)) and got[3].tolist() == eager[3].tolist() == [0, 0, M.WINDOW]


# ------------------------------------------------------------------ 4. the front end
def _sampler(seed, **kw):
    from cmgan_amd.mixing import RoomSampler
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return RoomSampler(dims=((4.0, 3.0, 2.5), (4.0, 3.0, 2.5)), rt60=(0.3, 0.3), generator=gen, **kw)


@pytest.mark.parametrize("bands", [None, 3])
def test_simulated_bank_is_images_to_the_junction_and_a_tail_behind_it(eng, bands):
    from cmgan_amd.mixing import RirBank
    kw = dict(tail_ms=60.0) if bands is None else dict(tail_ms=60.0, bands=bands, tilt=(0.0, 0.1), filter_taps=255)
    R, K = 2, int(0.3 * FS)
    bank = RirBank.simulate(eng, _sampler(91, **kw), R, seconds=0.3, sample_rate=FS)
    twice = RirBank.simulate(eng, _sampler(91, **kw), R, seconds=0.3, sample_rate=FS)
    assert torch.equal(bank.data, twice.data) and torch.equal(bank.length, twice.length)
    assert bank.length.tolist() == [K, K] and bank.tail.status.tolist() == [0, 0] and bool((bank.tail.gain > 0).all())
    # the early part: a plain image-source call with the junctions the sampler drew
    s = _sampler(91, **kw)
    rooms, junction = s.draw(R, K, FS, device=eng.device)
    assert bool((junction < K).all()) and bool((junction >= 960).all()) and s.n_images(K, FS) < _sampler(91).n_images(K, FS)
    if bands is None:
        early, n = eng.rir(rooms, junction, K, s.n_images(K, FS), fs=FS)
    else:
        early, n = eng.rir_bands(rooms, s.draw_bands(rooms), junction, K, s.filters(FS, eng.device), s.n_images(K, FS), fs=FS)
    assert torch.equal(n, junction) and torch.equal(bank.rooms, rooms)
    for r in range(R):
        kx = int(junction[r])
        assert torch.equal(bank.data[r, :kx], early[r, :kx]) and not bool(early[r, kx:].any())
        tail = bank.data[r, kx:]
        assert int(torch.count_nonzero(tail)) > 0.5 * tail.numel() and float(tail.abs().max()) > 1e-4 * float(bank.data[r].abs().max())
    stats = bank.measure(eng, FS, None if bands is None else s.filters(FS, eng.device))
    for name in ("energy", "drr_db", "c50_db", "d50", "ts", "edt", "t20", "t30"):
        assert bool(torch.isfinite(getattr(stats, name)).all()), name


def test_dynamic_mixer_with_tails_for_talkers_and_sources(eng):
    from cmgan_amd.mixing import DynamicMixer, NoiseBank
    rng = np.random.default_rng(33)
    nb = NoiseBank.from_arrays([rng.standard_normal(n).astype(np.float32) for n in (300, 5000)], device=DEV)
    B, L, K = 4, 2100, int(0.3 * FS)
    cd = torch.from_numpy((0.1 * rng.standard_normal((B, L))).astype(np.float32)).to(DEV)

    def mixer(**kw):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(5)
        return DynamicMixer(eng, nb, rooms=_sampler(105, tail_ms=60.0), snr_db=(0.0, 15.0), early_ms=10.0, p_reverb=0.5, peak=100.0,
                            generator=gen, rir_seconds=0.3, sources=(1, 2), room_stats=True, **kw)

    a, b = mixer(), mixer()
    outs = [m(cd) for m in (a, b)]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and bool(torch.isfinite(outs[0][1]).all())
    d, t, sim = a.last_draw, a.last_tail, a.last_bank
    wet = d.rir_index < B
    assert bool(wet.any()) and bool((~wet).any())                  # (seed 5 draws dry and wet rows)
    assert torch.equal(d.rir_len, sim.length[:B]) and torch.equal(d.rir_len, torch.where(wet, t.n_full, torch.ones_like(t.n_full)))
    assert torch.equal(d.src_rir_len, sim.length[B + 1:].reshape(B, 2)) and bool((d.src_rir_len == K).all())
    assert tuple(t.src_junction.shape) == (B, 2) and bool((t.src_junction < K).all())
    for row, kx in zip(sim.data[B + 1:], t.src_junction.flatten().tolist()):
        assert int(torch.count_nonzero(row[kx:])) > 0.5 * (K - kx)
    assert bool(torch.isfinite(a.last_room_stats.t30[wet]).all()) and a.n_images == a.rooms.n_images(K, FS)
