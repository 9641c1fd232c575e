"""The banded room simulator on the GPU (cmgan_amd/csrc/rir.hip; include/cmgan_hip.h, "Room impulse responses in
frequency bands"): Engine.rir_bands against the float64 numpy model of tests/rir_bands_model.py over the kernels' tile
and list edges, band counts and filter lengths, oversized image ranges, invalid rows, bit-reproducibility and row
independence, hipGraph replay with the tables changed in place, and the front end (RirBank.simulate and
DynamicMixer(rooms=...) with a banded RoomSampler) through Engine.mix.

The bound, for every tap (rir_bands_model.rir_bands_row):
    |gpu[k] - h[k]| <= 2^-24 |h[k]| + sum_b sum_j |g_b[j]| 64 2^-53 (K + D + tw) A_b[k + D - j]
                                    + (NB NF + 1) 2^-53 sum_b sum_j |g_b[j] h_b[k + D - j]|
the float32 rounding, the delay term of test_gpu_rir.py's bound (a band is cmgan_rir's sum over K + D taps, with
exp(-m d) one more factor of a few ulps in the amplitude) carried through the filters, and the join's NB NF fused
multiply-adds in float64."""
import functools

import numpy as np
import pytest
import torch

import mix_model as MM
import rir_bands_model as BM
import rir_cases as RC
import rir_model as M
from test_gpu_rir import _check_mix

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS, C = 16000, 343.0
U32 = 2.0 ** -24

ROOM = [4.0, 3.0, 2.5, 1.1, 0.9, 1.3, 2.9, 2.2, 1.6] + [float("nan")] * 6      # (columns 9 - 14 are never read)
WALLS = np.array([0.9, 0.8, 0.85, 0.7, 0.6, 0.95])


@pytest.fixture(scope="module")
def eng():
    from cmgan_amd.engine import Engine
    return Engine(device=DEV)


@pytest.fixture(scope="module")
def TILE():
    from cmgan_amd import _lib
    return int(_lib.load().cmgan_rir_tile())


def _bands(NB, walls=WALLS, air=0.004):
    """Band b: the walls a little more absorbing per band, m_b = air b."""
    return np.array([list(walls * (1.0 - 0.05 * b)) + [air * b] for b in range(NB)])


@functools.lru_cache(maxsize=None)
def _filters(NB, NF):
    if NF == 1:
        return np.array([[1.0 - 0.25 * b] for b in range(NB)])
    return np.random.default_rng(100 * NB + NF).standard_normal((NB, NF)) / np.sqrt(NF)


def _images(K, NF, tw, size=ROOM[0:3]):
    """The image ranges that leave out no image of K + D taps."""
    reach = (K + (NF - 1) // 2 + tw) * C / FS
    return tuple(int(np.ceil(reach / (2 * l))) + 1 for l in size)


def _run(eng, rooms, bands, n_taps, K, filt, N, tw=40, out=None):
    rooms_d = torch.tensor(np.asarray(rooms, dtype=np.float64).reshape(-1, 15), device=DEV)
    bands_d = torch.tensor(np.asarray(bands, dtype=np.float64).reshape(rooms_d.size(0), -1, 7), device=DEV)
    taps_d = torch.tensor(np.asarray(n_taps, dtype=np.int32).reshape(-1), device=DEV)
    filt_d = torch.tensor(np.asarray(filt, dtype=np.float64), device=DEV)
    rir, length = eng.rir_bands(rooms_d, bands_d, taps_d, K, filt_d, N, fs=FS, c=C, tw=tw, out=out)
    assert rir.dtype == torch.float32 and tuple(rir.shape) == (rooms_d.size(0), K) and length.dtype == torch.int32
    return rir.cpu().numpy(), length.cpu().numpy()


def _check(tag, got, rooms, bands, n_taps, K, filt, N, tw=40):
    """Every tap of every row of `got` against the model under the bound; taps >= k_r bit-zero; lengths.  Returns the
    worst error / bound."""
    rir, length = got
    rooms = np.asarray(rooms, dtype=np.float64).reshape(-1, 15)
    bands = np.asarray(bands, dtype=np.float64).reshape(rooms.shape[0], -1, 7)
    worst = 0.0
    for r in range(rooms.shape[0]):
        h, bd, _, _, kr = BM.rir_bands_row(rooms[r], bands[r], int(np.asarray(n_taps).reshape(-1)[r]), K, N, filt, FS, C, tw)
        assert length[r] == kr, f"{tag} row {r}: len {length[r]}, model {kr}"
        assert not rir[r, kr:].view(np.uint32).any(), f"{tag} row {r}: taps >= k_r are not bit-zero"
        err = np.abs(rir[r].astype(np.float64) - h)
        bad = ~(err <= bd)
        assert not bad.any(), (f"{tag} row {r}: {int(bad.sum())} of {K} taps outside the bound, first at {int(np.argmax(bad))}, "
                               f"worst err {np.nanmax(err[bad]):.3e} at bound {bd[bad][np.nanargmax(err[bad])]:.3e}")
        if kr > 1 and BM.row_is_valid(rooms[r], bands[r]):
            assert np.max(np.abs(h)) > 0.0
        worst = max(worst, float(np.max(err[bd > 0] / bd[bd > 0])) if (bd > 0).any() else 0.0)
    return worst


# ------------------------------------------------------------------ 1. the kernels against the model
@pytest.mark.parametrize("tw", [4, 40])
@pytest.mark.parametrize("NB,NF", [(1, 1), (3, 9), (7, 65), (8, 1023)])
@pytest.mark.parametrize("k_of_tile", [lambda T: T - 1, lambda T: T, lambda T: T + 1, lambda T: 2 * T + 3],
                         ids=["TILE-1", "TILE", "TILE+1", "2TILE+3"])
def test_kernels_match_the_float64_model(eng, TILE, k_of_tile, NB, NF, tw):
    """K + D crosses a tile edge of the band kernel wherever K does not: K = TILE - 1 and TILE with D = 4, 32 and 511."""
    K = k_of_tile(TILE)
    filt, bands, N = _filters(NB, NF), _bands(NB), _images(K, NF, tw)
    got = _run(eng, ROOM, bands, [K], K, filt, N, tw)
    worst = _check(f"K={K} NB={NB} NF={NF} tw={tw}", got, ROOM, bands, [K], K, filt, N, tw)
    print(f"[rir_bands] K={K} NB={NB} NF={NF} tw={tw}: worst error / bound {worst:.3f}")


def test_three_rooms_with_different_band_tables_and_lengths(eng, TILE):
    K, NB, NF = 2 * TILE + 3, 3, 9
    dead = np.zeros((NB, 7))                                      # every wall absorbs everything in every band
    dead[:, 6] = [0.0, 0.01, 0.02]
    one_zero = _bands(NB, WALLS * np.array([1, 0, 1, 1, 1, 1.0]), air=0.0)      # one absorbing wall, no air absorption
    rooms = [ROOM, [4.0, 3.0, 2.5, 0.5, 1.0, 1.0, 3.2, 1.7, 1.4] + [0.3] * 6, [4.0, 3.0, 2.5, 1.0, 0.7, 1.3, 2.2, 1.9, 0.8] + [0.0] * 6]
    bands, n_taps, filt, N = [_bands(NB), dead, one_zero], [K, K - 17, 1], _filters(NB, NF), _images(K, NF, 40)
    got = _run(eng, rooms, bands, n_taps, K, filt, N)
    _check("three rooms", got, rooms, bands, n_taps, K, filt, N)
    assert got[1].tolist() == [K, K - 17, 1]
    assert np.count_nonzero(got[0][0]) > K // 2 and 0 < np.count_nonzero(got[0][1]) <= 2 * 40 + NF - 1     # (dead: one window)


def test_one_band_with_a_unit_filter_is_engine_rir(eng, TILE):
    """NB = 1, g = delta, m = 0 against Engine.rir of the same room: both are within their bounds of the one model."""
    K, N = 2 * TILE + 3, _images(2 * TILE + 3, 1, 40)
    room = ROOM[0:9] + list(WALLS)
    bands = np.array([list(WALLS) + [0.0]])
    got = _run(eng, room, bands, [K], K, np.array([[1.0]]), N)
    rooms_d = torch.tensor([room], dtype=torch.float64, device=DEV)
    plain, plain_len = eng.rir(rooms_d, torch.tensor([K], dtype=torch.int32, device=DEV), K, N, fs=FS, c=C, tw=40)
    h, A, kr = M.rir_row(room, K, K, N, FS, C, 40)
    assert kr == K == int(plain_len[0]) == int(got[1][0]) and np.max(np.abs(h)) > 0.01
    assert np.all(np.abs(plain.cpu().numpy()[0].astype(np.float64) - h) <= M.bound(h, A, K, 40))
    hb, bd, _, _, _ = BM.rir_bands_row(room, bands, K, K, N, np.array([[1.0]]), FS, C, 40)
    assert np.array_equal(hb, h) or np.all(np.abs(hb - h) <= 1e-15 * A)          # the two models are one
    assert np.all(np.abs(got[0][0].astype(np.float64) - h) <= bd)


def test_air_absorption_alone_changes_the_late_taps_as_the_model_says(eng, TILE):
    """The same walls in both bands, m = (0, 0.05 Np/m); one-tap filters that pass one band each."""
    K, NB = 2 * TILE + 3, 2
    N = _images(K, 1, 40)
    bands = np.array([list(WALLS) + [0.0], list(WALLS) + [0.05]])
    out, model = [], []
    for pick in ([[1.0], [0.0]], [[0.0], [1.0]]):
        filt = np.array(pick)
        got = _run(eng, ROOM, bands, [K], K, filt, N)
        _check(f"air, filter {pick}", got, ROOM, bands, [K], K, filt, N)
        out.append(got[0][0].astype(np.float64))
        model.append(BM.rir_bands_row(ROOM, bands, K, K, N, filt, FS, C, 40)[0])
    late = slice(K - TILE, K)
    ratio = lambda pair: float(np.sum(pair[1][late] ** 2) / np.sum(pair[0][late] ** 2))
    print(f"[rir_bands] late energy with m = 0.05 over m = 0: model {ratio(model):.6f}, GPU {ratio(out):.6f}")
    assert 0.0 < ratio(model) < 1.0                              # the model: air absorption takes energy out of the late taps
    assert abs(ratio(out) / ratio(model) - 1.0) < 1e-5           # (every tap is within a few 2^-24 of the model's)
    assert not np.array_equal(out[0][:TILE], out[1][:TILE])


def test_more_images_in_a_tile_than_the_on_chip_list_holds(eng, TILE):
    """The lively small room of test_gpu_rir.py with 3 bands: the images that reach the band kernel's last tile are more
    than twice cmgan_rir_list_capacity(), so a round of the scan overflows the list and is consumed in chunks."""
    from cmgan_amd import _lib
    cap = int(_lib.load().cmgan_rir_list_capacity())
    room = [1.2, 1.2, 1.2, 0.3, 0.4, 0.5, 0.9, 0.8, 0.7] + [0.0] * 6
    NB, NF = 3, 9
    D = (NF - 1) // 2
    K = 3 * TILE - D                                              # K + D = 3 TILE: the band kernel's last tile is full
    N = _images(K, NF, 40, room[0:3])
    assert N == (9, 9, 9)
    bands = np.array([[0.97 - 0.01 * b] * 6 + [0.002 * b] for b in range(NB)])
    table = np.array(room)
    table[9:15] = bands[0, 0:6]
    tau = M.images(table, N)[0] * FS / C
    reach = (tau > K + D - TILE - 40) & (tau < K + D - 1 + 40)
    in_last = int(np.sum(reach))
    assert in_last > 2 * cap, (in_last, cap)
    per_col = reach.reshape(-1, 2 * N[2] + 1).sum(1)
    per_round = np.add.reduceat(per_col, np.arange(0, per_col.size, TILE))
    assert per_round.max() > cap, (per_round.max(), cap)
    filt = _filters(NB, NF)
    got = _run(eng, room, bands, [K], K, filt, N)
    worst = _check("lively cube", got, room, bands, [K], K, filt, N)
    print(f"[rir_bands] {in_last} images in the last tile (capacity {cap}): worst error / bound {worst:.3f}")


# ------------------------------------------------------------------ 2. the contract
def test_an_image_range_larger_than_needed_changes_no_bit(eng, TILE):
    K, NB, NF = TILE + 30, 3, 9
    filt, bands, N = _filters(NB, NF), _bands(NB), _images(TILE + 30, 9, 40)
    need = _run(eng, ROOM, bands, [K], K, filt, N)
    _check("needed", need, ROOM, bands, [K], K, filt, N)
    big = _run(eng, ROOM, bands, [K], K, filt, (N[0] + 4, N[1] + 9, N[2] + 30))
    assert np.array_equal(big[0].view(np.uint32), need[0].view(np.uint32))
    cut = _run(eng, ROOM, bands, [K], K, filt, (0, 0, 0))          # fewer than needed: another response, the model's with that N
    _check("N=(0,0,0)", cut, ROOM, bands, [K], K, filt, (0, 0, 0))
    assert not np.array_equal(cut[0], need[0])


def test_invalid_rows_are_zeros_with_length_one(eng, TILE):
    K, NB, NF = TILE + 9, 2, 9
    filt, good, N = _filters(NB, NF), _bands(NB), (3, 3, 3)
    other = [4.0, 3.0, 2.5, 1.0, 0.7, 1.3, 2.2, 1.9, 0.8] + [2.0] * 6                   # (columns 9 - 14: never read, never judged)

    def room_with(at, v):
        row = list(ROOM)
        row[at] = v
        return row, good

    def bands_with(at, v):
        t = good.copy()
        t[at] = v
        return ROOM, t

    bad = [room_with(4, np.nan), room_with(7, np.inf), room_with(1, -2.0), room_with(0, 0.0),      # non-finite, size <= 0
           bands_with((0, 2), np.nan), bands_with((1, 6), np.inf),                                # non-finite in the band table
           bands_with((1, 3), 1.5), bands_with((0, 0), -1e-9), bands_with((1, 6), -1e-9)]         # coefficient, negative m
    rows = [(ROOM, good), bad[0], bad[1], (other, good), *bad[2:], (ROOM, good)]
    rooms, bands = [r for r, _ in rows], [t for _, t in rows]
    n_taps = [K] * len(rows)
    out = (torch.full((len(rows), K), 7.0, dtype=torch.float32, device=DEV),
           torch.full((len(rows),), -5, dtype=torch.int32, device=DEV))
    rir, length = _run(eng, rooms, bands, n_taps, K, filt, N, out=out)
    valid = (0, 3, len(rows) - 1)
    assert length.tolist() == [K if r in valid else 1 for r in range(len(rows))]
    for r in range(len(rows)):
        if r not in valid:
            assert not rir[r].view(np.uint32).any(), r
    _check("invalid rows", (rir, length), rooms, bands, n_taps, K, filt, N)
    for r in valid:                                               # the neighbours are what they are alone
        alone = _run(eng, rooms[r], bands[r], [K], K, filt, N)
        assert np.array_equal(alone[0][0].view(np.uint32), rir[r].view(np.uint32)), r
        assert np.max(np.abs(rir[r])) > 0.0


def test_bit_identical_between_calls_and_row_independent(eng, TILE):
    K, NB, NF = 2 * TILE + 50, 4, 65
    filt, N = _filters(NB, NF), _images(2 * TILE + 50, 65, 40, (3.1, 2.3, 2.5))
    rooms = [ROOM, [3.1, 2.3, 2.6, 1.0, 0.7, 1.3, 2.2, 1.9, 0.8] + [0.0] * 6, [4.0, 3.0, 2.5, 0.4, 0.5, 0.6, 3.1, 1.2, 0.9] + [0.0] * 6]
    bands = [_bands(NB), _bands(NB, WALLS[::-1], 0.0), _bands(NB, WALLS * 0.9, 0.01)]
    n_taps = [K, TILE + 1, K - 3]
    a = _run(eng, rooms, bands, n_taps, K, filt, N)
    b = _run(eng, rooms, bands, n_taps, K, filt, N)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    assert a[1].tolist() == n_taps
    for r in range(3):
        one = _run(eng, rooms[r], bands[r], n_taps[r:r + 1], K, filt, N)
        assert np.array_equal(one[0][0].view(np.uint32), a[0][r].view(np.uint32)), r
        assert one[1][0] == a[1][r] and np.max(np.abs(one[0][0])) > 0.0


def test_captured_call_replays_with_new_room_and_band_tables(eng, TILE):
    K, NB, NF, N = TILE + 30, 3, 9, (4, 4, 5)
    filt = torch.tensor(_filters(NB, NF), dtype=torch.float64, device=DEV)
    rooms = torch.tensor([ROOM, ROOM], dtype=torch.float64, device=DEV)
    bands = torch.tensor(np.stack([_bands(NB), _bands(NB)]), dtype=torch.float64, device=DEV)
    n_taps = torch.tensor([K, K], dtype=torch.int32, device=DEV)
    eager, eager_len = eng.rir_bands(rooms, bands, n_taps, K, filt, N)          # the warm-up call (grows the workspace)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_rir, g_len = eng.rir_bands(rooms, bands, n_taps, K, filt, N)
    graph.replay()
    assert torch.equal(g_rir, eager) and torch.equal(g_len, eager_len)
    # new tables and new lengths, written in place into the tensors the graph reads
    new_rooms = np.array([[3.1, 2.3, 2.6, 1.0, 0.7, 1.3, 2.2, 1.9, 0.8] + [0.0] * 6, ROOM[0:9] + [0.0] * 6])
    new_bands = np.stack([_bands(NB, WALLS[::-1], 0.01), _bands(NB)])
    new_bands[1, 2, 4] = np.nan                                   # row 1 turns invalid
    rooms.copy_(torch.tensor(new_rooms, dtype=torch.float64, device=DEV))
    bands.copy_(torch.tensor(new_bands, dtype=torch.float64, device=DEV))
    n_taps.copy_(torch.tensor([K - 40, K], dtype=torch.int32, device=DEV))
    graph.replay()
    again, again_len = eng.rir_bands(rooms, bands, n_taps, K, filt, N)
    assert not torch.equal(again, eager)
    assert torch.equal(g_rir, again) and torch.equal(g_len, again_len)
    assert again_len.tolist() == [K - 40, 1]
    _check("replayed", (g_rir.cpu().numpy(), g_len.cpu().numpy()), new_rooms, new_bands, [K - 40, K], K, _filters(NB, NF), N)


# ------------------------------------------------------------------ 3. the front end
def _banded_sampler(seed, **kw):
    from cmgan_amd.mixing import RoomSampler
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    opts = dict(bands=4, tilt=(0.2, 0.6), air=[(0.0, 0.0), (0.0, 0.002), (0.001, 0.004), (0.002, 0.01)], filter_taps=63)
    opts.update(kw)
    return RoomSampler(dims=((2.0, 2.0, 2.0), (3.0, 3.0, 2.5)), rt60=(0.06, 0.2), margin=0.3, generator=gen, **opts)


def _model_bank(rooms, bands, n_taps, K, N, filt, rows):
    """test_gpu_rir.py's _model_bank for the banded model: the model's responses as the float32 bank Engine.mix would be
    given, and per tap dh >= |gpu float32 - model float32|."""
    h, bd, length = BM.rir_bands(rooms, bands, n_taps, K, N, filt, FS, C, 40)
    bank = np.zeros((rows, K), dtype=np.float32)
    bank[:len(h)] = h.astype(np.float32)
    dh = np.zeros((rows, K))
    dh[:len(h)] = bd + U32 * np.abs(h)
    if rows > len(h):
        bank[len(h), 0] = 1.0
    return bank, dh, length


def test_simulated_banded_bank_feeds_the_mixer(eng):
    from cmgan_amd.mixing import RirBank, octave_filterbank
    sampler = _banded_sampler(21)
    R, seconds = 3, 0.1
    bank = RirBank.simulate(eng, sampler, R, seconds=seconds, sample_rate=FS)
    K, N = 1600, sampler.n_images(1600, FS)
    assert tuple(bank.data.shape) == (R, K) and tuple(bank.rooms.shape) == (R, 15) and tuple(bank.bands.shape) == (R, 4, 7)
    filt = octave_filterbank(FS, 4, 63).numpy()
    rooms, bands, length = bank.rooms.cpu().numpy(), bank.bands.cpu().numpy(), bank.length.cpu().numpy()
    assert np.all(length >= int(0.06 * FS)) and np.all(length <= K)
    assert np.all(bands[:, 3, 0] < bands[:, 0, 0])                # a positive tilt: more absorption at the top
    _check("simulate", (bank.data.cpu().numpy(), length), rooms, bands, length, K, filt, N)
    rng = np.random.default_rng(22)
    B, L, early = 4, 2100, 160
    clean = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    noise = rng.standard_normal(3000).astype(np.float32)
    start, nlen = np.array([0, 100, 500, 0], dtype=np.int64), np.array([3000, 700, 2500, 1], dtype=np.int64)
    off = np.array([5, 9999, 0, 0], dtype=np.int64)
    snr = np.array([0.0, 5.0, 10.0, 20.0], dtype=np.float32)
    idx = np.array([0, 1, 2, 1], dtype=np.int32)
    rlen = length[idx].astype(np.int32)
    t = lambda a: torch.from_numpy(a).to(DEV)
    noisy, target, info = eng.mix(t(clean), t(noise), t(start), t(nlen), t(off), t(snr), bank.data, t(idx), t(rlen),
                                  peak=100.0, early=early)
    mbank, dh, mlen = _model_bank(rooms, bands, length, K, N, filt, R)
    assert np.array_equal(mlen, length)
    rows = MM.mix_batch(clean, noise, start, nlen, off, snr, mbank, idx, rlen, 100.0, early)
    _check_mix("simulated banded bank", noisy.cpu().numpy(), target.cpu().numpy(), rows, clean, mbank, dh, idx, rlen, L, early)


def test_dynamic_mixer_with_banded_rooms_and_sources(eng):
    from cmgan_amd.mixing import DynamicMixer, NoiseBank, SceneDraw, octave_filterbank
    rng = np.random.default_rng(23)
    nb = NoiseBank.from_arrays([rng.standard_normal(n).astype(np.float32) for n in (1, 300, 5000)], device=DEV)
    B, L, S = 4, 2100, 2
    cd = torch.from_numpy((0.1 * rng.standard_normal((B, L))).astype(np.float32)).to(DEV)

    def mixer(seed, **kw):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(seed)
        return DynamicMixer(eng, nb, rooms=_banded_sampler(seed + 100, **kw), snr_db=(0.0, 15.0), early_ms=10.0, p_reverb=0.5,
                            peak=100.0, generator=gen, rir_seconds=0.05, sources=(0, S))

    m1, m2 = mixer(5), mixer(5)
    K = m1.rir_taps
    assert K == 800 and m1.n_images == m1.rooms.n_images(K, FS)
    t1, n1, i1 = m1(cd)
    t2, n2, i2 = m2(cd)
    assert torch.equal(t1, t2) and torch.equal(n1, n2) and all(torch.equal(a, b) for a, b in zip(i1, i2))
    assert bool(torch.isfinite(n1).all()) and bool(torch.isfinite(t1).all()) and float(n1.abs().max()) > 0.0
    d, bands = m1.last_draw, m1.last_bands
    assert type(d) is SceneDraw and tuple(bands.shape) == (B, 4, 7) and torch.equal(bands, m2.last_bands)
    sim = m1.last_bank
    assert tuple(sim.data.shape) == (B + 1 + B * S, K) and sim.data[B].cpu().tolist() == [1.0] + [0.0] * (K - 1)
    # the bank rows against the model for the drawn tables: the talkers', then the sources' with their room's band table
    filt = octave_filterbank(FS, 4, 63).numpy()
    g = lambda v: v.cpu().numpy()
    rows = (sim.data.cpu().numpy(), sim.length.cpu().numpy())
    _check("talkers", (rows[0][:B], rows[1][:B]), g(d.rooms), g(bands), g(d.rir_len), K, filt, m1.n_images)
    _check("sources", (rows[0][B + 1:], rows[1][B + 1:]), g(d.src_rooms).reshape(B * S, 15), np.repeat(g(bands), S, axis=0),
           g(d.src_rir_len).reshape(B * S), K, filt, m1.n_images)
    assert np.array_equal(rows[1][:B], g(d.rir_len)) and int(sim.length[B]) == 1
    # the draws are those of the same mixer without bands; the responses are not
    plain = mixer(5, bands=None, tilt=(0.0, 0.0), air=None)
    plain(cd)
    for name in d._fields:
        x, y = getattr(d, name), getattr(plain.last_draw, name)
        assert (x is None and y is None) or all(torch.equal(a, b) for a, b in zip(*[v if isinstance(v, tuple) else (v,) for v in (x, y)])), name
    assert plain.last_bands is None and not torch.equal(plain.last_bank.data, sim.data)


# ------------------------------------------------------------------ 4. the recorded bits
@pytest.mark.parametrize("name", RC.RIR_BANDS_NAMES)
def test_the_bits_are_the_recorded_ones(eng, TILE, name):
    """Engine.rir_bands on the cases of tests/rir_cases.py against tests/golden/rir_parent_bits.npz (make_rir_bits.py): the
    model-based tests above bound the error, this one sees a changed rounding or a changed enumeration order."""
    import os
    from mixer_cases import assert_recorded_bits
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rir_parent_bits.npz"))
    assert_recorded_bits(f"rir_bands/{name}", RC.run(eng, RC.rir_bands_cases(TILE)[name], DEV), want)
