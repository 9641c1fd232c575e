"""cmgan_rir_stats / Engine.rir_stats on the GPU against the long-double model of tests/rir_stats_model.py, within the
bounds that model derives (its docstring): the values, the decay curve sample by sample, and - exactly - k0, the status
bits and every threshold index; per-row lengths with NaN where nothing may be read, the special rows, bit reproducibility
and row independence, hipGraph replay, and the front end (RirBank.simulate(measure=True) / where, DynamicMixer(room_stats=)).

The responses are exponentially decaying seeded noise plus a direct spike (rir_stats_model.decaying_noise): the level
falls 0.05 dB per sample or faster, far above the bounds, so no decision of a row lies within reach of rounding.  Every
comparison asserts that first (guard_hits == 0): a condition on the inputs, checked on the CPU when they were chosen.
Nothing here asserts a physical expectation (a T30 near its Sabine value, a T30 that falls with the band): those figures
are measured by tools/rir_stats_bench.py."""
import functools

import numpy as np
import pytest
import torch

import rir_stats_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS = 16000


@pytest.fixture(scope="module")
def eng():
    from cmgan_amd.engine import Engine
    return Engine(device=DEV)


@pytest.fixture(scope="module")
def TILE():
    from cmgan_amd import _lib
    return int(_lib.load().cmgan_rir_stats_tile())


# ------------------------------------------------------------------ inputs (pure numpy: importable without a GPU)
@functools.lru_cache(maxsize=None)
def filters(NB, NF):
    """The test filterbanks: octave bands where the length allows a design, seeded noise for the short ones."""
    from cmgan_amd.mixing import octave_filterbank
    if NB == 0:
        return None
    if NF >= 63:
        return octave_filterbank(FS, NB + 1, NF).numpy()[:NB].copy()
    return np.random.default_rng(100 * NB + NF).standard_normal((NB, NF)) / np.sqrt(NF)


def value_rows(T):
    """(n, k0) of the value test: every length around the tile with the direct spike at 0, at the tile's edges and at the
    row's end, where the direct window and the 50 / 80 ms limits are clipped."""
    rows = []
    for n in (1, 2, T - 1, T, T + 1, 2 * T + 3):
        rows += [(n, k0) for k0 in sorted({0, T - 1, T, n - 1}) if k0 < n]
    return rows


def value_bank(T, seed=0):
    rows = value_rows(T)
    K = 2 * T + 3
    bank = np.zeros((len(rows), K), dtype=np.float32)
    for r, (n, k0) in enumerate(rows):
        bank[r, :n] = M.decaying_noise(seed + r, n, 0.05 + 0.01 * (r % 3), k0)
    return bank, np.array([n for n, _ in rows], dtype=np.int32)


VALUE_FILTERS = ((0, 1), (1, 1), (8, 3), (3, 511), (1, 1023))        # NB 0, 1, 3, 8 and NF 1, 3, 511, the longest (> n for some rows)


def special_bank():
    """Rows 0, 2, 4, 6, 8 are ordinary; between them all zeros, a NaN and an inf within n, a response whose curve stays
    above -25 dB (a spike in its last sample holds 1.5 % of the energy), and a tie for the maximum."""
    n = 1500
    bank = np.stack([M.decaying_noise(40 + r, n, 0.06) for r in range(10)])
    bank[1] = 0.0
    bank[3, 700] = np.nan
    bank[5, 1499] = np.inf
    short = M.decaying_noise(47, n, 0.012, spike=1.0)
    short[n - 1] = np.sqrt(0.015 * float(np.sum(short.astype(np.float64) ** 2)))
    bank[7] = short
    bank[9] = M.decaying_noise(49, n, 0.06, k0=300)
    bank[9, 301] = -bank[9, 300]
    return bank, np.full(10, n, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _model_cached(row_bytes, n, NB, NF, fs, direct_ms):
    h = np.frombuffer(row_bytes, dtype=np.float32)
    return M.rir_stats_row(h, n, filters(NB, NF), fs, direct_ms)


def model(h, n, NB, NF, fs=FS, direct_ms=2.5):
    """The model of one row, computed once however many tests ask for it; nobody writes into what it returns."""
    n = min(max(int(n), 1), len(h))
    return _model_cached(np.ascontiguousarray(h[:n], dtype=np.float32).tobytes(), n, NB, NF, fs, direct_ms)


# ------------------------------------------------------------------ helpers
def run(eng, bank, lens, NB, NF, edc=True, fs=FS, direct_ms=2.5):
    """Engine.rir_stats of a numpy bank: (stats float64 [R, S, P], status [R, S], curve [R, S, K] or None) as numpy."""
    rir = bank if isinstance(bank, torch.Tensor) else torch.from_numpy(bank).to(DEV)
    length = None if lens is None else (lens if isinstance(lens, torch.Tensor) else torch.from_numpy(np.asarray(lens, dtype=np.int32)).to(DEV))
    filt = filters(NB, NF)
    out = eng.rir_stats(rir, length, None if filt is None else torch.from_numpy(filt).to(DEV), fs=fs, direct_ms=direct_ms, edc=edc)
    st, curve = out if edc else (out, None)
    assert all(t.dtype == torch.float64 and tuple(t.shape) == (rir.size(0), NB + 1) for t in st[:10]) and st.status.dtype == torch.int32
    stats = torch.stack(list(st[:10]), dim=2).cpu().numpy()
    return stats, st.status.cpu().numpy(), None if curve is None else curve.cpu().numpy()


def check(tag, got, bank, lens, NB, NF, fs=FS, direct_ms=2.5):
    stats, status, curve = got
    K = bank.shape[1]
    worst = 0.0
    for r in range(bank.shape[0]):
        n = K if lens is None else min(max(int(lens[r]), 1), K)
        m = model(bank[r], n, NB, NF, fs, direct_ms)
        assert m["guard_hits"] == 0, (tag, r, m["guard_hits"])
        assert status[r].tolist() == m["status"].tolist(), (tag, r, status[r], m["status"])
        for s in range(NB + 1):
            for c in range(M.P):
                g, v, b = stats[r, s, c], m["values"][s, c], m["bounds"][s, c]
                if np.isnan(v) or np.isinf(v):
                    assert (np.isnan(g) and np.isnan(v)) or g == v, (tag, r, s, c, g, v)
                else:
                    assert abs(g - v) <= b, (tag, r, s, c, g, v, b)
                    if b > 0:
                        worst = max(worst, abs(g - v) / b)
            if curve is None or status[r, s] & M.NONFINITE:
                continue
            assert np.all(np.abs(curve[r, s, :n] - m["edc"][s]) <= m["edc_bound"][s]), (tag, r, s)
            assert not curve[r, s, n:].any(), (tag, r, s)
            if status[r, s] & M.ZERO:
                continue
            # the threshold indices the kernel took: what its own curve and its own E give
            for x, cx in enumerate(M.DOWN):
                under = np.nonzero(curve[r, s, :n] <= cx * stats[r, s, 0])[0]
                assert (int(under[0]) if under.size else n) == m["ka"][s, x], (tag, r, s, x)
    print(f"[rir_stats] {tag}: worst error over bound {worst:.3g}")


# ------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("NB,NF", VALUE_FILTERS)
def test_values_match_the_model_within_its_bounds(eng, TILE, NB, NF):
    bank, lens = value_bank(TILE)
    got = run(eng, bank, lens, NB, NF)
    check(f"NB={NB} NF={NF}", got, bank, lens, NB, NF)
    assert got[0][:, 0, M.K0].tolist() == [float(k0) for _, k0 in value_rows(TILE)]
    ok = got[1][:, 0] == 0
    assert ok.sum() >= 6 and np.all(np.isfinite(got[0][ok][:, 0, M.EDT:]))     # the long rows are fitted: the regressions ran


def test_other_sample_rate_and_direct_window(eng, TILE):
    bank, lens = value_bank(TILE)
    for fs, ms in ((8000, 0.0), (48000, 10.0)):
        check(f"fs={fs} direct_ms={ms}", run(eng, bank[8:], lens[8:], 3, 511, fs=fs, direct_ms=ms), bank[8:], lens[8:], 3, 511, fs, ms)


def longest_bank():
    """Two rows of the longest response there is, 64 tiles: one full, one a sample short of its last tile's second sample."""
    K = 65536
    return np.stack([M.decaying_noise(90, K, 0.002, k0=3), M.decaying_noise(91, K, 0.002, k0=40000)]), np.array([K, K - 1022], dtype=np.int32)


def test_the_longest_response(eng):
    bank, lens = longest_bank()
    check("K = 65536", run(eng, bank, lens, 1, 3), bank, lens, 1, 3)


# ------------------------------------------------------------------ 2. per-row lengths
def test_nothing_is_read_beyond_a_rows_length_or_between_rows(eng, TILE):
    K, ld = 1500, 1600
    lens = np.array([700, 1500, 0, 5000, TILE], dtype=np.int32)      # 0 and 5000 are clamped to 1 and K
    real = np.array([700, 1500, 1, 1500, TILE])
    clean = np.stack([np.pad(M.decaying_noise(20 + r, n, 0.06), (0, K - n)) for r, n in enumerate(real)])
    buf = torch.full((len(lens), ld), float("nan"), dtype=torch.float32, device=DEV)
    for r, n in enumerate(real):
        buf[r, :n] = torch.from_numpy(clean[r, :n]).to(DEV)
    got = run(eng, buf[:, :K], lens, 3, 511)
    assert not np.any(got[1] & M.NONFINITE)
    check("NaN beyond n", got, clean, real, 3, 511)
    # without a length table every row has K samples: the zeros the rows were padded with count as samples
    dense = run(eng, clean, None, 3, 511)
    check("len = NULL", dense, clean, None, 3, 511)
    assert np.array_equal(dense[0][1], got[0][1])                  # row 1 has n = K either way


# ------------------------------------------------------------------ 3. special rows
def test_special_rows_and_their_neighbours(eng):
    bank, lens = special_bank()
    got = run(eng, bank, lens, 2, 511)
    check("special", got, bank, lens, 2, 511)
    stats, status, curve = got
    dead = M.NO_EDT | M.NO_T20 | M.NO_T30
    assert np.all(status[1] == (M.ZERO | dead)) and np.all(stats[1, :, 0] == 0.0) and np.all(np.isnan(stats[1, :, 1:]))
    assert not curve[1].any()
    for r in (3, 5):
        assert np.all(status[r] == (M.NONFINITE | dead)) and np.all(np.isnan(stats[r])) and np.all(np.isnan(curve[r]))
    assert status[7, 0] == (M.NO_T20 | M.NO_T30) and np.isfinite(stats[7, 0, M.EDT]) and np.all(np.isnan(stats[7, 0, M.T20:]))
    assert stats[9, 0, M.K0] == 300.0 and abs(bank[9, 300]) == abs(bank[9, 301])
    # the ordinary rows, alone: the same bits
    alone = run(eng, bank[0::2].copy(), lens[0::2], 2, 511)
    for a, b in zip(alone, got):
        assert np.array_equal(a, b[0::2], equal_nan=True)
    assert np.all(alone[1] == 0)


# ------------------------------------------------------------------ 4. bit reproducibility and independence
def test_bit_identical_between_calls_and_row_independent(eng, TILE):
    n, K = 2 * TILE + 3, 2 * TILE + 3
    rng = np.random.default_rng(7)
    row = M.decaying_noise(60, n, 0.05, k0=17)
    others = [np.stack([M.decaying_noise(61 + 4 * v + r, K, 0.05) for r in range(4)]) for v in range(2)]
    one = run(eng, row[None, :], [n], 3, 511)
    again = run(eng, row[None, :], [n], 3, 511)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(one, again))
    check("one row", one, row[None, :], [n], 3, 511)
    for v, place in ((0, 2), (1, 4)):                              # a batch of 5, the row in two places among different rows
        batch = np.insert(others[v], place, row, axis=0)
        got = run(eng, batch, [K] * 5, 3, 511)
        assert all(np.array_equal(a[0], b[place], equal_nan=True) for a, b in zip(one, got)), (v, place)
    # another row stride, and K enlarged beyond n (with NaN where nothing may be read)
    K2 = K + TILE + 77
    wide = torch.full((3, K2 + 5), float("nan"), dtype=torch.float32, device=DEV)
    wide[1, :n] = torch.from_numpy(row).to(DEV)
    wide[0, :K2] = torch.from_numpy(rng.standard_normal(K2).astype(np.float32)).to(DEV)
    wide[2, :K2] = wide[0, :K2]
    got = run(eng, wide[:, :K2], [K2, n, K2], 3, 511)
    assert np.array_equal(got[0][1], one[0][0], equal_nan=True) and np.array_equal(got[1][1], one[1][0])
    assert np.array_equal(got[2][1][:, :K], one[2][0]) and not got[2][1][:, K:].any()
    # slice 0 whatever the filterbank is
    for NB, NF in ((0, 1), (8, 3), (1, 1023)):
        other = run(eng, row[None, :], [n], NB, NF)
        assert np.array_equal(other[0][0, 0], one[0][0, 0], equal_nan=True) and np.array_equal(other[2][0, 0], one[2][0, 0])


# ------------------------------------------------------------------ 5. hipGraph
def test_captured_call_replays_with_new_bank_lengths_and_filters(eng, TILE):
    K, NB, NF = TILE + 200, 3, 511
    mk = lambda seed: np.stack([M.decaying_noise(seed + r, K, 0.06, k0=5 * r) for r in range(3)])
    first, second = mk(70), mk(80)
    rir = torch.from_numpy(first).to(DEV)
    length = torch.tensor([K, K - 100, TILE], dtype=torch.int32, device=DEV)
    filt = torch.from_numpy(filters(NB, NF)).to(DEV)
    eager = eng.rir_stats(rir, length, filt, edc=True)               # (also grows the workspace before the capture)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_stats, g_curve = eng.rir_stats(rir, length, filt, edc=True)
    graph.replay()
    same = lambda a, b: torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
    assert all(same(a, b) for a, b in zip(g_stats, eager[0])) and same(g_curve, eager[1])
    # a new bank, new lengths and new filters, written in place into the tensors the graph reads
    rir.copy_(torch.from_numpy(second).to(DEV))
    length.copy_(torch.tensor([TILE - 1, K, K - 7], dtype=torch.int32, device=DEV))
    filt.copy_(torch.from_numpy(filters(NB + 1, NF)[1:].copy()).to(DEV))
    graph.replay()
    again = eng.rir_stats(rir, length, filt, edc=True)
    assert not same(again[0].t30, eager[0].t30)
    assert all(same(a, b) for a, b in zip(g_stats, again[0])) and same(g_curve, again[1])


# ------------------------------------------------------------------ 6. the front end
def _sampler(seed, **kw):
    from cmgan_amd.mixing import RoomSampler
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return RoomSampler(dims=((3.0, 3.0, 2.5), (5.0, 4.0, 3.0)), rt60=(0.15, 0.25), generator=gen, **kw)


@pytest.mark.parametrize("bands", [None, 3])
def test_simulated_bank_is_measured_and_selected_by_t30(eng, bands):
    from cmgan_amd.mixing import RirBank
    kw = {} if bands is None else dict(bands=bands, tilt=(0.1, 0.4), filter_taps=255)
    sampler = _sampler(31, **kw)
    bank = RirBank.simulate(eng, sampler, 4, seconds=0.25, sample_rate=FS, measure=True)
    NB = bands or 0
    assert tuple(bank.data.shape) == (4, 4000) and tuple(bank.stats.t30.shape) == (4, NB + 1)
    filt = None if bands is None else sampler.filters(FS, "cpu").numpy()
    h, lens = bank.data.cpu().numpy(), bank.length.cpu().numpy()
    t30 = np.zeros(4)
    for r in range(4):
        m = M.rir_stats_row(h[r], lens[r], filt, FS)
        assert m["guard_hits"] == 0, (r, m["guard_hits"])
        assert bank.stats.status[r].tolist() == m["status"].tolist()
        for c, name in enumerate(bank.stats._fields[:10]):
            g, v, b = getattr(bank.stats, name)[r].cpu().numpy(), m["values"][:, c], m["bounds"][:, c]
            fin = np.isfinite(v)
            assert np.all(np.abs(g[fin] - v[fin]) <= b[fin]) and np.array_equal(g[~fin], v[~fin], equal_nan=True), (r, name, g, v, b)
        t30[r] = m["values"][0, M.T30]
    assert np.all(np.isfinite(t30))
    # the two middle rows by the model's T30, with half the gap to their neighbours as the margin
    order = np.argsort(t30)
    lo, hi = 0.5 * (t30[order[0]] + t30[order[1]]), 0.5 * (t30[order[2]] + t30[order[3]])
    assert min(t30[order[1]] - lo, hi - t30[order[2]]) > 1e-6       # (a condition on the drawn rooms)
    keep = sorted(order[1:3].tolist())
    sub = bank.where(t30=(lo, hi))
    assert len(sub) == 2 and torch.equal(sub.data, bank.data[keep]) and torch.equal(sub.length, bank.length[keep])
    assert torch.equal(sub.rooms, bank.rooms[keep]) and torch.equal(sub.stats.t30, bank.stats.t30[keep])
    assert (sub.bands is None) == (bands is None) and (bands is None or torch.equal(sub.bands, bank.bands[keep]))


def test_dynamic_mixer_labels_the_batch_with_its_rooms(eng):
    from cmgan_amd.mixing import DynamicMixer, NoiseBank, RirBank
    rng = np.random.default_rng(33)
    nb = NoiseBank.from_arrays([rng.standard_normal(n).astype(np.float32) for n in (300, 5000)], device=DEV)
    B, L = 4, 2100
    cd = torch.from_numpy((0.1 * rng.standard_normal((B, L))).astype(np.float32)).to(DEV)
    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t

    def mixer(rooms_kw=None, bank=None, **kw):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(5)
        rooms = None if rooms_kw is None else _sampler(105, **rooms_kw)
        return DynamicMixer(eng, nb, bank, rooms=rooms, snr_db=(0.0, 15.0), early_ms=10.0, p_reverb=0.5, peak=100.0,
                            generator=gen, rir_seconds=0.1, **kw)

    for rooms_kw in ({}, dict(bands=3, tilt=(0.1, 0.4), filter_taps=255)):
        on, off, base = mixer(rooms_kw, room_stats=True), mixer(rooms_kw, room_stats=False), mixer(rooms_kw)
        outs = [m(cd) for m in (on, off, base)]
        for o in outs[:2]:                                         # targets, noisy rows and info: the same bits
            assert torch.equal(o[0], outs[2][0]) and torch.equal(o[1], outs[2][1])
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(o[2], outs[2][2]))
        for m in (on, off):
            for a, b in zip(m.last_draw, base.last_draw):
                assert (a is None and b is None) or torch.equal(a, b)
            assert torch.equal(m.last_bank.data, base.last_bank.data)
        assert off.last_room_stats is None and base.last_room_stats is None
        filt = None if not rooms_kw else on.rooms.filters(FS, eng.device)
        want = eng.rir_stats(on.last_bank.data[:B], on.last_bank.length[:B], filt, fs=FS)
        got = on.last_room_stats
        assert tuple(got.t30.shape) == (B, (3 if rooms_kw else 0) + 1)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, want))
        assert torch.equal(on.last_bank.length[:B], on.last_draw.rir_len)
    # a fixed, measured bank: the gather by the drawn index, the identity's row for the dry ones
    fixed = RirBank.simulate(eng, _sampler(41), 5, seconds=0.1, sample_rate=FS, measure=True)
    m = mixer(None, fixed, room_stats=True)
    m(cd)
    index = m.last_draw.rir_index.long()
    assert bool((index == 5).any()) and bool((index < 5).any())      # (seed 5 draws dry and wet rows)
    for got, have in zip(m.last_room_stats, m.rir_bank.stats):
        assert torch.equal(bits(got), bits(have[index]))
    # what with_identity wrote for the identity is what the kernels give it
    lone = eng.rir_stats(m.rir_bank.data[5:6], m.rir_bank.length[5:6], fs=FS)
    for have, want in zip(m.rir_bank.stats, lone):
        assert torch.equal(bits(have[5:6]), bits(want))
