"""Transmission on the GPU (cmgan_amd/csrc/transmit.hip; include/cmgan_hip.h, "Transmission"): Engine.transmit against the
numpy model of tests/transmit_model.py - the three codecs on every int16 value, on the halves between them, beyond +-1
and on non-finite samples; runs of lost frames at the row's start, with a short history, at a partial last frame, in front
of a good frame shorter than the fade, one good frame apart, longer than the fade-out, over the whole row and not at all,
with and without concealment in one batch; rows that tie, a silent row and a NaN in the window; the edges of the lag
range, the window and the frame; per-row lengths with NaN tails, unused table columns filled with 255, invalid rows; in
place against out of place, bit-reproducibility, independence of B, of the neighbours, of the padding and of L; hipGraph
replay with the signal and the three tables changed in place; and DynamicMixer(transmission=...).

Acceptance (transmit_model's docstring).  The lag of every frame and the status are compared with the model's for
EQUALITY, and so are the codec's samples and every zero.  A concealed sample g is accepted against the model's long-double
w when |g - w| <= ulp32(w) / 2 + E, E per row from the model alone, 8 x max |d - w|; every row used is registered in
transmit_model.build_rows, where the host test checks E <= 2^-10 x ulp32(rms) / 2 and the margin of every searched run
without a GPU; every check prints E and the worst excess.

Measured on an MI355X: every compared lag was equal (2239 frames over the 54 row checks, frames of 16 .. 320 samples, lags 16
.. 1024, windows 64 .. 1024, tables of up to 513 frames), and so were every status, every codec sample and every zero.  The
largest E of any row is 8.7e-16 (at most 8.1e-5 of the bound above), and the worst |g - w| - ulp32(w) / 2 over the 341 770
samples judged is 2.2e-18, on a row whose E is 1.1e-16: no sample lies further from w than half an ulp and a fiftieth of
its row's E."""
import numpy as np
import pytest
import torch

import transmit_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def eng():
    from cmgan_amd.engine import Engine
    M.build_rows()
    return Engine(device=DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(eng, keys, L=None, lengths=True, pad=0, extra=None, more_columns=0, fill=255, inplace=False):
    """The registered rows as one batch -> (y float32 [B, L], status, lag [B, ldl]) as numpy.  The buffer is L (default: the
    longest row) + `pad` wide and NaN wherever a row has no sample; the table has `more_columns` beyond ceil(L / F) and
    holds `fill` wherever a row has no frame; `extra` = (x, n, lost, codec, plc) rows that are not registered are appended
    as they are."""
    rows = [M.ROWS[k] for k in keys]
    r0 = rows[0]
    par = (r0.F, r0.pmin, r0.pmax, r0.W, r0.A)
    assert all((r.F, r.pmin, r.pmax, r.W, r.A) == par for r in rows)
    specs = [(r.x, r.n, r.lost, r.codec, r.plc) for r in rows] + list(extra or [])
    B = len(specs)
    L = max(max(len(s[0]) for s in specs), 1) if L is None else L
    ldl = -(-L // r0.F) + more_columns
    buf = np.full((B, L + pad), NAN, dtype=np.float32)
    tab = np.full((B, ldl), fill, dtype=np.uint8)
    for b, (x, n, lost, _, _) in enumerate(specs):
        buf[b, :len(x)] = x
        tab[b, :len(lost)] = lost
    buf = torch.from_numpy(buf).to(DEV)
    wav = buf[:, :L]
    if lengths:
        ld = torch.tensor([s[1] for s in specs], dtype=torch.int32, device=DEV)
    else:
        assert all(s[1] == L for s in specs)
        ld = None
    lost = torch.from_numpy(tab).to(DEV)
    codec = torch.tensor([s[3] for s in specs], dtype=torch.int32, device=DEV)
    plc = torch.tensor([s[4] for s in specs], dtype=torch.int32, device=DEV)
    if inplace:
        ybuf = buf
    else:
        ybuf = torch.full((B, L + pad), NAN, dtype=torch.float32, device=DEV)
    y, st, lag = eng.transmit(wav, lost, r0.F, codec, plc, ld, pmin=r0.pmin, pmax=r0.pmax, window=r0.W, fade=r0.A,
                              out=ybuf[:, :L], info=True)
    assert y.dtype == torch.float32 and tuple(y.shape) == (B, L) and y.data_ptr() == ybuf.data_ptr()
    assert st.dtype == torch.int32 and tuple(st.shape) == (B,) and lag.dtype == torch.int32 and tuple(lag.shape) == (B, ldl)
    if pad:
        assert bool(torch.isnan(ybuf[:, L:]).all()), "the padding behind y was written"
    return tuple(t.cpu().numpy() for t in (y, st, lag))


TOTALS = {"lags": 0, "checks": 0, "E": 0.0, "samples": 0, "worst": -np.inf}


def _accept(tag, got, keys):
    """Every registered row of the batch against the model: the lags and the status for equality, zeros from n on, the
    samples under the rule."""
    y, st, lag = got
    for b, key in enumerate(keys):
        row = M.ROWS[key]
        res, E = M.case(key)
        K = len(res.lag)
        assert st[b] == 0, f"{tag} {key}: status {st[b]}"
        assert np.array_equal(lag[b, :K], res.lag), f"{tag} {key}: frames {np.flatnonzero(lag[b, :K] != res.lag)[:8]} differ: " \
                                                     f"{lag[b, :K][lag[b, :K] != res.lag][:8]} for {res.lag[lag[b, :K] != res.lag][:8]}"
        assert (lag[b, K:] == -1).all(), f"{tag} {key}: lags behind the last frame"
        assert not y[b, row.n:].any(), f"{tag} {key}: samples from n on are not zero"
        worst = M.excess(y[b, :row.n], res.w, E)
        print(f"[transmit] {tag} {key} (n = {row.n}, F = {row.F}, codec {row.codec}, plc {row.plc}, {K} lags equal, runs "
              f"{[(r.k0, r.k1, r.lag) for r in res.runs]}): E = {E:.3e}, worst |g - w| - ulp/2 = {worst + E:.3e}")
        assert worst <= 0.0, f"{tag} {key}: {worst + E:.3e} beyond half an ulp, E = {E:.3e}"
        TOTALS["lags"] += K
        TOTALS["checks"] += 1
        TOTALS["E"] = max(TOTALS["E"], E)
        TOTALS["samples"] += row.n
        TOTALS["worst"] = max(TOTALS["worst"], worst + E)
    print(f"[transmit] totals so far: {TOTALS}")


# ------------------------------------------------------------------ 1. the codecs
def _codec_call(eng, x, kinds):
    B, L = len(kinds), len(x)
    wav = torch.from_numpy(np.tile(x, (B, 1))).to(DEV)
    lost = torch.zeros(B, -(-L // 320), dtype=torch.uint8, device=DEV)
    y, st, lag = eng.transmit(wav, lost, codec=torch.tensor(kinds, dtype=torch.int32, device=DEV), info=True)
    assert not bool(st.any()) and not bool(lag.any())
    return y.cpu().numpy()


def test_codecs_on_every_int16_value(eng):
    q = np.arange(-32768, 32768, dtype=np.float64)
    kinds = [M.PCM16, M.ULAW, M.ALAW, M.NONE]
    for name, x in (("values", q / 32768.0), ("halves", (q + 0.5) / 32768.0)):
        x = x.astype(np.float32)
        y = _codec_call(eng, x, kinds)
        for b, kind in enumerate(kinds):
            bad = np.flatnonzero(_bits(y[b]) != _bits(M.codec(x, kind)))
            assert bad.size == 0, f"{name}, codec {kind}: {bad.size} samples differ, the first at q = {q[bad[0]]}"
    assert np.array_equal(_codec_call(eng, (q / 32768.0).astype(np.float32), [M.PCM16])[0], (q / 32768.0).astype(np.float32))


def test_codecs_beyond_full_scale_and_non_finite(eng):
    x = np.zeros(400, dtype=np.float32)
    x[:12] = [1.0, -1.0, 1.5, -1.5, 3.0e38, -3.0e38, np.inf, -np.inf, np.nan, 0.99999, -0.99999, 1e-30]
    x[12:14] = np.array([0x7FC12345, 0xFFA00001], dtype=np.uint32).view(np.float32)       # NaNs with payloads
    kinds = [M.NONE, M.PCM16, M.ULAW, M.ALAW]
    y = _codec_call(eng, x, kinds)
    assert np.array_equal(_bits(y[0]), _bits(x)), "codec 0 is not a bit copy"
    for b, kind in enumerate(kinds[1:], 1):
        want = M.codec(x, kind)
        assert np.isfinite(want).all() and np.array_equal(_bits(y[b]), _bits(want)), f"codec {kind}: {y[b, :14]} for {want[:14]}"
    assert y[1, 0] == 32767.0 / 32768.0 and y[1, 1] == -1.0 and y[1, 6] == y[1, 0] and y[1, 7] == -1.0 and y[1, 8] == 0.0


# ------------------------------------------------------------------ 2. the runs
RUNS = ("first", "second", "last-partial", "apart", "mid", "short-good", "all", "none", "gap", "plc")


@pytest.mark.parametrize("F", M.FRAMES)
def test_runs(eng, F):
    keys = [f"run-{F}-{name}" for name in RUNS]
    got = _run(eng, keys, pad=3)
    _accept(f"runs-{F}", got, keys)
    y, st, lag = got
    at = {name: b for b, name in enumerate(RUNS)}
    row = M.ROWS[keys[0]]
    assert lag[at["first"], 0] == row.pmin and not y[at["first"], :F].any()             # no history: zeros, the lag is pmin
    assert lag[at["all"], 0] == row.pmin and not lag[at["all"], 1:-(-M.N_ROW // F)].any() and not y[at["all"]].any()
    none = M.ROWS[keys[at["none"]]]
    assert np.array_equal(_bits(y[at["none"], :none.n]), _bits(none.x)) and not lag[at["none"], :-(-none.n // F)].any()
    gap = M.ROWS[keys[at["gap"]]]
    for k in (3, 9, 10):                                                 # plc = 0 beside plc = 1: hard gaps, no lag
        assert not y[at["gap"], k * F:(k + 1) * F].any() and lag[at["gap"], k] == 0
    assert np.array_equal(y[at["gap"], :3 * F], M.codec(gap.x[:3 * F], gap.codec)) and y[at["plc"], 3 * F:4 * F].any()
    part = M.ROWS[keys[at["last-partial"]]]
    assert part.n % F != 0 and lag[at["last-partial"], -(-part.n // F) - 1] > 0
    short = M.ROWS[keys[at["short-good"]]]
    assert 0 < short.n % F < lag[at["short-good"], -(-short.n // F) - 2] // 4
    apart = M.case(keys[at["apart"]])[0].runs
    assert len(apart) == 2 and apart[1].k0 == apart[0].k1 + 1


def test_a_run_longer_than_the_fade_ends_in_zeros(eng):
    keys = ["long-run", "bench-pattern"]
    got = _run(eng, keys, lengths=False)
    _accept("long", got, keys)
    y = got[0]
    row = M.ROWS["long-run"]
    s, e = 10 * row.F, 15 * row.F
    assert e - s > 6 * row.A and y[0, s:s + 6 * row.A - 1].any() and not y[0, s + 6 * row.A:e].any()   # (+-0: g = 0 times the period)
    assert M.case("long-run")[0].runs[0].lag > 0 and y[0, e:e + 4].any()


def test_every_codec_in_front_of_a_concealed_run(eng):
    keys = [f"codec-{k}" for k in (M.NONE, M.PCM16, M.ULAW, M.ALAW)]
    got = _run(eng, keys, lengths=False, pad=1)
    _accept("codec", got, keys)


# ------------------------------------------------------------------ 3. ties and non-finite rows
def test_ties_and_non_finite_rows(eng):
    keys = ["tie-period", "tie-silence", "nan-window"]
    got = _run(eng, keys, lengths=False)
    _accept("ties", got, keys)
    y, st, lag = got
    row = M.ROWS["tie-period"]
    s = 9 * row.F
    assert lag[0, 9] == 100                                              # not 200: the smallest of equal maxima
    assert np.array_equal(_bits(y[0, s:s + 75]), _bits(row.x[s - 100:s - 25]))            # the first P - Q samples: bit copies
    assert lag[1, 4] == row.pmin and lag[1, 20] == row.pmin and not y[1].any()
    assert lag[2, 8] == row.pmin                                         # every score is NaN: -inf, the smallest lag


# ------------------------------------------------------------------ 4. range edges
@pytest.mark.parametrize("key", ["edge-one-lag", "edge-1024", "edge-f16"])
def test_range_edges(eng, key):
    got = _run(eng, [key], pad=2)
    _accept("edge", got, [key])
    row, res = M.ROWS[key], M.case(key)[0]
    assert all(row.pmin <= r.lag <= row.pmax for r in res.runs)


@pytest.mark.parametrize("key", ["walk-64", "walk-256", "walk-513"])
def test_tables_longer_than_one_pass_of_the_walk(eng, key):
    """Runs that cross, start at and end at the 64- and 256-frame boundaries of the kernel's walk over the table, and runs
    that end at K where K is a multiple of either."""
    got = _run(eng, [key], pad=1, more_columns=2)
    _accept("walk", got, [key])
    res = M.case(key)[0]
    assert [(r.k0, r.k1) for r in res.runs] == [(int(a), int(b)) for a, b in M.runs(M.ROWS[key].lost, len(res.lag))]
    assert int((got[2][0] > 0).sum()) == len(res.runs)


# ------------------------------------------------------------------ 5. tables and invalid rows
def test_lengths_with_nan_tails_and_unused_columns(eng):
    keys = [f"len-{i}" for i in range(5)]
    a = _run(eng, keys, pad=4, more_columns=3, fill=255)
    _accept("lengths", a, keys)
    b = _run(eng, keys, pad=0, more_columns=0, fill=1)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2][:, :b[2].shape[1]], b[2])
    assert (a[2][:, b[2].shape[1]:] == -1).all()


def test_invalid_rows(eng):
    keys = [f"inv-ok-{i}" for i in range(4)]
    x = M.speech(85, 2000)
    t = M.table(7, 2)
    bad = [(x, 2000, t, 4, 1), (x, 2000, t, -1, 1), (x, 2000, t, 2, 2), (x, 2000, t, 2, -1), (x, -1, t, 2, 1), (x, 2001, t, 2, 1),
           (x, 2 ** 31 - 1, t, 0, 0)]
    got = _run(eng, keys, extra=bad, pad=2)
    _accept("invalid", got, keys)
    y, st, lag = got
    assert st.tolist() == [0] * 4 + [1] * len(bad)
    assert not y[4:].any() and (lag[4:] == -1).all()


def test_a_column_slice_of_a_wider_table(eng):
    """`lost` as the first columns of a table whose rows are further apart: the kernels take ONE leading dimension for
    `lost` and `lag`, so the lags come back as a view of a table that wide, equal to those of the contiguous call, and
    everything the kernel wrote lies inside it: -1 behind every row's last frame, guards on either side untouched."""
    keys = [f"bits-{i}" for i in range(3)]
    rows = [M.ROWS[k] for k in keys]
    B, L, K, wide = 3, 8000, 25, 1000
    buf = np.full((B, L), NAN, dtype=np.float32)
    tab = np.full((B, wide), 255, dtype=np.uint8)
    for b, r in enumerate(rows):
        buf[b, :r.n] = r.x
        tab[b, :len(r.lost)] = r.lost
    wav = torch.from_numpy(buf).to(DEV)
    ld = torch.tensor([r.n for r in rows], dtype=torch.int32, device=DEV)
    codec = torch.tensor([r.codec for r in rows], dtype=torch.int32, device=DEV)
    plc = torch.tensor([r.plc for r in rows], dtype=torch.int32, device=DEV)
    big = torch.from_numpy(tab).to(DEV)
    y0, st0, lag0 = eng.transmit(wav, big[:, :K].contiguous(), 320, codec, plc, ld, info=True)
    before = torch.full((4096,), 77, dtype=torch.int32, device=DEV)     # neighbours in the allocator's pool
    y1, st1, lag1 = eng.transmit(wav, big[:, :K], 320, codec, plc, ld, info=True)
    after = torch.full((4096,), 77, dtype=torch.int32, device=DEV)
    assert tuple(lag1.shape) == (B, K) and lag1.stride(0) == wide and lag1._base is not None and tuple(lag1._base.shape) == (B, wide)
    assert torch.equal(y0, y1) and torch.equal(st0, st1) and torch.equal(lag0, lag1)
    assert bool((lag1._base[:, K:] == -1).all()) and bool((before == 77).all()) and bool((after == 77).all())
    _accept("slice", (y1.cpu().numpy(), st1.cpu().numpy(), lag1.cpu().numpy()), keys)
    one = eng.transmit(wav[:1], big[:1, :K], 320, codec[:1], plc[:1], ld[:1], info=True)      # B = 1: the width is n_frames
    assert tuple(one[2].shape) == (1, K) and torch.equal(one[2], lag0[:1]) and torch.equal(one[0], y0[:1])


# ------------------------------------------------------------------ 6. independence and replay
def test_bits_do_not_depend_on_the_batch_the_padding_or_the_place(eng):
    keys = [f"bits-{i}" for i in range(3)]
    same = lambda p, q: all(np.array_equal(_bits(u), _bits(v)) if u.dtype == np.float32 else np.array_equal(u, v) for u, v in zip(p, q))
    a = _run(eng, keys)
    _accept("bits", a, keys)
    assert same(a, _run(eng, keys)), "two runs differ"
    assert same(a, _run(eng, keys, inplace=True)), "in place differs from out of place"
    rev = _run(eng, keys[::-1])
    assert same(a, tuple(v[::-1] for v in rev))
    L, K = a[0].shape[1], a[2].shape[1]
    wide = _run(eng, keys, L=L + 777, pad=5, more_columns=2, fill=7)
    assert same(a, (wide[0][:, :L], wide[1], wide[2][:, :K])) and not wide[0][:, L:].any()
    for i, k in enumerate(keys):                                         # alone, in a buffer cut to its own length
        n = M.ROWS[k].n
        one = _run(eng, [k], lengths=False)
        Kn = -(-n // M.ROWS[k].F)
        assert same((a[0][i:i + 1, :n], a[1][i:i + 1], a[2][i:i + 1, :Kn]), one), k
    x = M.speech(95, 100)
    other = _run(eng, keys[:1], L=L, extra=[(x, 100, np.ones(1, dtype=np.uint8), 3, 0), (x, -5, np.ones(1, dtype=np.uint8), 9, 9)])
    assert same(tuple(v[:1] for v in a), tuple(v[:1] for v in other))


def test_captured_call_replays_with_new_signal_and_tables(eng):
    keys = [f"graph-{i}" for i in range(4)]
    L, K = 4000, 13
    wav = torch.from_numpy(np.stack([M.speech(200 + b, L) for b in range(4)])).to(DEV)
    lost = torch.zeros(4, K, dtype=torch.uint8, device=DEV)
    lost[:, 5] = 1
    codec = torch.tensor([2, 2, 0, 1], dtype=torch.int32, device=DEV)
    plc = torch.tensor([1, 1, 0, 1], dtype=torch.int32, device=DEV)
    call = lambda: eng.transmit(wav, lost, 320, codec, plc, info=True)
    eager = call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = call()
    graph.replay()
    assert all(torch.equal(p, q) for p, q in zip(got, eager))
    wav.copy_(torch.from_numpy(np.stack([M.ROWS[k].x for k in keys])).to(DEV))
    lost.copy_(torch.from_numpy(np.stack([M.ROWS[k].lost for k in keys])).to(DEV))
    codec.copy_(torch.tensor([M.ROWS[k].codec for k in keys], dtype=torch.int32, device=DEV))
    plc.copy_(torch.tensor([M.ROWS[k].plc for k in keys], dtype=torch.int32, device=DEV))
    graph.replay()
    again = call()
    assert not torch.equal(again[0], eager[0])
    assert all(torch.equal(p, q) for p, q in zip(got, again))
    _accept("replayed", tuple(t.cpu().numpy() for t in got), keys)
    codec[1] = 7                                                         # an invalid row: the replay reports it
    graph.replay()
    assert got[1].tolist() == [0, 1, 0, 0] and not bool(got[0][1].any()) and bool((got[2][1] == -1).all())


# ------------------------------------------------------------------ 7. the mixer
def _mixer(eng, seed, **kw):
    from cmgan_amd.mixing import DynamicMixer, NoiseBank
    rng = np.random.default_rng(5)
    nb = NoiseBank.from_arrays([0.01 * rng.standard_normal(9000), 0.005 * rng.standard_normal(4321)], device=DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return DynamicMixer(eng, nb, None, snr_db=(20.0, 30.0), early_ms=None, generator=gen, **kw)


@pytest.mark.parametrize("on", ["noisy", "both"])
def test_mixer_with_transmission(eng, on):
    from cmgan_amd.mixing import TransmissionSampler, TransmitDraw, TransmitInfo
    B, L = 6, 8000
    clean = torch.from_numpy(np.stack([M.speech(300 + b, L) for b in range(B)])).to(DEV)
    plain = _mixer(eng, 41)
    target0, noisy0, _ = plain(clean)
    assert plain.last_transmission is None
    gen = torch.Generator(device=DEV)
    gen.manual_seed(77)
    sampler = TransmissionSampler(p=0.8, loss=(0.05, 0.25), burst=(1.0, 3.0), generator=gen)
    mixer = _mixer(eng, 41, transmission=sampler, transmission_on=on)
    target, noisy, _ = mixer(clean)
    for p, q in zip(plain.last_draw, mixer.last_draw):                   # every other draw is what it was
        assert (p is None and q is None) or torch.equal(p, q)
    assert torch.equal(plain.generator.get_state(), mixer.generator.get_state())
    info = mixer.last_transmission
    assert isinstance(info, TransmitInfo) and isinstance(info.draw, TransmitDraw)
    d = info.draw
    K = -(-L // 320)
    assert tuple(d.lost.shape) == (B, K) and d.lost.dtype == torch.uint8 and d.codec.dtype == torch.int32 and d.plc.dtype == torch.int32
    assert bool(d.lost.any()) and not bool(info.status.any())
    y, st, lag = eng.transmit(noisy0, d.lost, 320, d.codec, d.plc, info=True)           # the stage is this call, in place
    assert torch.equal(noisy, y) and torch.equal(info.lag, lag)
    if on == "both":
        y2, _, lag2 = eng.transmit(target0, d.lost, 320, d.codec, d.plc, info=True)
        assert torch.equal(target, y2) and torch.equal(info.target_lag, lag2)
    else:
        assert torch.equal(target, target0) and info.target_lag is None
    # against the model fed the mixer's own draw: the rows all of whose runs are decided beyond one ulp of their history
    x0, lost, codec, plc = (t.cpu().numpy() for t in (noisy0, d.lost, d.codec, d.plc))
    got, lags, judged, dropped = noisy.cpu().numpy(), lag.cpu().numpy(), 0, []
    for b in range(B):
        res = M.transmit(x0[b], L, lost[b], int(codec[b]), int(plc[b]))
        if not M.margins_ok(res):
            dropped.append((b, [(r.k0, r.lag, r.margin / (M.MARGIN * r.energy)) for r in res.runs if r.lag]))
            continue
        E = M.slack(res)
        assert E <= M.condition(res)
        assert np.array_equal(lags[b], res.lag), f"row {b}: lags {lags[b]} for {res.lag}"
        worst = M.excess(got[b], res.w, E)
        print(f"[transmit] mixer {on} row {b} (codec {codec[b]}, plc {plc[b]}, lost {int(lost[b].sum())} of {K}): E = {E:.3e}, "
              f"worst |g - w| - ulp/2 = {worst + E:.3e}")
        assert worst <= 0.0
        judged += 1
    print(f"[transmit] mixer {on}: {judged} of {B} rows judged against the model, dropped for a thin margin: {dropped}")
    assert judged == B, f"rows whose runs are not decided by 2^-12 of the window's energy: {dropped}"
