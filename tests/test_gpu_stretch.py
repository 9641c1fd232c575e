"""Tempo and pitch perturbation on the GPU (cmgan_amd/csrc/stretch.hip; include/cmgan_hip.h, "Tempo perturbation"):
Engine.stretch against the numpy model of tests/stretch_model.py at the frame edges, at every rate in one batch, on rows
that tie and rows whose best splice sits at either end of the search range or is cut by the row's ends, at every (hop,
search) edge, on a row longer than 2^16, per-row lengths with NaN tails, invalid rows, non-finite samples,
bit-reproducibility and independence of B, of the neighbours, of the padding and of L, hipGraph replay with the input,
the rates and the lengths changed in place, and the consumers: Engine.pitch_shift and DynamicMixer(tempo=, pitch=).

Acceptance (stretch_model's docstring).  The positions q_k of every frame, out_len, searched and status are compared with
the model's for EQUALITY.  A sample g is accepted against the model's long-double w when |g - w| <= ulp32(w) / 2 + E, E
per row from the model alone, 8 x max |direct - w|; every row used is registered in stretch_model.build_rows, where the
host test checks E <= 2^-10 x ulp32(rms) / 2 without a GPU; every check prints E and the worst excess.

Measured on an MI355X: every compared position was equal (2304 frames over the 58 row checks, rates 0.25 .. 4, hop
16 .. 1024, search 0 .. 1024), as were out_len, searched and status.  The largest E of any row is 2.4e-16 (at most 6.1e-5 of
the bound above), and the worst |g - w| - ulp32(w) / 2 over the 135 018 samples judged is 0.0: it is reached at i = H / 2,
where f = g = 1 / 2 makes w the exact midpoint of two float32 values, so no sample lies further than half an ulp from w
and E was never needed."""
import numpy as np
import pytest
import torch

import stretch_model as M

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


def _run(eng, keys, L=None, lengths=True, rates=None, pad=0, extra=None, H=None, D=None, N=None):
    """The registered rows as one batch -> (y float32 [B, N], out_len, status, pos, searched) as numpy.  The buffer is L
    (default: the longest row) + `pad` wide and NaN wherever a row has no sample; `extra` = (x, n, r) rows that are not
    registered are appended as they are."""
    rows = [M.ROWS[k] for k in keys]
    specs = [(r.x, r.n, r.r) for r in rows] + list(extra or [])
    N = rows[0].N if N is None else N
    H = rows[0].H if H is None else H
    D = rows[0].D if D is None else D
    assert all(r.N == N and r.H == H and r.D == D for r in rows)
    B = len(specs)
    L = max(max(len(x) for x, _, _ in specs), 1) if L is None else L
    buf = torch.full((B, L + pad), NAN, dtype=torch.float32)
    for b, (x, n, _) in enumerate(specs):
        buf[b, :len(x)] = torch.from_numpy(np.array(x))
    buf = buf.to(DEV)
    wav = buf[:, :L]
    if lengths:
        ld = torch.tensor([n for _, n, _ in specs], dtype=torch.int32, device=DEV)
    else:
        assert all(n == L for _, n, _ in specs)
        ld = None
    rate = torch.tensor([r for _, _, r in specs] if rates is None else rates, dtype=torch.float64, device=DEV)
    ybuf = torch.full((B, N + pad), NAN, dtype=torch.float32, device=DEV)
    y, n_out, st, pos, srch = eng.stretch(wav, rate, N, ld, H, D, out=ybuf[:, :N], info=True)
    assert y.dtype == torch.float32 and tuple(y.shape) == (B, N) and y.data_ptr() == ybuf.data_ptr()
    for t in (n_out, st, srch):
        assert t.dtype == torch.int32 and tuple(t.shape) == (B,)
    assert pos.dtype == torch.int32 and tuple(pos.shape) == (B, -(-N // H))
    if pad:
        assert bool(torch.isnan(ybuf[:, N:]).all()), "the padding behind y was written"
    return tuple(t.cpu().numpy() for t in (y, n_out, st, pos, srch))


def _accept(tag, got, keys):
    """Every registered row of the batch against the model: positions, out_len, searched and status for equality, the
    samples under the rule.  Returns (largest E, worst |g - w| - ulp / 2, positions compared)."""
    y, n_out, st, pos, srch = got
    top, worst_over, n_pos = 0.0, -np.inf, 0
    for b, key in enumerate(keys):
        row = M.ROWS[key]
        (q, c, s), E, w = M.case(key)
        Mb, K = len(w), len(q)
        assert st[b] == 0 and n_out[b] == Mb, f"{tag} {key}: status {st[b]}, out_len {n_out[b]} for {Mb}"
        assert np.array_equal(pos[b, :K], q), f"{tag} {key}: frames {np.flatnonzero(pos[b, :K] != q)[:8]} sit elsewhere"
        assert (pos[b, K:] == -1).all() and srch[b] == int(s.sum()), f"{tag} {key}: searched {srch[b]} for {int(s.sum())}"
        assert not y[b, Mb:].any(), f"{tag} {key}: outputs from out_len on are not zero"
        worst = M.excess(y[b, :Mb], w, E)
        print(f"[stretch] {tag} {key} (n = {row.n}, r = {row.r}, H = {row.H}, D = {row.D}, {Mb} outputs, {K} frames equal, "
              f"{int(s.sum())} searched): E = {E:.3e}, worst |g - w| - ulp/2 = {worst + E:.3e}")
        assert worst <= 0.0, f"{tag} {key}: {worst + E:.3e} beyond half an ulp, E = {E:.3e}"
        top, worst_over, n_pos = max(top, E), max(worst_over, worst + E), n_pos + K
    return top, worst_over, n_pos


# ------------------------------------------------------------------ 1. frame edges
@pytest.mark.parametrize("k", M.EDGE_FRAMES)
def test_frame_edges(eng, k):
    """M = kH - 1, kH and kH + 1 outputs, asked for with N = M and with N = M - 1."""
    for Mk in (k * M.H_S - 1, k * M.H_S, k * M.H_S + 1):
        for N in (Mk, Mk - 1):
            key = f"edge-{Mk}-{N}"
            got = _run(eng, [key], pad=5)
            _accept("edge", got, [key])
            assert got[1][0] == N


def test_rows_shorter_than_a_frame(eng):
    """n = 1, H - 1 and a row shorter than D; n = 0: out_len 0, zeros, no frame."""
    for n in (1, M.H_S - 1, M.D_S - 10):
        key = f"short-{n}"
        got = _run(eng, [key], pad=3, extra=[(np.zeros(0, dtype=np.float32), 0, M.ROWS[key].r)])
        _accept("short", got, [key])
        y, n_out, st, pos, srch = got
        assert n_out[1] == 0 and st[1] == 0 and srch[1] == 0 and not y[1].any() and (pos[1] == -1).all()


# ------------------------------------------------------------------ 2. the rates in one batch
def test_rates_in_one_batch(eng):
    keys = [f"rates-{i}" for i in range(len(M.RATES))]
    got = _run(eng, keys, lengths=False, pad=1)
    E, over, n_pos = _accept("rates", got, keys)
    print(f"[stretch] rates: largest E {E:.3e}, worst excess over half an ulp {over:.3e}, {n_pos} positions equal")
    y, n_out, st, pos, srch = got
    assert n_out.tolist() == [M.count(3000, r) for r in M.RATES]
    assert M.RATES[0] == 1.0 and srch[0] == 0 and np.array_equal(_bits(y[0, :3000]), _bits(M.ROWS[keys[0]].x))
    assert srch.tolist() == [int(M.case(k)[0][2].sum()) for k in keys] and (srch[2:] > 0).all()


# ------------------------------------------------------------------ 3. ties and windows
def test_ties_and_windows(eng):
    for keys in (["tie-silence"], ["tie-constant"], ["tie-period"], ["match-lo", "match-hi"], ["cut"]):
        got = _run(eng, keys, pad=2)
        _accept("ties", got, keys)
        pos = got[3]
        for b, key in enumerate(keys):
            row = M.ROWS[key]
            q, c, s = M.case(key)[0]
            p = np.array([M.nominal(k, row.r, row.H) for k in range(len(q))])
            if key == "tie-silence":                                     # d = 0 wherever it searches
                assert s.sum() > 3 and np.array_equal(pos[b, :len(q)][s], p[s])
            elif key.startswith("tie-"):                                 # and wherever the windows lie inside the row
                inside = s & (p >= row.D) & (p + row.D + row.H <= row.n) & (c + row.H <= row.n)
                assert inside.sum() > 3 and np.array_equal(pos[b, :len(q)][inside], p[inside])
            elif key.startswith("match-"):
                assert s[1] and pos[b, 1] == p[1] + (-row.D if key == "match-lo" else row.D)
    nan_row = np.full(600, np.nan, dtype=np.float32)                     # an all-NaN row: every score is -inf, d = 0
    y, n_out, st, pos, srch = _run(eng, ["tie-silence"], extra=[(nan_row, 600, 0.8)], N=1000)
    q, c, s = M.positions(nan_row, 600, 0.8, M.H_S, M.D_S)
    assert st[1] == 0 and n_out[1] == 750 and srch[1] == int(s.sum()) > 3 and np.array_equal(pos[1, :len(q)], q)
    assert np.array_equal(q[s], [M.nominal(k, 0.8, M.H_S) for k in np.flatnonzero(s)])
    w = M.direct(nan_row, 600, 0.8, M.H_S, M.D_S, pos=(q, c, s))          # NaN, and 0 where both segments lie past the row
    assert np.isnan(w).sum() > 700 and np.array_equal(np.isnan(y[1, :750]), np.isnan(w)) and not y[1][~np.isnan(y[1])].any()


# ------------------------------------------------------------------ 4. every (hop, search) edge
@pytest.mark.parametrize("H,D", M.HOP_SEARCH)
def test_hop_and_search_edges(eng, H, D):
    key = f"hd-{H}-{D}"
    got = _run(eng, [key], lengths=False, pad=3)
    _accept("hop-search", got, [key])
    assert got[4][0] > 0


# ------------------------------------------------------------------ 5. a long row
def test_long_row(eng):
    """n = 70 000 (past 2^16) at r = 1.03 and the defaults: every frame, the last as the first, is accepted."""
    row = M.ROWS["long"]
    assert row.n == 70000 and row.N == M.count(70000, 1.03) > 65536 and (row.H, row.D) == (M.HOP, M.SEARCH)
    got = _run(eng, ["long"], lengths=False)
    _accept("long", got, ["long"])
    assert got[1][0] == row.N and np.isfinite(got[0]).all() and got[0][0, -300:].any()


# ------------------------------------------------------------------ 6. invalid rows, non-finite samples
def test_invalid_rows_are_zeros_with_status(eng):
    L, N = 400, 500
    ok = [f"inv-ok-{i}" for i in range(M.INVALID_NEIGHBOURS)]
    x = M.voiced(99, L)
    bad = [(x, L, NAN), (x, L, 0.2), (x, L, 4.5), (x, -1, 1.0), (x, L + 1, 1.0)]
    order = []
    for i in range(M.INVALID_NEIGHBOURS):                                # valid, invalid, valid, ..., valid
        order.append(ok[i])
        if i < len(bad):
            order.append(bad[i])
    rows = [(M.ROWS[e].x, M.ROWS[e].n, M.ROWS[e].r) if isinstance(e, str) else e for e in order]
    valid = np.array([isinstance(e, str) for e in order])
    buf = torch.full((len(rows), L + 3), NAN, dtype=torch.float32)
    buf[:, :L] = torch.from_numpy(np.stack([r[0] for r in rows]))
    buf = buf.to(DEV)
    lengths = torch.tensor([r[1] for r in rows], dtype=torch.int32, device=DEV)
    rate = torch.tensor([r[2] for r in rows], dtype=torch.float64, device=DEV)
    got = tuple(t.cpu().numpy() for t in eng.stretch(buf[:, :L], rate, N, lengths, M.H_S, M.D_S, info=True))
    y, n_out, st, pos, srch = got
    assert st.tolist() == [0 if v else 1 for v in valid], st
    assert not y[~valid].any() and not n_out[~valid].any() and not srch[~valid].any() and (pos[~valid] == -1).all()
    _accept("valid rows", tuple(a[valid] for a in got), ok)
    alone = _run(eng, ok, lengths=False)
    assert np.array_equal(_bits(alone[0]), _bits(y[valid])) and np.array_equal(alone[3], pos[valid])
    # the ends of the range themselves are valid
    _, n_edge, st_edge, _, _ = eng.stretch(buf[:2, :L], torch.tensor([0.25, 4.0], dtype=torch.float64, device=DEV), N,
                                           None, M.H_S, M.D_S, info=True)
    assert st_edge.tolist() == [0, 0] and n_edge.tolist() == [N, 100]


def test_non_finite_samples_stay_in_their_row(eng):
    """A row holding NaN and +-inf: its positions are the model's (a NaN score counts as -inf) and its outputs are
    non-finite exactly where the model's are; the rows beside it come out as they do alone."""
    x = np.array(M.voiced(612, 600))
    x[[100, 101, 333, 480]] = [np.nan, np.inf, -np.inf, np.nan]
    r = 1.21
    got = _run(eng, ["nf-a", "nf-b"], extra=[(x, 600, r)])
    _accept("non-finite", got, ["nf-a", "nf-b"])
    y, n_out, st, pos, srch = got
    q, c, s = M.positions(x, 600, r, M.H_S, M.D_S, 700)
    w = M.direct_ld(x, 600, r, M.H_S, M.D_S, 700, (q, c, s))
    assert st[2] == 0 and n_out[2] == len(w) and srch[2] == int(s.sum()) and np.array_equal(pos[2, :len(q)], q)
    bad = ~np.isfinite(w.astype(np.float64))
    assert 0 < bad.sum() < len(w) // 2 and np.array_equal(~np.isfinite(y[2, :len(w)]), bad)
    E = 8.0 * float(np.max(np.abs(M.direct(x, 600, r, M.H_S, M.D_S, 700, (q, c, s))[~bad].astype(M.LD) - w[~bad])))
    assert M.excess(y[2, :len(w)][~bad], w[~bad], E) <= 0.0              # the finite outputs, under the rule
    clean = _run(eng, ["nf-a", "nf-b"])
    assert np.array_equal(_bits(clean[0]), _bits(y[:2])) and np.array_equal(clean[3], pos[:2])


# ------------------------------------------------------------------ 7. independence and replay
def test_bits_depend_on_the_row_alone(eng):
    keys = [f"bits-{i}" for i in range(5)]
    a = _run(eng, keys, pad=7)                                           # NaN tails behind every length, NaN padding
    _accept("bits", a, keys)
    same = lambda u, v: all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(u, v))
    assert same(a, _run(eng, keys, pad=7))                               # a second call
    assert same(a, _run(eng, keys))                                      # other row strides
    assert same(a, _run(eng, keys, L=1500, pad=1))                       # a longer buffer: L beyond the lengths
    rev = _run(eng, keys[::-1])                                          # other neighbours
    assert same(a, tuple(v[::-1] for v in rev))
    for i, k in enumerate(keys):                                         # alone, in a buffer cut to its own length
        one = _run(eng, [k], lengths=False)
        assert same(tuple(v[i:i + 1] for v in a), one), k
    other = _run(eng, keys, rates=[M.ROWS[keys[0]].r, 3.3, 0.27, NAN, M.ROWS[keys[4]].r])   # a neighbour's rate
    assert same(tuple(v[[0, 4]] for v in a), tuple(v[[0, 4]] for v in other))


def test_captured_call_replays_with_new_input_rates_and_lengths(eng):
    keys = ["graph-0", "graph-1"]
    L, N = 600, 640
    wav = torch.from_numpy(np.stack([M.voiced(7100 + b, L) for b in range(2)])).to(DEV)
    rate = torch.tensor([1.2, 0.85], dtype=torch.float64, device=DEV)
    lengths = torch.tensor([L, L - 50], dtype=torch.int32, device=DEV)
    call = lambda: eng.stretch(wav, rate, N, lengths, M.H_S, M.D_S, info=True)
    eager = call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = call()
    graph.replay()
    assert all(torch.equal(p, q) for p, q in zip(got, eager))
    new = np.full((2, L), NAN, dtype=np.float32)
    for b, k in enumerate(keys):
        new[b, :M.ROWS[k].n] = M.ROWS[k].x
    wav.copy_(torch.from_numpy(new).to(DEV))
    rate.copy_(torch.tensor([M.ROWS[k].r for k in keys], dtype=torch.float64, device=DEV))
    lengths.copy_(torch.tensor([M.ROWS[k].n for k in keys], dtype=torch.int32, device=DEV))
    graph.replay()
    again = call()
    assert not torch.equal(again[0], eager[0])
    assert all(torch.equal(p, q) for p, q in zip(got, again))
    _accept("replayed", tuple(t.cpu().numpy() for t in got), keys)
    rate[1] = 5.0                                                        # an invalid row: the replay reports it
    graph.replay()
    assert got[2].tolist() == [0, 1] and got[1].tolist()[1] == 0 and not bool(got[0][1].any())


# ------------------------------------------------------------------ 8. Engine.pitch_shift
def _lag(y, lo=40, hi=160):
    w = np.asarray(y[4000:8096], dtype=np.float64)
    ac = np.correlate(w, w, "full")[len(w) - 1:]
    return lo + int(np.argmax(ac[lo:hi]))


def test_pitch_shift(eng):
    """A 1 s harmonic tone at 200 Hz, 16 kHz: the autocorrelation peak sits at lag 80, after +2 semitones at round(80 /
    2^(2/12)) = 71 +- 1, after -2 at 90 +- 1; the length stays within a hop of the input's; factor 1 is Engine.warp at 1."""
    L = 16000
    t = np.arange(L) / 16000.0
    x = (0.1 * sum(np.sin(2 * np.pi * 200.0 * h * t) / h for h in range(1, 6))).astype(np.float32)
    assert _lag(x) == 80
    wav = torch.from_numpy(np.stack([x, x, x, x])).to(DEV)
    up, down = 2.0 ** (2 / 12.0), 2.0 ** (-2 / 12.0)
    factor = torch.tensor([up, down, 1.0, 2.5], dtype=torch.float64, device=DEV)
    y = eng.pitch_shift(wav, factor)
    assert y.dtype == torch.float32 and tuple(y.shape) == (4, L)
    y = y.cpu().numpy()
    assert abs(_lag(y[0]) - 71) <= 1 and abs(_lag(y[1]) - 90) <= 1 and _lag(y[2]) == 80
    for b in range(3):                                                   # the length: within a hop of the input's
        assert np.abs(y[b, L - 256 - 64:L - 256]).max() > 0.01
    ones = torch.ones(4, dtype=torch.float64, device=DEV)
    assert np.array_equal(_bits(y[2]), _bits(eng.warp(wav, ones, L)[2].cpu().numpy()))
    assert not y[3].any()                                                # a factor outside [1/2, 2]: zeros
    longer = eng.pitch_shift(wav, factor, n_out=L + 500).cpu().numpy()
    ends = [int(np.flatnonzero(longer[b])[-1]) + 1 for b in range(3)]
    assert all(abs(e - L) <= 256 for e in ends), ends
    assert np.array_equal(_bits(longer[:, :L - 600]), _bits(y[:, :L - 600]))


# ------------------------------------------------------------------ 9. the mixer
def _speechlike(B, L):
    t = np.arange(L) / 16000.0
    return np.stack([(M.voiced(300 + b, L, 80.0 + b) * (0.6 + 0.4 * np.sin(2 * np.pi * (2.0 + b) * t))).astype(np.float32)
                     for b in range(B)])


def _mixer(eng, seed, **kw):
    from cmgan_amd.mixing import DynamicMixer, NoiseBank
    rng = np.random.default_rng(5)
    nb = NoiseBank.from_arrays([0.1 * rng.standard_normal(5000), 0.05 * rng.standard_normal(1234)], device=DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return DynamicMixer(eng, nb, None, snr_db=(0.0, 15.0), early_ms=None, generator=gen, level_db=(-30.0, -20.0), **kw)


def test_mixer_at_the_defaults_is_unchanged(eng):
    B, L = 3, 2 * 256 + 17
    clean = torch.from_numpy(_speechlike(B, L)).to(DEV)
    for kw in (dict(), dict(speed=(0.9, 1.1), p_speed=0.5)):
        a = _mixer(eng, 12, **kw)
        b = _mixer(eng, 12, tempo=None, p_tempo=0.3, pitch=None, p_pitch=0.3, stretch_hop=64, stretch_search=9, **kw)
        ta, na, ia = a(clean)
        tb, nb_, ib = b(clean)
        assert torch.equal(ta, tb) and torch.equal(na, nb_) and all(torch.equal(p, q) for p, q in zip(ia, ib))
        assert type(a.last_draw) is type(b.last_draw) and len(a.last_draw) == len(b.last_draw)
        for p, q in zip(a.last_draw, b.last_draw):
            assert (p is None and q is None) or torch.equal(p, q)
        assert a.last_stretch is None and b.last_stretch is None
        assert torch.equal(a.generator.get_state(), b.generator.get_state())


@pytest.mark.parametrize("which", ["tempo", "pitch", "all"])
def test_mixer_with_tempo_and_pitch(eng, which):
    from cmgan_amd.mixing import stretch_len, warp_len
    B, L = 8, 3000
    clean = torch.from_numpy(_speechlike(B, L)).to(DEV)
    kw = {"tempo": dict(tempo=(0.9, 1.1)), "pitch": dict(pitch=(-2.0, 2.0), p_pitch=0.7),
          "all": dict(tempo=(0.9, 1.1), p_tempo=0.6, pitch=(-2.0, 3.0), speed=(0.95, 1.05))}[which]
    plain = _mixer(eng, 31, **({"speed": kw["speed"]} if "speed" in kw else {}))
    plain(clean)
    mixer = _mixer(eng, 31, **kw)
    target, noisy, info = mixer(clean)
    N = stretch_len(L, kw.get("tempo"), kw.get("pitch"), kw.get("speed"), kw.get("p_tempo", 1.0), kw.get("p_pitch", 1.0))
    assert N == mixer.stretch_len(L) and tuple(target.shape) == (B, N) and tuple(noisy.shape) == (B, N)
    d, s = mixer.last_draw, mixer.last_stretch
    for p, q in zip(plain.last_draw, d):                                 # every other draw is what it was
        assert (p is None and q is None) or torch.equal(p, q)
    v = d.speed if d.speed is not None else torch.ones(B, dtype=torch.float64, device=DEV)
    assert torch.equal(s.stretch_rate, s.tempo / s.pitch_factor)
    if which == "tempo":
        assert s.warp_rate is None and bool((s.pitch_factor == 1.0).all())
    else:
        assert torch.equal(s.warp_rate, v * s.pitch_factor)
    (t_lo, t_hi), (f_lo, f_hi), (v_lo, v_hi) = mixer._ranges()
    N1 = warp_len(L, t_hi / f_lo)
    long, n1, st1, _, _ = eng.stretch(clean, s.stretch_rate, N1, info=True)
    assert not bool(st1.any()) and n1.tolist() == [N1] * B               # every row is full
    if s.warp_rate is not None:
        long, n2, st2 = eng.warp(long, s.warp_rate, warp_len(N1, v_hi * f_hi), info=True)
        assert not bool(st2.any()) and n2.tolist() == [N] * B
    lv = eng.speech_level(long, fs=16000)
    scaled = (long * mixer.level_gain(lv, d.level_db)[:, None]).contiguous()
    noisy2, target2, _ = eng.mix(scaled, mixer.noise_bank.data, d.noise_start, d.noise_len, d.noise_off, d.snr_db,
                                 None, None, None, peak=mixer.peak, early=-1)
    assert torch.equal(target, target2) and torch.equal(noisy, noisy2)
    assert bool(torch.isfinite(noisy).all()) and bool((target[:, -32:].abs().amax(dim=1) > 0).all())


def test_mixer_with_probability_zero_copies_the_rows(eng):
    B, L = 4, 2000
    clean = torch.from_numpy(_speechlike(B, L)).to(DEV)
    from cmgan_amd.mixing import DynamicMixer, NoiseBank
    nb = NoiseBank.from_arrays([0.1 * np.random.default_rng(5).standard_normal(5000)], device=DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    mixer = DynamicMixer(eng, nb, None, snr_db=(0.0, 15.0), early_ms=None, generator=gen, tempo=(0.8, 1.25), p_tempo=0.0,
                         p_pitch=0.0)
    target, noisy, _ = mixer(clean)
    d, s = mixer.last_draw, mixer.last_stretch
    assert bool((s.stretch_rate == 1.0).all()) and s.warp_rate is None
    N = mixer.stretch_len(L)
    assert N == M.count(L, 1.25) and tuple(target.shape) == (B, N)
    y, n_out, st, pos, srch = eng.stretch(clean, s.stretch_rate, N, info=True)
    assert torch.equal(y, clean[:, :N]) and not bool(srch.any())         # rate-1 rows are copies
    noisy2, target2, _ = eng.mix(clean[:, :N].contiguous(), nb.data, d.noise_start, d.noise_len, d.noise_off, d.snr_db,
                                 None, None, None, peak=mixer.peak, early=-1)
    assert torch.equal(target, target2) and torch.equal(noisy, noisy2)


def test_mixing_loader_clamps_the_lengths(eng):
    from cmgan_amd.mixing import MixingLoader
    B, L = 4, 1500
    clips = torch.from_numpy(_speechlike(B, L))
    mixer = _mixer(eng, 5, tempo=(0.95, 1.05))
    target, noisy, length = next(iter(MixingLoader([(clips, torch.tensor([L, L - 10, 50, 5 * L]))], mixer)))
    N = mixer.stretch_len(L)
    assert N == M.count(L, 1.05) and tuple(noisy.shape) == (B, N) and length.tolist() == [N, N, 50, N]
