"""The noise suppressor on the GPU (cmgan_amd/csrc/suppress.hip; include/cmgan_hip.h, "Suppression"): Engine.suppress
against the numpy model of tests/suppress_model.py - rows of 1, h - 1, h, h + 1, 2 h, 5 h + 37, 2000 and 0 samples at N = 256
(F = 129: two waves and one lane), the three rules and rule 0 in one batch, minimum windows of 1, 3 and more than the row's
frames, a_dd = 0, a_n = 0, g_min = 1, xi_min = 0 and 1, digital silence at the start and inside, a row of peak 4.0, N = 512
and 1024, a key that is not the signal and one that is, in place against out of place, per-row lengths with NaN tails and
NaN padding, invalid rows of every kind, a NaN sample, bit-reproducibility, independence of B, of the neighbours, of the
padding and of L, hipGraph replay with the signal, the table and the lengths changed in place, DynamicMixer(suppressor=...)
and evaluation.suppress_one_track.

Acceptance (suppress_model's docstring).  Status words, zeros and bit copies are compared for EQUALITY.  A sample g is
accepted against the model's long-double w when |g - w| <= ulp32(w) / 2 + E, and a gain when |G - G_w| <= E_G; E and E_G per
row from the model alone (8 x the larger distance of two float64 evaluations from w); every row used is registered in
suppress_model.build_rows, where the host test checks E <= 2^-10 x ulp32(rms) / 2 and E_G <= 2^-30 without a GPU; every check
prints E, E_G and the worst excesses.

Measured on an MI355X: every status, every zero and every bit copy was equal.  Over the 46 row checks (52 766 samples, 64 956
gains; N = 256, 512 and 1024) the largest E of any row is 1.3e-14 (the row of peak 4.0; 1.6e-15 among the others) and the
worst |g - w| - ulp32(w) / 2 is 1.4e-17, on the row that starts in silence, whose E is 1.3e-15: a hundredth of it; no
sample of any other row lies beyond half an ulp at all.  The largest E_G is 2.5e-13 and the worst |G - G_w| 3.0e-14, on a row
whose E_G is 8.6e-14 (0.35 of it).  The mixer's rows (n_fft 512, windows of 49 .. 84 frames) and the 1-second tracks of
suppress_one_track stay inside half an ulp as well."""
import numpy as np
import pytest
import torch

import suppress_model as M

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


def _run(eng, names, L=None, lengths=True, pad=0, extra=None, inplace=False, key_is_x=False, info=True):
    """The registered rows as one batch -> (y float32 [B, L], status, gain [B, T, F]) as numpy.  The buffers are L (default:
    the longest row) + `pad` wide and NaN wherever a row has no sample; `extra` = (x, n, table row) rows that are not
    registered are appended as they are.  A key batch is passed when a row has one (the others' key is their signal), or
    with key_is_x for every row."""
    rows = [M.ROWS[k] for k in names]
    N = rows[0].N
    assert all(r.N == N for r in rows)
    specs = [(r.x, r.n, r.p, r.key) for r in rows] + [(x, n, p, None) for x, n, p in (extra or [])]
    B = len(specs)
    L = max(max(len(s[0]) for s in specs), 1) if L is None else L
    buf = np.full((B, L + pad), NAN, dtype=np.float32)
    kbuf = np.full((B, L + pad), NAN, dtype=np.float32)
    for b, (x, n, p, key) in enumerate(specs):
        buf[b, :len(x)] = x
        kbuf[b, :len(x)] = x if key is None else key
    buf = torch.from_numpy(buf).to(DEV)
    wav = buf[:, :L]
    key = torch.from_numpy(kbuf).to(DEV)[:, :L] if key_is_x or any(s[3] is not None for s in specs) else None
    if lengths:
        ld = torch.tensor([s[1] for s in specs], dtype=torch.int32, device=DEV)
    else:
        assert all(s[1] == L for s in specs)
        ld = None
    table = torch.from_numpy(np.stack([s[2] for s in specs])).to(DEV)
    ybuf = buf if inplace else torch.full((B, L + pad), NAN, dtype=torch.float32, device=DEV)
    got = eng.suppress(wav, table, N, ld, key, out=ybuf[:, :L], info=info)
    if not info:
        return got.cpu().numpy()
    y, st, gain = got
    assert y.dtype == torch.float32 and tuple(y.shape) == (B, L) and y.data_ptr() == ybuf.data_ptr()
    assert st.dtype == torch.int32 and tuple(st.shape) == (B,)
    assert gain.dtype == torch.float64 and tuple(gain.shape) == (B, -(-L // (N // 2)) + 1, N // 2 + 1)
    if pad:
        assert bool(torch.isnan(ybuf[:, L:]).all()), "the padding behind y was written"
    return tuple(t.cpu().numpy() for t in (y, st, gain))


TOTALS = {"checks": 0, "samples": 0, "gains": 0, "E": 0.0, "worst": -np.inf, "E_G": 0.0, "worst_G": -np.inf,
          "worst_over_E": -np.inf, "worst_G_over_E_G": -np.inf}


def _accept(tag, got, names):
    """Every registered row of the batch against the model: the status for equality, zeros from n on and behind the row's
    last frame, rule 0 bit for bit, the samples and the gains under the rule."""
    y, st, gain = got
    for b, name in enumerate(names):
        row = M.ROWS[name]
        res, E, EG = M.case(name)
        Tb = res.G.shape[0]
        assert st[b] == 0, f"{tag} {name}: status {st[b]}"
        assert not y[b, row.n:].any(), f"{tag} {name}: samples from n on are not zero"
        assert not gain[b, Tb:].any(), f"{tag} {name}: gains behind the last frame are not zero"
        if int(row.p[0]) == M.OFF:
            assert np.array_equal(_bits(y[b, :row.n]), _bits(row.x)) and (gain[b, :Tb] == 1.0).all(), f"{tag} {name}: rule 0"
            continue
        worst = M.excess(y[b, :row.n], res.w, E)
        worst_g = M.gain_excess(gain[b, :Tb], res.G, EG)
        print(f"[suppress] {tag} {name} (n = {row.n}, N = {row.N}, rule {int(row.p[0])}, D = {int(row.p[3])}): E = {E:.3e}, worst "
              f"|g - w| - ulp/2 = {worst + E:.3e}; E_G = {EG:.3e}, worst |G - G_w| = {worst_g + EG:.3e}")
        assert worst <= 0.0, f"{tag} {name}: {worst + E:.3e} beyond half an ulp, E = {E:.3e}"
        assert worst_g <= 0.0, f"{tag} {name}: a gain {worst_g + EG:.3e} from the model's, E_G = {EG:.3e}"
        TOTALS["checks"] += 1
        TOTALS["samples"] += row.n
        TOTALS["gains"] += res.G.size
        TOTALS["E"], TOTALS["E_G"] = max(TOTALS["E"], E), max(TOTALS["E_G"], EG)
        TOTALS["worst"], TOTALS["worst_G"] = max(TOTALS["worst"], worst + E), max(TOTALS["worst_G"], worst_g + EG)
        if E > 0.0:
            TOTALS["worst_over_E"] = max(TOTALS["worst_over_E"], (worst + E) / E)
        if EG > 0.0:
            TOTALS["worst_G_over_E_G"] = max(TOTALS["worst_G_over_E_G"], (worst_g + EG) / EG)
    print(f"[suppress] totals so far: {TOTALS}")


# ------------------------------------------------------------------ 1. the definition
def test_lengths_in_one_batch(eng):
    names = [f"len-{n}" for n in M.LENGTHS]
    _accept("lengths", _run(eng, names, pad=3), names)


def test_every_rule_in_one_batch(eng):
    names = [f"rule-{r}" for r in (M.OFF, M.WIENER, M.SPECSUB, M.LOGMMSE)]
    _accept("rules", _run(eng, names, lengths=False), names)


def test_minimum_windows(eng):
    names = [f"D-{D}" for D in (1, 3, 128)]
    _accept("windows", _run(eng, names, lengths=False), names)


def test_extreme_table_values(eng):
    names = ["a_dd-0", "a_n-0", "g_min-1", "xi_min-0", "xi_min-1"]
    got = _run(eng, names, lengths=False)
    _accept("extremes", got, names)
    assert (got[2][2] == 1.0).all()                                     # g_min = 1: every gain is 1


def test_digital_silence_and_a_loud_row(eng):
    names = ["silence-start", "silence-inside", "loud"]
    assert np.abs(M.ROWS["loud"].x).max() == 4.0
    _accept("silence", _run(eng, names, lengths=False), names)


@pytest.mark.parametrize("N", [512, 1024])
def test_other_transform_sizes(eng, N):
    names = [f"N-{N}-{r}" for r in (M.WIENER, M.SPECSUB, M.LOGMMSE)]
    _accept(f"N = {N}", _run(eng, names, lengths=False), names)


# ------------------------------------------------------------------ 2. the key, in place
def test_key_that_is_not_the_signal(eng):
    names = [f"key-{r}" for r in (M.WIENER, M.SPECSUB, M.LOGMMSE)]
    got = _run(eng, names, lengths=False)
    _accept("key", got, names)
    again = _run(eng, names, lengths=False, inplace=True)               # in place, with a key
    assert all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(got, again))


def test_key_that_is_the_signal_gives_the_bits_of_no_key(eng):
    names = ["ok-0", "ok-1", "ok-2", "ok-3"]
    a = _run(eng, names, lengths=False)
    b = _run(eng, names, lengths=False, key_is_x=True)
    assert all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(a, b))
    _accept("key = x", b, names)


def test_in_place_equals_out_of_place(eng):
    names = [f"rowlen-{i}" for i in range(4)] + ["rule-0"]
    a = _run(eng, names, pad=2)
    b = _run(eng, names, pad=2, inplace=True)
    assert all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(a, b))
    y = _run(eng, names, pad=2, info=False)                             # and without the info outputs
    assert np.array_equal(_bits(y), _bits(a[0]))


# ------------------------------------------------------------------ 3. lengths, invalid rows, non-finite samples
def test_per_row_lengths_with_nan_tails_and_padding(eng):
    names = [f"rowlen-{i}" for i in range(4)]
    _accept("row lengths", _run(eng, names, L=2100, pad=7), names)


def _invalid_rows():
    ok = M.params(rule=M.WIENER)
    bad = []
    for col, vals in ((0, (-1.0, 4.0, 1.5, NAN)), (1, (-0.1, 1.0, NAN, np.inf)), (2, (-0.1, 1.0, NAN)), (3, (0.0, 129.0, 2.5, NAN)),
                      (4, (0.0, -1.0, 16.5, np.inf, NAN)), (5, (0.0, 1.5, -0.5, NAN)), (6, (-0.1, 1.5, NAN))):
        for v in vals:
            p = ok.copy()
            p[col] = v
            bad.append((p, 300))
    p = M.params(rule=M.OFF)                                             # rule 0 does not excuse a bad entry
    p[4] = 0.0
    bad.append((p, 300))
    bad.append((ok.copy(), -1))
    bad.append((ok.copy(), 1001))
    return bad


def test_invalid_rows_beside_good_ones(eng):
    names = ["ok-0", "ok-1", "ok-2", "ok-3"]
    alone = _run(eng, names, lengths=False)
    x = M.noisy(95, 1000)
    bad = _invalid_rows()
    got = _run(eng, names, L=1000, extra=[(x, n, p) for p, n in bad])
    assert got[1].tolist() == [0] * 4 + [1] * len(bad)
    assert not got[0][4:].any() and not got[2][4:].any()
    assert all(np.array_equal(p[:4].view(np.uint8), q.view(np.uint8)) for p, q in zip(got, alone))
    _accept("beside invalid rows", tuple(v[:4] for v in got), names)


def test_a_nan_sample_stays_in_its_row(eng):
    names = ["ok-0", "ok-1", "ok-2", "ok-3"]
    alone = _run(eng, names, lengths=False)
    x = M.noisy(96, 1000).copy()
    x[500] = NAN
    x[700] = np.inf
    got = _run(eng, names, L=1000, extra=[(x, 1000, M.params(rule=M.LOGMMSE)), (x, 1000, M.params(rule=M.OFF))])
    assert got[1].tolist() == [0] * 6
    assert all(np.array_equal(p[:4].view(np.uint8), q.view(np.uint8)) for p, q in zip(got, alone))
    assert np.array_equal(_bits(got[0][5]), _bits(x))                   # rule 0: the copy, NaN included


# ------------------------------------------------------------------ 4. bits
def test_bits_repeat_and_do_not_depend_on_the_batch(eng):
    names = [f"rowlen-{i}" for i in range(4)]
    same = lambda p, q: all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(p, q))
    L = 2000
    T = lambda n: -(-n // M.H) + 1
    a = _run(eng, names)
    assert same(a, _run(eng, names))
    wide = _run(eng, names, L=L + 777, pad=5)                           # L and the padding
    assert same(a, (wide[0][:, :L], wide[1], wide[2][:, :T(L)])) and not wide[0][:, L:].any() and not wide[2][:, T(L):].any()
    for i, k in enumerate(names):                                       # alone, in a buffer cut to its own length
        n = M.ROWS[k].n
        one = _run(eng, [k], lengths=False)
        assert same((a[0][i:i + 1, :n], a[1][i:i + 1], a[2][i:i + 1, :T(n)]), one), k
    inside = ["ok-0", "ok-1", names[0], "rule-0", "ok-2", "D-128", "ok-3", "len-677", "len-0"]       # the row inside 9
    nine = _run(eng, inside, L=L)
    assert same(tuple(v[2:3] for v in nine), tuple(v[:1] for v in a))
    x = M.noisy(97, 100)                                                 # other neighbours: another rule, a short row, an invalid one
    other = _run(eng, names[:1], L=L, extra=[(x, 100, M.params(rule=M.SPECSUB, D=1)), (x, -5, M.params())])
    assert same(tuple(v[:1] for v in a), tuple(v[:1] for v in other))


def test_captured_call_replays_with_new_signal_table_and_lengths(eng):
    names = [f"graph-{i}" for i in range(4)]
    L = 1100
    wav = torch.from_numpy(np.stack([M.noisy(200 + b, L) for b in range(4)])).to(DEV)
    table = torch.from_numpy(np.stack([M.params(rule=M.WIENER, D=7)] * 4)).to(DEV)
    lengths = torch.tensor([L, 900, 500, 1], dtype=torch.int32, device=DEV)
    call = lambda: eng.suppress(wav, table, 256, lengths, info=True)
    eager = call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = call()
    graph.replay()
    assert all(torch.equal(p, q) for p, q in zip(got, eager))
    wav.copy_(torch.from_numpy(np.stack([M.ROWS[k].x for k in names])).to(DEV))
    table.copy_(torch.from_numpy(np.stack([M.ROWS[k].p for k in names])).to(DEV))
    lengths.fill_(L)
    graph.replay()
    again = call()
    assert not torch.equal(again[0], eager[0])
    assert all(torch.equal(p, q) for p, q in zip(got, again))
    _accept("replayed", tuple(t.cpu().numpy() for t in got), names)
    table[1, 3] = 0.0                                                   # an invalid row: the replay reports it
    graph.replay()
    assert got[1].tolist() == [0, 1, 0, 0] and not bool(got[0][1].any()) and not bool(got[2][1].any())


# ------------------------------------------------------------------ 5. the mixer, the baseline
def _mixer(eng, seed, **kw):
    from cmgan_amd.mixing import DynamicMixer, NoiseBank
    rng = np.random.default_rng(5)
    nb = NoiseBank.from_arrays([0.01 * rng.standard_normal(9000), 0.005 * rng.standard_normal(4321)], device=DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return DynamicMixer(eng, nb, None, snr_db=(5.0, 15.0), early_ms=None, generator=gen, **kw)


@pytest.mark.parametrize("on", ["noisy", "both"])
def test_mixer_with_suppressor(eng, on):
    from cmgan_amd.mixing import SuppressDraw, SuppressorSampler
    B, L = 6, 4000
    clean = torch.from_numpy(np.stack([M.noisy(300 + b, L, sigma=0.002) for b in range(B)])).to(DEV)
    plain = _mixer(eng, 41)
    target0, noisy0, _ = plain(clean)
    assert plain.last_suppression is None
    none = _mixer(eng, 41, suppressor=None, suppressor_on=on)            # None: the bits of a mixer built without the argument
    target1, noisy1, _ = none(clean)
    assert torch.equal(target1, target0) and torch.equal(noisy1, noisy0) and none.last_suppression is None
    gen = torch.Generator(device=DEV)
    gen.manual_seed(78)
    mixer = _mixer(eng, 41, suppressor=SuppressorSampler(p=0.8, generator=gen), suppressor_on=on)
    target, noisy, _ = mixer(clean)
    for p, q in zip(plain.last_draw, mixer.last_draw):                   # every other draw is what it was
        assert (p is None and q is None) or torch.equal(p, q)
    assert torch.equal(plain.generator.get_state(), mixer.generator.get_state())
    d = mixer.last_suppression
    assert isinstance(d, SuppressDraw) and d.n_fft == 512 and tuple(d.table.shape) == (B, 7) and d.table.dtype == torch.float64
    rules = d.table[:, 0].tolist()
    assert 0.0 in rules and any(r > 0.0 for r in rules), rules
    y, st, _ = eng.suppress(noisy0, d.table, 512, info=True)             # the stage is this call, in place
    assert torch.equal(noisy, y) and not bool(st.any())
    if on == "both":
        assert torch.equal(target, eng.suppress(target0, d.table, 512, key=noisy0))
    else:
        assert torch.equal(target, target0)
    x0, tab, got = noisy0.cpu().numpy(), d.table.cpu().numpy(), noisy.cpu().numpy()
    for b in range(B):                                                   # against the model fed the mixer's own draw
        res = M.suppress(x0[b], L, tab[b], 512)
        E = M.slack(res)
        assert E <= M.condition(res)
        worst = M.excess(got[b], res.w, E)
        print(f"[suppress] mixer {on} row {b} (rule {int(tab[b, 0])}, D = {int(tab[b, 3])}): E = {E:.3e}, worst |g - w| - ulp/2 = "
              f"{worst + E:.3e}")
        assert worst <= 0.0


def test_suppress_one_track(eng):
    from cmgan_amd.evaluation import suppress_one_track
    from cmgan_amd.mixing import suppress_params
    x = M.noisy(400, 16000)
    track = torch.from_numpy(x[None]).to(DEV)
    for rule in ("logmmse", "wiener", "specsub"):
        y = suppress_one_track(eng, track, rule=rule)
        assert y.dtype == torch.float32 and tuple(y.shape) == (1, 16000)
        p = suppress_params(rule, fs=16000, n_fft=512).numpy()
        res = M.suppress(x, 16000, p, 512)
        E = M.slack(res)
        assert E <= M.condition(res)
        worst = M.excess(y[0].cpu().numpy(), res.w, E)
        print(f"[suppress] one track, {rule}: E = {E:.3e}, worst |g - w| - ulp/2 = {worst + E:.3e}, energy out / in = "
              f"{float((res.w.astype(np.float64) ** 2).sum() / (x.astype(np.float64) ** 2).sum()):.3f}")
        assert worst <= 0.0
    assert torch.equal(suppress_one_track(eng, track, rule="off"), track)
    with pytest.raises(ValueError):
        suppress_one_track(eng, track[0])
