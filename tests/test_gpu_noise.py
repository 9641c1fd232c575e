"""The synthetic noise on the GPU (cmgan_amd/csrc/noise.hip; include/cmgan_hip.h, "Synthetic noise"): Engine.noise against
the float64 model of tests/noise_model.py at the tile, filter, start and counter edges, the envelope's hops, the tones'
phases, the clicks' thresholds, the chunking guarantee, bit-reproducibility and independence of N, of the neighbours, of
the row order, of the padding and of K beyond len, invalid rows beside valid ones, hipGraph replay with every table changed
in place, and the consumers (NoiseBank.synthesize, DynamicMixer(noise=)).

Acceptance (noise_model's docstring): a sample g is accepted against the model's float64 w when |g - w| <= ulp32(w) / 2 + E +
CAP.  E and CAP are computed per row from the model alone; every check prints them and the worst excess.  Every sample of
every row is judged.

Measured on an MI355X: the largest E of any case here is 4.4e-14 (the 1023-tap rows), the largest CAP 2.5e-12, and the worst
|g - w| - ulp32(w) / 2 of any generated sample is -4.5e-17: every sample is the correctly rounded one, and no case needed
its E or its CAP."""
import numpy as np
import pytest
import torch

import mix_model
import noise_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def eng():
    from cmgan_amd.engine import Engine
    return Engine(device=DEV)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _tables(c, rows=None):
    """The case's tables on the device (a sub-batch or another order with rows=[...]): the keyword arguments of Engine.noise."""
    pick = (lambda a: a) if rows is None else (lambda a: None if a is None else a[list(rows)])
    return dict(seed=_dev(pick(c["seed"])), fir=_dev(pick(c["fir"])), n=c["K"], lengths=_dev(pick(c["len"])), start=_dev(pick(c["start"])),
                env=_dev(pick(c["env"])), env_hop=c["H"] if c["env"] is not None else None, tones=_dev(pick(c["tones"])),
                n_tones=_dev(pick(c["n_tones"])), impulse=_dev(pick(c["imp"])))


def _run(eng, c, rows=None, **over):
    kw = _tables(c, rows)
    kw.update(over)
    y, st = eng.noise(info=True, **kw)
    N = kw["seed"].numel()
    assert y.dtype == torch.float32 and tuple(y.shape) == (N, kw["n"]) and st.dtype == torch.int32 and tuple(st.shape) == (N,)
    return y.cpu().numpy(), st.cpu().numpy()


def _accept(tag, y, name, rows=None):
    """Every row of the case `name` - or of a case itself - (or of the sub-batch rows=[...]) against the model.  Returns the
    worst |g - w| - ulp32(w) / 2."""
    model = M.case_model(name) if isinstance(name, str) else M.model_of(name)
    top = -np.inf
    for b, r in enumerate(range(len(model)) if rows is None else rows):
        w, E, cap, status = model[r]
        made = w != 0.0                                            # (the rest is padding: zeros, bit for bit)
        assert not y[b][~made].any(), f"{tag} row {r}: samples past the row's length are not zero"
        worst = M.excess(y[b][made], w[made], 0.0)
        print(f"[noise] {tag} row {r}: E = {E:.3e}, cap = {cap:.3e}, worst |g - w| - ulp/2 = {worst:.3e}")
        assert worst <= E + cap, f"{tag} row {r}: {worst:.3e} beyond half an ulp, E = {E:.3e}, cap = {cap:.3e}"
        top = max(top, worst)
    return top


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ 1. tile edges: K and len
@pytest.mark.parametrize("K", M.EDGES, ids=lambda K: f"K={K}")
def test_tile_edges(eng, K):
    c = M.get(f"edge-{K}")
    y, st = _run(eng, c)
    assert not st.any()
    _accept(f"K = {K}", y, f"edge-{K}")
    for b, n in enumerate(c["len"]):
        assert not y[b, n:].any() and (n == 0 or y[b, :n].any())


# ------------------------------------------------------------------ 2. filter lengths and the q < 0 region
@pytest.mark.parametrize("NF", M.FILTERS, ids=lambda NF: f"NF={NF}")
def test_filter_lengths_and_starts(eng, NF):
    y, st = _run(eng, M.get(f"filter-{NF}"))
    assert not st.any()
    _accept(f"NF = {NF}", y, f"filter-{NF}")


# ------------------------------------------------------------------ 3. the counter's word boundary and the last index
def test_counter_word_boundary_and_last_index(eng):
    c = M.get("far")
    assert c["start"].tolist() == [2 ** 32 - 100, 2 ** 40 - c["K"]]
    y, st = _run(eng, c)
    assert not st.any()
    _accept("far", y, "far")


# ------------------------------------------------------------------ 4. the envelope
@pytest.mark.parametrize("H", sorted(M.HOPS), ids=lambda H: f"H={H}")
def test_envelope_hops(eng, H):
    c = M.get(f"hop-{H}")
    assert c["K"] > (c["P"] - 1) * H or H == 5000                 # the last point holds (H = 5000: one segment only)
    y, st = _run(eng, c)
    assert not st.any()
    _accept(f"H = {H}", y, f"hop-{H}")


def test_envelope_of_one_point_and_none(eng):
    c = M.get("one-point")
    y, st = _run(eng, c)
    assert not st.any()
    _accept("P = 1", y, "one-point")
    bare, _ = _run(eng, c, env=None, env_hop=None)                # g = 1: the rows at half and twice that
    assert np.array_equal(y[0], (0.5 * bare[0].astype(np.float64)).astype(np.float32))
    assert np.array_equal(y[1], (2.0 * bare[1].astype(np.float64)).astype(np.float32))


# ------------------------------------------------------------------ 5. tones
def test_tones(eng):
    c = M.get("tones")
    assert c["n_tones"].tolist() == [0, 8, 2, 1] and np.isnan(c["tones"][0]).all() and np.isnan(c["tones"][2, 2:]).all()
    y, st = _run(eng, c)
    assert not st.any() and not np.isnan(y).any()
    _accept("tones", y, "tones")
    # without the table row 0 - which uses none - keeps its bits
    bare, _ = _run(eng, c, tones=None, n_tones=None)
    assert np.array_equal(_bits(bare[0]), _bits(y[0])) and not np.array_equal(bare[1], y[1])


# ------------------------------------------------------------------ 6. clicks
def test_clicks(eng):
    c = M.get("clicks")
    assert c["imp"][:, 0].tolist() == [0.0, 1.0, 2.0 ** 31, 2.0 ** 32 - 1.0, 2.0 ** 26]
    y, st = _run(eng, c)
    assert not st.any()
    _accept("clicks", y, "clicks")
    bare, _ = _run(eng, c, impulse=None)
    assert np.array_equal(_bits(bare[0]), _bits(y[0]))            # threshold 0: the row without clicks
    assert not np.array_equal(bare[2], y[2]) and not np.array_equal(bare[3], y[3])


# ------------------------------------------------------------------ 7. whole = chunks
def test_whole_row_is_its_chunks(eng):
    c = M.get("whole")
    whole, st = _run(eng, c)
    assert not st.any()
    _accept("whole", whole, "whole")
    a, _ = _run(eng, c, n=256)
    b, _ = _run(eng, c, n=744, start=torch.tensor([256], dtype=torch.int64, device=DEV))
    assert np.array_equal(_bits(np.concatenate([a[0], b[0]])), _bits(whole[0]))
    # and cut by a length instead of K
    a2, _ = _run(eng, c, lengths=torch.tensor([256], dtype=torch.int32, device=DEV))
    assert np.array_equal(_bits(a2[0, :256]), _bits(whole[0, :256])) and not a2[0, 256:].any()


# ------------------------------------------------------------------ 8. bit-reproducible, row-independent
def test_bit_reproducible_and_row_independent(eng):
    c = M.get("mixed")
    K, lens = c["K"], c["len"].tolist()
    y, st = _run(eng, c)
    assert not st.any()
    _accept("mixed", y, "mixed")
    again, _ = _run(eng, c)
    assert np.array_equal(_bits(again), _bits(y))
    for rows in ([0], [2, 0, 1], [1, 1, 2, 0, 0]):                # batch sizes and row orders
        sub, _ = _run(eng, c, rows)
        assert np.array_equal(_bits(sub), _bits(y[rows])), rows
        _accept(f"rows {rows}", sub, "mixed", rows)
    buf = torch.full((3, K + 37), NAN, dtype=torch.float32, device=DEV)      # a padded ld: the padding stays
    padded, _ = _run(eng, c, out=buf[:, :K])
    assert np.array_equal(_bits(padded), _bits(y)) and bool(torch.isnan(buf[:, K:]).all())
    grown, _ = _run(eng, c, n=K + 300, lengths=_dev(c["len"]))    # K grown beyond len
    assert np.array_equal(_bits(grown[:, :K]), _bits(y)) and not grown[:, K:].any()
    for b, n in enumerate(lens):
        assert not y[b, n:].any()


# ------------------------------------------------------------------ 9. invalid rows beside valid ones
def _edit(key, value, index=None):
    def apply(c):
        a = np.array(c[key])
        if index is None:
            a[1] = value
        else:
            a[(1,) + index] = value
        c[key] = a
    return apply


_INVALID = {
    "fir NaN": _edit("fir", NAN, (4,)), "fir inf": _edit("fir", INF, (0,)), "env -inf": _edit("env", -INF, (3,)),
    "env NaN": _edit("env", NAN, (0,)), "tone amp NaN": _edit("tones", NAN, (0, 1)), "tone phase inf": _edit("tones", INF, (0, 2)),
    "tone nu NaN": _edit("tones", NAN, (0, 0)), "nu above 1/2": _edit("tones", 0.5000001, (0, 0)), "nu below 0": _edit("tones", -1e-9, (0, 0)),
    "click amp NaN": _edit("imp", NAN, (1,)), "thr fraction": _edit("imp", 1.5, (0,)), "thr 2^32": _edit("imp", 2.0 ** 32, (0,)),
    "thr negative": _edit("imp", -1.0, (0,)), "thr NaN": _edit("imp", NAN, (0,)), "len -1": _edit("len", -1), "len K+1": _edit("len", 301),
    "n_tones -1": _edit("n_tones", -1), "n_tones M+1": _edit("n_tones", 3), "start -1": _edit("start", -1),
    "start past 2^40": _edit("start", 2 ** 40 - 300 + 1),
}


def test_invalid_rows_are_zeros_with_status(eng):
    base = M.get("mixed")
    good, _ = _run(eng, base)
    for what, apply in _INVALID.items():
        c = dict(base)
        apply(c)
        assert [M.invalid(r, c["K"], c["M"]) for r in M.rows_of(c)] == [False, True, False], what
        buf = torch.full((3, c["K"]), NAN, dtype=torch.float32, device=DEV)
        y, st = _run(eng, c, out=buf)
        assert st.tolist() == [0, 1, 0], what
        assert not y[1].any(), what                                # K zeros, whatever len says
        assert np.array_equal(_bits(y[[0, 2]]), _bits(good[[0, 2]])), what
    # what a row does not use does not count: row 1 uses one tone, its second column may hold anything
    c = dict(base)
    _edit("tones", NAN, (1, 1))(c)
    y, st = _run(eng, c)
    assert st.tolist() == [0, 0, 0] and np.array_equal(_bits(y), _bits(good))


# ------------------------------------------------------------------ 10. graph replay
def test_captured_call_replays_with_every_table_rewritten(eng):
    a, b = M.get("mixed"), dict(M.get("mixed"))
    rng = np.random.default_rng(900)
    b.update(seed=M._seeds(rng, 3), fir=M.colour(rng, 3, 9), start=np.array([5, 0, 2 ** 33], dtype=np.int64),
             len=np.array([100, 300, 256], dtype=np.int32), env=0.5 + rng.random((3, 4)), n_tones=np.array([1, 2, 0], dtype=np.int32),
             tones=np.array(a["tones"])[[2, 0, 1]], imp=np.array([[0.0, 1.0], [2.0 ** 29, 4.0], [2.0 ** 27, 9.0]]))
    kw = _tables(a)
    out = torch.empty(3, a["K"], dtype=torch.float32, device=DEV)
    eager, eager_st = (t.clone() for t in eng.noise(out=out, info=True, **kw))        # the warm-up call (grows the workspace)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_y, g_st = eng.noise(out=out, info=True, **kw)
    graph.replay()
    assert torch.equal(g_y, eager) and torch.equal(g_st, eager_st)
    new = _tables(b)
    for key in ("seed", "fir", "lengths", "start", "env", "tones", "n_tones", "impulse"):
        kw[key].copy_(new[key])
    graph.replay()
    want, want_st = eng.noise(info=True, **new)
    assert not torch.equal(want, eager) and torch.equal(g_y, want) and torch.equal(g_st, want_st) and not bool(want_st.any())
    kw["fir"][2, 3] = NAN                                          # the replay judges the tables as they are now
    graph.replay()
    assert g_st.tolist() == [0, 0, 1] and not bool(g_y[2].any()) and torch.equal(g_y[:2], want[:2])


# ------------------------------------------------------------------ 11. NoiseBank.synthesize
def _sampler(seed, **kw):
    from cmgan_amd.mixing import NoiseSampler
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return NoiseSampler(generator=gen, **kw)


def test_bank_synthesize_is_engine_noise_on_its_draw(eng):
    from cmgan_amd.mixing import NoiseBank
    items, K, fs = 5, 700, 16000
    kw = dict(p_hum=0.6, p_clicks=0.6, n_taps=63, env_hop_ms=5.0)
    bank = NoiseBank.synthesize(eng, _sampler(3, **kw), items, K / fs, fs)
    d = bank.draw
    assert len(bank) == items and bank.data.dtype == torch.float32 and tuple(bank.data.shape) == (items * K,)
    assert bank.start.tolist() == [k * K for k in range(items)] and bank.length.tolist() == [K] * items
    assert all(torch.equal(p, q) for p, q in zip(d, _sampler(3, **kw).draw(items, K, fs, device=DEV)))
    rows, st = eng.noise(d.seed, d.fir, K, env=d.env, env_hop=80, tones=d.tones, n_tones=d.n_tones, impulse=d.impulse, info=True)
    assert not bool(st.any()) and torch.equal(bank.data.view(items, K), rows)
    rms = rows.double().pow(2).mean(dim=1).sqrt()
    assert bool((rms > 0.2).all()) and bool((rms < 20.0).all())
    # the rows against the model, through the draw
    drawn = M.case(d.seed.cpu().numpy(), K, d.fir.cpu().numpy(), env=d.env.cpu().numpy(), H=80, tones=d.tones.cpu().numpy(),
                   n_tones=d.n_tones.cpu().numpy(), imp=d.impulse.cpu().numpy())
    _accept("bank", rows.cpu().numpy(), drawn)


# ------------------------------------------------------------------ 12. the mixer
def _clean(B, L):
    rng = np.random.default_rng(40)
    return (0.1 * rng.standard_normal((B, L)) * np.sin(np.arange(L) / 50.0)[None, :]).astype(np.float32)


def _mixer(eng, seed, bank, **kw):
    from cmgan_amd.mixing import DynamicMixer
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return DynamicMixer(eng, bank, None, snr_db=(0.0, 15.0), early_ms=None, generator=gen, **kw)


def test_mixer_without_noise_sampler_is_unchanged(eng):
    from cmgan_amd.mixing import NoiseBank
    rng = np.random.default_rng(5)
    nb = NoiseBank.from_arrays([0.02 * rng.standard_normal(5000), 0.01 * rng.standard_normal(1234)], device=DEV)
    clean = torch.from_numpy(_clean(3, 600)).to(DEV)
    a, b = _mixer(eng, 12, nb), _mixer(eng, 12, nb, noise=None)
    default = torch.cuda.get_rng_state(0)
    ta, na, ia = a(clean)
    tb, nb_, ib = b(clean)
    assert torch.equal(ta, tb) and torch.equal(na, nb_) and all(torch.equal(p, q) for p, q in zip(ia, ib))
    assert type(a.last_draw) is type(b.last_draw) and len(a.last_draw) == len(b.last_draw)
    for p, q in zip(a.last_draw, b.last_draw):
        assert (p is None and q is None) or torch.equal(p, q)
    assert torch.equal(a.generator.get_state(), b.generator.get_state()) and torch.equal(torch.cuda.get_rng_state(0), default)
    assert b.last_noise is None and b.noise_bank is nb
    # the model of Engine.mix, fed with the draws: what the batch was before the option existed
    d = a.last_draw
    g = lambda t: t.cpu().numpy()
    rows = mix_model.mix_batch(g(clean), g(nb.data), g(d.noise_start), g(d.noise_len), g(d.noise_off), g(d.snr_db), peak=a.peak)
    for r, row in enumerate(rows):
        want = row["noisy"].astype(np.float32).astype(np.float64)
        assert np.max(np.abs(g(na)[r] - want)) <= 2.0 ** -23 * np.max(np.abs(want))


def test_mixer_synthesizes_its_noise(eng):
    B, L, fs = 4, 900, 16000
    clean = torch.from_numpy(_clean(B, L)).to(DEV)
    kw = dict(p_hum=0.5, p_clicks=0.5, n_taps=63, env_hop_ms=5.0)
    mixer = _mixer(eng, 21, None, noise=_sampler(8, **kw))
    target, noisy, info = mixer(clean)
    assert tuple(noisy.shape) == (B, L) and tuple(target.shape) == (B, L)
    d, drawn, bank = mixer.last_draw, mixer.last_noise, mixer.noise_bank
    assert len(bank) == B and tuple(bank.data.shape) == (B * L,) and bank.start.tolist() == [b * L for b in range(B)]
    # the rows are Engine.noise on the sampler's first draw
    first = _sampler(8, **kw).draw(B, L, fs, device=DEV)
    assert all(torch.equal(p, q) for p, q in zip(drawn, first))
    rows = eng.noise(first.seed, first.fir, L, env=first.env, env_hop=80, tones=first.tones, n_tones=first.n_tones,
                     impulse=first.impulse)
    assert torch.equal(bank.data.view(B, L), rows)
    # the item, offset and SNR draws are those of a mixer over a recorded bank of B items of L samples
    ref = _mixer(eng, 21, bank)
    t_ref, n_ref, _ = ref(clean)
    assert all((p is None and q is None) or torch.equal(p, q) for p, q in zip(d, ref.last_draw))
    assert torch.equal(noisy, n_ref) and torch.equal(target, t_ref)
    # noisy - target of a dry row is the synthesized row, wrapped from its offset and scaled to the drawn SNR
    g = lambda t: t.cpu().numpy()
    model = mix_model.mix_batch(g(clean), g(bank.data), g(d.noise_start), g(d.noise_len), g(d.noise_off), g(d.snr_db), peak=mixer.peak)
    for r, row in enumerate(model):
        want = row["noisy"].astype(np.float32).astype(np.float64)
        assert np.max(np.abs(g(noisy)[r] - want)) <= 2.0 ** -23 * np.max(np.abs(want)), r
        added = g(noisy)[r].astype(np.float64) - g(target)[r].astype(np.float64)
        scaled = row["scale"] * row["g"] * row["noise"]
        assert np.max(np.abs(added - scaled)) <= 2.0 ** -22 * np.max(np.abs(want)), r
        snr = 10.0 * np.log10(row["Ps"] / (row["g"] ** 2 * row["Pn"]))
        assert abs(snr - float(d.snr_db[r])) < 1e-6 and abs(float(info.g[r]) - row["g"]) <= 1e-12 * row["g"]
    # a second call: fresh noise in the same allocation
    before, ptr = bank.data.clone(), bank.data.data_ptr()
    _, noisy2, _ = mixer(clean)
    assert mixer.noise_bank.data.data_ptr() == ptr and not torch.equal(mixer.noise_bank.data, before)
    assert not torch.equal(mixer.last_noise.seed, drawn.seed) and not torch.equal(noisy2, noisy)


def test_mixer_sources_take_the_synthesized_rows(eng):
    B, L = 3, 600
    clean = torch.from_numpy(_clean(B, L)).to(DEV)
    mixer = _mixer(eng, 31, None, noise=_sampler(9, n_taps=9), sources=(1, 2))
    target, noisy, info = mixer(clean)
    assert mixer.source_bank is mixer.noise_bank and tuple(noisy.shape) == (B, L) and bool(torch.isfinite(noisy).all())
    d = mixer.last_draw
    assert type(d).__name__ == "SceneDraw" and bool((d.src_len == L).all()) and bool((d.src_start % L == 0).all())
    ref = _mixer(eng, 31, mixer.noise_bank, sources=(1, 2))
    _, n_ref, _ = ref(clean)
    assert torch.equal(noisy, n_ref)
