"""Speed perturbation on the GPU (cmgan_amd/csrc/warp.hip; include/cmgan_hip.h, "Speed perturbation"): Engine.warp
against the numpy model of tests/warp_model.py at the kernel's tile edges, on rows shorter than the filter, at every rate
and filter in one batch, on a row longer than 2^16, per-row lengths with NaN tails, invalid rows, non-finite samples,
bit-reproducibility and independence of B, of the neighbours, of the padding and of L, hipGraph replay with the input,
the rates and the lengths changed in place, and the consumer in DynamicMixer (speed=, p_speed=).

Acceptance (warp_model's docstring): a sample g is accepted against the model's long-double w when
|g - w| <= ulp32(w) / 2 + E.  E is computed per row from the model alone, 8 x max(|direct - w|, |as_kernel - w|); every
row used is registered in warp_model.build_rows, where the host test checks E <= 2^-10 x ulp32(rms) / 2 without a GPU;
every check prints E and the worst excess.

Measured on an MI355X: the largest E of any row here is 3.2e-14 (zeros = 64, rolloff = 1, r = 4; 1.0e-14 - 1.9e-14 at the
default filter), at most 0.5 % of the bound above, and the worst |g - w| - ulp32(w) / 2 over all rows is -3.8e-14 (zeros =
4, rolloff = 0.5): no sample lies further than half an ulp from w, so E was not needed - every one of the 41 427 samples
judged is the correctly rounded float32 of the long-double value."""
import numpy as np
import pytest
import torch

import warp_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def eng():
    from cmgan_amd.engine import Engine
    return Engine(device=DEV)


@pytest.fixture(scope="module")
def T():
    from cmgan_amd import _lib
    T = int(_lib.load().cmgan_warp_tile())
    M.build_rows(T)
    return T


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(eng, keys, N=None, zeros=None, rolloff=None, L=None, lengths=True, rates=None, pad=0, extra=None):
    """The registered rows as one batch -> (float32 [B, N], out_len [B], status [B]) as numpy.  The buffer is L (default:
    the longest row) + `pad` wide and NaN wherever a row has no sample; `extra` = (x, n, r) rows that are not registered
    are appended as they are."""
    rows = [M.ROWS[k] for k in keys]
    specs = [(r.x, r.n, r.r) for r in rows] + list(extra or [])
    N = rows[0].N if N is None else N
    zeros = rows[0].zeros if zeros is None else zeros
    rolloff = rows[0].rolloff if rolloff is None else rolloff
    assert all(r.N == N and r.zeros == zeros and r.rolloff == rolloff for r in rows)
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
    y, n_out, st = eng.warp(wav, rate, N, ld, zeros, rolloff, out=ybuf[:, :N], info=True)
    assert y.dtype == torch.float32 and tuple(y.shape) == (B, N) and y.data_ptr() == ybuf.data_ptr()
    assert n_out.dtype == torch.int32 and tuple(n_out.shape) == (B,) and st.dtype == torch.int32 and tuple(st.shape) == (B,)
    if pad:
        assert bool(torch.isnan(ybuf[:, N:]).all()), "the padding behind y was written"
    return y.cpu().numpy(), n_out.cpu().numpy(), st.cpu().numpy()


def _accept(tag, y, n_out, st, keys):
    """Every registered row of the batch against the model under the rule.  Returns (largest E, worst |g - w| - ulp / 2)."""
    top, worst_over = 0.0, -np.inf
    for b, key in enumerate(keys):
        row = M.ROWS[key]
        E, w, ns = M.case(key)
        Mb = min(M.count(row.n, row.r), y.shape[1])
        assert st[b] == 0 and n_out[b] == Mb, f"{tag} {key}: status {st[b]}, out_len {n_out[b]} for {Mb}"
        assert not y[b, Mb:].any(), f"{tag} {key}: outputs from out_len on are not zero"
        worst = M.excess(y[b, ns], w, E)
        print(f"[warp] {tag} {key} (n = {row.n}, r = {row.r}, {len(ns)} outputs): E = {E:.3e}, "
              f"worst |g - w| - ulp/2 = {worst + E:.3e}")
        assert worst <= 0.0, f"{tag} {key}: {worst + E:.3e} beyond half an ulp, E = {E:.3e}"
        top, worst_over = max(top, E), max(worst_over, worst + E)
    return top, worst_over


# ------------------------------------------------------------------ 1. tile and support edges
@pytest.mark.parametrize("edge", ["1", "T-1", "T", "T+1", "2T+1"])
def test_tile_edges(eng, T, edge):
    """N outputs asked for, from rows that give exactly N (M = N) and exactly N - 1 (M = N - 1, one zero at the end)."""
    N = dict(zip(["1", "T-1", "T", "T+1", "2T+1"], M.edge_cases(T)))[edge]
    keys = [f"edge-{N}-{r}-{kind}" for r in M.EDGE_RATES for kind in ("full", "short")]
    keys = [k for k in keys if k in M.ROWS]                              # (N = 1: the short row has no sample at all)
    y, n_out, st = _run(eng, keys, pad=5)
    _accept(f"N={edge}", y, n_out, st, keys)
    want = [N if k.endswith("full") else N - 1 for k in keys]
    assert n_out.tolist() == want


def test_rows_shorter_than_the_filter(eng, T):
    """n = 1, 2 and 2W - 1: the filter is cut at both ends of the row.  n = 0: out_len 0 and zeros."""
    for r in (1.1, 0.8):
        W = M.geometry(r, 24, 0.95)[1]
        for n in (1, 2, int(2 * W) - 1):
            key = f"short-{r}-{n}"
            y, n_out, st = _run(eng, [key], pad=3, extra=[(np.zeros(0, dtype=np.float32), 0, r)])
            _accept("short", y, n_out, st, [key])
            assert n_out[1] == 0 and st[1] == 0 and not y[1].any()


# ------------------------------------------------------------------ 2. the rates in one batch, for every filter
@pytest.mark.parametrize("rolloff", [0.5, 0.95, 1.0])
@pytest.mark.parametrize("zeros", [4, 24, 64])
def test_rates_in_one_batch(eng, T, zeros, rolloff):
    keys = [f"rates-{zeros}-{rolloff}-{i}" for i in range(len(M.RATES))]
    y, n_out, st = _run(eng, keys, lengths=False, pad=1)
    E, over = _accept(f"zeros={zeros} rolloff={rolloff}", y, n_out, st, keys)
    print(f"[warp] zeros={zeros} rolloff={rolloff}: largest E {E:.3e}, worst excess over half an ulp {over:.3e}")
    assert n_out.tolist() == [M.count(300, r) for r in M.RATES]
    if rolloff == 1.0:                                                   # r = 1 at the full band: a copy, bit for bit
        assert M.RATES[0] == 1.0 and np.array_equal(_bits(y[0, :300]), _bits(M.ROWS[keys[0]].x))
    else:
        assert not np.array_equal(_bits(y[0, :300]), _bits(M.ROWS[keys[0]].x))


# ------------------------------------------------------------------ 3. a long row
def test_long_row(eng, T):
    """L = 70 000 (past 2^16) at the rate of a clock drift: the last tile is accepted as the first is."""
    row = M.ROWS["long"]
    assert row.n == 70000 and row.N == M.count(70000, 1.0001) > 65536
    y, n_out, st = _run(eng, ["long"], lengths=False)
    _accept("long", y, n_out, st, ["long"])
    assert n_out[0] == row.N and np.isfinite(y).all()
    ns = M.case("long")[2]
    assert ns[0] == 0 and ns[-1] == row.N - 1 and len(ns) > T


# ------------------------------------------------------------------ 4. bits
def test_bits_depend_on_the_row_alone(eng, T):
    keys = [f"bits-{i}" for i in range(5)]
    a, n_a, st_a = _run(eng, keys, pad=7)                                # NaN tails behind every length, NaN padding
    _accept("bits", a, n_a, st_a, keys)
    b, n_b, _ = _run(eng, keys, pad=7)                                   # a second call
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(n_a, n_b)
    c, _, _ = _run(eng, keys)                                            # other row strides
    assert np.array_equal(_bits(a), _bits(c))
    d, _, _ = _run(eng, keys, L=1500, pad=1)                             # a longer buffer: L beyond the lengths
    assert np.array_equal(_bits(a), _bits(d))
    rev, n_rev, _ = _run(eng, keys[::-1])                                # other neighbours
    assert np.array_equal(_bits(rev[::-1]), _bits(a)) and np.array_equal(n_rev[::-1], n_a)
    for i, k in enumerate(keys):                                         # alone, in a buffer cut to its own length
        one, n_one, _ = _run(eng, [k], lengths=False)
        assert np.array_equal(_bits(one[0]), _bits(a[i])) and n_one[0] == n_a[i], k
    # a neighbour's rate does not matter either
    other, _, _ = _run(eng, keys, rates=[M.ROWS[keys[0]].r, 3.3, 0.27, NAN, M.ROWS[keys[4]].r])
    assert np.array_equal(_bits(other[0]), _bits(a[0])) and np.array_equal(_bits(other[4]), _bits(a[4]))


# ------------------------------------------------------------------ 5. invalid rows
def test_invalid_rows_are_zeros_with_status(eng, T):
    L, N = 400, 500
    bad_rates = [NAN, float("inf"), 0.0, -1.0, float(np.nextafter(4.0, 5.0)), float(np.nextafter(0.25, 0.0))]
    ok = [f"inv-ok-{i}" for i in range(M.INVALID_NEIGHBOURS)]
    x = M.noise(99, L)
    specs, valid, order = [], [], []
    bad = [(x, L, r) for r in bad_rates] + [(x, -1, 1.0), (x, L + 1, 1.0)]
    for i in range(M.INVALID_NEIGHBOURS):                                # valid, invalid, valid, ..., valid
        order.append(ok[i])
        if i < len(bad):
            order.append(bad[i])
    rows = [(M.ROWS[e].x, M.ROWS[e].n, M.ROWS[e].r) if isinstance(e, str) else e for e in order]
    valid = np.array([isinstance(e, str) for e in order])
    buf = torch.from_numpy(np.stack([r[0] for r in rows])).to(DEV)
    lengths = torch.tensor([r[1] for r in rows], dtype=torch.int32, device=DEV)
    rate = torch.tensor([r[2] for r in rows], dtype=torch.float64, device=DEV)
    y, n_out, st = (t.cpu().numpy() for t in eng.warp(buf, rate, N, lengths, info=True))
    assert st.tolist() == [0 if v else 1 for v in valid], st
    assert not y[~valid].any() and not n_out[~valid].any()
    _accept("valid rows", y[valid], n_out[valid], st[valid], ok)
    alone, _, _ = _run(eng, ok, lengths=False)
    assert np.array_equal(_bits(alone), _bits(y[valid]))
    # the ends of the range themselves are valid
    edge, n_edge, st_edge = (t.cpu().numpy() for t in eng.warp(
        buf[:2], torch.tensor([0.25, 4.0], dtype=torch.float64, device=DEV), N, info=True))
    assert st_edge.tolist() == [0, 0] and n_edge.tolist() == [N, 100] and edge[0].any() and edge[1, :100].any()


# ------------------------------------------------------------------ 6. non-finite samples
def test_a_non_finite_sample_spoils_the_outputs_that_hold_it(eng, T):
    keys = ["nf-a", "nf-nan", "nf-inf", "nf-b", "nf--inf"]
    y, n_out, st = _run(eng, keys, lengths=False)
    _accept("non-finite", y, n_out, st, keys)                            # the bad rows: on the outputs that do not hold it
    for b in (1, 2, 4):
        row = M.ROWS[keys[b]]
        hold = M.holders(row.n, row.r, row.zeros, row.rolloff, M.NONFINITE_AT, row.N)
        Mb = len(hold)
        assert 20 < int(hold.sum()) < 80
        assert not np.isfinite(y[b, :Mb][hold]).any() and np.isfinite(y[b, :Mb][~hold]).all(), keys[b]
    clean, _, _ = _run(eng, ["nf-a", "nf-b"], lengths=False)
    assert np.array_equal(_bits(clean[0]), _bits(y[0])) and np.array_equal(_bits(clean[1]), _bits(y[3]))


# ------------------------------------------------------------------ 7. graph replay
def test_captured_call_replays_with_new_input_rates_and_lengths(eng, T):
    keys = ["graph-0", "graph-1"]
    L, N = 600, 640
    wav = torch.from_numpy(np.stack([M.noise(7100 + b, L) for b in range(2)])).to(DEV)
    rate = torch.tensor([1.2, 0.85], dtype=torch.float64, device=DEV)
    lengths = torch.tensor([L, L - 50], dtype=torch.int32, device=DEV)
    eager = eng.warp(wav, rate, N, lengths, info=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = eng.warp(wav, rate, N, lengths, info=True)
    graph.replay()
    assert all(torch.equal(p, q) for p, q in zip(got, eager))
    new = np.full((2, L), NAN, dtype=np.float32)
    for b, k in enumerate(keys):
        new[b, :M.ROWS[k].n] = M.ROWS[k].x
    wav.copy_(torch.from_numpy(new).to(DEV))
    rate.copy_(torch.tensor([M.ROWS[k].r for k in keys], dtype=torch.float64, device=DEV))
    lengths.copy_(torch.tensor([M.ROWS[k].n for k in keys], dtype=torch.int32, device=DEV))
    graph.replay()
    again = eng.warp(wav, rate, N, lengths, info=True)
    assert not torch.equal(again[0], eager[0])
    assert all(torch.equal(p, q) for p, q in zip(got, again))
    _accept("replayed", *(t.cpu().numpy() for t in got), keys)
    rate[1] = 5.0                                                        # an invalid row: the replay reports it
    graph.replay()
    assert got[2].tolist() == [0, 1] and got[1].tolist()[1] == 0 and not bool(got[0][1].any())


# ------------------------------------------------------------------ 8, 9. the mixer
def _speechlike(B, L):
    t = np.arange(L) / 16000.0
    return np.stack([(M.noise(300 + b, L, 0.1) * (0.6 + 0.4 * np.sin(2 * np.pi * (2.0 + b) * t))).astype(np.float32)
                     for b in range(B)])


def _mixer(eng, seed, **kw):
    from cmgan_amd.mixing import DynamicMixer, NoiseBank
    rng = np.random.default_rng(5)
    nb = NoiseBank.from_arrays([0.1 * rng.standard_normal(5000), 0.05 * rng.standard_normal(1234)], device=DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return DynamicMixer(eng, nb, None, snr_db=(0.0, 15.0), early_ms=None, generator=gen, level_db=(-30.0, -20.0), **kw)


def test_mixer_without_speed_is_unchanged(eng, T):
    B, L = 3, 2 * T + 17
    clean = torch.from_numpy(_speechlike(B, L)).to(DEV)
    a = _mixer(eng, 12)
    b = _mixer(eng, 12, speed=None, p_speed=0.3)
    ta, na, ia = a(clean)
    tb, nb_, ib = b(clean)
    assert tuple(ta.shape) == (B, L)
    assert torch.equal(ta, tb) and torch.equal(na, nb_) and all(torch.equal(p, q) for p, q in zip(ia, ib))
    assert len(a.last_draw) == len(b.last_draw)
    for p, q in zip(a.last_draw, b.last_draw):
        assert (p is None and q is None) or torch.equal(p, q)
    assert a.last_draw.speed is None and b.last_draw.speed is None
    assert torch.equal(a.generator.get_state(), b.generator.get_state())


def test_mixer_with_speed(eng, T):
    """Every row goes through Engine.warp with the mixer's zeros / rolloff, the rows drawn as exactly 1.0 too: they are
    filtered (band-limited at the rolloff), not copied."""
    from cmgan_amd.mixing import warp_len
    B, L = 16, 2 * T + 117
    clean = torch.from_numpy(_speechlike(B, L)).to(DEV)
    plain = _mixer(eng, 31)
    plain(clean)
    mixer = _mixer(eng, 31, speed=(0.9, 1.1), p_speed=0.5)
    target, noisy, info = mixer(clean)
    N = warp_len(L, 1.1)
    assert N == M.count(L, 1.1) < L and tuple(target.shape) == (B, N) and tuple(noisy.shape) == (B, N)
    d = mixer.last_draw
    for p, q in zip(plain.last_draw[:-1], d[:-1]):                       # the other draws are what they were
        assert (p is None and q is None) or torch.equal(p, q)
    s = d.speed
    assert s.dtype == torch.float64 and tuple(s.shape) == (B,) and bool(((s >= 0.9) & (s <= 1.1)).all())
    ones = s == 1.0
    assert 0 < int(ones.sum()) < B
    warped, n_out, st = eng.warp(clean, s, N, info=True)
    assert not bool(st.any()) and n_out.tolist() == [N] * B              # every row is full
    assert not torch.equal(warped[ones], clean[ones][:, :N])             # filtered, not copied
    lv = eng.speech_level(warped, fs=16000)
    scaled = (warped * mixer.level_gain(lv, d.level_db)[:, None]).contiguous()
    noisy2, target2, _ = eng.mix(scaled, mixer.noise_bank.data, d.noise_start, d.noise_len, d.noise_off, d.snr_db,
                                 None, None, None, peak=mixer.peak, early=-1)
    assert torch.equal(target, target2) and torch.equal(noisy, noisy2)
    assert bool(torch.isfinite(noisy).all()) and bool((target.abs().amax(dim=1) > 0).all())


def test_mixing_loader_clamps_the_lengths(eng, T):
    from cmgan_amd.mixing import MixingLoader, warp_len
    B, L = 4, T + 44
    clips = torch.from_numpy(_speechlike(B, L))
    loader = [(clips, torch.tensor([L, L - 10, 50, 5 * L]))]
    mixer = _mixer(eng, 5, speed=(0.95, 1.05))
    target, noisy, length = next(iter(MixingLoader(loader, mixer)))
    N = warp_len(L, 1.05)
    assert tuple(noisy.shape) == (B, N) and tuple(target.shape) == (B, N) and length.tolist() == [N, N, 50, N]
