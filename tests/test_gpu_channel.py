"""The recording channel on the GPU (cmgan_amd/csrc/channel.hip; include/cmgan_hip.h, "Recording channel"):
Engine.channel against the float64 model of tests/channel_model.py (scipy.signal.sosfilt) at the kernel's run, tile and
fold-chunk edges, per-row section counts, lengths with NaN tails, clipping, in place, invalid rows, non-finite samples,
bit-reproducibility and independence of B, of the neighbours and of S, hipGraph replay with the tables changed in place,
and the consumer in DynamicMixer (channel=, channel_on=).

Acceptance (channel_model's docstring): a sample g is accepted against the model's float64 w when
|g - w| <= ulp32(w) / 2 + E, and a sample the model clips by more than E must be f32(+-clip) exactly.  E is computed per
row from the model alone, 8 x max(|filt - filt_ld|, |tiled - filt_ld|); every check prints it and the worst excess.

Measured on an MI355X: the largest E of any case here is 2.1e-10 (the 257-tile rows; 7.1e-11 for the hard S = 8 cascade at
three tiles), over 100 times below a float32 half-ulp at the rows' levels, and the worst |g - w| - ulp32(w) / 2 is 2.2e-11,
a tenth of that row's E: every sample is the correctly rounded one unless w lies that close to a tie."""
import functools

import numpy as np
import pytest
import torch

import channel_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INF = float("inf")
NAN = float("nan")


@pytest.fixture(scope="module")
def eng():
    from cmgan_amd.engine import Engine
    return Engine(device=DEV)


@pytest.fixture(scope="module")
def T():
    from cmgan_amd import _lib
    return int(_lib.load().cmgan_channel_tile())


_ROWS = {}


def _register(key, x, sos):
    """A test row: float32 samples and its own sections [m, 6]; registered once, shared, read-only."""
    if key not in _ROWS:
        x = np.ascontiguousarray(x, dtype=np.float32)
        sos = np.ascontiguousarray(sos, dtype=np.float64).reshape(-1, 6)
        x.setflags(write=False)
        sos.setflags(write=False)
        _ROWS[key] = (x, sos)
    return _ROWS[key]


@functools.lru_cache(maxsize=None)
def _slack(key, n, tile):
    x, sos = _ROWS[key]
    return M.slack(x, n, sos, len(sos), tile)


def _first(fs=M.FS):
    return M.peaking(25.0, 12.0, 4.0, fs)                                # low-frequency, high-Q: its state outlives many tiles


def _run(eng, keys, S, lengths=None, clip=None, pad=0, fill=0.0, inplace=False, m=None, status=True):
    """The registered rows as one batch (equal lengths) -> (float32 [B, L] numpy, int32 [B] status numpy)."""
    rows = [_ROWS[k][0] for k in keys]
    B, L = len(rows), len(rows[0])
    buf = torch.full((B, L + pad), fill, dtype=torch.float32, device=DEV)
    wav = buf[:, :L]
    wav.copy_(torch.from_numpy(np.stack(rows)))
    sos = torch.from_numpy(np.stack([M.padded(_ROWS[k][1], S) for k in keys])).to(DEV)
    nsec = torch.tensor([len(_ROWS[k][1]) for k in keys] if m is None else m, dtype=torch.int32, device=DEV)
    ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
    cl = None if clip is None else torch.tensor(clip, dtype=torch.float64, device=DEV)
    y, st = eng.channel(wav, sos, nsec, cl, ld, out=wav if inplace else None, status=True)
    assert y.dtype == torch.float32 and tuple(y.shape) == (B, L) and st.dtype == torch.int32 and tuple(st.shape) == (B,)
    if inplace:
        assert y.data_ptr() == wav.data_ptr()
        if pad:
            assert bool(torch.isnan(buf[:, L:]).all()) if fill != fill else bool((buf[:, L:] == fill).all())
    return y.cpu().numpy(), st.cpu().numpy()


def _accept(tag, y, keys, lengths, T, clip=None):
    """Every row against the model under the rule.  Returns the largest E."""
    top = 0.0
    for b, (key, n) in enumerate(zip(keys, lengths)):
        x, sos = _ROWS[key]
        E = _slack(key, n, T)
        c = None if clip is None else clip[b]
        worst, exact = M.excess(y[b, :n], x, n, sos, len(sos), c, E)
        print(f"[channel] {tag} row {b} (n = {n}, m = {len(sos)}): E = {E:.3e}, worst |g - w| - ulp/2 = {worst + E:.3e}")
        assert worst <= 0.0, f"{tag} row {b}: {worst + E:.3e} beyond half an ulp, E = {E:.3e}"
        assert exact, f"{tag} row {b}: a clipped sample is not f32(clip)"
        assert not y[b, n:].any(), f"{tag} row {b}: samples past the row's length are not zero"
        top = max(top, E)
    return top


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ 1. run and tile edges
_EDGES = {"1": lambda T, R: 1, "R-1": lambda T, R: R - 1, "R": lambda T, R: R, "R+1": lambda T, R: R + 1,
          "T-1": lambda T, R: T - 1, "T": lambda T, R: T, "T+1": lambda T, R: T + 1, "2T+1": lambda T, R: 2 * T + 1}


@pytest.mark.parametrize("edge", list(_EDGES))
def test_run_and_tile_edges(eng, T, edge):
    R = T // 256
    L = max(_EDGES[edge](T, R), 1)
    keys = [f"edge-{edge}-{r}" for r in range(3)]
    for r, k in enumerate(keys):
        _register(k, M.noise(10 * len(edge) + r, L), np.concatenate([[_first()], M.sampler_like(20 + r, 3)[1:]]))
    y, st = _run(eng, keys, 3, pad=37, fill=NAN)                         # B = 3 with a row stride larger than L, NaN between
    assert not st.any() and np.isfinite(y).all()
    E = _accept(f"L={edge}={L}", y, keys, [L] * 3, T)
    print(f"[channel] L={edge}: largest E {E:.3e}")


# ------------------------------------------------------------------ 2. more tiles than one chunk of the fold
def test_state_carries_across_the_fold_chunk(eng, T):
    L = 257 * T + 5
    keys = ["chunk-0", "chunk-1"]
    for r, k in enumerate(keys):
        _register(k, M.noise(500 + r, L), np.concatenate([[_first()], M.sampler_like(30 + r, 3)[1:]]))
    y, st = _run(eng, keys, 3)
    assert not st.any()
    _accept("257 tiles", y, keys, [L] * 2, T)
    # the state really carries across tile 256: from zero state there, the last samples come out differently
    x, sos = _ROWS[keys[0]]
    fresh = M.filt(x[256 * T:], L - 256 * T, sos, 3)
    assert np.max(np.abs(fresh[-5:] - y[0, -5:])) > 1e-4


# ------------------------------------------------------------------ 3. section counts
def _mixed_rows(L):
    keys = ["count-0", "count-1", "count-5", "count-8"]
    _register(keys[0], M.noise(40, L), np.zeros((0, 6)))
    _register(keys[1], M.noise(41, L), M.sampler_like(41, 1))
    _register(keys[2], M.noise(42, L), np.concatenate([[_first()], M.sampler_like(42, 5)[1:]]))
    _register(keys[3], M.noise(43, L), M.hard_cascade())
    return keys


def test_section_counts_in_one_batch(eng, T):
    L = 3 * T + 17
    keys = _mixed_rows(L)
    y, st = _run(eng, keys, 8, pad=3, fill=NAN)
    assert not st.any()
    E = _accept("m = 0, 1, 5, 8", y, keys, [L] * 4, T)
    assert np.array_equal(_bits(y[0]), _bits(_ROWS[keys[0]][0]))          # m = 0 copies the row
    print(f"[channel] hard S = 8 cascade: E {_slack(keys[3], L, T):.3e}; largest of the batch {E:.3e}")


# ------------------------------------------------------------------ 4. independence of S
def test_bits_do_not_depend_on_the_padding(eng, T):
    L = 2 * T + 9
    keys = [f"pad-{m}" for m in (0, 1, 3, 4)]
    for m, k in zip((0, 1, 3, 4), keys):
        secs = np.concatenate([[_first()], M.sampler_like(50 + m, max(m, 1))[1:]])[:m] if m else np.zeros((0, 6))
        _register(k, M.noise(50 + m, L), secs)
    y4, _ = _run(eng, keys, 4)
    y8, _ = _run(eng, keys, 8)
    _accept("S = 4", y4, keys, [L] * 4, T)
    assert np.array_equal(_bits(y4), _bits(y8))
    y1, _ = _run(eng, keys[:2], 1)
    y2, _ = _run(eng, keys[:2], 2)
    y3, _ = _run(eng, keys[:3], 3)
    y5, _ = _run(eng, keys, 5)
    assert np.array_equal(_bits(y1), _bits(y4[:2])) and np.array_equal(_bits(y2), _bits(y4[:2]))
    assert np.array_equal(_bits(y3), _bits(y4[:3])) and np.array_equal(_bits(y5), _bits(y4))


# ------------------------------------------------------------------ 5. independence of B and of the neighbours
def test_bit_reproducible_and_row_independent(eng, T):
    L = 3 * T + 5
    keys = [f"indep-{r}" for r in range(5)]
    for r, k in enumerate(keys):
        _register(k, M.noise(60 + r, L), np.concatenate([[_first()], M.sampler_like(60 + r, 2 + r)[1:]]))
    a, _ = _run(eng, keys, 8)
    b, _ = _run(eng, keys, 8)
    assert np.array_equal(_bits(a), _bits(b))
    for r, k in enumerate(keys):
        one, _ = _run(eng, [k], 8)
        assert np.array_equal(_bits(one[0]), _bits(a[r])), r
    rev, _ = _run(eng, keys[::-1], 8)
    assert np.array_equal(_bits(rev[::-1]), _bits(a))


# ------------------------------------------------------------------ 6. per-row lengths
def test_per_row_lengths_with_nan_tails(eng, T):
    L = 2 * T + 301
    lengths = [0, 1, T, L]
    keys = [f"len-{r}" for r in range(4)]
    for r, (k, n) in enumerate(zip(keys, lengths)):
        x = M.noise(70 + r, L)
        x[n:] = np.nan                                                   # samples from a row's length on are never read
        _register(k, x, np.concatenate([[_first()], M.sampler_like(70 + r, 3)[1:]]))
    y, st = _run(eng, keys, 3, lengths, pad=3, fill=NAN)
    assert not st.any() and np.isfinite(y).all() and not y[0].any()
    _accept("lengths", y, keys, lengths, T)
    for b, n in enumerate(lengths[1:], start=1):                          # the same row alone, cut to its own length
        _register(f"{keys[b]}-cut", _ROWS[keys[b]][0][:n], _ROWS[keys[b]][1])
        alone, _ = _run(eng, [f"{keys[b]}-cut"], 3)
        assert np.array_equal(_bits(alone[0]), _bits(y[b, :n])), b
    # lengths outside [0, L] are clamped
    z, _ = _run(eng, [keys[3], keys[3]], 3, [-5, L + 1000])
    assert not z[0].any() and np.array_equal(_bits(z[1]), _bits(y[3]))


# ------------------------------------------------------------------ 7. clipping
def test_clipping_is_exact(eng, T):
    L = 2 * T + 33
    keys = [f"clip-{r}" for r in range(4)]
    for r, k in enumerate(keys):
        _register(k, M.noise(80 + r, L), np.concatenate([[_first()], M.sampler_like(80 + r, 3)[1:]]) if r < 3 else np.zeros((0, 6)))
    raw = [M.filt(_ROWS[k][0], L, _ROWS[k][1], len(_ROWS[k][1])) for k in keys]
    level = [float(np.quantile(np.abs(r), 2.0 / 3.0)) for r in raw]
    clip = [INF, level[1], 0.3 * level[2] + 1e-3, level[3]]               # none | a third | most | a plain copy, clipped
    for b in (1, 3):
        frac = float(np.mean(np.abs(raw[b]) > clip[b]))
        assert 0.10 < frac < 0.60, frac                                  # a condition on the INPUT: the level clips about a third
    y, st = _run(eng, keys, 4, clip=clip)
    assert not st.any()
    _accept("clip", y, keys, [L] * 4, T, clip=clip)
    for b in (1, 2, 3):
        hit = np.abs(raw[b]) > clip[b] * (1 + 1e-9)
        assert hit.any() and np.all(np.abs(y[b][hit]) == np.float32(clip[b]))
        assert np.all(np.abs(y[b]) <= np.float32(clip[b]))
    free, _ = _run(eng, keys[:1], 4)
    assert np.array_equal(_bits(free[0]), _bits(y[0]))                   # +inf is no clipping at all


# ------------------------------------------------------------------ 8. in place
def test_in_place(eng, T):
    L = T + 700
    keys = [f"inplace-{r}" for r in range(3)]
    for r, k in enumerate(keys):
        _register(k, M.noise(90 + r, L), np.concatenate([[_first()], M.sampler_like(90 + r, 4)[1:]]))
    lengths, clip = [L, L - 100, T], [INF, 0.2, 0.5]
    a, _ = _run(eng, keys, 4, lengths, clip)
    b, _ = _run(eng, keys, 4, lengths, clip, inplace=True)
    c, _ = _run(eng, keys, 4, lengths, clip, pad=5, fill=NAN, inplace=True)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))
    _accept("in place", b, keys, lengths, T, clip=clip)


# ------------------------------------------------------------------ 9. invalid rows
def test_invalid_rows_are_zeros_with_status(eng, T):
    L = T + 50
    good = np.concatenate([[_first()], M.sampler_like(100, 3)[1:]])
    bad = {}
    s = good.copy(); s[1, 2] = np.nan; bad["nan"] = (s, 3, 1.0)
    s = good.copy(); s[0, 3] = 2.0; bad["a0"] = (s, 3, 1.0)
    s = good.copy(); s[2, 5] = 1.0; bad["a2"] = (s, 3, 1.0)
    s = good.copy(); s[1, 4] = -(1.0 + s[1, 5]); bad["a1"] = (s, 3, 1.0)
    s = good.copy(); s[1, 4] = 1.0 + s[1, 5]; bad["a1+"] = (s, 3, 1.0)
    bad["m"] = (good.copy(), 9, 1.0)
    bad["m-"] = (good.copy(), -1, 1.0)
    bad["clip0"] = (good.copy(), 3, 0.0)
    bad["clip-"] = (good.copy(), 3, -0.5)
    bad["clipnan"] = (good.copy(), 3, NAN)
    bad["inf"] = (np.where(np.arange(18).reshape(3, 6) == 0, np.inf, good), 3, 1.0)
    names = list(bad)
    keys, m, clip, valid = [], [], [], []
    for r in range(len(names) + 1):                                      # valid, invalid, valid, ..., valid
        k = f"inv-ok-{r}"
        _register(k, M.noise(110 + r, L), good)
        keys.append(k); m.append(3); clip.append(0.7); valid.append(True)
        if r < len(names):
            secs, mm, c = bad[names[r]]
            k = f"inv-{names[r]}"
            _register(k, M.noise(130 + r, L), secs)
            keys.append(k); m.append(mm); clip.append(c); valid.append(False)
    valid = np.array(valid)
    y, st = _run(eng, keys, 8, clip=clip, m=m, pad=2, fill=NAN)
    assert st.tolist() == [0 if v else 1 for v in valid], st
    assert not y[~valid].any()
    ok_keys = [k for k, v in zip(keys, valid) if v]
    alone, st2 = _run(eng, ok_keys, 8, clip=[0.7] * len(ok_keys))
    assert not st2.any() and np.array_equal(_bits(alone), _bits(y[valid]))
    _accept("valid rows", y[valid], ok_keys, [L] * len(ok_keys), T, clip=[0.7] * len(ok_keys))
    # what a row does not use is not judged: garbage behind its own sections
    s = M.padded(good, 8); s[5] = np.nan; s[6, 5] = 4.0
    _register("inv-unused", M.noise(110, L), s)
    z, st3 = _run(eng, ["inv-unused"], 8, clip=[0.7], m=[3])
    assert st3.tolist() == [0] and np.array_equal(_bits(z[0]), _bits(y[0]))


# ------------------------------------------------------------------ 10. a non-finite sample
def test_non_finite_sample_spoils_its_row_from_there_on(eng, T):
    L, i = 2 * T + 100, T + 700
    secs = np.concatenate([[_first()], M.sampler_like(140, 3)[1:]])
    base = M.noise(140, L)
    for name, v in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf)):
        x = base.copy()
        x[i] = v
        _register(f"nf-{name}", x, secs)
    _register("nf-a", M.noise(141, L), secs)
    _register("nf-b", M.noise(142, L), secs)
    keys = ["nf-a", "nf-nan", "nf-inf", "nf-b", "nf--inf"]
    y, st = _run(eng, keys, 3)
    assert not st.any()
    clean, _ = _run(eng, ["nf-a", "nf-b"], 3)
    assert np.array_equal(_bits(clean[0]), _bits(y[0])) and np.array_equal(_bits(clean[1]), _bits(y[3]))
    _accept("neighbours", clean, ["nf-a", "nf-b"], [L] * 2, T)
    _register("nf-head", base[:i], secs)
    for b in (1, 2, 4):
        assert not np.isfinite(y[b, i:]).any(), keys[b]                  # from i on: non-finite
        E = _slack("nf-head", i, T)
        w = M.filt(base, i, secs, 3)
        worst = float(np.max(np.abs(y[b, :i].astype(np.float64) - w) - 0.5 * M.ulp32(w) - E))
        print(f"[channel] {keys[b]}: E = {E:.3e}, worst |g - w| - ulp/2 before the sample = {worst + E:.3e}")
        assert worst <= 0.0


# ------------------------------------------------------------------ 11. graph replay
def test_captured_call_replays_with_new_input_and_sections(eng, T):
    L = 2 * T + 9
    new_keys = ["graph-0", "graph-1"]
    _register(new_keys[0], M.noise(150, L), np.concatenate([[_first()], M.sampler_like(150, 4)[1:]]))
    _register(new_keys[1], M.noise(151, L), M.sampler_like(151, 2))
    wav = torch.from_numpy(np.stack([M.noise(152 + r, L) for r in range(2)])).to(DEV)
    sos = torch.from_numpy(np.stack([M.padded(M.sampler_like(153 + r, 3), 4) for r in range(2)])).to(DEV)
    nsec = torch.tensor([3, 3], dtype=torch.int32, device=DEV)
    clip = torch.tensor([INF, 0.4], dtype=torch.float64, device=DEV)
    lengths = torch.tensor([L, L - 100], dtype=torch.int32, device=DEV)
    eager, eager_st = eng.channel(wav, sos, nsec, clip, lengths, status=True)      # the warm-up call (grows the workspace)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_y, g_st = eng.channel(wav, sos, nsec, clip, lengths, status=True)
    graph.replay()
    assert torch.equal(g_y, eager) and torch.equal(g_st, eager_st)
    wav.copy_(torch.from_numpy(np.stack([_ROWS[k][0] for k in new_keys])).to(DEV))
    sos.copy_(torch.from_numpy(np.stack([M.padded(_ROWS[k][1], 4) for k in new_keys])).to(DEV))
    nsec.copy_(torch.tensor([4, 2], dtype=torch.int32, device=DEV))
    clip.copy_(torch.tensor([0.5, INF], dtype=torch.float64, device=DEV))
    lengths.copy_(torch.tensor([T + 1, L], dtype=torch.int32, device=DEV))
    graph.replay()
    again, again_st = eng.channel(wav, sos, nsec, clip, lengths, status=True)
    assert not torch.equal(again, eager)
    assert torch.equal(g_y, again) and torch.equal(g_st, again_st)
    _accept("replayed", g_y.cpu().numpy(), new_keys, [T + 1, L], T, clip=[0.5, INF])
    sos[1, 0, 5] = 1.5                                                   # an unstable row: the replay reports it
    graph.replay()
    assert g_st.tolist() == [0, 1] and not bool(g_y[1].any())


# ------------------------------------------------------------------ 12 - 14. the mixer
def _speechlike(B, L):
    t = np.arange(L) / M.FS
    return np.stack([(M.noise(300 + b, L, 0.1) * (0.6 + 0.4 * np.sin(2 * np.pi * (2.0 + b) * t))).astype(np.float32)
                     for b in range(B)])


def _mixer(eng, seed, **kw):
    from cmgan_amd.mixing import DynamicMixer, NoiseBank
    rng = np.random.default_rng(5)
    nb = NoiseBank.from_arrays([0.1 * rng.standard_normal(5000), 0.05 * rng.standard_normal(1234)], device=DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return DynamicMixer(eng, nb, None, snr_db=(0.0, 15.0), early_ms=None, generator=gen, **kw)


def _sampler(seed, **kw):
    from cmgan_amd.mixing import ChannelSampler
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return ChannelSampler(generator=gen, **kw)


def test_mixer_without_a_channel_is_unchanged(eng, T):
    B, L = 3, 2 * T + 17
    clean = torch.from_numpy(_speechlike(B, L)).to(DEV)
    a = _mixer(eng, 12)
    b = _mixer(eng, 12, channel=None, channel_on="noisy")
    ta, na, ia = a(clean)
    tb, nb_, ib = b(clean)
    assert torch.equal(ta, tb) and torch.equal(na, nb_) and all(torch.equal(p, q) for p, q in zip(ia, ib))
    assert len(a.last_draw) == len(b.last_draw)
    for p, q in zip(a.last_draw, b.last_draw):
        assert (p is None and q is None) or torch.equal(p, q)
    assert a.last_draw.channel is None and b.last_draw.channel is None
    assert torch.equal(a.generator.get_state(), b.generator.get_state())


def test_mixer_channel_on_noisy(eng, T):
    from cmgan_amd.mixing import DynamicMixer
    B, L = 6, 2 * T + 17
    clean = torch.from_numpy(_speechlike(B, L)).to(DEV)
    plain = _mixer(eng, 21)
    t0, n0, i0 = plain(clean)
    mixer = _mixer(eng, 21, channel=_sampler(3, p_highpass=0.7, p_bandlimit=0.5, p_clip=0.6))
    t1, n1, i1 = mixer(clean)
    sos, nsec, shared, rel = mixer.last_draw.channel
    assert tuple(sos.shape) == (B, 8, 6) and sos.device.type == "cuda" and torch.equal(nsec, shared)
    for p, q in zip(plain.last_draw[:8], mixer.last_draw[:8]):
        assert (p is None and q is None) or torch.equal(p, q)
    clip = rel * n0.abs().amax(dim=1).double()
    assert bool(torch.isfinite(rel).any()) and bool(torch.isinf(rel).any()) and int(nsec.max()) >= 3
    assert torch.equal(torch.where(torch.isfinite(rel), clip, torch.full_like(clip, INF)), DynamicMixer.channel_clip(rel, n0))
    want, st = eng.channel(n0, sos, nsec, DynamicMixer.channel_clip(rel, n0), status=True)
    assert not bool(st.any())
    assert torch.equal(n1, want) and not torch.equal(n1, n0)
    assert torch.equal(t1, t0) and all(torch.equal(p, q) for p, q in zip(i0, i1))         # the target is untouched
    on = torch.isfinite(rel)
    assert bool((n1[on].abs().amax(dim=1) <= clip[on].float()).all())
    # against the model, for the row with the most sections
    b = int(torch.argmax(nsec))
    m = int(nsec[b])
    _register("mixer-row", n0[b].cpu().numpy(), sos[b, :m].cpu().numpy())
    _accept("mixer", n1[b:b + 1].cpu().numpy(), ["mixer-row"], [L], T, clip=[float(DynamicMixer.channel_clip(rel, n0)[b])])


def test_mixer_channel_on_both(eng, T):
    B, L = 4, T + 99
    clean = torch.from_numpy(_speechlike(B, L)).to(DEV)
    plain = _mixer(eng, 22)
    t0, n0, _ = plain(clean)
    noisy_only = _mixer(eng, 22, channel=_sampler(4, p_highpass=1.0, p_clip=1.0))
    t1, n1, _ = noisy_only(clean)
    both = _mixer(eng, 22, channel=_sampler(4, p_highpass=1.0, p_clip=1.0), channel_on="both")
    t2, n2, _ = both(clean)
    sos, nsec, shared, rel = both.last_draw.channel
    assert all(torch.equal(p, q) for p, q in zip(both.last_draw.channel, noisy_only.last_draw.channel))
    assert torch.equal(n2, n1) and torch.equal(t1, t0)
    want = eng.channel(t0, sos, shared)                                  # the sections only: no clipping
    assert torch.equal(t2, want) and not torch.equal(t2, t0)
    assert bool((t2.abs().amax(dim=1) > 0).all())
