"""The gain control on the GPU (cmgan_amd/csrc/dynamics.hip; include/cmgan_hip.h, "Dynamics"): Engine.dynamics against
the float64 model of tests/dynamics_model.py at the kernel's tile, block and fold-chunk edges, a long release over 257
tiles, per-row parameter mixes, lengths with NaN tails and a padded stride, a separate key, in place, the rows that are
copied bit for bit, invalid rows, non-finite samples, peak_reduction_db, bit-reproducibility and independence of B, of the
neighbours and of the padding, hipGraph replay with the table changed in place, and the consumer in DynamicMixer
(dynamics=, dynamics_on=).

Acceptance (dynamics_model's docstring): a sample g is accepted against the model's float64 w when
|g - w| <= ulp32(w) / 2 + E.  E is computed per row from the model alone, 8 x max(|serial64 - serial_ld|, |tiled64 -
serial_ld|); every check prints it and the worst excess.  Every sample of every row is judged.

Measured on an MI355X: the largest E of any case here is 9.2e-14 (the 257-tile row; 1e-14 and less for the others), five to
six orders below a float32 half-ulp at the rows' levels, and the worst |g - w| - ulp32(w) / 2 of any sample is -7.0e-16:
every sample is the correctly rounded one, and no case needed its E."""
import functools

import numpy as np
import pytest
import torch

import dynamics_model as M

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
    T = int(_lib.load().cmgan_dynamics_tile())
    assert T == M.TILE
    return T


_ROWS = {}


def _register(name, x, dyn, key=None):
    """A test row: float32 samples, its table row and its key (None: itself); registered once, shared, read-only."""
    if name not in _ROWS:
        x = np.ascontiguousarray(x, dtype=np.float32)
        dyn = np.ascontiguousarray(dyn, dtype=np.float64)
        key = None if key is None else np.ascontiguousarray(key, dtype=np.float32)
        for a in (x, dyn, key):
            if a is not None:
                a.setflags(write=False)
        _ROWS[name] = (x, dyn, key)
    return name


@functools.lru_cache(maxsize=None)
def _slack(name, n):
    x, dyn, key = _ROWS[name]
    return M.slack(x, key, n, dyn)


def _run(eng, names, lengths=None, pad=0, fill=0.0, inplace=False, keyed=None):
    """The registered rows as one batch (equal buffer lengths) -> float32 [B, L], int32 [B] status, float64 [B] peak reduction
    (numpy).  keyed: None - a key tensor where the rows have one; "wav" - key = wav itself."""
    rows = [_ROWS[k] for k in names]
    B, L = len(rows), len(rows[0][0])
    buf = torch.full((B, L + pad), fill, dtype=torch.float32, device=DEV)
    wav = buf[:, :L]
    wav.copy_(torch.from_numpy(np.stack([r[0] for r in rows])))
    key = None
    if keyed == "wav":
        key = wav
    elif rows[0][2] is not None:
        key = torch.from_numpy(np.stack([r[2] for r in rows])).to(DEV)
    dyn = torch.from_numpy(np.stack([r[1] for r in rows])).to(DEV)
    ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
    y, st, pk = eng.dynamics(wav, dyn, key, ld, out=wav if inplace else None, info=True)
    assert y.dtype == torch.float32 and tuple(y.shape) == (B, L) and st.dtype == torch.int32 and tuple(st.shape) == (B,)
    assert pk.dtype == torch.float64 and tuple(pk.shape) == (B,)
    if inplace:
        assert y.data_ptr() == wav.data_ptr()
    if pad:
        assert bool(torch.isnan(buf[:, L:]).all()) if fill != fill else bool((buf[:, L:] == fill).all())
    return y.cpu().numpy(), st.cpu().numpy(), pk.cpu().numpy()


def _accept(tag, y, names, lengths, pk=None):
    """Every row against the model under the rule (and peak_reduction_db within Ey).  Returns the largest E."""
    top = 0.0
    for b, (name, n) in enumerate(zip(names, lengths)):
        x, dyn, key = _ROWS[name]
        E, Ey = _slack(name, n)
        worst, same = M.excess(y[b, :n], x, key, n, dyn, E)
        print(f"[dynamics] {tag} row {b} {name} (n = {n}): E = {E:.3e}, worst |g - w| - ulp/2 = {worst + E:.3e}")
        assert worst <= 0.0, f"{tag} row {b} {name}: {worst + E:.3e} beyond half an ulp, E = {E:.3e}"
        assert same, f"{tag} row {b} {name}: a non-finite sample of the model is another one on the GPU"
        assert not y[b, n:].any(), f"{tag} row {b} {name}: samples past the row's length are not zero"
        if pk is not None:
            want = float(M.serial(x, key, n, dyn)[1].max(initial=0.0))
            print(f"[dynamics] {tag} row {b} {name}: peak reduction {pk[b]:.6f} dB, model {want:.6f} dB, Ey = {Ey:.3e}")
            assert abs(pk[b] - want) <= Ey, f"{tag} row {b} {name}: peak reduction {pk[b]!r} vs {want!r}, Ey = {Ey:.3e}"
        top = max(top, E)
    return top


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_BASE = M.params(-28.0, 6.0, 6.0, 5.0, 120.0, 2.0)
_SLOW = M.params(-30.0, 8.0, 6.0, 40.0, 10.0, 4.0)                       # attack slower than release: the negated scan


# ------------------------------------------------------------------ 1. tile, block and fold-chunk edges
@pytest.mark.parametrize("n", M.edge_lengths(), ids=lambda n: f"n={n}")
def test_edges(eng, T, n):
    names = [_register(f"edge-{n}", M.bursts(40 + M.edge_lengths().index(n), n), _BASE),
             _register(f"edge-slow-{n}", M.bursts(60 + M.edge_lengths().index(n), n), _SLOW)]
    y, st, pk = _run(eng, names)
    assert st.tolist() == [0, 0]
    _accept(f"n = {n}", y, names, [n, n], pk)


# ------------------------------------------------------------------ 2. a release of 2 s over 257 tiles
def test_long_release_over_257_tiles(eng, T):
    n = 257 * T
    names = [_register("long", M.bursts(9, n), M.params(-26.0, 5.0, 6.0, 5.0, 2000.0, 1.0))]
    y, st, pk = _run(eng, names)
    assert st.tolist() == [0] and pk[0] > 3.0
    _accept("257 tiles", y, names, [n], pk)


# ------------------------------------------------------------------ 3. per-row parameters in one batch
def _mix_names(n=2577):
    return [_register(f"mix-{k}", M.bursts(20 + i, n), dyn) for i, (k, dyn) in enumerate(M.mix_rows().items())]


def test_parameter_mixes_in_one_batch(eng, T):
    names = _mix_names()
    y, st, pk = _run(eng, names)
    assert not st.any()
    _accept("mixes", y, names, [2577] * len(names), pk)
    assert pk[names.index("mix-slope0")] == 0.0 and pk[names.index("mix-limiter")] > 6.0


# ------------------------------------------------------------------ 4. lengths, NaN beyond them, a padded stride
def test_per_row_lengths_with_nan_tails_and_padding(eng, T):
    lengths = M.edge_lengths() + [0]
    L = max(lengths)
    names = []
    for i, n in enumerate(lengths):
        x = M.bursts(80 + i, L)
        x[n:] = NAN                                                      # never read
        names.append(_register(f"len-{n}", x, _BASE if i % 2 else _SLOW))
    y, st, pk = _run(eng, names, lengths=lengths, pad=37, fill=NAN)
    assert not st.any() and pk[-1] == 0.0
    _accept("lengths", y, names, lengths, pk)
    # the bits of a row do not depend on L beyond its length, on the stride or on what lies there
    for b in (3, 6):
        n = lengths[b]
        x, dyn, _ = _ROWS[names[b]]
        alone = _register(f"alone-{n}", x[:n], dyn)
        y1, _, pk1 = _run(eng, [alone])
        assert np.array_equal(_bits(y1[0]), _bits(y[b, :n])) and pk1[0] == pk[b]


# ------------------------------------------------------------------ 5. a separate key, and in place
def test_separate_key_and_in_place(eng, T):
    n = 5 * T + 9
    x, k = M.bursts(100, n), M.bursts(101, n)
    keyed = [_register("keyed-0", x, _BASE, key=k), _register("keyed-1", M.bursts(102, n), _SLOW, key=M.bursts(103, n))]
    y, st, pk = _run(eng, keyed)
    _accept("key", y, keyed, [n, n], pk)
    assert not np.array_equal(y[0], _run(eng, [_register("unkeyed-0", x, _BASE)])[0][0])
    yi, _, pki = _run(eng, keyed, inplace=True, pad=5, fill=7.0)          # out = wav, the key elsewhere
    assert np.array_equal(_bits(yi), _bits(y)) and np.array_equal(pki, pk)
    own = [_register("own-0", x, _BASE), _register("own-1", M.bursts(102, n), _SLOW)]
    y0, _, pk0 = _run(eng, own)
    _accept("own key", y0, own, [n, n], pk0)
    for kw in (dict(inplace=True), dict(inplace=True, keyed="wav"), dict(keyed="wav")):   # out = wav = key
        y1, _, pk1 = _run(eng, own, **kw)
        assert np.array_equal(_bits(y1), _bits(y0)) and np.array_equal(pk1, pk0), kw
    # out = key: the gain that the key drives replaces the key
    wav, key = torch.from_numpy(np.stack([x, x])).to(DEV), torch.from_numpy(np.stack([k, k])).to(DEV)
    dyn = torch.from_numpy(np.stack([_BASE, _BASE])).to(DEV)
    out = eng.dynamics(wav, dyn, key, out=key)
    assert out.data_ptr() == key.data_ptr() and np.array_equal(_bits(out[0].cpu().numpy()), _bits(y[0]))


# ------------------------------------------------------------------ 6. the rows that are copied bit for bit
def test_identity_rows_are_copied_bit_for_bit(eng, T):
    n = 3 * T + 5
    x = M.bursts(110, n)
    x[[0, 7, 100]] = [0.0, -0.0, 1e-42]                                  # signed zeros and a denormal keep their bits
    names = [_register("copy-slope0", x, M.params(-30.0, 1.0, 6.0, 5.0, 100.0)),
             _register("copy-under-knee", x, M.params(10.0, 8.0, 4.0, 5.0, 100.0)),
             _register("copy-under-hard-knee", x, M.params(0.0, INF, 0.0, 0.0, 100.0)),
             _register("copy-slow", x, M.params(10.0, 8.0, 4.0, 100.0, 5.0))]
    for kw in (dict(), dict(inplace=True)):
        y, st, pk = _run(eng, names, **kw)
        assert not st.any() and not pk.any()
        for b in range(len(names)):
            assert np.array_equal(_bits(y[b]), _bits(x)), names[b]


# ------------------------------------------------------------------ 7. invalid rows
def test_invalid_rows_are_zeros_with_status(eng, T):
    n = 2 * T + 3
    good = M.params(-28.0, 6.0, 6.0, 5.0, 120.0, 2.0)
    bad = []
    for col, v in ((0, NAN), (0, INF), (1, -0.01), (1, 1.01), (1, NAN), (2, -1.0), (2, INF), (3, 1.0), (3, -0.1), (4, 1.0), (4, NAN),
                   (5, -INF), (5, NAN)):
        d = good.copy()
        d[col] = v
        bad.append(d)
    tables = [good] + bad + [good]
    names = [_register(f"inv-{i}", M.bursts(120 + i, n), d) for i, d in enumerate(tables)]
    y, st, pk = _run(eng, names, pad=3, fill=5.0)
    assert st.tolist() == [0] + [1] * len(bad) + [0]
    assert not y[1:-1].any() and not pk[1:-1].any()
    _accept("beside invalid rows", y[[0, -1]], [names[0], names[-1]], [n, n], pk[[0, -1]])
    # a length outside [0, L] makes the row invalid too; its neighbours are what they are alone
    lengths = [n, -1, n + 1, n - 1]
    four = names[:1] + [names[0], names[-1], names[-1]]
    y2, st2, pk2 = _run(eng, four, lengths=lengths, inplace=True)
    assert st2.tolist() == [0, 1, 1, 0] and not y2[1:3].any() and not pk2[1:3].any()
    assert np.array_equal(_bits(y2[0]), _bits(y[0]))
    _accept("beside bad lengths", y2[[3]], [names[-1]], [n - 1], pk2[[3]])


# ------------------------------------------------------------------ 8. non-finite samples stay where they are
def test_non_finite_samples_stay_at_their_index(eng, T):
    n = 4 * T + 11
    x, k = M.bursts(130, n), M.bursts(131, n)
    spots = [0, T - 1, T, 2 * T + 5, n - 1]
    bx, bk = x.copy(), k.copy()
    bx[spots] = [NAN, INF, -INF, NAN, INF]
    bk[[3, T, 3 * T]] = [NAN, INF, -INF]
    names = [_register("nf-wav", bx, _BASE), _register("nf-wav-slow", bx, _SLOW), _register("nf-key", x, _BASE, key=bk),
             _register("nf-both", bx, _SLOW, key=bk)]
    y, st, pk = _run(eng, names[:2])
    assert not st.any() and np.isfinite(pk).all()
    _accept("non-finite wav", y, names[:2], [n, n], pk)
    for b in range(2):
        assert np.isnan(y[b, 0]) and y[b, T - 1] == INF and y[b, T] == -INF and np.isfinite(np.delete(y[b], spots)).all()
    y, st, pk = _run(eng, names[2:])
    _accept("non-finite key", y, names[2:], [n, n], pk)
    assert np.isfinite(y[0]).all() and np.isfinite(np.delete(y[1], spots)).all()


# ------------------------------------------------------------------ 9. the same bits whatever surrounds a row
def test_bit_reproducible_and_row_independent(eng, T):
    names = _mix_names()
    y, _, pk = _run(eng, names)
    y2, _, pk2 = _run(eng, names)
    assert np.array_equal(_bits(y), _bits(y2)) and np.array_equal(pk, pk2)
    for b in (0, 4):                                                     # B = 1 against the same row inside the batch
        y1, _, pk1 = _run(eng, [names[b]])
        assert np.array_equal(_bits(y1[0]), _bits(y[b])) and pk1[0] == pk[b]
    order = [4, 7, 0, 2, 0]                                              # other neighbours, another stride, other padding
    y3, _, pk3 = _run(eng, [names[b] for b in order], pad=129, fill=INF)
    for r, b in enumerate(order):
        assert np.array_equal(_bits(y3[r]), _bits(y[b])) and pk3[r] == pk[b]


# ------------------------------------------------------------------ 10. graph replay
def test_captured_call_replays_with_new_input_and_table(eng, T):
    L = 6 * T + 9
    new = [_register("graph-0", M.bursts(150, L), _SLOW), _register("graph-1", M.bursts(151, L), M.mix_rows()["limiter"])]
    wav = torch.from_numpy(np.stack([M.bursts(152 + r, L) for r in range(2)])).to(DEV)
    dyn = torch.from_numpy(np.stack([_BASE, M.mix_rows()["wide_knee"]])).to(DEV)
    lengths = torch.tensor([L, L - 100], dtype=torch.int32, device=DEV)
    eager, eager_st, eager_pk = eng.dynamics(wav, dyn, None, lengths, info=True)   # the warm-up call (grows the workspace)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_y, g_st, g_pk = eng.dynamics(wav, dyn, None, lengths, info=True)
    graph.replay()
    assert torch.equal(g_y, eager) and torch.equal(g_st, eager_st) and torch.equal(g_pk, eager_pk)
    wav.copy_(torch.from_numpy(np.stack([_ROWS[k][0] for k in new])).to(DEV))
    dyn.copy_(torch.from_numpy(np.stack([_ROWS[k][1] for k in new])).to(DEV))
    lengths.copy_(torch.tensor([T + 1, L], dtype=torch.int32, device=DEV))
    graph.replay()
    again, again_st, again_pk = eng.dynamics(wav, dyn, None, lengths, info=True)
    assert not torch.equal(again, eager)
    assert torch.equal(g_y, again) and torch.equal(g_st, again_st) and torch.equal(g_pk, again_pk)
    _accept("replayed", g_y.cpu().numpy(), new, [T + 1, L], g_pk.cpu().numpy())
    dyn[1, 4] = 1.0                                                      # a release coefficient of 1: the replay reports it
    graph.replay()
    assert g_st.tolist() == [0, 1] and not bool(g_y[1].any()) and g_pk[1].item() == 0.0


# ------------------------------------------------------------------ 11 - 14. the mixer
def _speechlike(B, L):
    return np.stack([(0.4 * M.bursts(300 + b, L)).astype(np.float32) for b in range(B)])


def _mixer(eng, seed, **kw):
    from cmgan_amd.mixing import DynamicMixer, NoiseBank
    rng = np.random.default_rng(5)
    nb = NoiseBank.from_arrays([0.02 * rng.standard_normal(5000), 0.01 * rng.standard_normal(1234)], device=DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return DynamicMixer(eng, nb, None, snr_db=(5.0, 15.0), early_ms=None, generator=gen, **kw)


def _sampler(seed, **kw):
    from cmgan_amd.mixing import DynamicsSampler
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return DynamicsSampler(generator=gen, **kw)


def test_mixer_without_dynamics_is_unchanged(eng, T):
    B, L = 3, 2 * T + 17
    clean = torch.from_numpy(_speechlike(B, L)).to(DEV)
    a = _mixer(eng, 12)
    b = _mixer(eng, 12, dynamics=None, dynamics_on="noisy")
    ta, na, ia = a(clean)
    tb, nb_, ib = b(clean)
    assert torch.equal(ta, tb) and torch.equal(na, nb_) and all(torch.equal(p, q) for p, q in zip(ia, ib))
    assert type(a.last_draw) is type(b.last_draw) and len(a.last_draw) == len(b.last_draw)
    for p, q in zip(a.last_draw, b.last_draw):
        assert (p is None and q is None) or torch.equal(p, q)
    assert a.last_draw.dynamics is None and b.last_draw.dynamics is None and b.last_dynamics is None
    assert torch.equal(a.generator.get_state(), b.generator.get_state())


@pytest.mark.parametrize("on", ["noisy", "both"])
def test_mixer_dynamics(eng, T, on):
    from cmgan_amd.mixing import DynamicsSampler
    B, L = 6, 9 * T + 17
    clean = torch.from_numpy(_speechlike(B, L)).to(DEV)
    t0, n0, _ = _mixer(eng, 21)(clean)                                   # what the stage gets: the same draws without it
    mixer = _mixer(eng, 21, dynamics=_sampler(4, p=0.7, makeup=(0.0, 0.0)), dynamics_on=on)   # no make-up: the guard stays out
    t1, n1, _ = mixer(clean)
    d = mixer.last_draw
    table = d.dynamics
    assert table.dtype == torch.float64 and tuple(table.shape) == (B, 6) and type(d).__name__ == "Draw" and len(d) == 10
    assert torch.equal(table, DynamicsSampler.table(_sampler(4, p=0.7, makeup=(0.0, 0.0)).draw(B, 16000, device=DEV), n0))
    pk = mixer.last_dynamics
    assert pk.dtype == torch.float64 and tuple(pk.shape) == (B,)
    chosen = table[:, 1] > 0
    assert 0 < int(chosen.sum()) < B and bool((pk[chosen] > 0).all()) and not bool(pk[~chosen].any())
    tab, n0_, t0_ = table.cpu().numpy(), n0.cpu().numpy(), t0.cpu().numpy()
    names_n = [_register(f"mixer-{on}-noisy-{b}", n0_[b], tab[b]) for b in range(B)]
    _accept(f"mixer {on}: noisy", n1.cpu().numpy(), names_n, [L] * B, pk.cpu().numpy())
    if on == "noisy":
        assert torch.equal(t1, t0)
    else:                                                                # target_out / target_in = noisy_out / noisy_in: the same gain
        names_t = [_register(f"mixer-both-target-{b}", t0_[b], tab[b], key=n0_[b]) for b in range(B)]
        _accept("mixer both: target", t1.cpu().numpy(), names_t, [L] * B)
        assert not torch.equal(t1[chosen], t0[chosen])
    assert torch.equal(n1[~chosen], n0[~chosen]) and torch.equal(t1[~chosen], t0[~chosen])


def test_mixer_peak_guard_after_the_make_up_gain(eng, T):
    from cmgan_amd.mixing import DynamicsSampler
    B, L = 6, 9 * T + 17
    clean = torch.from_numpy(2.0 * _speechlike(B, L)).to(DEV)             # loud: the mix's own guard has set max |noisy| = peak
    t0, n0, _ = _mixer(eng, 22)(clean)
    kw = dict(p=1.0, threshold_rel_db=(-30.0, -20.0), makeup=(1.0, 1.0), attack_ms=(20.0, 30.0))   # slow attack, full make-up: overshoot
    mixer = _mixer(eng, 22, dynamics=_sampler(6, **kw), dynamics_on="both")
    t1, n1, _ = mixer(clean)
    peak = mixer.peak
    top = n1.abs().amax(dim=1).double()
    print(f"[dynamics] guard: max |noisy| per row {top.tolist()}, peak {peak}")
    assert bool((top <= peak * (1.0 + 2.0 ** -22)).all())                # a float32 factor and a float32 product: two roundings
    # the factor is the guard's rule, m > peak ? peak / m : 1, and the same one scales the target
    table = mixer.last_draw.dynamics
    tm = eng.dynamics(t0, table, key=n0)
    nm = eng.dynamics(n0, table)
    m = nm.abs().amax(dim=1)
    s = torch.where(m > peak, peak / m, torch.ones_like(m))[:, None]
    assert int((m > peak).sum()) >= 1
    assert torch.equal(n1, nm * s) and torch.equal(t1, tm * s)
