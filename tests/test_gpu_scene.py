"""Scenes on the GPU (cmgan_amd/csrc/scene.hip; include/cmgan_hip.h, "Scenes"): Engine.scene against the long-double model
of tests/scene_model.py under the rule |g - w| <= ulp32(w) / 2 + E on every registered row (tile, chunk and wrap edges,
mixed source counts, bad table entries), the bits of Engine.mix without sources, row independence and reproducibility,
the peak guard, hipGraph replay with rewritten tables, and the front end (DynamicMixer(sources=...), draw_sources)."""
import numpy as np
import pytest
import torch

import scene_model as M
from mixer_cases import assert_recorded_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U32 = 2.0 ** -24
T0 = M.TPB * M.OPT
JUDGED = [f"tile-{L}" for L in M.tile_lengths(T0)] + ["chunk", "bad", "peak", "located", "bits"]
TABLES = ("noise_start", "noise_len", "noise_off", "snr_db", "n_src", "src_start", "src_len", "src_off", "src_snr_db",
          "rir_index", "rir_len", "src_rir_index", "src_rir_len")


@pytest.fixture(scope="module")
def eng():
    from cmgan_amd.engine import Engine
    return Engine(device=DEV)


@pytest.fixture(scope="module")
def batches():
    from cmgan_amd.mixing import tile
    assert tile() == T0
    return M.build_batches(tile())


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the registered arrays are read-only)


def _rows(bt, rows):
    """The batch cut to some of its rows (the banks stay whole, so every index stays valid)."""
    rows = list(rows)
    cut = {k: getattr(bt, k)[rows] for k in ("clean",) + TABLES if getattr(bt, k) is not None}
    return bt._replace(**cut)


def _dev(bt):
    """The arguments of Engine.scene for a batch, on the device, in call order."""
    return [_t(getattr(bt, k)) for k in ("clean", "noise_bank", "noise_start", "noise_len", "noise_off", "snr_db", "n_src",
                                          "src_bank", "src_start", "src_len", "src_off", "src_snr_db", "rir", "rir_index",
                                          "rir_len", "src_rir_index", "src_rir_len")]


def _np(out):
    noisy, target, info = out
    return noisy.cpu().numpy(), target.cpu().numpy(), [v.cpu().numpy() for v in info]


def _scene(eng, bt):
    return _np(eng.scene(*_dev(bt), peak=bt.peak, early=bt.early))


def _same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               for x, y in zip([a[0], a[1], *a[2]], [b[0], b[1], *b[2]]))


def _judge(tag, name, got, rows=None):
    """Every row of `got` under the rule against the registered batch `name` (rows: which of its rows `got` holds).
    Returns (worst excess, worst error in units of ulp32 / 2)."""
    noisy, target, (g, scale, ps, p) = got
    bt = M.BATCHES[name]
    rows = range(len(bt.clean)) if rows is None else rows
    worst, units = -np.inf, 0.0
    for k, b in enumerate(rows):
        sl, ld = M.case(name, b)
        for key, a in (("noisy", noisy[k]), ("target", target[k])):
            E, w = sl[key]
            x = M.excess(a, w, E)
            assert x <= 0.0, f"{tag} row {b} {key}: worst |g - w| - ulp32 / 2 - E = {x:.3e} (E = {E:.3e})"
            worst = max(worst, x)
            units = max(units, float(np.max(np.abs(a.astype(M.LD) - w).astype(np.float64) / (0.5 * M.ulp32(w.astype(np.float64))))))
        sb = len(ld["g"]) - 1
        for j in range(g.shape[1]):
            wg, wp = (float(ld["g"][j]), float(ld["P"][j])) if j <= sb else (0.0, 0.0)
            assert abs(g[k, j] - wg) <= 1e-12 * wg and abs(p[k, j] - wp) <= 1e-12 * wp, f"{tag} row {b} source {j}: g {g[k, j]!r} / {wg!r}, P {p[k, j]!r} / {wp!r}"
        assert abs(ps[k] - float(ld["Ps"])) <= 1e-12 * float(ld["Ps"]) and abs(scale[k] - float(ld["scale"])) <= 1e-12
    return worst, units


# ------------------------------------------------------------------ 1. the kernels against the model
@pytest.mark.parametrize("name", JUDGED)
def test_kernel_meets_the_rule_on_every_registered_row(eng, batches, name):
    """|g - w| <= ulp32(w) / 2 + E for noisy and target of every row, w the long-double model, E from the model alone
    (tests/test_scene_host.py holds E to 2^-10 of half an ulp of the row's rms); gains and powers to 1e-12."""
    got = _scene(eng, batches[name])
    assert all(np.all(np.isfinite(v)) for v in (got[0], got[1], *got[2]))
    worst, units = _judge(name, name, got)
    print(f"[scene] {name}: worst excess {worst:.3e}, worst error {units:.6f} half-ulps")


def test_invalid_entries_and_absent_noise_have_exact_zeros(eng, batches):
    bad = _scene(eng, batches["bad"])
    g, p = bad[2][0], bad[2][3]
    assert np.all(g[0, 1:4] == 0.0) and np.all(p[0, 1:4] == 0.0) and g[0, 4] > 0.0          # three silent segments, one good
    assert np.all(g[3, 1:] == 0.0) and np.all(p[3, 1:] == 0.0)                              # n_src = -2: none
    assert g[1, 0] == 0.0 and p[1, 0] == 0.0 and g[2, 0] == 0.0                             # the dry noise's bad segments
    assert np.all(g[2, 1:4] > 0.0)                                                          # n_src = 9: four, one of them silent
    loc = _scene(eng, batches["located"])
    assert np.all(loc[2][0][:, 0] == 0.0) and np.all(loc[2][3][:, 0] == 0.0)                # no dry noise at all
    assert np.array_equal(loc[1].view(np.uint32), batches["located"].clean.view(np.uint32)) or np.any(loc[2][1] != 1.0)


# ------------------------------------------------------------------ 2. without sources: Engine.mix
@pytest.fixture(scope="module")
def parent_bits():
    """Engine.mix's bits at the commit before cmgan_mix became the S = 0 case of cmgan_scene (tests/golden/make_mix_bits.py)."""
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mix_parent_bits.npz"))


@pytest.mark.parametrize("name", [f"tile-{T0 - 1}", f"tile-{2 * T0 + T0 // 2 + 7}", "chunk", "peak"])
def test_without_sources_the_bits_are_engine_mix(eng, batches, parent_bits, name):
    """Engine.mix and both source-free forms of Engine.scene give each other's bits - which one code path would do by
    construction - and the bits Engine.mix had when it was a separate implementation, recorded outside this tree's code."""
    bt = batches[name]
    for early in (-1, 20):
        for rir in (True, False):
            a = _dev(bt)
            if not rir:
                a[12] = a[13] = a[14] = a[15] = a[16] = None
            case = f"{name}/early{early}/{'rir' if rir else 'dry'}"
            n1, t1, i1 = eng.mix(a[0], a[1], a[2], a[3], a[4], a[5], a[12], a[13], a[14], peak=bt.peak, early=early)
            assert_recorded_bits(case, dict(noisy=n1, target=t1, g=i1.g, scale=i1.scale, Ps=i1.Ps, Pn=i1.Pn), parent_bits)
            no_src = a[:6] + [None] * 6 + a[12:15] + [None, None]
            zero = list(a)
            zero[6] = torch.zeros_like(a[6])                                               # or: four columns, none used
            for args in (no_src, zero):
                n2, t2, i2 = eng.scene(*args, peak=bt.peak, early=early)
                assert_recorded_bits(case, dict(noisy=n2, target=t2, g=i2.g[:, 0], scale=i2.scale, Ps=i2.Ps, Pn=i2.P[:, 0]),
                                     parent_bits)
                assert torch.equal(n1.view(torch.int32), n2.view(torch.int32)) and torch.equal(t1.view(torch.int32), t2.view(torch.int32))
                assert torch.equal(i1.g, i2.g[:, 0]) and torch.equal(i1.Pn, i2.P[:, 0])
                assert torch.equal(i1.scale, i2.scale) and torch.equal(i1.Ps, i2.Ps)
                assert bool((i2.g[:, 1:] == 0).all()) and bool((i2.P[:, 1:] == 0).all())


# ------------------------------------------------------------------ 3. determinism
def test_bit_identical_between_calls_and_row_independent(eng, batches):
    bt = batches["bits"]
    B, L = bt.clean.shape
    a = _scene(eng, bt)
    assert _same_bits(a, _scene(eng, bt))
    rng = np.random.default_rng(1)
    for b in range(B):
        one = _scene(eng, _rows(bt, [b]))                                                 # alone
        assert _same_bits(one, ([a[0][b:b + 1], a[1][b:b + 1], [v[b:b + 1] for v in a[2]]])), b
    # other neighbours, with other source counts; NaN and wild entries in the unused source columns
    other = {k: getattr(bt, k).copy() for k in ("clean",) + TABLES}
    for b in (0, 1, 3, 4):
        other["clean"][b] = (0.3 * rng.standard_normal(L)).astype(np.float32)
        other["n_src"][b] = (other["n_src"][b] + 2) % 5
        other["src_off"][b] += 17
    sb = int(bt.n_src[2])
    other["src_snr_db"][2, sb:] = np.nan
    other["src_start"][2, sb:] = 2 ** 62
    other["src_len"][2, sb:] = -1
    other["src_rir_index"][2, sb:] = 10 ** 9
    other["src_rir_len"][2, sb:] = -(10 ** 9)
    big = _rows(bt._replace(**other), [4, 3, 2, 2, 1, 0, 2])
    c = _scene(eng, big)
    for k in (2, 3, 6):
        assert _same_bits(([c[0][k:k + 1], c[1][k:k + 1], [v[k:k + 1] for v in c[2]]]),
                          ([a[0][2:3], a[1][2:3], [v[2:3] for v in a[2]]])), k
    assert all(np.all(np.isfinite(v)) for v in (c[0], c[1], *c[2]))


def test_padding_behind_the_rows_is_neither_read_nor_written(eng, batches):
    """The native call with ld > L and ld_out > L: NaN between the rows of clean changes no bit, and what lies between the
    rows of the outputs stays as it was."""
    bt = batches["bits"]
    B, L = bt.clean.shape
    a = _dev(bt)
    want = eng.scene(*a, peak=bt.peak, early=bt.early)
    ld, ld_out, S = L + 37, L + 5, 4
    clean = torch.full((B, ld), float("nan"), dtype=torch.float32, device=DEV)
    clean[:, :L] = a[0]
    noisy = torch.full((B, ld_out), -7.0, dtype=torch.float32, device=DEV)
    target = torch.full((B, ld_out), -7.0, dtype=torch.float32, device=DEV)
    gp = torch.empty(2, B, 1 + S, dtype=torch.float64, device=DEV)
    info = torch.empty(2, B, dtype=torch.float64, device=DEV)
    ws = eng._grow("scene", int(eng.lib.cmgan_scene_workspace_bytes(eng._h, B, L, bt.rir.shape[1], S)))
    with torch.cuda.device(eng.device):
        eng._call("cmgan_scene", clean, B, L, ld, a[1], a[1].numel(), a[2], a[3], a[4], a[5], a[7], a[7].numel(), S, a[6], a[8],
                  a[9], a[10], a[11], a[12], a[12].size(0), a[12].size(1), a[13], a[14], a[15], a[16], float(bt.peak),
                  int(bt.early), noisy, target, ld_out, gp[0], gp[1], info[0], info[1], ws, ws.numel())
    assert torch.equal(noisy[:, :L].contiguous().view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(target[:, :L].contiguous().view(torch.int32), want[1].view(torch.int32))
    assert bool((noisy[:, L:] == -7.0).all()) and bool((target[:, L:] == -7.0).all())
    assert torch.equal(gp[0], want[2].g) and torch.equal(gp[1], want[2].P) and torch.equal(info[0], want[2].Ps)


# ------------------------------------------------------------------ 4. the peak guard
def test_the_sources_engage_the_peak_guard(eng, batches):
    bt = batches["peak"]
    noisy, target, (g, scale, ps, p) = _scene(eng, bt)
    pk = float(np.float32(bt.peak))
    assert np.all(scale < 1.0) and np.max(np.abs(noisy)) <= pk
    assert np.all(np.max(np.abs(noisy), axis=1) >= pk * (1 - 1e-6))                        # the guard scales TO the peak
    quiet = _scene(eng, bt._replace(n_src=np.zeros(2, dtype=np.int32)))
    assert np.all(quiet[2][1] == 1.0)                                                      # it is the sources that push it over
    for b in range(2):
        sb = int(bt.n_src[b])
        got_snr = 10.0 * np.log10(ps[b] / (g[b, 1:1 + sb] ** 2 * p[b, 1:1 + sb]))
        assert np.max(np.abs(got_snr + 25.0)) < 1e-9


# ------------------------------------------------------------------ 5. hipGraph
def test_captured_scene_replays_with_rewritten_tables(eng, batches):
    b0, b1 = batches["graph-0"], batches["graph-1"]
    dev = _dev(b0)
    call = lambda: eng.scene(*dev, peak=b0.peak, early=b0.early)
    eager = call()                                              # the warm-up call (grows the workspace)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out = call()
    graph.replay()
    assert torch.equal(g_out[0], eager[0]) and torch.equal(g_out[1], eager[1])
    _judge("graph-0", "graph-0", _np(g_out))
    for k, new in zip(range(len(dev)), _dev(b1)):               # the new tables, written into the tensors the graph reads
        if new is not None and not torch.equal(dev[k], new):
            dev[k].copy_(new)
    graph.replay()
    again = call()
    assert not torch.equal(again[0], eager[0])
    assert torch.equal(g_out[0], again[0]) and torch.equal(g_out[1], again[1])
    assert all(torch.equal(x, y) for x, y in zip(g_out[2], again[2]))
    _judge("graph-1", "graph-1", _np(g_out))


# ------------------------------------------------------------------ 6. the front end
def _front(rng):
    from cmgan_amd.mixing import NoiseBank, RirBank
    nb = NoiseBank.from_arrays([rng.standard_normal(n).astype(np.float32) for n in (1, 300, 5000, 1234)], device=DEV)
    sb = NoiseBank.from_arrays([(0.2 * rng.standard_normal(n)).astype(np.float32) for n in (900, 7, 4000)], device=DEV)
    rb = RirBank.from_arrays([M.rirs(1, k, rng)[0] for k in (1, 30, 200)], device=DEV)
    return nb, sb, rb


def _gens(seed):
    g1, g2 = torch.Generator(device=DEV), torch.Generator(device=DEV)
    g1.manual_seed(seed)
    g2.manual_seed(seed + 1)
    return g1, g2


def _model_of_draw(clean, mixer, rir, d):
    """The float64 model fed with a mixer's draws, read back here once: a Batch for scene_model."""
    g = lambda t: None if t is None else t.cpu().numpy()
    dry = mixer.dry_noise
    bt = M.Batch(clean, g(mixer.noise_bank.data) if dry else None, *((g(d.noise_start), g(d.noise_len), g(d.noise_off), g(d.snr_db))
                 if dry else (None,) * 4), g(d.n_src), g(mixer.source_bank.data), g(d.src_start), g(d.src_len), g(d.src_off),
                 g(d.src_snr_db), g(rir), g(d.rir_index), g(d.rir_len), g(d.src_rir_index), g(d.src_rir_len), mixer.peak,
                 mixer.early if rir is not None else -1)
    return [M.direct(M.row_of(bt, b)) for b in range(len(clean))]


def _assert_rows32(tag, got, rows, key):
    """Against the float64 model rounded to float32: the kernel's sum may round the other way where the two straddle a
    tie, so up to one float32 ulp of the row's peak, 2 * 2^-24 max|want| (the front-end bound of tests/test_gpu_mix.py)."""
    for b, r in enumerate(rows):
        want = r[key].astype(np.float32).astype(np.float64)
        err = np.max(np.abs(got[b].astype(np.float64) - want))
        assert err <= 2.0 * U32 * np.max(np.abs(want)) + 1e-30, f"{tag} row {b} {key}: {err:.3e}"


def test_dynamic_mixer_without_sources_is_what_it_was(eng):
    """sources=None against the mixer without the argument: outputs, draws and both generators' states, bit for bit."""
    from cmgan_amd.mixing import ChannelSampler, Draw, DynamicMixer, RoomSampler
    rng = np.random.default_rng(21)
    nb, sb, rb = _front(rng)
    cd = _t((0.1 * rng.standard_normal((5, 1500))).astype(np.float32))
    out = []
    for kw in ({}, dict(sources=None, source_bank=None, source_snr_db=(1.0, 2.0), dry_noise=True)):
        g1, g2 = _gens(31)
        g3 = torch.Generator(device=DEV)
        g3.manual_seed(5)
        m = DynamicMixer(eng, nb, rooms=RoomSampler(generator=g2), rir_seconds=0.02, p_reverb=0.7, generator=g1,
                         level_db=(-30.0, -20.0), channel=ChannelSampler(generator=g3), **kw)
        first = m(cd)
        second = m(cd)
        out.append((first, second, m.last_draw, m.last_bank.data.clone(), g1.get_state(), g2.get_state(), g3.get_state()))
    a, b = out
    from cmgan_amd.engine import MixInfo
    assert isinstance(a[0][2], MixInfo) and isinstance(b[0][2], MixInfo)
    for k in (0, 1):
        assert torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1]) and all(torch.equal(x, y) for x, y in zip(a[k][2], b[k][2]))
    assert all(torch.equal(x, y) for x, y in zip(a[3:], b[3:]))
    for name in Draw._fields:
        x, y = getattr(a[2], name), getattr(b[2], name)
        if name == "channel":
            assert all(torch.equal(p, q) for p, q in zip(x, y))
        else:
            assert (x is None and y is None) or torch.equal(x, y), name
    assert type(a[2]) is Draw and type(b[2]) is Draw


def test_dynamic_mixer_simulates_every_source_in_its_room(eng):
    from cmgan_amd.engine import SceneInfo
    from cmgan_amd.mixing import DynamicMixer, RoomSampler
    rng = np.random.default_rng(22)
    nb, sb, rb = _front(rng)
    B, L, S = 4, 1500, 3
    clean = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    g1, g2 = _gens(41)
    sampler = RoomSampler(generator=g2)
    m = DynamicMixer(eng, nb, rooms=sampler, rir_seconds=0.02, p_reverb=0.5, early_ms=2.0, generator=g1, sources=(1, S),
                     source_bank=sb, source_snr_db=(0.0, 10.0))
    before = g2.get_state()
    target, noisy, info = m(_t(clean))
    d, bank = m.last_draw, m.last_bank
    K = m.rir_taps
    assert isinstance(info, SceneInfo) and tuple(info.g.shape) == (B, 1 + S) and bool(torch.isfinite(noisy).all())
    n = d.n_src.cpu().numpy()
    assert n.min() >= 1 and n.max() <= S and K == 320 and tuple(bank.data.shape) == (B + 1 + B * S, K)
    # the tables are draw_sources' of the batch's rooms, drawn after them from the sampler's generator
    g2.set_state(before)
    rooms, taps = sampler.draw(B, K, 16000, device=torch.device(DEV))
    assert torch.equal(rooms, d.rooms) and torch.equal(sampler.draw_sources(rooms, S), d.src_rooms)
    assert torch.equal(d.src_rir_len, taps[:, None].expand(B, S)) and tuple(d.src_rooms.shape) == (B, S, 15)
    # every source response is Engine.rir on its table, where src_rir_index says
    want, wlen = eng.rir(d.src_rooms.reshape(B * S, 15), d.src_rir_len.reshape(B * S), K, m.n_images, fs=16000)
    idx = d.src_rir_index.reshape(B * S).long()
    assert idx.tolist() == list(range(B + 1, B + 1 + B * S))
    assert torch.equal(bank.data[idx].view(torch.int32), want.view(torch.int32)) and torch.equal(bank.length[idx], wlen)
    assert bool((want.abs().amax(dim=1) > 0).all())
    talker, _ = eng.rir(d.rooms, d.rir_len, K, m.n_images, fs=16000)
    assert torch.equal(bank.data[:B], talker) and float(bank.data[B, 0]) == 1.0
    # and the mix is the model's, fed with the draws and the simulated bank
    rows = _model_of_draw(clean, m, bank.data, d)
    _assert_rows32("rooms", noisy.cpu().numpy(), rows, "noisy")
    _assert_rows32("rooms", target.cpu().numpy(), rows, "target")
    for b, r in enumerate(rows):
        for j in range(1, 1 + int(n[b])):
            assert float(r["g"][j]) > 0 and abs(float(info.g[b, j]) - float(r["g"][j])) <= 1e-12 * float(r["g"][j])
        assert bool((info.g[b, 1 + int(n[b]):] == 0).all())
    # the next call reuses the allocation
    ptr = bank.data.data_ptr()
    m(_t(clean))
    assert m.last_bank.data.data_ptr() == ptr


@pytest.mark.parametrize("mode", ["bank", "dry"])
def test_dynamic_mixer_with_a_rir_bank_and_with_dry_sources(eng, mode):
    from cmgan_amd.mixing import DynamicMixer
    rng = np.random.default_rng(23)
    nb, sb, rb = _front(rng)
    B, L = 6, 1700
    clean = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    mixers = []
    for _ in range(2):
        g1, _ = _gens(51)
        mixers.append(DynamicMixer(eng, nb, rb if mode == "bank" else None, p_reverb=0.5, early_ms=2.0, generator=g1,
                                   sources=(0, 4), source_bank=sb, source_snr_db=(-5.0, 5.0), dry_noise=mode == "bank",
                                   snr_on="active" if mode == "dry" else "rms"))
    m = mixers[0]
    target, noisy, info = m(_t(clean))
    t2, n2, i2 = mixers[1](_t(clean))
    assert torch.equal(noisy, n2) and torch.equal(target, t2) and all(torch.equal(x, y) for x, y in zip(info, i2))
    d = m.last_draw
    assert tuple(d.src_start.shape) == (B, 4) and int(d.n_src.min()) >= 0 and int(d.n_src.max()) <= 4
    if mode == "bank":
        idx = d.src_rir_index.cpu().numpy()
        assert idx.min() >= 0 and idx.max() < len(rb)                                     # never the identity of p_reverb
        assert torch.equal(d.src_rir_len, m.rir_bank.length[d.src_rir_index.long()])
        rows = _model_of_draw(clean, m, m.rir_bank.data, d)
    else:
        assert d.src_rir_index is None and d.src_rir_len is None and bool((info.g[:, 0] == 0).all())
        lv = m.last_level
        delta = -10.0 * torch.log10(lv.activity)
        rows = _model_of_draw(clean, m, None, d._replace(src_snr_db=(d.src_snr_db.double() - delta[:, None]).float()))
        assert torch.equal(target, _t(clean)) or bool((info.scale != 1).any())
    _assert_rows32(mode, noisy.cpu().numpy(), rows, "noisy")
    _assert_rows32(mode, target.cpu().numpy(), rows, "target")
