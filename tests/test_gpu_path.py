"""Paths on the GPU (cmgan_amd/csrc/scene.hip; include/cmgan_hip.h, "Paths"): Engine.scene_path against the long-double
model of tests/path_model.py under the rule |g - w| <= ulp32(w) / 2 + E on every registered row (hops inside, equal to and
straddling a tile, paths that end before and after the clip, chunked and over-long responses, direct paths that differ
along a path, clamped counts), the bits of Engine.scene for rows that stand still, row independence and reproducibility,
padding, hipGraph replay with rewritten path tables, and the front end (DynamicMixer(motion=...), draw_path)."""
import numpy as np
import pytest
import torch

import path_model as M
import scene_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U32 = 2.0 ** -24
T0 = scene_model.TPB * scene_model.OPT
JUDGED = ["h37", "htile", "h1500", "hfar"]
TABLES = ("n_path", "rir_index", "rir_len", "noise_start", "noise_len", "noise_off", "snr_db", "n_src", "src_start", "src_len",
          "src_off", "src_snr_db", "src_n_path", "src_rir_index", "src_rir_len")
ORDER = ("n_path", "rir", "rir_index", "rir_len", "noise_bank", "noise_start", "noise_len", "noise_off", "snr_db", "n_src",
         "src_bank", "src_start", "src_len", "src_off", "src_snr_db", "src_n_path", "src_rir_index", "src_rir_len")


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
    return bt._replace(**{k: getattr(bt, k)[rows] for k in ("clean",) + TABLES if getattr(bt, k) is not None})


def _dev(bt):
    """The tensor arguments of Engine.scene_path behind (clean, hop), on the device, in call order."""
    return [_t(getattr(bt, k)) for k in ORDER]


def _np(out):
    noisy, target, info = out
    return noisy.cpu().numpy(), target.cpu().numpy(), [v.cpu().numpy() for v in info]


def _path(eng, bt):
    return _np(eng.scene_path(_t(bt.clean), bt.H, *_dev(bt), peak=bt.peak, early=bt.early))


def _same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               for x, y in zip([a[0], a[1], *a[2]], [b[0], b[1], *b[2]]))


def _row_of(out, k):
    return [out[0][k:k + 1], out[1][k:k + 1], [v[k:k + 1] for v in out[2]]]


def _judge(tag, name, got, rows=None):
    """Every row of `got` under the rule against the registered batch `name` (rows: which of its rows `got` holds).
    Returns (worst excess, worst error in units of ulp32 / 2, samples judged)."""
    noisy, target, (g, scale, ps, p) = got
    bt = M.BATCHES[name]
    rows = range(len(bt.clean)) if rows is None else rows
    worst, units, judged = -np.inf, 0.0, 0
    for k, b in enumerate(rows):
        sl, ld = M.case(name, b)
        for key, a in (("noisy", noisy[k]), ("target", target[k])):
            E, w = sl[key]
            x = M.excess(a, w, E)
            assert x <= 0.0, f"{tag} row {b} {key}: worst |g - w| - ulp32 / 2 - E = {x:.3e} (E = {E:.3e})"
            worst = max(worst, x)
            units = max(units, float(np.max(np.abs(a.astype(M.LD) - w).astype(np.float64) / (0.5 * M.ulp32(w.astype(np.float64))))))
            judged += len(w)
        sb = len(ld["g"]) - 1
        for j in range(g.shape[1]):                                       # the gains and the c-derived powers
            wg, wp = (float(ld["g"][j]), float(ld["P"][j])) if j <= sb else (0.0, 0.0)
            assert abs(g[k, j] - wg) <= 1e-12 * wg and abs(p[k, j] - wp) <= 1e-12 * wp, f"{tag} row {b} source {j}: g {g[k, j]!r} / {wg!r}, P {p[k, j]!r} / {wp!r}"
        assert abs(ps[k] - float(ld["Ps"])) <= 1e-12 * float(ld["Ps"]) and abs(scale[k] - float(ld["scale"])) <= 1e-12
    return worst, units, judged


# ------------------------------------------------------------------ 1. the kernels against the model
@pytest.mark.parametrize("name", JUDGED)
def test_kernel_meets_the_rule_on_every_registered_row(eng, batches, name):
    """|g - w| <= ulp32(w) / 2 + E for noisy and target of every row, w the long-double model, E from the model alone
    (tests/test_path_host.py holds E to 2^-10 of half an ulp of the row's rms); gains and powers to 1e-12."""
    got = _path(eng, batches[name])
    assert all(np.all(np.isfinite(v)) for v in (got[0], got[1], *got[2]))
    worst, units, judged = _judge(name, name, got)
    print(f"[path] {name}: {judged} samples judged, worst excess {worst:.3e}, worst error {units:.6f} half-ulps")
    bt = batches[name]
    g, p = got[2][0], got[2][3]
    assert g[0, 1] > 0 and g[0, 2] > 0 and g[2, 1] > 0 and g[2, 2] == 0.0 and p[2, 2] == 0.0      # row 2: one invalid segment
    assert np.all(g[4, 1:] == 0.0) and g[5, 1] > 0 and g[5, 2] == 0.0                             # n_src = 0 and 1
    if bt.early < 0:
        assert np.array_equal(got[1][4].view(np.uint32), bt.clean[4].view(np.uint32)) or got[2][1][4] != 1.0


# ------------------------------------------------------------------ 2. a row that stands still: Engine.scene
@pytest.mark.parametrize("name", ["h37", "htile", "h1500"])
def test_one_waypoint_has_the_bits_of_engine_scene(eng, batches, name):
    """n_path = 1 and src_n_path = 1 against Engine.scene with column 0 of the tables, computed here: S = 2 and S = 0, both
    tile-edge lengths, the chunked K = 1300 (row 0 and the source of row 1), with and without the target's prefix."""
    bt = batches[name]
    st = M.static_batch(bt)
    k = ("clean", "noise_bank", "noise_start", "noise_len", "noise_off", "snr_db", "n_src", "src_bank", "src_start", "src_len",
         "src_off", "src_snr_db", "rir", "rir_index", "rir_len", "src_rir_index", "src_rir_len")
    for ones in (1, 0, -7):                                               # 0 and -7 are clamped to 1
        one = bt._replace(n_path=np.full_like(bt.n_path, ones), src_n_path=np.full_like(bt.src_n_path, ones))
        want = _np(eng.scene(*[_t(getattr(st, f)) for f in k], peak=bt.peak, early=bt.early))
        assert _same_bits(_path(eng, one), want), (name, ones)
    # without sources, and with the target's other form
    src = ("n_src", "src_bank", "src_start", "src_len", "src_off", "src_snr_db", "src_n_path", "src_rir_index", "src_rir_len")
    bare = one._replace(**{f: None for f in src}, early=-1 if bt.early >= 0 else 30)
    sb = st._replace(**{f: None for f in src if f in st._fields}, early=bare.early)
    want = _np(eng.scene(*[_t(getattr(sb, f)) for f in k], peak=bt.peak, early=sb.early))
    got = _path(eng, bare)
    assert _same_bits(got, want) and got[2][0].shape == (len(bt.clean), 1)
    # and a path does change the row
    assert not np.array_equal(_path(eng, bt)[0][0], want[0][0])


# ------------------------------------------------------------------ 3. determinism
def test_bit_identical_between_calls_and_row_independent(eng, batches):
    bt = batches["htile"]
    B, L = bt.clean.shape
    P = bt.rir_index.shape[1]
    a = _path(eng, bt)
    assert _same_bits(a, _path(eng, bt))
    for b in range(B):
        assert _same_bits(_path(eng, _rows(bt, [b])), _row_of(a, b)), b                    # alone
    # other neighbours with other paths and source counts; wild entries in the columns nobody reads
    rng = np.random.default_rng(1)
    other = {k: getattr(bt, k).copy() for k in ("clean",) + TABLES}
    for b in (0, 1, 3, 4, 5):
        other["clean"][b] = (0.3 * rng.standard_normal(L)).astype(np.float32)
        other["n_path"][b] = (other["n_path"][b] + 2) % (P + 1)
        other["src_n_path"][b] = (other["src_n_path"][b] + 1) % (P + 1)
        other["n_src"][b] = (other["n_src"][b] + 1) % 3
    pb = min(max(int(bt.n_path[2]), 1), P)
    assert pb < P
    other["rir_index"][2, pb:] = 10 ** 9
    other["rir_len"][2, pb:] = -(10 ** 9)
    for j in range(2):
        sp = min(max(int(bt.src_n_path[2, j]), 1), P)
        other["src_rir_index"][2, j, sp:] = -(10 ** 9)
        other["src_rir_len"][2, j, sp:] = 2 ** 31 - 1
    big = _rows(bt._replace(**other), [4, 3, 2, 2, 1, 0])
    c = _path(eng, big)
    for k in (2, 3):
        assert _same_bits(_row_of(c, k), _row_of(a, 2)), k
    assert all(np.all(np.isfinite(v)) for v in (c[0], c[1], *c[2]))


def test_padding_behind_the_rows_is_neither_read_nor_written(eng, batches):
    """The native call with ld > L and ld_out > L: NaN between the rows of clean changes no bit, and what lies between the
    rows of the outputs stays as it was."""
    bt = batches["h37"]
    B, L = bt.clean.shape
    P, S = bt.rir_index.shape[1], 2
    a = dict(zip(ORDER, _dev(bt)))
    want = eng.scene_path(_t(bt.clean), bt.H, *a.values(), peak=bt.peak, early=bt.early)
    ld, ld_out = L + 37, L + 5
    clean = torch.full((B, ld), float("nan"), dtype=torch.float32, device=DEV)
    clean[:, :L] = _t(bt.clean)
    noisy = torch.full((B, ld_out), -7.0, dtype=torch.float32, device=DEV)
    target = torch.full((B, ld_out), -7.0, dtype=torch.float32, device=DEV)
    gp = torch.empty(2, B, 1 + S, dtype=torch.float64, device=DEV)
    info = torch.empty(2, B, dtype=torch.float64, device=DEV)
    ws = eng._grow("scene_path", int(eng.lib.cmgan_scene_path_workspace_bytes(eng._h, B, L, bt.rir.shape[1], S, P)))
    with torch.cuda.device(eng.device):
        eng._call("cmgan_scene_path", clean, B, L, ld, a["noise_bank"], a["noise_bank"].numel(), a["noise_start"], a["noise_len"],
                  a["noise_off"], a["snr_db"], a["src_bank"], a["src_bank"].numel(), S, a["n_src"], a["src_start"], a["src_len"],
                  a["src_off"], a["src_snr_db"], a["rir"], a["rir"].size(0), a["rir"].size(1), P, int(bt.H), a["n_path"],
                  a["rir_index"], a["rir_len"], a["src_n_path"], a["src_rir_index"], a["src_rir_len"], float(bt.peak),
                  int(bt.early), noisy, target, ld_out, gp[0], gp[1], info[0], info[1], ws, ws.numel())
    assert torch.equal(noisy[:, :L].contiguous().view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(target[:, :L].contiguous().view(torch.int32), want[1].view(torch.int32))
    assert bool((noisy[:, L:] == -7.0).all()) and bool((target[:, L:] == -7.0).all())
    assert torch.equal(gp[0], want[2].g) and torch.equal(gp[1], want[2].P) and torch.equal(info[0], want[2].Ps)


# ------------------------------------------------------------------ 4. hipGraph
def test_captured_path_replays_with_rewritten_tables(eng, batches):
    b0, b1 = batches["graph-0"], batches["graph-1"]
    clean, dev = _t(b0.clean), _dev(b0)
    call = lambda: eng.scene_path(clean, b0.H, *dev, peak=b0.peak, early=b0.early)
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


# ------------------------------------------------------------------ 5. the front end
def _front(rng):
    from cmgan_amd.mixing import NoiseBank
    nb = NoiseBank.from_arrays([rng.standard_normal(n).astype(np.float32) for n in (1, 300, 5000, 1234)], device=DEV)
    sb = NoiseBank.from_arrays([(0.2 * rng.standard_normal(n)).astype(np.float32) for n in (900, 7, 4000)], device=DEV)
    return nb, sb


def _gens(seed):
    g1, g2 = torch.Generator(device=DEV), torch.Generator(device=DEV)
    g1.manual_seed(seed)
    g2.manual_seed(seed + 1)
    return g1, g2


def _model_of_draw(clean, mixer, d):
    """The float64 model fed with a mixer's draws and its simulated bank, read back here once."""
    g = lambda t: None if t is None else t.cpu().numpy()
    B = len(clean)
    S = 0 if d.n_src is None else d.src_start.shape[1]
    still = lambda t: g(t)[..., None]
    bt = M.PathBatch(clean, mixer.motion_hop, g(d.n_path), g(mixer.last_bank.data), g(d.rir_index), g(d.rir_len),
                     g(mixer.noise_bank.data), g(d.noise_start), g(d.noise_len), g(d.noise_off), g(d.snr_db), g(d.n_src),
                     None if not S else g(mixer.source_bank.data), g(d.src_start), g(d.src_len), g(d.src_off), g(d.src_snr_db),
                     None if not S else (g(d.src_n_path) if d.src_n_path is not None else np.ones((B, S), dtype=np.int32)),
                     None if not S else (g(d.src_rir_index) if d.src_rir_index.dim() == 3 else still(d.src_rir_index)),
                     None if not S else (g(d.src_rir_len) if d.src_rir_len.dim() == 3 else still(d.src_rir_len)),
                     mixer.peak, mixer.early)
    return [M.direct(M.row_of(bt, b)) for b in range(B)]


def _assert_rows32(tag, got, rows, key):
    """Against the float64 model rounded to float32: the kernel's sum may round the other way where the two straddle a
    tie, so up to one float32 ulp of the row's peak, 2 * 2^-24 max|want| (the front-end bound of tests/test_gpu_scene.py)."""
    for b, r in enumerate(rows):
        want = r[key].astype(np.float32).astype(np.float64)
        err = np.max(np.abs(got[b].astype(np.float64) - want))
        assert err <= 2.0 * U32 * np.max(np.abs(want)) + 1e-30, f"{tag} row {b} {key}: {err:.3e}"


@pytest.mark.parametrize("tail", [None, 12.0])
def test_dynamic_mixer_moves_the_talker_and_the_sources(eng, tail):
    from cmgan_amd.engine import SceneInfo
    from cmgan_amd.mixing import DynamicMixer, PathDraw, RoomSampler
    rng = np.random.default_rng(22)
    nb, sb = _front(rng)
    B, L, S = 4, T0 + 300, 2
    clean = (0.1 * rng.standard_normal((B, L))).astype(np.float32)

    def mixer(**kw):
        g1, g2 = _gens(41)
        sampler = RoomSampler(generator=g2, tail_ms=tail, tail_window_ms=5.0) if tail else RoomSampler(generator=g2)
        return DynamicMixer(eng, nb, rooms=sampler, rir_seconds=0.05, early_ms=2.0, generator=g1, sources=(1, S), source_bank=sb,
                            source_snr_db=(0.0, 10.0), motion=(0.5, 1.5), p_motion=0.5, motion_hop_ms=25.0,
                            source_motion=(0.2, 0.4), **kw)

    m = mixer()
    target, noisy, info = m(_t(clean))
    d, bank = m.last_draw, m.last_bank
    H, K = m.motion_hop, m.rir_taps
    P = 1 + -(-(L - 1) // H)
    assert H == 400 and P == m.waypoints(L) == 5 and K == 800 and type(d) is PathDraw
    assert isinstance(info, SceneInfo) and tuple(info.g.shape) == (B, 1 + S) and bool(torch.isfinite(noisy).all())
    assert tuple(d.path.shape) == (B, P, 15) and tuple(d.src_path.shape) == (B, S, P, 15)
    assert tuple(d.rir_index.shape) == tuple(d.rir_len.shape) == (B, P) and tuple(d.src_rir_index.shape) == (B, S, P)
    n = d.n_path.cpu().numpy()
    assert d.n_path.dtype == torch.int32 and set(n.tolist()) <= {1, P}
    assert tuple(d.src_n_path.shape) == (B, S) and bool((d.src_n_path == P).all())
    # the path starts at the drawn source, and is simulated where the tables say
    assert torch.equal(d.path[:, 0], d.rooms) and torch.equal(d.src_path[:, :, 0], d.src_rooms)
    assert tuple(bank.data.shape) == (B * P + B * S * P, K)
    assert d.rir_index.flatten().tolist() == list(range(B * P))
    assert d.src_rir_index.flatten().tolist() == list(range(B * P, B * P + B * S * P))
    moved = bank.data[d.rir_index[:, -1].long()] != bank.data[d.rir_index[:, 0].long()]
    assert bool(moved.any(dim=1).all())                                                   # other positions, other responses
    if tail is None:
        want, wlen = eng.rir(d.path.reshape(B * P, 15), d.rir_len.reshape(B * P), K, m.n_images, fs=16000)
        assert torch.equal(bank.data[:B * P].view(torch.int32), want.view(torch.int32))
        want, _ = eng.rir(d.src_path.reshape(B * S * P, 15), d.src_rir_len.reshape(B * S * P), K, m.n_images, fs=16000)
        assert torch.equal(bank.data[B * P:].view(torch.int32), want.view(torch.int32))
    else:
        # ONE seed and decay per path: beyond their junctions the waypoints of a path carry the SAME noise at fitted
        # levels (normalised correlation 1), two paths do not
        t = m.last_tail
        assert tuple(t.seed.shape) == (B,) and tuple(t.src_seed.shape) == (B, S) and len(set(t.seed.tolist())) == B
        assert bool((d.rir_len == t.n_full[:, None]).all()) and bool((d.src_rir_len == t.n_full[:, None, None]).all())
        junction = m.rooms._junction(d.path, t.n_full[:, None], 16000).cpu().numpy()      # where each waypoint's tail begins
        data, full = bank.data.cpu().numpy().astype(np.float64), t.n_full.cpu().numpy()
        corr = lambda x, y: float(np.dot(x, y) / np.sqrt(np.dot(x, x) * np.dot(y, y)))
        seen = 0
        for b in range(B):
            k0 = int(junction[b].max())
            if full[b] - k0 < 100:
                continue
            tails = data[b * P:(b + 1) * P, k0:full[b]]
            assert all(abs(corr(tails[0], tails[p])) > 0.9999 for p in range(1, P)), b
            other = data[((b + 1) % B) * P, k0:full[b]]
            assert abs(corr(tails[0], other)) < 0.5 or not other.any(), b
            seen += 1
        assert seen >= 2
    # and the mix is the model's, fed with the draws and the simulated bank
    rows = _model_of_draw(clean, m, d)
    _assert_rows32("moving", noisy.cpu().numpy(), rows, "noisy")
    _assert_rows32("moving", target.cpu().numpy(), rows, "target")
    for b, r in enumerate(rows):
        assert len(r["d"]) == int(n[b])
        for j in range(1, 1 + int(d.n_src[b])):
            assert float(r["g"][j]) > 0 and abs(float(info.g[b, j]) - float(r["g"][j])) <= 1e-12 * float(r["g"][j])
    # room_stats measures waypoint 0 and draws nothing
    ms = mixer(room_stats=True)
    t2, n2, _ = ms(_t(clean))
    assert torch.equal(n2, noisy) and torch.equal(t2, target)
    want = eng.rir_stats(bank.data[d.rir_index[:, 0].long()].contiguous(), d.rir_len[:, 0].contiguous(), fs=16000)
    assert torch.equal(ms.last_room_stats.drr_db, want.drr_db) and torch.equal(ms.last_room_stats.c50_db, want.c50_db)
    assert tuple(want.drr_db.shape) == (B, 1) and bool(torch.isfinite(want.drr_db).all())


def test_dynamic_mixer_moves_only_the_sources_in_banded_rooms(eng):
    """source_motion alone, with bands and dry rows: the talkers keep ONE response (and the identity where dry) in every
    column, n_path is 1 without a draw, and every waypoint of a source is simulated with its room's band table."""
    from cmgan_amd.mixing import DynamicMixer, PathDraw, RoomSampler
    rng = np.random.default_rng(24)
    nb, sb = _front(rng)
    B, L, S = 5, 1300, 2
    clean = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    g1, g2 = _gens(61)
    m = DynamicMixer(eng, nb, rooms=RoomSampler(generator=g2, bands=3, tilt=(0.0, 0.5), filter_taps=63), rir_seconds=0.03,
                     p_reverb=0.6, early_ms=2.0, generator=g1, sources=(1, S), source_bank=sb, source_motion=(0.5, 1.0),
                     motion_hop_ms=25.0)
    state = g1.get_state()
    target, noisy, info = m(_t(clean))
    d, bank, K = m.last_draw, m.last_bank, m.rir_taps
    P = m.waypoints(L)
    assert type(d) is PathDraw and P == 5 and d.path is None and bool((d.n_path == 1).all())
    assert tuple(bank.data.shape) == (B + 1 + B * S * P, K) and float(bank.data[B, 0]) == 1.0
    assert bool((d.rir_index == d.rir_index[:, :1]).all()) and set(d.rir_index[:, 0].tolist()) <= set(range(B + 1))
    dry = d.rir_index[:, 0] == B
    assert bool((d.rir_len[dry] == 1).all()) and bool((d.rir_len[~dry] > 1).all())
    print(f"[path] {int(dry.sum())} of {B} rows dry")
    assert d.src_rir_index.flatten().tolist() == list(range(B + 1, B + 1 + B * S * P))
    want, _ = eng.rir_bands(d.src_path.reshape(B * S * P, 15), m.last_bands.repeat_interleave(S * P, dim=0),
                            d.src_rir_len.reshape(B * S * P), K, m.rooms.filters(16000, eng.device), m.n_images, fs=16000)
    assert torch.equal(bank.data[B + 1:].view(torch.int32), want.view(torch.int32))
    rows = _model_of_draw(clean, m, d)
    _assert_rows32("sources", noisy.cpu().numpy(), rows, "noisy")
    _assert_rows32("sources", target.cpu().numpy(), rows, "target")
    # no Bernoulli was drawn: the mixer's generator is where the same mixer without source_motion leaves it
    after = g1.get_state()
    g1.set_state(state)
    DynamicMixer(eng, nb, rooms=RoomSampler(generator=g2, bands=3, tilt=(0.0, 0.5), filter_taps=63), rir_seconds=0.03, p_reverb=0.6,
                 early_ms=2.0, generator=g1, sources=(1, S), source_bank=sb)(_t(clean))
    assert torch.equal(g1.get_state(), after)


def test_without_motion_the_mixer_is_what_it_was(eng):
    """motion=None, source_motion=None against the mixer without the arguments: outputs, draws, banks and every
    generator's state, bit for bit, with rooms, tails and sources in play."""
    from cmgan_amd.mixing import DynamicMixer, RoomSampler, SceneDraw
    rng = np.random.default_rng(21)
    nb, sb = _front(rng)
    cd = _t((0.1 * rng.standard_normal((5, 1500))).astype(np.float32))
    out = []
    for kw in ({}, dict(motion=None, p_motion=0.3, motion_hop_ms=100.0, source_motion=None)):
        g1, g2 = _gens(31)
        m = DynamicMixer(eng, nb, rooms=RoomSampler(generator=g2, tail_ms=12.0, tail_window_ms=5.0), rir_seconds=0.05, p_reverb=0.7,
                         generator=g1, sources=(0, 2), source_bank=sb, **kw)
        first = m(cd)
        once = m.last_draw
        second = m(cd)
        out.append((first, second, m.last_draw, m.last_bank.data.clone(), g1.get_state(), g2.get_state(), once))
    a, b = out
    for k in (0, 1):
        assert torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1]) and all(torch.equal(x, y) for x, y in zip(a[k][2], b[k][2]))
    assert all(torch.equal(x, y) for x, y in zip(a[3:6], b[3:6]))
    assert type(a[2]) is SceneDraw and type(b[2]) is SceneDraw                            # no PathDraw, no path field
    for name in SceneDraw._fields:
        x, y = getattr(a[2], name), getattr(b[2], name)
        assert (x is None and y is None) or torch.equal(x, y), name
    # the same mixer with motion draws the same leading numbers: the paths come after every other draw
    g1, g2 = _gens(31)
    m = DynamicMixer(eng, nb, rooms=RoomSampler(generator=g2, tail_ms=12.0, tail_window_ms=5.0), rir_seconds=0.05, p_reverb=0.7,
                     generator=g1, sources=(0, 2), source_bank=sb, motion=(0.5, 1.5), motion_hop_ms=25.0)
    m(cd)
    for name in ("noise_start", "noise_off", "snr_db", "rooms", "n_src", "src_start", "src_off", "src_snr_db", "src_rooms"):
        assert torch.equal(getattr(m.last_draw, name), getattr(a[6], name)), name
    assert m.last_draw.src_path is None and tuple(m.last_tail.seed.shape) == (5,)
    assert bool((m.last_draw.src_n_path == 1).all()) and tuple(m.last_draw.src_rir_index.shape) == (5, 2, m.waypoints(1500))
    dry = m.last_draw.rir_index[:, 0] == 5 * m.waypoints(1500)                            # p_reverb: the identity in every column
    assert bool((m.last_draw.rir_index[dry] == 5 * m.waypoints(1500)).all()) and bool((m.last_draw.rir_len[dry] == 1).all())
