"""The directional room simulator on the GPU (cmgan_amd/csrc/rir.hip; include/cmgan_hip.h, "Room impulse responses of
directional sources and receivers"): Engine.rir(orient=, pattern=) and Engine.rir_bands(orient=, pattern=) against the
float64 numpy model of tests/rir_dir_model.py over the kernel's tile and list edges, all-ones patterns against the plain
calls bit for bit, invalid rows, row independence, hipGraph replay with the two tables rewritten in place, and the front
end (RoomSampler.draw_dirs through RirBank.simulate and DynamicMixer).

The bound, for every tap (rir_dir_model.bound):  |gpu[k] - h[k]| <= 2^-24 |h[k]| + (64 (K + tw) + 52) 2^-53 A[k]
with A[k] = sum |a| over the images whose window reaches tap k, taken BEFORE the gains (|g| <= 1): rir_model.bound, whose
terms tests/test_gpu_rir.py derives, plus the 52 ulps of the gain's own arithmetic that rir_dir_model.GAIN_ULPS derives.
tests/test_rir_dir_host.py shows the directional responses to differ from the omni ones by more than 10^4 bounds."""
import numpy as np
import pytest
import torch

import rir_cases as RC
import rir_dir_model as DM
import rir_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS, C = 16000, 343.0

ROOM = [2.5, 2.0, 2.2, 0.7, 0.9, 1.1, 1.9, 0.6, 1.4, 0.9, 0.8, 0.85, 0.7, 0.6, 0.95]      # the reciprocity room
OTHER = [3.1, 2.3, 2.6, 1.0, 0.7, 1.3, 2.2, 1.9, 0.8, 0.9, 0.7, 0.8, 0.85, 0.75, 0.9]
THIRD = [1.5, 1.7, 1.4, 0.4, 0.5, 0.6, 1.1, 1.2, 0.9, 0.95, 0.9, 0.92, 0.97, 0.9, 0.93]
N5 = (5, 5, 5)                 # every image a response of up to 700 + 40 samples can see in ROOM
OBLIQUE = [0.3, -1.0, 0.4, -0.7, 0.2, 0.6]
PAIRS = {"cardioids": (0.5, 0.5), "eight-hyper": (0.0, 0.25), "sub-omni": (0.75, 1.0)}


@pytest.fixture(scope="module")
def eng():
    from cmgan_amd.engine import Engine
    return Engine(device=DEV)


@pytest.fixture(scope="module")
def TILE():
    from cmgan_amd import _lib
    return int(_lib.load().cmgan_rir_tile())


def _f64(a, *shape):
    return torch.tensor(np.asarray(a, dtype=np.float64).reshape(*shape), device=DEV)


def _run(eng, rooms, orient, pattern, n_taps, K, N, tw=40, out=None):
    rooms_d = _f64(rooms, -1, 15)
    R = rooms_d.size(0)
    taps_d = torch.tensor(np.asarray(n_taps, dtype=np.int32).reshape(-1), device=DEV)
    rir, length = eng.rir(rooms_d, taps_d, K, N, fs=FS, c=C, tw=tw, out=out, orient=_f64(orient, R, 6), pattern=_f64(pattern, R, 1, 2))
    assert rir.dtype == torch.float32 and tuple(rir.shape) == (R, K) and length.dtype == torch.int32
    return rir.cpu().numpy(), length.cpu().numpy()


def _plain(eng, rooms, n_taps, K, N, tw=40):
    rir, length = eng.rir(_f64(rooms, -1, 15), torch.tensor(np.asarray(n_taps, dtype=np.int32).reshape(-1), device=DEV), K, N,
                          fs=FS, c=C, tw=tw)
    return rir.cpu().numpy(), length.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _judge_row(tag, rir, length, h, bd, kr, K):
    """One row against the model under the bound: every tap, taps >= k_r bit-zero, the length.  Returns worst err / bound."""
    assert length == kr, f"{tag}: len {length}, model {kr}"
    assert not _bits(rir[kr:]).any(), f"{tag}: taps >= k_r are not bit-zero"
    err = np.abs(rir.astype(np.float64) - h)
    print(f"[rir_dir] {tag}: max err {err.max():.3e}, worst err / bound {float(np.max(err[bd > 0] / bd[bd > 0])) if (bd > 0).any() else 0.0:.3f}")
    bad = err > bd
    assert not bad.any(), (f"{tag}: {int(bad.sum())} of {K} taps outside the bound, first at {int(np.argmax(bad))}, "
                           f"worst err {err[bad].max():.3e} at bound {bd[bad][np.argmax(err[bad])]:.3e}")
    return float(np.max(err[bd > 0] / bd[bd > 0])) if (bd > 0).any() else 0.0


def _check(tag, got, rooms, orient, pattern, n_taps, K, N, tw=40, live=True):
    rir, length = got
    rooms = np.asarray(rooms, dtype=np.float64).reshape(-1, 15)
    orient, pattern = np.asarray(orient, dtype=np.float64).reshape(-1, 6), np.asarray(pattern, dtype=np.float64).reshape(-1, 2)
    worst = 0.0
    for r in range(rooms.shape[0]):
        h, A, kr = DM.rir_dir_row(rooms[r], orient[r], pattern[r], int(np.asarray(n_taps).reshape(-1)[r]), K, N, FS, C, tw)
        worst = max(worst, _judge_row(f"{tag} row {r}", rir[r], length[r], h, DM.bound(h, A, K, tw), kr, K))
        if live and kr > 1 and M.row_is_valid(rooms[r]) and DM.dirs_are_valid(orient[r], pattern[r]):
            assert np.max(np.abs(h)) > 1e-3
    return worst


# ------------------------------------------------------------------ 1. the kernel against the model
@pytest.mark.parametrize("tw", [4, 40])
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("k_of_tile", [lambda T: T - 1, lambda T: T + 1, lambda T: 2 * T + 3], ids=["TILE-1", "TILE+1", "2TILE+3"])
def test_kernel_matches_the_float64_model(eng, TILE, k_of_tile, pair, tw):
    K = k_of_tile(TILE)
    got = _run(eng, ROOM, OBLIQUE, PAIRS[pair], [K], K, N5, tw)
    _check(f"K={K} tw={tw} {pair}", got, ROOM, OBLIQUE, PAIRS[pair], [K], K, N5, tw)
    omni = _plain(eng, ROOM, [K], K, N5, tw)                      # and it is another response than the omni one
    assert np.max(np.abs(got[0] - omni[0])) > 1e-3


# ------------------------------------------------------------------ 2. all-ones patterns, row independence, repeatability
def test_all_ones_rows_have_the_bits_of_the_plain_call_and_rows_are_independent(eng, TILE):
    K, N = 2 * TILE + 50, (5, 5, 5)
    rooms = [ROOM, OTHER, THIRD, ROOM]
    orient = [OBLIQUE, [0.0] * 6, [1e100, -3e-7, 5.0, -1e-300, 0.0, 4e99], [0.0, 0.0, -2.0, 1.0, 1.0, 0.0]]
    pattern = [(0.5, 0.25), (1.0, 1.0), (1.0, 1.0), (0.0, 0.6)]
    n_taps = [K, TILE + 1, K - 3, K]
    a = _run(eng, rooms, orient, pattern, n_taps, K, N)
    assert a[1].tolist() == n_taps
    _check("four rows", a, rooms, orient, pattern, n_taps, K, N)
    for r in (1, 2):
        plain = _plain(eng, rooms[r], n_taps[r:r + 1], K, N)
        assert np.array_equal(_bits(plain[0][0]), _bits(a[0][r])) and plain[1][0] == a[1][r], r
    for r in (0, 3):
        one = _run(eng, rooms[r], orient[r], pattern[r], n_taps[r:r + 1], K, N)
        assert np.array_equal(_bits(one[0][0]), _bits(a[0][r])) and one[1][0] == a[1][r], r
    assert not np.array_equal(_bits(a[0][0]), _bits(a[0][3]))      # (the same room, facing elsewhere)
    b = _run(eng, rooms, orient, pattern, n_taps, K, N)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------ 3. the edge rooms, with directivity
@pytest.mark.parametrize("name,room", [
    # a source 5 cm from the wall at x = 0: each image pair (p_x = 0, 1) is 10 cm apart and faces opposite ways in x
    ("source at a wall", [3.0, 4.0, 2.5, 0.05, 2.0, 1.2, 2.5, 1.0, 1.0, 0.9, 0.8, 0.85, 0.7, 0.6, 0.95]),
    # a direct path of 0.245 m = 11.4 samples, shorter than tw = 40: its window is cut at k < 0
    ("direct path inside the window", [3.0, 4.0, 2.5, 1.0, 1.0, 1.0, 1.2, 1.1, 0.9, 0.9, 0.8, 0.85, 0.7, 0.6, 0.95]),
    # source on the receiver: d = 0, both cosines 0, the direct amplitude alpha_s alpha_m / (4 pi CMGAN_RIR_DMIN)
    ("source on the receiver", [3.0, 4.0, 2.5, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.9, 0.8, 0.85, 0.7, 0.6, 0.95]),
])
def test_close_images_and_windows_cut_at_zero(eng, TILE, name, room):
    K, N = TILE + 44, (3, 2, 3)
    got = _run(eng, room, OBLIQUE, (0.5, 0.25), [K], K, N)
    _check(name, got, room, OBLIQUE, (0.5, 0.25), [K], K, N)
    if name == "source on the receiver":
        anechoic = room[0:9] + [0.0] * 6
        h = _run(eng, anechoic, OBLIQUE, (0.5, 0.25), [K], K, (0, 0, 0))[0][0]
        assert h[0] == np.float32(0.5 * 0.25 / (4 * np.pi * M.DMIN)) and np.max(np.abs(h[1:])) < 1e-14 * h[0]


def test_more_images_in_a_tile_than_the_on_chip_list_holds(eng, TILE):
    """The lively 1.2 m cube of tests/test_gpu_rir.py: a round of the scan overflows the list, so the chunked path runs the
    directional entry code."""
    from cmgan_amd import _lib
    cap = int(_lib.load().cmgan_rir_list_capacity())
    room = [1.2, 1.2, 1.2, 0.3, 0.4, 0.5, 0.9, 0.8, 0.7] + [0.97] * 6
    K, N = 3 * TILE, (9, 9, 9)
    tau = M.images(room, N)[0] * FS / C
    reach = (tau > K - TILE - 40) & (tau < K - 1 + 40)
    per_round = np.add.reduceat(reach.reshape(-1, 2 * N[2] + 1).sum(1), np.arange(0, reach.size // (2 * N[2] + 1), TILE))
    assert int(reach.sum()) > 2 * cap and per_round.max() > cap
    got = _run(eng, room, OBLIQUE, (0.25, 0.5), [K], K, N)
    _check("lively cube", got, room, OBLIQUE, (0.25, 0.5), [K], K, N)


# ------------------------------------------------------------------ 4. image ranges
def test_image_range_smaller_and_larger_than_the_response_needs(eng):
    K, pat = 700, (0.5, 0.25)
    full = _run(eng, ROOM, OBLIQUE, pat, [K], K, N5)
    _check("N5", full, ROOM, OBLIQUE, pat, [K], K, N5)
    cut = _run(eng, ROOM, OBLIQUE, pat, [K], K, (1, 1, 1))
    _check("N=(1,1,1)", cut, ROOM, OBLIQUE, pat, [K], K, (1, 1, 1))
    assert not np.array_equal(cut[0], full[0])
    big = _run(eng, ROOM, OBLIQUE, pat, [K], K, (9, 8, 10))
    assert np.array_equal(_bits(big[0]), _bits(full[0]))
    huge = _run(eng, ROOM, OBLIQUE, pat, [K], K, (40, 3, 70))     # (Ny = 3 cuts; compare with the same cut)
    small = _run(eng, ROOM, OBLIQUE, pat, [K], K, (5, 3, 5))
    assert np.array_equal(_bits(huge[0]), _bits(small[0])) and not np.array_equal(_bits(huge[0]), _bits(full[0]))


# ------------------------------------------------------------------ 5. invalid rows
def test_invalid_rows_are_zeros_with_length_one(eng, TILE):
    K, N = TILE + 9, (2, 2, 2)
    good_o, good_p = OBLIQUE, (0.5, 0.25)
    nan_o = list(OBLIQUE)
    nan_o[4] = np.nan
    wild_o = list(OBLIQUE)
    wild_o[2] = 1e200
    rows = [(ROOM, good_o, good_p), (ROOM, nan_o, good_p), (ROOM, good_o, (1.5, 0.25)), (OTHER, good_o, good_p),
            (ROOM, good_o, (0.5, -0.1)), (ROOM, [0.0, 0.0, 0.0, 1.0, 0.0, 0.0], (0.5, 1.0)), (ROOM, wild_o, (1.0, 1.0)),
            (ROOM, [1.0, 0.0, 0.0, 0.0, 0.0, 0.0], (0.5, 0.999)), (ROOM, good_o, (np.nan, 0.5)), (THIRD, good_o, good_p)]
    rooms, orient, pattern = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    n_taps = [K] * len(rows)
    out = (torch.full((len(rows), K), 7.0, dtype=torch.float32, device=DEV),
           torch.full((len(rows),), -5, dtype=torch.int32, device=DEV))
    rir, length = _run(eng, rooms, orient, pattern, n_taps, K, N, out=out)
    assert length.tolist() == [K, 1, 1, K, 1, 1, 1, 1, 1, K]
    for r in (1, 2, 4, 5, 6, 7, 8):
        assert not _bits(rir[r]).any(), r
    _check("invalid rows", (rir, length), rooms, orient, pattern, n_taps, K, N)
    for r in (0, 3, 9):                                           # the neighbours are what they are alone
        alone = _run(eng, rooms[r], orient[r], pattern[r], [K], K, N)
        assert np.array_equal(_bits(alone[0][0]), _bits(rir[r])), r


# ------------------------------------------------------------------ 6. bands
def _band_case(TILE, NB):
    K, NF = TILE + 44, 33
    rng = np.random.default_rng(60 + NB)
    pattern = {1: [(0.5, 0.25)], 3: [(0.9, 0.5), (0.5, 0.5), (0.1, 0.5)]}.get(
        NB, [(round(a, 3), round(m, 3)) for a, m in zip(np.linspace(1.0, 0.0, NB), rng.uniform(0.0, 1.0, NB))])
    return dict(K=K, NF=NF, bands=RC.band_table(NB), filt=RC.filters(NB, NF), pattern=np.array(pattern),
                N=RC.images_for(K + (NF - 1) // 2, 40, ROOM[0:3]))


def _run_bands(eng, case, rooms, orient, pattern=None, n_taps=None, dirs=True):
    R = len(rooms)
    rooms_d, bands_d = _f64(rooms, R, 15), _f64([case["bands"]] * R, R, -1, 7)
    taps_d = torch.tensor(n_taps or [case["K"]] * R, dtype=torch.int32, device=DEV)
    kw = dict(orient=_f64(orient, R, 6), pattern=_f64(pattern, R, -1, 2)) if dirs else {}
    rir, length = eng.rir_bands(rooms_d, bands_d, taps_d, case["K"], _f64(case["filt"], *case["filt"].shape), case["N"], fs=FS, c=C,
                                tw=40, **kw)
    return rir.cpu().numpy(), length.cpu().numpy()


@pytest.mark.parametrize("NB", [1, 3, 8])
def test_banded_kernel_matches_the_float64_model(eng, TILE, NB):
    case = _band_case(TILE, NB)
    K = case["K"]
    banded = ROOM[0:9] + [float("nan")] * 6                        # columns 9 - 14 of a banded row are never read
    ones = np.ones((NB, 2))
    rooms, orient = [banded, banded, banded], [OBLIQUE, [0.0] * 6, OBLIQUE]
    pattern, n_taps = [case["pattern"], ones, case["pattern"]], [K, K, TILE - 5]
    assert len({tuple(p) for p in case["pattern"]}) == NB          # distinct per band
    rir, length = _run_bands(eng, case, rooms, orient, pattern, n_taps)
    for r in range(3):
        h, bd, kr = DM.rir_bands_dir_row(banded, case["bands"], orient[r], pattern[r], n_taps[r], K, case["N"], case["filt"], FS, C)
        _judge_row(f"NB={NB} row {r}", rir[r], length[r], h, bd, kr, K)
        assert np.max(np.abs(h)) > 1e-3
    plain = _run_bands(eng, case, [banded], None, n_taps=[K], dirs=False)
    assert np.array_equal(_bits(plain[0][0]), _bits(rir[1])) and plain[1][0] == length[1]      # all ones: Engine.rir_bands' bits
    assert np.max(np.abs(rir[0] - rir[1])) > 1e-3
    again = _run_bands(eng, case, rooms, orient, pattern, n_taps)
    assert np.array_equal(_bits(again[0]), _bits(rir))
    alone = _run_bands(eng, case, rooms[2:], orient[2:], pattern[2:], n_taps[2:])
    assert np.array_equal(_bits(alone[0][0]), _bits(rir[2]))
    # an invalid pattern in one band of one row
    broken = case["pattern"].copy()
    broken[NB - 1, 0] = 1.25
    rir2, length2 = _run_bands(eng, case, rooms, orient, [case["pattern"], broken, case["pattern"]], n_taps)
    assert length2.tolist() == [K, 1, TILE - 5] and not _bits(rir2[1]).any()
    assert np.array_equal(_bits(rir2[0]), _bits(rir[0])) and np.array_equal(_bits(rir2[2]), _bits(rir[2]))


# ------------------------------------------------------------------ 7. graph capture
def test_captured_call_replays_with_new_orient_and_pattern_tables(eng, TILE):
    K, N = TILE + 30, (3, 3, 3)
    rooms = torch.tensor([ROOM, OTHER], dtype=torch.float64, device=DEV)
    n_taps = torch.tensor([K, K - 7], dtype=torch.int32, device=DEV)
    orient, pattern = _f64([OBLIQUE, OBLIQUE], 2, 6), _f64([(0.5, 0.25), (0.75, 1.0)], 2, 1, 2)
    call = lambda: eng.rir(rooms, n_taps, K, N, orient=orient, pattern=pattern)
    eager, eager_len = call()                                     # the warm-up call (grows the workspace)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_rir, g_len = call()
    graph.replay()
    assert torch.equal(g_rir, eager) and torch.equal(g_len, eager_len)
    new_o, new_p = [[0.0, 0.0, 1.0, -1.0, 2.0, 0.5], [1.0, 1.0, 1.0, 0.0, 0.0, 0.0]], [(0.0, 0.5), (0.25, 0.5)]
    orient.copy_(_f64(new_o, 2, 6))
    pattern.copy_(_f64(new_p, 2, 1, 2))
    graph.replay()
    again, again_len = call()
    assert not torch.equal(again, eager)
    assert torch.equal(g_rir.view(torch.int32), again.view(torch.int32)) and torch.equal(g_len, again_len)
    assert again_len.tolist() == [K, 1]                            # (row 1: a zero vector at a directional microphone)
    _check("replayed", (g_rir.cpu().numpy(), g_len.cpu().numpy()), rooms.cpu().numpy(), new_o, new_p, [K, K - 7], K, N)


# ------------------------------------------------------------------ 8. the front end
def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _sampler(seed, **kw):
    from cmgan_amd.mixing import RoomSampler
    return RoomSampler(dims=((2.0, 2.0, 2.0), (3.0, 3.0, 2.5)), rt60=(0.06, 0.2), margin=0.3, generator=_gen(seed), **kw)


def test_dynamic_mixer_simulates_directional_talkers_and_sources(eng):
    from cmgan_amd.mixing import DynamicMixer, NoiseBank, PathDraw
    rng = np.random.default_rng(8)
    nb = NoiseBank.from_arrays([rng.standard_normal(n).astype(np.float32) for n in (300, 5000, 1234)], device=DEV)
    B, L, S = 3, 2000, 2
    clean = torch.tensor((0.1 * rng.standard_normal((B, L))).astype(np.float32), device=DEV)
    aim = dict(source_pattern=(0.25, 0.75), mic_pattern=(0.5, 1.0), facing_deg=(0.0, 60.0))
    m = DynamicMixer(eng, nb, rooms=_sampler(81, **aim), rir_seconds=0.03, early_ms=2.0, generator=_gen(80), sources=(1, S),
                     source_snr_db=(0.0, 10.0), motion=(0.5, 1.5), motion_hop_ms=25.0, source_motion=(0.2, 0.4))
    target, noisy, info = m(clean)
    d, bank, K, H = m.last_draw, m.last_bank, m.rir_taps, m.motion_hop
    P = m.waypoints(L)
    assert type(d) is PathDraw and K == 480 and H == 400 and P == 6 and tuple(bank.data.shape) == (B * P + B * S * P, K)
    # the tables re-drawn from the same seed, in the mixer's order: rooms, sources, the walks, then the directions
    twin = _sampler(81, **aim)
    rooms, taps = twin.draw(B, K, FS, device=DEV)
    src = twin.draw_sources(rooms, S)
    seconds = (P - 1) * H / float(FS)
    path, src_path = twin.draw_path(rooms, P, seconds, speed=m.motion), twin.draw_path(src, P, seconds, speed=m.source_motion)
    orient, pattern = twin.draw_dirs(path, path=True)
    src_orient, src_pattern = twin.draw_dirs(src_path, path=True, facing_deg=(0.0, 180.0))
    assert torch.equal(path, d.path) and torch.equal(src_path, d.src_path)
    (o1, p1), (o2, p2) = m.last_dirs
    assert torch.equal(o1, orient) and torch.equal(p1, pattern) and torch.equal(o2, src_orient) and torch.equal(p2, src_pattern)
    assert tuple(orient.shape) == (B, P, 6) and tuple(src_pattern.shape) == (B, S, P, 1, 2)
    want, wlen = eng.rir(path.reshape(B * P, 15), d.rir_len.reshape(B * P), K, m.n_images, fs=FS, orient=orient.reshape(B * P, 6),
                         pattern=pattern.reshape(B * P, 1, 2))
    assert torch.equal(bank.data[:B * P].view(torch.int32), want.view(torch.int32)) and torch.equal(bank.length[:B * P], wlen)
    want, _ = eng.rir(src_path.reshape(B * S * P, 15), d.src_rir_len.reshape(B * S * P), K, m.n_images, fs=FS,
                      orient=src_orient.reshape(B * S * P, 6), pattern=src_pattern.reshape(B * S * P, 1, 2))
    assert torch.equal(bank.data[B * P:].view(torch.int32), want.view(torch.int32))
    omni, _ = eng.rir(path.reshape(B * P, 15), d.rir_len.reshape(B * P), K, m.n_images, fs=FS)
    assert float((omni - bank.data[:B * P]).abs().max()) > 1e-3 and float(bank.data.abs().max()) > 1e-2
    # and the mix is Engine.scene_path on that bank
    n2, t2, _ = eng.scene_path(clean, H, d.n_path, bank.data, d.rir_index, d.rir_len, nb.data, d.noise_start, d.noise_len,
                               d.noise_off, d.snr_db, d.n_src, nb.data, d.src_start, d.src_len, d.src_off, d.src_snr_db,
                               d.src_n_path, d.src_rir_index, d.src_rir_len, peak=m.peak, early=m.early)
    assert torch.equal(n2.view(torch.int32), noisy.view(torch.int32)) and torch.equal(t2.view(torch.int32), target.view(torch.int32))
    assert bool(torch.isfinite(noisy).all()) and float(noisy.abs().max()) > 0.0


def test_a_talker_facing_the_microphone_measures_a_larger_drr_than_one_facing_away(eng):
    """Engine.rir_stats takes the response's PEAK as the direct arrival, so the inequality is asked where it follows from
    the geometry whichever arrival that is: 4 m cubes with both ends inside the central 0.4 m (margin 1.8 m).  Facing the
    microphone, the direct path (at most 0.7 m) is the peak and every reflection has travelled at least 3.6 m: at least 14 dB
    weaker each.  Facing away, the direct path is the cardioid's null, the peak is one reflection among its like, and the
    window around it holds a small part of the energy.  (The float64 models - rir_dir_model into rir_stats_model - give
    +11 .. +16 dB against -7 .. -10 dB over 40 such rooms.)"""
    from cmgan_amd.mixing import RirBank, RoomSampler
    banks, K = {}, 1600
    make = lambda **kw: RoomSampler(dims=((4.0, 4.0, 4.0), (4.0, 4.0, 4.0)), rt60=(0.3, 0.5), margin=1.8, generator=_gen(91), **kw)
    for deg in (0.0, 180.0):
        banks[deg] = RirBank.simulate(eng, make(source_pattern=(0.5, 0.5), facing_deg=(deg, deg)), 4, seconds=0.1, sample_rate=FS,
                                      measure=True)
        assert tuple(banks[deg].orient.shape) == (4, 6) and tuple(banks[deg].pattern.shape) == (4, 1, 2)
    assert torch.equal(banks[0.0].rooms, banks[180.0].rooms) and torch.equal(banks[0.0].length, banks[180.0].length)
    front, back = banks[0.0].stats.drr_db[:, 0], banks[180.0].stats.drr_db[:, 0]
    print(f"[rir_dir] DRR facing {front.tolist()} dB, facing away {back.tolist()} dB")
    assert bool(torch.isfinite(front).all()) and bool((front > back).all())
    # RirBank.simulate passes the tables on: the bank is the explicit call's
    b = banks[0.0]
    want, _ = eng.rir(b.rooms, b.length, K, make().n_images(K, FS), fs=FS, orient=b.orient, pattern=b.pattern)
    assert torch.equal(want.view(torch.int32), b.data.view(torch.int32))
