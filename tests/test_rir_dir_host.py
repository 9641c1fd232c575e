"""CPU side of the directional room simulator (cmgan_amd/csrc/rir.hip; include/cmgan_hip.h, "Room impulse responses of
directional sources and receivers"): the float64 model the GPU tests compare the kernels with (tests/rir_dir_model.py)
against its own definition as a naive loop, against rir_model (all alpha = 1: bit for bit), reciprocity and anechoic known
answers; RoomSampler's directivity draws; the workspace formulas; and every argument error of cmgan_rir_dir,
cmgan_rir_bands_dir, Engine.rir and Engine.rir_bands, all judged before a handle or a GPU is needed."""
import math

import numpy as np
import pytest
import torch

import rir_bands_model as BM
import rir_dir_model as DM
import rir_model as M
from cmgan_amd import _lib
from cmgan_amd.engine import check_rir_dir_args
from cmgan_amd.mixing import RoomSampler

BADARG, UNSUPPORTED = -1, -3
FS, C = 16000, 343.0
ROOM = [2.5, 2.0, 2.2, 0.7, 0.9, 1.1, 1.9, 0.6, 1.4, 0.9, 0.8, 0.85, 0.7, 0.6, 0.95]      # the reciprocity room
N5 = (5, 5, 5)


# ------------------------------------------------------------------ the model
def _naive(room, orient, pattern, n_taps, K, N, fs, c, tw):
    L, s, m, beta = room[0:3], room[3:6], room[6:9], room[9:15]
    u = np.array(orient[0:3]) / math.sqrt(sum(x * x for x in orient[0:3]))
    v = np.array(orient[3:6]) / math.sqrt(sum(x * x for x in orient[3:6]))
    kr = min(max(n_taps, 1), K)
    h = np.zeros(K)
    for nx in range(-N[0], N[0] + 1):
        for ny in range(-N[1], N[1] + 1):
            for nz in range(-N[2], N[2] + 1):
                n = (nx, ny, nz)
                for p in np.ndindex(2, 2, 2):
                    off = [(1 - 2 * p[i]) * s[i] + 2 * n[i] * L[i] - m[i] for i in range(3)]
                    d = math.sqrt(sum(o * o for o in off))
                    a = 1.0 / (4 * math.pi * max(d, M.DMIN))
                    for i in range(3):
                        a *= beta[2 * i] ** abs(n[i] - p[i]) * beta[2 * i + 1] ** abs(n[i])
                    cos_m = sum(off[i] * v[i] for i in range(3)) / d if d > 0 else 0.0
                    cos_s = -sum(off[i] * (1 - 2 * p[i]) * u[i] for i in range(3)) / d if d > 0 else 0.0
                    a *= (pattern[0] + (1 - pattern[0]) * cos_s) * (pattern[1] + (1 - pattern[1]) * cos_m)
                    tau = d * fs / c
                    for k in range(kr):
                        t = k - tau
                        if abs(t) < tw:
                            sinc = 1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)
                            h[k] += a * 0.5 * (1 + math.cos(math.pi * t / tw)) * sinc
    return h, kr


@pytest.mark.parametrize("N,n_taps,tw,pattern", [((1, 1, 1), 40, 5, (0.5, 0.25)), ((1, 0, 1), 57, 3, (0.0, 1.0)),
                                                 ((0, 1, 0), 64, 8, (0.75, 0.6))])
def test_model_is_the_defining_loop(N, n_taps, tw, pattern):
    room = np.array([1.1, 0.9, 1.3, 0.3, 0.5, 0.4, 0.8, 0.2, 0.9, 0.9, 0.7, 0.8, 0.6, 0.95, 0.5])
    orient = [0.3, -1.0, 0.4, -0.7, 0.2, 0.6]
    h, A, kr = DM.rir_dir_row(room, orient, pattern, n_taps, 64, N, FS, C, tw)
    want, kr_want = _naive(room, orient, pattern, n_taps, 64, N, FS, C, tw)
    assert kr == kr_want
    assert np.max(np.abs(want)) > 1e-3
    assert np.max(np.abs(h - want)) <= 1e-14 * np.max(A)
    assert not h[kr:].any()


def test_all_ones_patterns_are_the_omni_model_bit_for_bit():
    K = 700
    for orient in ([0.3, -1.0, 0.4, -0.7, 0.2, 0.6], [0.0] * 6, [1e100, -3e-7, 5.0, 0.0, 0.0, -1e-30]):
        h, A, kr = DM.rir_dir_row(ROOM, orient, (1.0, 1.0), K, K, N5, FS, C)
        h0, A0, kr0 = M.rir_row(ROOM, K, K, N5, FS, C)
        assert kr == kr0 and np.array_equal(h, h0) and np.array_equal(A, A0)
    # one end omni with a zero vector, the other directional: valid, and the band model agrees with one band and a delta
    h, A, kr = DM.rir_dir_row(ROOM, [0, 0, 0, 1, 2, 3], (1.0, 0.5), K, K, N5, FS, C)
    assert kr == K and not np.array_equal(h, h0)
    bands = np.array([ROOM[9:15] + [0.0]])
    hb, _, krb = DM.rir_bands_dir_row(ROOM, bands, [0, 0, 0, 1, 2, 3], [(1.0, 0.5)], K, K, N5, np.ones((1, 1)), FS, C)
    assert krb == K and np.max(np.abs(hb - h)) <= 1e-15 * np.max(A)
    hb1, _, _ = DM.rir_bands_dir_row(ROOM, bands, [5, 5, 5, 1, 2, 3], [(1.0, 1.0)], K, K, N5, np.ones((1, 1)), FS, C)
    assert np.array_equal(hb1, BM.rir_bands_row(ROOM, bands, K, K, N5, np.ones((1, 1)), FS, C)[0])


def test_reciprocity_with_vectors_and_patterns_swapped():
    K = 700
    u, v, a_s, a_m = [0.3, -1.0, 0.4], [-0.7, 0.2, 0.6], 0.5, 0.25
    swapped = ROOM[0:3] + ROOM[6:9] + ROOM[3:6] + ROOM[9:15]
    h1, A, _ = DM.rir_dir_row(ROOM, u + v, (a_s, a_m), K, K, N5, FS, C)
    h2, _, _ = DM.rir_dir_row(swapped, v + u, (a_m, a_s), K, K, N5, FS, C)
    worst = float(np.max(np.abs(h1 - h2) / np.where(A > 0, A, 1.0)))
    print(f"[rir_dir] reciprocity: max |h1 - h2| / A = {worst:.2e}")
    assert np.all(np.abs(h1 - h2) <= 4e-15 * A) and np.max(np.abs(h1)) > 0.01
    # and the response is far from the omni one: an omni kernel cannot pass for a directional one
    h0, A0, _ = M.rir_row(ROOM, K, K, N5, FS, C)
    assert np.max(np.abs(h1 - h0)) > 0.02 and np.max(np.abs(h0)) > 0.04
    assert np.max(np.abs(h1 - h0)) > 1e4 * np.max(DM.bound(h1, A, K, 40))


def test_anechoic_known_answers():
    room = [4.0, 5.0, 3.0, 1.0, 1.5, 1.2, 2.5, 3.0, 1.7] + [0.0] * 6
    s, m = np.array(room[3:6]), np.array(room[6:9])
    d = float(np.linalg.norm(m - s))
    K = int(d * FS / C) + 60
    h0, _, _ = M.rir_row(room, K, K, (0, 0, 0), FS, C)
    toward, away = list(m - s), list(s - m)
    # a cardioid source aimed at the receiver (mic omni): the omni direct path
    h, _, _ = DM.rir_dir_row(room, toward + [0, 0, 0], (0.5, 1.0), K, K, (0, 0, 0), FS, C)
    assert np.max(np.abs(h - h0)) <= 4e-16 * np.max(np.abs(h0)) and np.max(np.abs(h0)) > 0.5 / (4 * np.pi * d)
    # aimed away: the null (not asserted as exactly zero: cos is -1 only to rounding)
    h, _, _ = DM.rir_dir_row(room, away + [0, 0, 0], (0.5, 1.0), K, K, (0, 0, 0), FS, C)
    assert np.max(np.abs(h)) < 1e-15 / (4 * np.pi * d)
    # a cardioid microphone aimed at / away from the source, and a figure-of-eight seen from the side and from behind
    h, _, _ = DM.rir_dir_row(room, [0, 0, 0] + away, (1.0, 0.5), K, K, (0, 0, 0), FS, C)
    assert np.max(np.abs(h - h0)) <= 4e-16 * np.max(np.abs(h0))
    h, _, _ = DM.rir_dir_row(room, [0, 0, 0] + toward, (1.0, 0.5), K, K, (0, 0, 0), FS, C)
    assert np.max(np.abs(h)) < 1e-15 / (4 * np.pi * d)
    side = list(np.cross(m - s, [0.0, 0.0, 1.0]))
    h, _, _ = DM.rir_dir_row(room, side + [0, 0, 0], (0.0, 1.0), K, K, (0, 0, 0), FS, C)
    assert np.max(np.abs(h)) < 1e-15 / (4 * np.pi * d)
    h, _, _ = DM.rir_dir_row(room, away + [0, 0, 0], (0.0, 1.0), K, K, (0, 0, 0), FS, C)
    assert np.max(np.abs(h + h0)) <= 4e-16 * np.max(np.abs(h0))               # the rear lobe is negative
    # source on the receiver: cosines 0, amplitude alpha_s alpha_m / (4 pi DMIN)
    on = room[0:6] + room[3:6] + [0.0] * 6
    h, _, _ = DM.rir_dir_row(on, [1, 2, 3, -1, 0, 0], (0.5, 0.25), 50, 50, (0, 0, 0), FS, C)
    assert h[0] == 0.5 * 0.25 / (4 * np.pi * M.DMIN) and np.max(np.abs(h[1:])) < 1e-15 * h[0]   # (sin(pi k) is not 0)


def test_invalid_rows_of_the_model():
    ok = ([1, 0, 0, 0, 1, 0], [[0.5, 0.5]])
    assert DM.dirs_are_valid(*ok)
    assert DM.dirs_are_valid([0, 0, 0, 0, 0, 0], [[1.0, 1.0], [1.0, 1.0]]) and DM.dirs_are_valid([0, 0, 0, 0, 1, 0], [[1.0, 0.0]])
    for orient, pattern in (([np.nan, 0, 0, 0, 1, 0], ok[1]), ([1, 0, 0, 0, np.inf, 0], ok[1]), (ok[0], [[1.5, 0.5]]),
                            (ok[0], [[0.5, -0.1]]), (ok[0], [[np.nan, 0.5]]), ([0, 0, 0, 0, 1, 0], ok[1]),
                            ([1, 0, 0, 0, 0, 0], [[1.0, 1.0], [1.0, 0.5]]), ([1e200, 0, 0, 0, 1, 0], ok[1]),
                            ([1, 0, 0, 0, -1.1e100, 0], [[1.0, 1.0]])):
        assert not DM.dirs_are_valid(orient, pattern), (orient, pattern)
        if len(pattern) == 1:
            h, A, kr = DM.rir_dir_row(ROOM, orient, pattern[0], 100, 100, (1, 1, 1), FS, C)
            assert kr == 1 and not h.any() and not A.any()


# ------------------------------------------------------------------ RoomSampler
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_sampler_without_directivity_draws_what_it_drew():
    plain = RoomSampler(generator=_gen(5))
    same = RoomSampler(generator=_gen(5), source_pattern=None, facing_deg=(0.0, 180.0), mic_pattern=None, pattern_tilt=(0.0, 0.0))
    aimed = RoomSampler(generator=_gen(5), source_pattern=(0.25, 0.75), mic_pattern=(0.5, 1.0), facing_deg=(10.0, 20.0))
    assert not plain.directional and not same.directional and aimed.directional
    for s in (plain, same, aimed):
        s.rooms_drawn = s.draw(4, 3000, FS)
        s.src = s.draw_sources(s.rooms_drawn[0], 2)
        s.path = s.draw_path(s.src, 3, 0.5)
    for s in (same, aimed):                                        # the directivity options change no existing draw
        assert torch.equal(s.rooms_drawn[0], plain.rooms_drawn[0]) and torch.equal(s.rooms_drawn[1], plain.rooms_drawn[1])
        assert torch.equal(s.src, plain.src) and torch.equal(s.path, plain.path)
    assert torch.equal(same.generator.get_state(), plain.generator.get_state())
    for s in (plain, same):
        with pytest.raises(ValueError, match="no source_pattern or mic_pattern"):
            s.draw_dirs(s.rooms_drawn[0])
    state = aimed.generator.get_state()
    aimed.draw_dirs(aimed.rooms_drawn[0])
    want = _gen(0)
    want.set_state(state)
    torch.rand(4, 7, dtype=torch.float64, generator=want)                         # ONE rand, after every other draw
    assert torch.equal(aimed.generator.get_state(), want.get_state())


def _angle_deg(orient, tables):
    w = tables[..., 6:9] - tables[..., 3:6]
    w = w / torch.linalg.vector_norm(w, dim=-1, keepdim=True)
    return torch.rad2deg(torch.acos((orient[..., 0:3] * w).sum(-1).clamp(-1.0, 1.0)))


def test_draw_dirs_shapes_cone_and_sphere():
    s = RoomSampler(generator=_gen(7), source_pattern=(0.25, 0.75), mic_pattern=(0.5, 1.0), facing_deg=(30.0, 60.0))
    rooms, _ = s.draw(64, 3000, FS)
    orient, pattern = s.draw_dirs(rooms)
    assert tuple(orient.shape) == (64, 6) and tuple(pattern.shape) == (64, 1, 2)
    assert orient.dtype == pattern.dtype == torch.float64 and orient.is_contiguous() and pattern.is_contiguous()
    ang = _angle_deg(orient, rooms)
    assert float(ang.min()) >= 30.0 - 1e-6 and float(ang.max()) <= 60.0 + 1e-6 and float(ang.max() - ang.min()) > 10.0
    for part in (orient[:, 0:3], orient[:, 3:6]):
        assert torch.allclose(torch.linalg.vector_norm(part, dim=-1), torch.ones(64, dtype=torch.float64), atol=1e-14, rtol=0)
    assert float(orient[:, 3:6].mean(0).abs().max()) < 0.35 and float(orient[:, 5].min()) < -0.5 < 0.5 < float(orient[:, 5].max())
    assert float(pattern[:, 0, 0].min()) >= 0.25 and float(pattern[:, 0, 0].max()) <= 0.75
    assert float(pattern[:, 0, 1].min()) >= 0.5 and float(pattern[:, 0, 1].max()) <= 1.0
    # the azimuth spreads u around the cone: the components across the axis have no preferred side
    src = s.draw_sources(rooms, 3)
    orient, pattern = s.draw_dirs(src)
    assert tuple(orient.shape) == (64, 3, 6) and tuple(pattern.shape) == (64, 3, 1, 2)
    path = s.draw_path(src, 4, 1.0)
    orient, pattern = s.draw_dirs(path, path=True)
    assert tuple(orient.shape) == (64, 3, 4, 6) and tuple(pattern.shape) == (64, 3, 4, 1, 2)
    assert orient.is_contiguous() and pattern.is_contiguous()
    ang = _angle_deg(orient, path)
    assert torch.allclose(ang, ang[..., 0:1].expand_as(ang), atol=1e-6, rtol=0)       # the same angle at every waypoint ...
    assert not torch.equal(orient[..., 0, 0:3], orient[..., 3, 0:3])                  # ... around its own direction
    assert torch.equal(orient[..., 3:6], orient[..., 0:1, 3:6].expand(64, 3, 4, 3))   # the microphone does not turn
    assert torch.equal(pattern, pattern[..., 0:1, :, :].expand_as(pattern))
    orient, pattern = s.draw_dirs(s.draw_path(rooms, 2, 1.0), path=True)
    assert tuple(orient.shape) == (64, 2, 6) and tuple(pattern.shape) == (64, 2, 1, 2)
    # the fixed ends of the range, an override, and an omni end
    facing = RoomSampler(generator=_gen(1), source_pattern=(0.5, 0.5), facing_deg=(0.0, 0.0))
    orient, pattern = facing.draw_dirs(rooms)
    assert float(_angle_deg(orient, rooms).max()) < 1e-5 and torch.all(pattern[:, 0, 0] == 0.5) and torch.all(pattern[:, 0, 1] == 1.0)
    orient, _ = facing.draw_dirs(rooms, facing_deg=(180.0, 180.0))
    assert float(_angle_deg(orient, rooms).min()) > 180.0 - 1e-5
    # a source on the receiver has no direction to face: the x axis stands in, and the vectors stay finite units
    on = rooms.clone()
    on[:, 6:9] = on[:, 3:6]
    orient, _ = facing.draw_dirs(on)
    assert torch.equal(orient[:, 0:3], torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64).expand(64, 3))


def test_draw_dirs_tilts_the_source_pattern_over_the_bands_and_clamps():
    s = RoomSampler(generator=_gen(3), bands=7, source_pattern=(0.3, 0.3), mic_pattern=(0.6, 0.6), pattern_tilt=(0.2, 0.2))
    rooms, _ = s.draw(5, 3000, FS)
    _, pattern = s.draw_dirs(rooms)
    assert tuple(pattern.shape) == (5, 7, 2) and s.band_ref == 3
    want = np.clip(0.3 - 0.2 * (np.arange(7) - 3), 0.0, 1.0)                          # 0.9 0.7 0.5 0.3 0.1 0 (clamped) 0
    assert want[-1] == 0.0 and want[-2] == 0.0 and want[0] == pytest.approx(0.9)
    assert np.allclose(pattern[:, :, 0].numpy(), want[None, :], atol=1e-15, rtol=0)
    assert torch.all(pattern[:, :, 1] == 0.6)
    up = RoomSampler(generator=_gen(3), bands=3, source_pattern=(0.9, 0.9), pattern_tilt=(0.5, 0.5))       # b_ref = 2
    assert torch.equal(up.draw_dirs(rooms)[1][:, :, 0], torch.tensor([1.0, 1.0, 0.9], dtype=torch.float64).expand(5, 3))   # clamped at 1 too
    ranged = RoomSampler(generator=_gen(4), bands=4, source_pattern=(0.5, 0.5), pattern_tilt=(0.0, 0.1))
    p = ranged.draw_dirs(rooms)[1]
    slope = (p[:, 3, 0] - p[:, 2, 0])
    assert float(slope.min()) >= -0.1 - 1e-15 and float(slope.max()) <= 0.0 and float(slope.max() - slope.min()) > 0.0


def test_sampler_directivity_argument_rules():
    for kw, text in ((dict(source_pattern=(0.5, 1.5)), "source_pattern"), (dict(source_pattern=(-0.1, 0.5)), "source_pattern"),
                     (dict(source_pattern=(0.6, 0.5)), "source_pattern"), (dict(source_pattern=0.5), "source_pattern"),
                     (dict(mic_pattern=(0.0, 2.0)), "mic_pattern"), (dict(mic_pattern="ab"), "mic_pattern"),
                     (dict(source_pattern=(0.5, 0.5), facing_deg=(0.0, 181.0)), "facing_deg"),
                     (dict(source_pattern=(0.5, 0.5), facing_deg=(-1.0, 10.0)), "facing_deg"),
                     (dict(source_pattern=(0.5, 0.5), facing_deg=(20.0, 10.0)), "facing_deg"),
                     (dict(facing_deg=(0.0, 90.0)), "belong to directivity"), (dict(pattern_tilt=(0.0, 0.1)), "belong to directivity"),
                     (dict(source_pattern=(0.5, 0.5), pattern_tilt=(0.0, 0.1)), "bands=n and source_pattern"),
                     (dict(bands=3, mic_pattern=(0.5, 0.5), pattern_tilt=(0.0, 0.1)), "bands=n and source_pattern"),
                     (dict(bands=3, source_pattern=(0.5, 0.5), pattern_tilt=(0.0, math.inf)), "pattern_tilt")):
        with pytest.raises(ValueError, match=text):
            RoomSampler(**kw)
    s = RoomSampler(generator=_gen(2), mic_pattern=(0.5, 0.5))
    rooms, _ = s.draw(3, 100, FS)
    for bad, kw in ((rooms.float(), {}), (rooms[:, :14], {}), (rooms.numpy(), {}), (rooms, dict(path=True)),
                    (rooms[None, None, None], dict(path=True)), (rooms[None, None], {})):
        with pytest.raises(ValueError, match="tables must be"):
            s.draw_dirs(bad, **kw)
    with pytest.raises(ValueError, match="facing_deg"):
        s.draw_dirs(rooms, facing_deg=(0.0, 200.0))


# ------------------------------------------------------------------ the library
def test_exported_symbols_and_constants():
    lib = _lib.load()
    for name in ("cmgan_rir_dir", "cmgan_rir_dir_workspace_bytes", "cmgan_rir_bands_dir", "cmgan_rir_bands_dir_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.cmgan_abi_version() == _lib.ABI_VERSION >= 19


def test_header_declares_the_four_entry_points():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "cmgan_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|const char\*|void|cmgan_handle\*|float|double)\s+(cmgan_\w+)\(", header, re.M))
    assert {"cmgan_rir_dir", "cmgan_rir_dir_workspace_bytes", "cmgan_rir_bands_dir", "cmgan_rir_bands_dir_workspace_bytes"} <= declared
    assert re.search(r"#define CMGAN_ABI_VERSION (\d+)", header).group(1) == str(_lib.ABI_VERSION)


def test_workspace_bytes_monotone_and_rejects_unsupported_shapes():
    lib = _lib.load()
    ws = lambda R=4, K=8000, tw=40: int(lib.cmgan_rir_dir_workspace_bytes(None, R, K, tw))
    wb = lambda R=4, K=8000, tw=40, NB=7, NF=511: int(lib.cmgan_rir_bands_dir_workspace_bytes(None, R, K, tw, NB, NF))
    for fn, axes in ((ws, (("R", (1, 2, 5, 32, 65535)), ("K", (1, 2, 255, 256, 257, 8000, 65536)), ("tw", (1, 4, 40, 64)))),
                     (wb, (("R", (1, 2, 5, 32, 65535)), ("K", (1, 2, 255, 256, 257, 8000, 65536)), ("tw", (1, 4, 40, 64)),
                           ("NB", (1, 2, 3, 7, 8)), ("NF", (1, 3, 9, 511, 1023))))):
        for name, values in axes:
            prev = 0
            for v in values:
                got = fn(**{name: v})
                assert got >= max(prev, 1) and got % 256 == 0, (name, v)
                prev = got
    # the records are longer than the plain calls' by u, v and the alphas; the band responses are the same
    assert ws(32) >= int(lib.cmgan_rir_workspace_bytes(None, 32, 8000, 40)) + 32 * 8 * 8 - 256
    assert wb(32) >= int(lib.cmgan_rir_bands_workspace_bytes(None, 32, 8000, 40, 7, 511)) + 32 * 20 * 8 - 256
    assert wb(32) >= 32 * 7 * (8000 + 255) * 8
    for kw in (dict(R=0), dict(R=-1), dict(R=65536), dict(K=0), dict(K=-5), dict(K=65537), dict(tw=0), dict(tw=-1), dict(tw=65)):
        assert ws(**kw) == 0 and wb(**kw) == 0, kw
    for kw in (dict(NB=0), dict(NB=-2), dict(NB=9), dict(NF=0), dict(NF=-1), dict(NF=2), dict(NF=510), dict(NF=1024), dict(NF=1025)):
        assert wb(**kw) == 0, kw


ORDER = ("h", "rooms", "orient", "pattern", "n_taps", "R", "K", "fs", "c", "tw", "Nx", "Ny", "Nz", "rir", "ld", "len", "ws",
         "ws_bytes", "stream")
ORDER_BANDS = ("h", "rooms", "bands", "orient", "pattern", "n_taps", "R", "K", "NB", "filt", "NF", "fs", "c", "tw", "Nx", "Ny",
               "Nz", "rir", "ld", "len", "ws", "ws_bytes", "stream")


def _call(banded, **over):
    """cmgan_rir_dir / cmgan_rir_bands_dir with plausible, aligned, never-dereferenced pointers: every error is raised
    before any is followed."""
    p = 0x10000
    a = dict(h=None, rooms=p, bands=p, orient=p, pattern=p, n_taps=p, R=2, K=100, NB=3, filt=p, NF=9, fs=16000, c=343.0, tw=40,
             Nx=3, Ny=3, Nz=3, rir=p, ld=100, len=p, ws=p, ws_bytes=1 << 30, stream=None)
    a.update(over)
    lib = _lib.load()
    if banded:
        rc = lib.cmgan_rir_bands_dir(*[a[k] for k in ORDER_BANDS])
    else:
        rc = lib.cmgan_rir_dir(*[a[k] for k in ORDER])
    return rc, lib.cmgan_last_error(None).decode()


COMMON_ERRORS = [
    (dict(rooms=None), BADARG, "null pointer"), (dict(orient=None), BADARG, "null pointer"), (dict(pattern=None), BADARG, "null pointer"),
    (dict(n_taps=None), BADARG, "null pointer"), (dict(rir=None), BADARG, "null pointer"), (dict(len=None), BADARG, "null pointer"),
    (dict(rooms=0x10004), BADARG, "8-byte aligned"), (dict(orient=0x10004), BADARG, "orient and pattern tables must be 8-byte aligned"),
    (dict(pattern=0x10004), BADARG, "orient and pattern tables must be 8-byte aligned"),
    (dict(n_taps=0x10002), BADARG, "4-byte aligned"), (dict(rir=0x10001), BADARG, "4-byte aligned"), (dict(len=0x10002), BADARG, "4-byte aligned"),
    (dict(R=0), BADARG, "R=0"), (dict(R=-3), BADARG, "R=-3"), (dict(R=65536), BADARG, "R=65536"),
    (dict(K=0), BADARG, "K=0"), (dict(ld=99), BADARG, "ld=99"),
    (dict(fs=0), BADARG, "fs=0"), (dict(fs=-16000), BADARG, "fs=-16000"),
    (dict(c=0.0), BADARG, "speed of sound"), (dict(c=-343.0), BADARG, "speed of sound"),
    (dict(c=float("nan")), BADARG, "speed of sound"), (dict(c=float("inf")), BADARG, "speed of sound"),
    (dict(tw=0), BADARG, "tw=0"), (dict(tw=-1), BADARG, "tw=-1"), (dict(tw=65), UNSUPPORTED, "tw=65"),
    (dict(Nx=-1), BADARG, "Nx=-1"), (dict(Ny=-1), BADARG, "Ny=-1"), (dict(Nz=-1), BADARG, "Nz=-1"),
    (dict(Nx=256), UNSUPPORTED, "Nx=256"), (dict(Ny=256), UNSUPPORTED, "Ny=256"), (dict(Nz=256), UNSUPPORTED, "Nz=256"),
    (dict(K=65537, ld=65537), UNSUPPORTED, "65536 taps"),
    (dict(), BADARG, "null handle"),                              # everything valid: only now is the handle missed
    (dict(Nx=0, Ny=0, Nz=0, K=65536, ld=65536, R=65535, tw=64), BADARG, "null handle"),
    (dict(Nx=255, Ny=255, Nz=200), BADARG, "null handle"),
]
BAND_ERRORS = [
    (dict(bands=None), BADARG, "null pointer"), (dict(filt=None), BADARG, "null pointer"),
    (dict(bands=0x10004), BADARG, "8-byte aligned"), (dict(filt=0x10004), BADARG, "8-byte aligned"),
    (dict(NB=0), BADARG, "NB=0"), (dict(NB=-1), BADARG, "NB=-1"), (dict(NB=9), BADARG, "NB=9"),
    (dict(NF=0), BADARG, "NF=0"), (dict(NF=-3), BADARG, "NF=-3"), (dict(NF=8), BADARG, "NF=8"), (dict(NF=1024), BADARG, "NF=1024"),
    (dict(NF=1025), UNSUPPORTED, "NF=1025"),
    (dict(NB=8, NF=1023), BADARG, "null handle"), (dict(NB=1, NF=1), BADARG, "null handle"),
]


@pytest.mark.parametrize("over,code,text", COMMON_ERRORS)
def test_abi_argument_errors_of_rir_dir_without_gpu(over, code, text):
    rc, msg = _call(False, **over)
    assert rc == code, (rc, msg)
    assert "cmgan_rir_dir:" in msg and text in msg, msg


@pytest.mark.parametrize("over,code,text", COMMON_ERRORS + BAND_ERRORS)
def test_abi_argument_errors_of_rir_bands_dir_without_gpu(over, code, text):
    rc, msg = _call(True, **over)
    assert rc == code, (rc, msg)
    assert "cmgan_rir_bands_dir:" in msg and text in msg, msg


# ------------------------------------------------------------------ argument errors of Engine.rir / rir_bands, on CPU tensors
def test_engine_directivity_argument_rules_without_gpu():
    cpu, f64 = torch.device("cpu"), dict(dtype=torch.float64)
    orient, pattern = torch.ones(3, 6, **f64), torch.ones(3, 4, 2, **f64)
    assert check_rir_dir_args(cpu, 3, 4, None, None) == (None, None)
    o, p = check_rir_dir_args(cpu, 3, 4, orient, pattern)
    assert o is orient and p.data_ptr() == pattern.data_ptr() and tuple(p.shape) == (3, 4, 2)
    o, p = check_rir_dir_args(cpu, 3, 1, orient, torch.ones(3, 2, **f64))               # [R, 2] for [R, 1, 2]
    assert tuple(p.shape) == (3, 1, 2)
    assert tuple(check_rir_dir_args(cpu, 3, 1, orient, torch.ones(3, 1, 2, **f64))[1].shape) == (3, 1, 2)
    cases = [
        (dict(orient=None), ValueError, "orient and pattern go together: orient is missing"),
        (dict(pattern=None), ValueError, "orient and pattern go together: pattern is missing"),
        (dict(orient=torch.ones(3, 6)), TypeError, "orient"), (dict(orient=np.ones((3, 6))), TypeError, "orient"),
        (dict(orient=torch.ones(3, 5, **f64)), ValueError, "orient"), (dict(orient=torch.ones(2, 6, **f64)), ValueError, "orient"),
        (dict(orient=torch.ones(18, **f64)), ValueError, "orient"), (dict(orient=torch.ones(6, 3, **f64).t()), ValueError, "contiguous"),
        (dict(pattern=torch.ones(3, 4, 2)), TypeError, "pattern"), (dict(pattern=torch.ones(3, 3, 2, **f64)), ValueError, "pattern"),
        (dict(pattern=torch.ones(3, 2, **f64)), ValueError, "pattern"),                # [R, 2] only where NB = 1
        (dict(pattern=torch.ones(3, 4, 3, **f64)), ValueError, "pattern"), (dict(pattern=torch.ones(2, 4, 2, **f64)), ValueError, "pattern"),
        (dict(pattern=torch.ones(3, 2, 4, **f64).transpose(1, 2)), ValueError, "contiguous"),
    ]
    for over, exc, text in cases:
        a = dict(orient=orient, pattern=pattern)
        a.update(over)
        with pytest.raises(exc, match=text):
            check_rir_dir_args(cpu, 3, 4, a["orient"], a["pattern"])
    with pytest.raises(RuntimeError, match="bound to"):
        check_rir_dir_args(torch.device("meta"), 3, 4, orient, pattern)
    # Engine.rir and Engine.rir_bands take the keywords
    import inspect
    from cmgan_amd.engine import Engine
    for fn in (Engine.rir, Engine.rir_bands):
        params = inspect.signature(fn).parameters
        assert params["orient"].default is None and params["pattern"].default is None
