"""CPU side of the room simulator (cmgan_amd/csrc/rir.hip; include/cmgan_hip.h, "Room impulse responses"): the float64
model the GPU tests compare the kernels with (tests/rir_model.py) against known answers and against its own definition
as a naive loop, the room sampler and Sabine's formula, the workspace formula, and every argument error of cmgan_rir,
Engine.rir and DynamicMixer(rooms=...), all of which are judged before a handle or a GPU is needed."""
import math

import numpy as np
import pytest
import torch

import rir_model as M
from cmgan_amd import _lib
from cmgan_amd.engine import RIR_MAX_TAPS, check_rir_args
from cmgan_amd.mixing import DynamicMixer, NoiseBank, RirBank, RoomSampler, sabine_beta

BADARG, UNSUPPORTED = -1, -3
FS, C = 16000, 343.0


# ------------------------------------------------------------------ the model
def test_model_anechoic_known_answer():
    """All walls absorb everything: the one image left is the direct path, 3.43 m = exactly 160 samples away."""
    room = [4, 5, 3, 0.5, 1, 1, 3.93, 1, 1, 0, 0, 0, 0, 0, 0]
    h, A, kr = M.rir_row(room, 400, 400, (1, 1, 1), FS, C, 40)
    assert kr == 400
    assert abs(h[160] * 4 * np.pi * 3.43 - 1.0) <= 1e-15
    rest = np.delete(h, 160)
    assert np.max(np.abs(rest)) < 1e-17
    assert abs(A[160] * 4 * np.pi * 3.43 - 1.0) <= 1e-15 and A[160 + 40] == 0.0 and A[160 + 39] > 0.0


RECIPROCITY_ROOM = [2.5, 2.0, 2.2, 0.7, 0.9, 1.1, 1.9, 0.6, 1.4, 0.9, 0.8, 0.85, 0.7, 0.6, 0.95]


def test_model_reciprocity():
    """Swapping source and receiver maps the image set onto itself with the same distances and amplitudes."""
    room = np.array(RECIPROCITY_ROOM)
    swapped = room.copy()
    swapped[3:6], swapped[6:9] = room[6:9], room[3:6]
    d, _ = M.images(room, (5, 5, 5))
    assert int(np.sum(d * FS / C - 40 < 700)) == 1521            # the images that reach the response
    h1, A1, _ = M.rir_row(room, 700, 700, (5, 5, 5), FS, C, 40)
    h2, A2, _ = M.rir_row(swapped, 700, 700, (5, 5, 5), FS, C, 40)
    assert np.max(np.abs(h1)) > 0.01
    assert np.all(np.abs(h1 - h2) <= 4e-15 * A1)
    assert np.all(np.abs(h1 - h2) <= M.bound(h1, A1, 700, 40))
    assert np.allclose(A1, A2, rtol=1e-12, atol=0)


def _naive(room, n_taps, K, N, fs, c, tw):
    L, s, m, b = room[0:3], room[3:6], room[6:9], room[9:15]
    kr = min(max(n_taps, 1), K)
    h, A = np.zeros(K), np.zeros(K)
    for nx in range(-N[0], N[0] + 1):
        for ny in range(-N[1], N[1] + 1):
            for nz in range(-N[2], N[2] + 1):
                n = (nx, ny, nz)
                for p in np.ndindex(2, 2, 2):
                    off = [(1 - 2 * p[i]) * s[i] + 2 * n[i] * L[i] - m[i] for i in range(3)]
                    d = math.sqrt(sum(o * o for o in off))
                    tau = d * fs / c
                    a = 1.0
                    for i in range(3):
                        a *= b[2 * i] ** abs(n[i] - p[i]) * b[2 * i + 1] ** abs(n[i])
                    a /= 4 * math.pi * max(d, M.DMIN)
                    for k in range(kr):
                        t = k - tau
                        if abs(t) < tw:
                            sinc = 1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)
                            h[k] += a * 0.5 * (1 + math.cos(math.pi * t / tw)) * sinc
                            A[k] += abs(a)
    return h, A, kr


@pytest.mark.parametrize("N,n_taps,tw", [((1, 2, 1), 60, 5), ((2, 1, 0), 37, 3), ((0, 0, 0), 90, 8)])
def test_model_is_the_defining_triple_loop(N, n_taps, tw):
    room = np.array([1.1, 0.9, 1.3, 0.3, 0.5, 0.4, 0.8, 0.2, 0.9, 0.9, 0.0, 0.7, 0.8, 1.0, 0.6])
    K = 64
    h, A, kr = M.rir_row(room, n_taps, K, N, 8000, C, tw)
    hn, An, krn = _naive(room, n_taps, K, N, 8000, C, tw)
    assert kr == krn == min(n_taps, K)
    assert np.max(np.abs(hn)) > 0.05
    assert np.allclose(h, hn, rtol=0, atol=1e-15 * np.max(An))
    assert np.allclose(A, An, rtol=1e-13, atol=0)
    assert np.all(h[kr:] == 0.0) and np.all(A[kr:] == 0.0)


def test_model_invalid_rows_and_length_clamp():
    good = np.array(RECIPROCITY_ROOM)
    for at, v in [(0, np.nan), (4, np.inf), (1, -2.0), (2, 0.0), (9, 1.5), (14, -0.1)]:
        room = good.copy()
        room[at] = v
        h, A, kr = M.rir_row(room, 50, 64, (1, 1, 1))
        assert kr == 1 and not h.any() and not A.any()
    assert M.rir_row(good, 0, 64, (1, 1, 1))[2] == 1 and M.rir_row(good, -7, 64, (1, 1, 1))[2] == 1
    assert M.rir_row(good, 1000, 64, (1, 1, 1))[2] == 64
    hs, As, ls = M.rir(np.stack([good, good]), [64, 10], 64, (1, 1, 1))
    assert hs.shape == As.shape == (2, 64) and ls.dtype == np.int32 and ls.tolist() == [64, 10]
    assert np.array_equal(hs[1, :10], hs[0, :10]) and not hs[1, 10:].any()


# ------------------------------------------------------------------ rooms
def test_sabine_beta_known_answer():
    beta = sabine_beta(0.5, [5.0, 4.0, 3.0])                      # V = 60 m^3, S = 94 m^2
    assert abs(float(1 - beta ** 2) - 0.20553) < 5e-6 and abs(float(beta) - 0.89133) < 5e-6
    dims = torch.tensor([[5.0, 4.0, 3.0], [3.0, 3.0, 2.5], [10.0, 8.0, 4.0]], dtype=torch.float64)
    rt = torch.tensor([0.5, 0.01, 1e9], dtype=torch.float64)
    b = sabine_beta(rt, dims)
    assert b.shape == (3,) and b.dtype == torch.float64
    assert abs(float(b[0]) - float(beta)) < 1e-15
    assert float(b[1]) == 0.0                                     # alpha clamped to 1: a dead room, not a NaN
    assert 1.0 - 1e-6 < float(b[2]) <= 1.0


def test_n_images_is_the_lower_bound_arithmetic():
    s = RoomSampler(dims=((3.0, 4.0, 2.5), (10.0, 8.0, 4.0)))
    K, tw = 8000, 40
    reach = (K + tw) * 343.0 / 16000                              # metres a K-tap response can see
    want = tuple(math.ceil(reach / (2 * l)) + 1 for l in (3.0, 4.0, 2.5))
    assert s.n_images(K, 16000) == s.n_images(K, 16000, 343.0, 40) == want == (30, 23, 36)
    assert s.n_images(100, 16000, 343.0, 4) == (2, 2, 2)
    # enough: an image with |n| = N + 1 on an axis lies at least 2 N Lmin > reach away, whatever the room and positions
    assert all(2 * n * l > reach for n, l in zip(want, (3.0, 4.0, 2.5)))


def test_room_sampler_draws_on_the_cpu_device():
    lo, hi, margin = (3.0, 3.0, 2.5), (10.0, 8.0, 4.0), 0.5
    s = RoomSampler((lo, hi), rt60=(0.2, 0.8), margin=margin, generator=torch.Generator().manual_seed(7))
    R, K, fs = 500, 8000, 16000
    rooms, n_taps = s.draw(R, K, fs)
    assert rooms.shape == (R, 15) and rooms.dtype == torch.float64 and rooms.is_contiguous()
    assert n_taps.shape == (R,) and n_taps.dtype == torch.int32
    size, src, rcv, beta = rooms[:, 0:3], rooms[:, 3:6], rooms[:, 6:9], rooms[:, 9:15]
    assert bool(((size >= torch.tensor(lo)) & (size <= torch.tensor(hi))).all())
    for pos in (src, rcv):
        assert bool(((pos >= margin) & (pos <= size - margin)).all())
    assert not torch.equal(src, rcv)
    assert bool((beta == beta[:, :1]).all()) and bool(((beta >= 0) & (beta <= 1)).all())
    # n_taps = min(K, ceil(rt60 fs)) with rt60 recovered from beta by Sabine's formula
    V = size.prod(1)
    S = 2 * (size[:, 0] * size[:, 1] + size[:, 1] * size[:, 2] + size[:, 0] * size[:, 2])
    rt = 0.161 * V / (S * (1 - beta[:, 0] ** 2))
    assert bool(((rt > 0.2 - 1e-9) & (rt < 0.8 + 1e-9)).all())
    want = torch.clamp(torch.ceil(rt * fs), max=K)
    assert bool(((n_taps - want).abs() <= 1).all())               # (1: rt60 went through beta and back)
    assert int(n_taps.max()) == K and int(n_taps.min()) >= int(0.2 * fs)
    assert all(M.row_is_valid(r) for r in rooms.numpy())
    # the same seed gives the same draws, another seed does not
    s2 = RoomSampler((lo, hi), rt60=(0.2, 0.8), margin=margin, generator=torch.Generator().manual_seed(7))
    r2, n2 = s2.draw(R, K, fs)
    assert torch.equal(rooms, r2) and torch.equal(n_taps, n2)
    r3, _ = s2.draw(R, K, fs)
    assert not torch.equal(rooms, r3)


def test_room_sampler_argument_rules():
    with pytest.raises(ValueError, match="margin"):
        RoomSampler(dims=((3, 3, 2.5), (10, 8, 4)), margin=1.25)             # the smallest room is 2.5 m high
    with pytest.raises(ValueError, match="margin"):
        RoomSampler(margin=-0.1)
    RoomSampler(dims=((3, 3, 2.5), (10, 8, 4)), margin=1.2)
    with pytest.raises(ValueError, match="dims"):
        RoomSampler(dims=((3, 3, 0.0), (10, 8, 4)))
    with pytest.raises(ValueError, match="dims"):
        RoomSampler(dims=((3, 3, 5.0), (10, 8, 4)))
    with pytest.raises(ValueError, match="dims"):
        RoomSampler(dims=((3, 3), (10, 8)))
    with pytest.raises(ValueError, match="rt60"):
        RoomSampler(rt60=(0.0, 0.5))
    with pytest.raises(ValueError, match="rt60"):
        RoomSampler(rt60=(0.6, 0.5))


# ------------------------------------------------------------------ the library
def test_exported_symbols_and_constants():
    lib = _lib.load()
    for name in ("cmgan_rir", "cmgan_rir_workspace_bytes", "cmgan_rir_tile", "cmgan_rir_list_capacity"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    tile, cap = lib.cmgan_rir_tile(), lib.cmgan_rir_list_capacity()
    assert tile > 0 and tile % 64 == 0 and cap >= tile
    assert lib.cmgan_abi_version() == _lib.ABI_VERSION >= 8


def test_workspace_bytes_monotone_and_rejects_unsupported_shapes():
    lib = _lib.load()
    ws = lambda R, K, tw: int(lib.cmgan_rir_workspace_bytes(None, R, K, tw))
    base = ws(1, 1, 1)
    assert base > 0 and base % 256 == 0
    prev = 0
    for R in (1, 2, 5, 32, 65535):
        assert ws(R, 8000, 40) >= max(prev, 1)
        prev = ws(R, 8000, 40)
    prev = 0
    for K in (1, 2, 255, 256, 257, 8000, 65536):
        assert ws(4, K, 40) >= max(prev, 1)
        prev = ws(4, K, 40)
    prev = 0
    for tw in (1, 4, 40, 64):
        assert ws(4, 8000, tw) >= max(prev, 1)
        prev = ws(4, 8000, tw)
    for R, K, tw in [(0, 10, 4), (-1, 10, 4), (65536, 10, 4), (1, 0, 4), (1, -5, 4), (1, 65537, 4), (1, 10, 0), (1, 10, -1),
                     (1, 10, 65)]:
        assert ws(R, K, tw) == 0, (R, K, tw)


def _call(**over):
    """cmgan_rir with plausible, aligned, never-dereferenced pointers: every error is raised before any is followed."""
    p = 0x10000
    a = dict(h=None, rooms=p, n_taps=p, R=2, K=100, fs=16000, c=343.0, tw=40, Nx=3, Ny=3, Nz=3, rir=p, ld=100, len=p, ws=p,
             ws_bytes=1 << 30, stream=None)
    a.update(over)
    lib = _lib.load()
    rc = lib.cmgan_rir(*[a[k] for k in ("h", "rooms", "n_taps", "R", "K", "fs", "c", "tw", "Nx", "Ny", "Nz", "rir", "ld",
                                        "len", "ws", "ws_bytes", "stream")])
    return rc, lib.cmgan_last_error(None).decode()


@pytest.mark.parametrize("over,code,text", [
    (dict(rooms=None), BADARG, "null pointer"), (dict(n_taps=None), BADARG, "null pointer"),
    (dict(rir=None), BADARG, "null pointer"), (dict(len=None), BADARG, "null pointer"),
    (dict(rooms=0x10004), BADARG, "8-byte aligned"), (dict(n_taps=0x10002), BADARG, "4-byte aligned"),
    (dict(rir=0x10001), BADARG, "4-byte aligned"), (dict(len=0x10002), BADARG, "4-byte aligned"),
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
    (dict(Nx=255, Ny=255, Nz=255), BADARG, "null handle"),        # 8 * 511^3 = 1 067 462 648 < 2^31: the largest range fits
])
def test_abi_argument_errors_without_gpu(over, code, text):
    rc, msg = _call(**over)
    assert rc == code, (rc, msg)
    assert text in msg, msg


# ------------------------------------------------------------------ argument errors of Engine.rir, on CPU tensors
def _args(R=3, K=50):
    return dict(rooms=torch.ones(R, 15, dtype=torch.float64), n_taps=torch.ones(R, dtype=torch.int32), K=K,
                n_images=(2, 3, 4))


def test_engine_rir_argument_rules_without_gpu():
    cpu = torch.device("cpu")
    assert check_rir_args(cpu, **_args()) == (3, 50, (2, 3, 4))
    out = (torch.zeros(3, 50), torch.zeros(3, dtype=torch.int32))
    assert check_rir_args(cpu, **_args(), out=out) == (3, 50, (2, 3, 4))
    cases = [
        (dict(rooms=torch.ones(3, 15)), TypeError, "rooms"), (dict(rooms=np.ones((3, 15))), TypeError, "rooms"),
        (dict(rooms=torch.ones(3, 14, dtype=torch.float64)), ValueError, "rooms"),
        (dict(rooms=torch.ones(15, dtype=torch.float64)), ValueError, "rooms"),
        (dict(rooms=torch.ones(0, 15, dtype=torch.float64)), ValueError, "rooms"),
        (dict(rooms=torch.ones(15, 3, dtype=torch.float64).t()), ValueError, "contiguous"),
        (dict(n_taps=torch.ones(3, dtype=torch.int64)), TypeError, "n_taps"),
        (dict(n_taps=torch.ones(4, dtype=torch.int32)), ValueError, "n_taps"),
        (dict(K=0), ValueError, "K"), (dict(K=RIR_MAX_TAPS + 1), ValueError, "K"), (dict(K=10.5), ValueError, "K"),
        (dict(n_images=(2, 3)), ValueError, "n_images"), (dict(n_images=5), ValueError, "n_images"),
        (dict(n_images=(2, -1, 3)), ValueError, "n_images"), (dict(n_images=(2, 256, 3)), ValueError, "n_images"),
        (dict(n_images=(1.5, 2, 3)), ValueError, "n_images"),
        (dict(fs=0), ValueError, "fs"), (dict(fs=16000.5), ValueError, "fs"),
        (dict(c=0.0), ValueError, "c must"), (dict(c=float("inf")), ValueError, "c must"), (dict(c=float("nan")), ValueError, "c must"),
        (dict(tw=0), ValueError, "tw"), (dict(tw=65), ValueError, "tw"), (dict(tw=4.5), ValueError, "tw"),
        (dict(out=torch.zeros(3, 50)), ValueError, "out"),
        (dict(out=(torch.zeros(3, 49), torch.zeros(3, dtype=torch.int32))), ValueError, r"out\[0\]"),
        (dict(out=(torch.zeros(3, 50, dtype=torch.float64), torch.zeros(3, dtype=torch.int32))), TypeError, r"out\[0\]"),
        (dict(out=(torch.zeros(3, 50), torch.zeros(3, dtype=torch.int64))), TypeError, r"out\[1\]"),
        (dict(out=(torch.zeros(3, 100)[:, :50], torch.zeros(3, dtype=torch.int32))), ValueError, "contiguous"),
    ]
    for over, exc, text in cases:
        a = _args()
        a.update(over)
        with pytest.raises(exc, match=text):
            check_rir_args(cpu, **a)
    with pytest.raises(RuntimeError, match="bound to"):
        check_rir_args(torch.device("meta"), **_args())


class _NoEngine:
    device = torch.device("cpu")


def test_dynamic_mixer_rooms_argument_rules_without_gpu():
    noise = NoiseBank.from_arrays([np.ones(10)])
    sampler = RoomSampler()
    m = DynamicMixer(_NoEngine(), noise, rooms=sampler, rir_seconds=0.25, p_reverb=0.5)
    assert m.rir_taps == 4000 and m.n_images == sampler.n_images(4000, 16000) and m.rir_bank is None
    with pytest.raises(ValueError, match="either a rir_bank or rooms"):
        DynamicMixer(_NoEngine(), noise, RirBank.from_arrays([[1.0, 0.5]]), rooms=sampler)
    with pytest.raises(ValueError, match="rir_seconds"):
        DynamicMixer(_NoEngine(), noise, rooms=sampler, rir_seconds=0.0)
    with pytest.raises(ValueError, match="rir_seconds"):
        DynamicMixer(_NoEngine(), noise, rooms=sampler, rir_seconds=5.0)
    with pytest.raises(ValueError, match="image ranges"):
        DynamicMixer(_NoEngine(), noise, rooms=RoomSampler(dims=((0.5, 3, 3), (4, 4, 4)), margin=0.1), rir_seconds=1.0)
    # the draw of a rooms mixer: one room per row, rir_index = arange(B) or B (the identity) for a dry row
    m.generator = torch.Generator().manual_seed(3)
    d = m.draw(64)
    assert d.rooms.shape == (64, 15) and d.rir_index.dtype == torch.int32 and d.rir_len.dtype == torch.int32
    dry = d.rir_index == 64
    assert 0 < int(dry.sum()) < 64
    assert torch.equal(d.rir_index[~dry], torch.arange(64, dtype=torch.int32)[~dry])
    assert bool((d.rir_len[dry] == 1).all()) and bool((d.rir_len[~dry] >= 3200).all()) and int(d.rir_len.max()) <= 4000
    # without rooms the draw has no table and the new field defaults to None
    assert DynamicMixer(_NoEngine(), noise).draw(4).rooms is None


# ------------------------------------------------------------------ the cases whose bits are recorded
def test_the_recorded_cases_are_not_trivial():
    """tests/rir_cases.py through the float64 model: what tests/golden/make_rir_bits.py asserts of the GPU's output."""
    import rir_cases as RC
    lib = _lib.load()
    T, cap = int(lib.cmgan_rir_tile()), int(lib.cmgan_rir_list_capacity())
    cases = RC.rir_cases(T)
    assert tuple(cases) == RC.RIR_NAMES
    for name, case in cases.items():
        h, length = RC.model(case)
        RC.nontrivial(name, case, h, length, T, cap)
