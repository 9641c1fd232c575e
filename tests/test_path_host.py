"""CPU side of the paths (cmgan_amd/csrc/scene.hip; include/cmgan_hip.h, "Paths"): the numpy model the GPU tests compare
the kernels with (tests/path_model.py) against facts that do not come from it, the condition on E for every row the GPU
tests judge, RoomSampler.draw_path, and every argument error of cmgan_scene_path, Engine.scene_path and
DynamicMixer(motion=, source_motion=), all of which are judged before a handle or a GPU is needed."""
import math

import numpy as np
import pytest
import torch

import path_model as M
import scene_model
from cmgan_amd import _lib
from cmgan_amd.engine import SCENE_MAX_WAYPOINTS, check_scene_path_args
from cmgan_amd.mixing import Draw, DynamicMixer, NoiseBank, PathDraw, RirBank, RoomSampler, SceneDraw

BADARG, UNSUPPORTED = -1, -3
CPU = torch.device("cpu")


# ------------------------------------------------------------------ the model against facts that are not its own
def test_the_forms_agree_with_a_naive_triple_loop():
    rng = np.random.default_rng(1)
    L, H, Pb, early = 23, 6, 3, 2
    hs = tuple(M.response(K, d, rng) for K, d in ((5, 0), (7, 3), (4, 1)))
    bank = rng.standard_normal(50).astype(np.float32)
    src = M.PathSource(3, 5, -2, np.float32(3.0), (M.response(4, 2, rng), M.response(6, 0, rng)))
    r = M.PathRowIn((0.1 * rng.standard_normal(L)).astype(np.float32), hs, H, None, None, bank, (src,), 100.0, early)

    def u(p, n, m):
        if (p == 0 and m <= 0) or (p == n - 1 and m >= p * H):
            return 1.0
        return max(H - abs(m - p * H), 0) / H

    speech, target, c = np.zeros(L), np.zeros(L), np.zeros(L)
    for i in range(L):
        for p, h in enumerate(hs):
            d = int(np.argmax(np.abs(h)))
            for k in range(len(h)):
                m = i + d - k
                if 0 <= m < L:
                    term = float(h[k]) * (u(p, Pb, m) * float(r.clean[m]))
                    speech[i] += term
                    if k <= d + early:
                        target[i] += term
        for p, h in enumerate(src.hs):
            for k in range(len(h)):
                m = i - k
                c[i] += float(h[k]) * (u(p, 2, m) * float(bank[3 + (m - 2) % 5]))
    for form in (M.direct, M.as_kernel, M.direct_ld):
        got = form(r)
        assert got["d"] == [0, 3, 1] and float(got["scale"]) == 1.0
        assert np.max(np.abs(got["speech"].astype(np.float64) - speech)) < 1e-15
        assert np.max(np.abs(got["target"].astype(np.float64) - target)) < 1e-15
        assert np.max(np.abs(got["c"][0].astype(np.float64) - c)) < 1e-15
    assert np.max(np.abs(target - speech)) > 1e-3 and np.max(np.abs(c)) > 1e-2


@pytest.mark.parametrize("H", [1, 2, 37, 1024, 1500, 2 ** 30])
def test_neighbouring_weights_sum_to_one_within_a_rounding(H):
    Pb = 4
    # around every waypoint, before the first and behind the last one, and 500 places in between
    near = (np.arange(Pb) * H)[:, None] + np.arange(-3, 4)[None, :]
    m = np.unique(np.concatenate([near.ravel(), np.random.default_rng(H).integers(0, 3 * H + 1, 500)]))
    u = np.stack([M.weights(p, Pb, H, m) for p in range(Pb)])
    assert u.dtype == np.float64 and np.all(u >= 0.0) and np.all(u <= 1.0)
    assert np.all((u > 0).sum(axis=0) <= 2)                                    # at most two waypoints meet a sample
    assert np.max(np.abs(u.sum(axis=0) - 1.0)) <= 2.0 ** -53
    for p in range(Pb):
        assert M.weights(p, Pb, H, [p * H])[0] == 1.0
        if p > 0:
            assert M.weights(p, Pb, H, [p * H - H])[0] == 0.0                  # the triangle ends at the neighbours
        if p < Pb - 1:
            assert M.weights(p, Pb, H, [p * H + H])[0] == 0.0
    assert np.all(M.weights(0, Pb, H, [-10 ** 12, -1, 0]) == 1.0) and np.all(M.weights(Pb - 1, Pb, H, [3 * H, 10 ** 12]) == 1.0)
    assert np.all(M.weights(0, 1, H, [-10 ** 9, 0, 1, H, 10 ** 9]) == 1.0)     # one waypoint: 1 everywhere
    if H > 2:                                                                  # the numerator is exact, the quotient one division
        assert M.weights(1, Pb, H, [H + 1])[0] == np.float64(H - 1) / np.float64(H)


def test_a_row_that_stands_still_is_the_scene_model_exactly():
    bt = M.build_batches(int(_lib.load().cmgan_mix_tile()))["htile"]
    one = bt._replace(n_path=np.ones_like(bt.n_path), src_n_path=np.ones_like(bt.src_n_path))
    st = M.static_batch(bt)
    for b in (0, 2, 5):
        for form, ref in ((M.direct, scene_model.direct), (M.as_kernel, scene_model.as_kernel)):
            got, want = form(M.row_of(one, b)), ref(scene_model.row_of(st, b))
            for key in ("noisy", "target", "speech"):
                assert np.array_equal(got[key], want[key]), (b, key)
            assert [float(v) for v in got["g"]] == [float(v) for v in want["g"]] and got["d"][0] == want["d"]
    # and a path changes the row: the registered one is not the static one
    assert not np.array_equal(M.direct(M.row_of(bt, 0))["noisy"], scene_model.direct(scene_model.row_of(st, 0))["noisy"])


def test_every_row_of_the_gpu_tests_respects_the_condition_on_E():
    """The rule |g - w| <= ulp32(w) / 2 + E may be used on a row only if E <= 2^-10 x ulp32(rms) / 2."""
    batches = M.build_batches(int(_lib.load().cmgan_mix_tile()))
    top, tight, rows = 0.0, 0.0, 0
    for name, bt in batches.items():
        for b in range(len(bt.clean)):
            sl, ld = M.case(name, b)
            for key in ("noisy", "target"):
                E, w = sl[key]
                bound = M.condition(w)
                assert len(w) == bt.clean.shape[1] and np.all(np.isfinite(w.astype(np.float64))), (name, b)
                assert E <= bound, f"{name} row {b} {key}: E = {E:.3e} above {bound:.3e}"
                top, tight = max(top, E), max(tight, E / bound)
            rows += 1
    assert rows == 36
    print(f"[path] {rows} rows: largest E {top:.3e}, at most {tight:.2e} of the bound")


def test_the_registered_batches_cover_the_walk():
    T = int(_lib.load().cmgan_mix_tile())
    bts = M.build_batches(T)
    long_L = 2 * T + T // 2 + 7
    assert {(bt.clean.shape[1], bt.H) for n, bt in bts.items() if n.startswith("h")} == {(T - 1, 37), (long_L, T), (long_L, 1500),
                                                                                        (T - 1, 4000)}
    assert sorted(bt.early for n, bt in bts.items() if n.startswith("h")) == [-1, 0, 200, 5000]
    for name in ("h37", "htile", "h1500", "hfar"):
        bt = bts[name]
        B, P = bt.rir_index.shape
        L = bt.clean.shape[1]
        assert B <= 6 and L <= long_L and bt.rir.shape[1] <= M.KBIG + 3 and P <= SCENE_MAX_WAYPOINTS
        assert bt.n_path.min() == 0 and bt.n_path.max() == P + 3 and (bt.n_path[1:-1] == 1).any()
        assert bt.src_n_path.max() == P + 3 and bt.src_n_path.min() == 0
        assert set(bt.rir_len[:, 0].tolist()) >= {1, 40, M.KBIG} and M.KBIG > scene_model.KC
        assert (bt.src_len == 1).any() and (bt.src_len == 3).any() and (bt.src_len == 0).any() and (bt.src_off < 0).any()
        assert bt.src_n_path[0, 1] < min(max(int(bt.n_path[0]), 1), P)             # a source path shorter than the talker's
        ds = M.case(name, 0)[1]["d"]
        assert set(ds[:3]) == {0, 5, 40}                                          # direct indices differ inside one path
    assert (28 - 1) * 37 < T - 1 and bts["h37"].rir_index.shape[1] == 28           # the last waypoint holds
    assert (5 - 1) * T - T >= long_L and bts["htile"].rir_index.shape[1] == 5      # column 4 is never reached
    assert bts["hfar"].H > bts["hfar"].clean.shape[1] and M.KBIG > T - 1            # K > L
    assert bts["hfar"].early >= M.KBIG


# ------------------------------------------------------------------ the library without a GPU
def test_symbols_and_abi():
    lib = _lib.load()
    for name in ("cmgan_scene_path", "cmgan_scene_path_workspace_bytes", "cmgan_scene_max_waypoints"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.cmgan_scene_max_waypoints() == SCENE_MAX_WAYPOINTS == 64
    assert lib.cmgan_abi_version() == _lib.ABI_VERSION >= 18


def test_workspace_bytes():
    lib = _lib.load()
    ws = lib.cmgan_scene_path_workspace_bytes
    assert ws(None, 0, 100, 1, 0, 1) == ws(None, 1, 0, 1, 0, 1) == ws(None, 1, 100, 0, 0, 1) == ws(None, 1, 100, 1, 5, 1) == 0
    assert ws(None, 1, 100, 1, 0, 0) == ws(None, 1, 100, 1, 0, 65) == ws(None, 1, 100, 65537, 0, 1) == 0
    base = ws(None, 4, 5000, 300, 2, 8)
    assert base > 0 and base % 256 == 0
    for B, L, K, S, P in ((5, 5000, 300, 2, 8), (4, 5001, 300, 2, 8), (4, 5000, 301, 2, 8), (4, 5000, 300, 3, 8),
                          (4, 5000, 300, 2, 9), (4, 5000, 300, 2, 64)):
        assert ws(None, B, L, K, S, P) >= base
    assert ws(None, 4, 5000, 300, 2, 64) > ws(None, 4, 5000, 300, 2, 1) >= lib.cmgan_scene_workspace_bytes(None, 4, 5000, 300, 2)
    assert ws(None, 4, 5000, 300, 2, 8) - lib.cmgan_scene_workspace_bytes(None, 4, 5000, 300, 2) >= 4 * 8 * 4      # d [B, P]


def _native(**over):
    """cmgan_scene_path with a NULL handle and plausible (never dereferenced) pointers: every argument error comes first."""
    a = dict(clean=4096, B=2, L=100, ld=100, noise_bank=4096, bank_len=10, noise_start=4096, noise_len=4096, noise_off=4096,
             snr_db=4096, src_bank=4096, src_bank_len=10, S=2, n_src=4096, src_start=4096, src_len=4096, src_off=4096,
             src_snr_db=4096, rir_bank=4096, R=3, Kmax=40, P=5, H=250, n_path=4096, rir_index=4096, rir_len=4096,
             src_n_path=4096, src_rir_index=4096, src_rir_len=4096, peak=0.99, early=-1, noisy=4096, target=4096, ld_out=100,
             g=4096, p=4096, ps=4096, scale=4096, ws=4096, ws_bytes=1 << 30, stream=None)
    a.update(over)
    lib = _lib.load()
    rc = lib.cmgan_scene_path(None, *a.values())
    return rc, (lib.cmgan_last_error(None) or b"").decode()


def test_native_argument_errors_come_before_the_handle():
    rc, msg = _native()
    assert rc == BADARG and "null handle" in msg
    need = int(_lib.load().cmgan_scene_path_workspace_bytes(None, 2, 100, 40, 2, 5))
    for over, code, word in (
            (dict(P=0), BADARG, "waypoints"), (dict(P=65), BADARG, "waypoints"), (dict(P=-1), BADARG, "waypoints"),
            (dict(H=0), BADARG, "hop"), (dict(H=-5), BADARG, "hop"), (dict(H=2 ** 30 + 1), BADARG, "hop"),
            (dict(rir_bank=None), BADARG, "a path needs a RIR bank"),
            (dict(n_path=None), BADARG, "n_path"), (dict(src_n_path=None), BADARG, "src_n_path"),
            (dict(rir_index=None), BADARG, "RIR bank needs"), (dict(src_rir_len=None), BADARG, "src_rir_index"),
            (dict(n_path=4098), BADARG, "4-byte"), (dict(src_n_path=4097), BADARG, "4-byte"), (dict(rir_index=4098), BADARG, "4-byte"),
            (dict(src_rir_index=4099), BADARG, "4-byte"), (dict(rir_len=4098), BADARG, "4-byte"),
            (dict(ws_bytes=need - 1), BADARG, "workspace"), (dict(ws_bytes=0), BADARG, "workspace"), (dict(ws=None), BADARG, "workspace"),
            (dict(ws=4096 + 64), BADARG, "workspace"),
            # and cmgan_scene's own
            (dict(clean=None), BADARG, "null pointer"), (dict(S=5), BADARG, "located sources"), (dict(B=0), BADARG, "need 0 < B"),
            (dict(early=-2), BADARG, "early"), (dict(peak=0.0), BADARG, "peak"), (dict(src_off=None), BADARG, "S > 0 needs"),
            (dict(Kmax=65537), UNSUPPORTED, "taps are supported"),
            (dict(L=2 ** 31 - 1, ld=2 ** 31, ld_out=2 ** 31), UNSUPPORTED, "samples are supported")):
        rc, msg = _native(**over)
        assert rc == code and msg.startswith("cmgan_scene_path: ") and word in msg, (over, rc, msg)
    # in order but for the handle: the limits themselves, no dry noise, no sources
    for over in (dict(P=1), dict(P=64), dict(H=1), dict(H=2 ** 30), dict(ws_bytes=need),
                 dict(noise_bank=None, noise_start=None, noise_len=None, noise_off=None, snr_db=None, bank_len=0),
                 dict(S=0, src_bank=None, n_src=None, src_start=None, src_len=None, src_off=None, src_snr_db=None,
                      src_n_path=None, src_rir_index=None, src_rir_len=None, src_bank_len=0)):
        rc, msg = _native(**over)
        assert rc == BADARG and "null handle" in msg, (over, msg)


# ------------------------------------------------------------------ Engine.scene_path's argument rules
class _NoNative:
    """An engine stand-in whose native side must never be reached."""
    device = CPU

    def __getattr__(self, name):
        raise AssertionError(f"the argument check let a call through to {name}")


def _args(B=3, L=50, S=2, R=4, K=20, P=5):
    f32, i64, i32 = torch.float32, torch.int64, torch.int32
    z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype)
    return dict(clean=z(B, L, dtype=f32), hop=10, n_path=z(B, dtype=i32), rir_bank=z(R, K, dtype=f32), rir_index=z(B, P, dtype=i32),
                rir_len=z(B, P, dtype=i32), noise_bank=z(100, dtype=f32), noise_start=z(B, dtype=i64), noise_len=z(B, dtype=i64),
                noise_off=z(B, dtype=i64), snr_db=z(B, dtype=f32), n_src=z(B, dtype=i32), src_bank=z(200, dtype=f32),
                src_start=z(B, S, dtype=i64), src_len=z(B, S, dtype=i64), src_off=z(B, S, dtype=i64),
                src_snr_db=z(B, S, dtype=f32), src_n_path=z(B, S, dtype=i32), src_rir_index=z(B, S, P, dtype=i32),
                src_rir_len=z(B, S, P, dtype=i32))


def test_check_scene_path_args():
    a = _args()
    assert check_scene_path_args(CPU, **a) == (3, 50, 4, 20, 2, 5)
    no_src = {k: (None if k.startswith("src_") or k == "n_src" else v) for k, v in a.items()}
    assert check_scene_path_args(CPU, **no_src) == (3, 50, 4, 20, 0, 5)
    f32, i64, i32 = torch.float32, torch.int64, torch.int32
    z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype)
    cases = [
        (dict(rir_bank=None), ValueError), (dict(rir_bank=z(4, 65537, dtype=f32)), ValueError), (dict(rir_bank=z(20, dtype=f32)), ValueError),
        (dict(hop=0), ValueError), (dict(hop=2 ** 30 + 1), ValueError), (dict(hop=2.5), ValueError), (dict(hop=True), ValueError),
        (dict(n_path=None), TypeError), (dict(n_path=z(3, dtype=i64)), TypeError), (dict(n_path=z(4, dtype=i32)), ValueError),
        (dict(rir_index=z(3, dtype=i32)), ValueError), (dict(rir_index=z(3, 65, dtype=i32)), ValueError),
        (dict(rir_index=z(3, 0, dtype=i32)), ValueError), (dict(rir_len=z(3, 4, dtype=i32)), ValueError),
        (dict(rir_len=z(3, 5, dtype=i64)), TypeError), (dict(rir_index=z(3, 10, dtype=i32)[:, ::2]), ValueError),
        (dict(src_n_path=None), ValueError), (dict(src_n_path=z(3, 3, dtype=i32)), ValueError),
        (dict(src_rir_index=z(3, 2, dtype=i32)), ValueError), (dict(src_rir_len=z(3, 2, 4, dtype=i32)), ValueError),
        (dict(src_rir_len=None), ValueError), (dict(src_rir_index=z(3, 2, 5, dtype=i64)), TypeError),
        (dict(clean=z(50, dtype=f32)), ValueError), (dict(noise_start=None), ValueError), (dict(src_off=None), ValueError),
        (dict(peak=0.0), ValueError), (dict(early=-2), ValueError)]
    for over, exc in cases:
        with pytest.raises(exc):
            check_scene_path_args(CPU, **{**a, **over})
    with pytest.raises(ValueError):
        check_scene_path_args(CPU, **{**no_src, "src_n_path": a["src_n_path"]})
    from cmgan_amd.engine import Engine
    for over, exc in cases:
        with pytest.raises(exc):
            Engine.scene_path.__wrapped__(_NoNative(), **{**a, **over})


# ------------------------------------------------------------------ draw_path
def test_draw_path_walks_a_segment_inside_the_room():
    gen = torch.Generator().manual_seed(3)
    sampler = RoomSampler(margin=0.4, generator=gen)
    rooms, n_taps = sampler.draw(40, 8000, 16000)
    state = gen.get_state()
    P, seconds, speed = 9, 2.0, (0.5, 1.5)
    path = sampler.draw_path(rooms, P, seconds, speed=speed)
    assert path.shape == (40, P, 15) and path.dtype == torch.float64 and path.is_contiguous()
    keep = [0, 1, 2, 6, 7, 8, 9, 10, 11, 12, 13, 14]
    assert torch.equal(path[:, :, keep], rooms[:, None, keep].expand(40, P, 12))            # size, receiver, coefficients
    assert torch.equal(path[:, 0, 3:6], rooms[:, 3:6])                                      # the start is the drawn source
    pos, size = path[:, :, 3:6], rooms[:, None, 0:3]
    assert bool((pos >= 0.4 - 1e-12).all()) and bool((pos <= size - 0.4 + 1e-12).all())
    step = pos[:, 1:] - pos[:, :-1]
    assert float((step - step[:, :1]).abs().max()) < 1e-12                                  # linearly spaced on a segment
    length = torch.linalg.vector_norm(pos[:, -1] - pos[:, 0], dim=-1)
    assert bool((length <= speed[1] * seconds + 1e-12).all()) and float(length.min()) > 0.0
    assert bool((length >= speed[0] * seconds - 1e-12).any())                               # some walks are cut to their speed
    # one rand(R, 4) from the sampler's generator, after the room draws: the same state gives the same path
    after = gen.get_state()
    gen.set_state(state)
    torch.rand(40, 4, dtype=torch.float64, generator=gen)
    assert torch.equal(gen.get_state(), after)
    gen.set_state(state)
    assert torch.equal(sampler.draw_path(rooms, P, seconds, speed=speed), path)
    assert path.reshape(-1, 15).shape == (40 * P, 15)
    # the [R, n, 15] tables of draw_sources walk the same way
    src = sampler.draw_sources(rooms, 3)
    sp = sampler.draw_path(src, 4, 1.0, speed=(1.0, 1.0))
    assert sp.shape == (40, 3, 4, 15) and torch.equal(sp[:, :, 0], src)
    walk = torch.linalg.vector_norm(sp[:, :, -1, 3:6] - sp[:, :, 0, 3:6], dim=-1)
    assert bool((walk <= 1.0 + 1e-12).all())
    one = sampler.draw_path(rooms, 1, 2.0)
    assert one.shape == (40, 1, 15) and torch.equal(one[:, 0], rooms)
    for bad in (dict(P=0), dict(P=65), dict(P=2.5), dict(P=True), dict(seconds=0.0), dict(seconds=math.inf), dict(speed=(2.0, 1.0)),
                dict(speed=(-1.0, 1.0)), dict(speed=1.0)):
        kw = {**dict(P=3, seconds=1.0, speed=(0.5, 1.0)), **bad}
        with pytest.raises(ValueError):
            sampler.draw_path(rooms, kw["P"], kw["seconds"], speed=kw["speed"])
    with pytest.raises(ValueError):
        sampler.draw_path(rooms[:, :14], 3, 1.0)
    with pytest.raises(ValueError):
        sampler.draw_path(rooms.to(torch.float32), 3, 1.0)


# ------------------------------------------------------------------ the mixer's options
def test_dynamic_mixer_motion_argument_errors():
    class Eng:
        device = CPU
    nb = NoiseBank.from_arrays([np.ones(10, dtype=np.float32)])
    rb = RirBank.from_arrays([np.ones(4, dtype=np.float32)])
    rooms = RoomSampler()
    for args, kw in (((rb,), dict(motion=(0.5, 1.0))),                               # a bank of fixed responses cannot move
                     ((), dict(motion=(0.5, 1.0))),                                  # nor can no room at all
                     ((), dict(rooms=rooms, motion=(1.0, 0.5))), ((), dict(rooms=rooms, motion=(-1.0, 0.5))),
                     ((), dict(rooms=rooms, motion=1.0)), ((), dict(rooms=rooms, motion=(0.5, 1.0), p_motion=1.5)),
                     ((), dict(rooms=rooms, motion=(0.5, 1.0), motion_hop_ms=0.0)),
                     ((), dict(rooms=rooms, motion=(0.5, 1.0), motion_hop_ms=math.inf)),
                     ((), dict(rooms=rooms, source_motion=(0.5, 1.0))),              # no sources to move
                     ((), dict(rooms=rooms, sources=(1, 2), source_motion=(2.0, 1.0))),
                     ((rb,), dict(sources=(1, 2), source_motion=(0.5, 1.0)))):
        with pytest.raises(ValueError):
            DynamicMixer(Eng(), nb, *args, **kw)
    m = DynamicMixer(Eng(), nb, rooms=rooms, motion=(0.5, 1.5), p_motion=0.25, motion_hop_ms=100.0, sources=(1, 2),
                     source_motion=(0.0, 0.3))
    assert m.motion == (0.5, 1.5) and m.p_motion == 0.25 and m.motion_hop == 1600 and m.source_motion == (0.0, 0.3)
    still = DynamicMixer(Eng(), nb, rooms=rooms)
    assert still.motion is None and still.source_motion is None
    # the draws of a mixer that moves: SceneDraw's fields, then the paths; Draw and SceneDraw are what they were
    names = PathDraw._fields
    assert names[:len(SceneDraw._fields)] == SceneDraw._fields and names[len(SceneDraw._fields):] == ("path", "n_path", "src_path", "src_n_path")
    assert all(getattr(PathDraw(*(torch.zeros(1),) * 6), n) is None for n in names[6:])
    assert Draw._fields[-1] == "speed" and SceneDraw._fields[-1] == "src_rooms"
    # P = 1 + ceil((N - 1) / H) waypoints: more than 64 is refused when the batch arrives
    assert m.waypoints(32000) == 21 and m.waypoints(1) == 1 and m.waypoints(1601) == 2 and m.waypoints(1602) == 3
    with pytest.raises(ValueError):
        DynamicMixer(Eng(), nb, rooms=rooms, motion=(0.5, 1.0), motion_hop_ms=10.0).waypoints(32000)
