"""CPU side of the scenes (cmgan_amd/csrc/scene.hip; include/cmgan_hip.h, "Scenes"): the numpy model the GPU tests compare
the kernels with (tests/scene_model.py) against facts that do not come from it, the condition on E for every row the GPU
tests judge, RoomSampler.draw_sources, and every argument error of cmgan_scene, Engine.scene and
DynamicMixer(sources=, source_bank=, source_snr_db=, dry_noise=), all of which are judged before a handle or a GPU is
needed."""
import numpy as np
import pytest
import torch

import mix_model
import scene_model as M
from cmgan_amd import _lib
from cmgan_amd.engine import SCENE_MAX_SOURCES, check_scene_args
from cmgan_amd.mixing import Draw, DynamicMixer, NoiseBank, RoomSampler, SceneDraw

BADARG, UNSUPPORTED = -1, -3
CPU = torch.device("cpu")


def _row(seed=1, L=900, K=40, sources=(), dry=True, early=15, peak=0.99, snr=7.5):
    rng = np.random.default_rng(seed)
    bank = rng.standard_normal(3000).astype(np.float32)
    return M.RowIn((0.1 * rng.standard_normal(L)).astype(np.float32), M.rirs(1, K, rng)[0], bank if dry else None,
                   (100, 777, 12345, np.float32(snr)) if dry else None, bank, tuple(sources), peak, early)


# ------------------------------------------------------------------ the model against facts that are not its own
@pytest.mark.parametrize("early", [-1, 0, 15, 1000])
def test_without_sources_the_model_is_the_mix_model(early):
    for peak in (0.99, 0.05):
        r = _row(early=early, peak=peak)
        want = mix_model.mix_row(r.clean, r.noise_bank, *r.noise, h=r.h, peak=peak, early=early)
        got = M.direct(r)
        assert np.array_equal(got["noisy"], want["noisy"]) and np.array_equal(got["target"], want["target"])
        assert got["g"][0] == want["g"] and got["Ps"] == want["Ps"] and got["P"][0] == want["Pn"] and got["scale"] == want["scale"]
        assert (want["scale"] < 1.0) == (peak == 0.05)


def test_one_dry_source_is_the_noise_of_the_mix_model():
    r = _row(sources=[M.Source(100, 777, 12345, np.float32(7.5), np.ones(1, dtype=np.float32))], dry=False)
    want = mix_model.mix_row(r.clean, r.src_bank, 100, 777, 12345, np.float32(7.5), h=r.h, peak=r.peak, early=r.early)
    for got in (M.direct(r), M.direct(r._replace(sources=(r.sources[0]._replace(h=None),)))):
        assert np.array_equal(got["noisy"], want["noisy"]) and np.array_equal(got["target"], want["target"])
        assert got["g"][1] == want["g"] and got["P"][1] == want["Pn"] and got["g"][0] == 0.0 and got["P"][0] == 0.0


@pytest.mark.parametrize("length,off", [(1, 0), (7, -3), (123, 10 ** 9), (500, -10 ** 12)])
def test_a_source_is_periodic_and_loops_both_ways(length, off):
    h = M.rirs(1, 40, np.random.default_rng(3))[0]
    r = _row(L=1100, sources=[M.Source(50, length, off, np.float32(3.0), h)])
    c = M.as_kernel(r)["c"][0]
    assert np.array_equal(c[length:], c[:-length])                            # the same taps meet the same samples
    assert float(np.max(np.abs(M.direct(r)["c"][0] - c))) < 1e-13
    # sample 0 reaches BACK into the segment: c[0] = sum_k h[k] seg[-k], by hand
    seg = r.src_bank[50:50 + length].astype(np.float64)
    want = sum(float(h[k]) * seg[(off - k) % length] for k in range(40))
    assert abs(c[0] - want) < 1e-13 and (length == 1 or abs(c[0] - float(h[0]) * seg[off % length]) > 1e-6)
    # an offset is one of its residues: off and off mod length give the same bits
    same = M.as_kernel(r._replace(sources=(r.sources[0]._replace(off=off % length),)))
    assert np.array_equal(same["noisy"], M.as_kernel(r)["noisy"])


def test_a_source_keeps_its_delay():
    """The talker's direct path is removed, a source's is not: an impulse response [0 0 0 1] delays the segment by 3."""
    h = np.array([0, 0, 0, 1], dtype=np.float32)
    r = _row(L=300, K=1, sources=[M.Source(0, 3000, 10, np.float32(0.0), h)], dry=False)
    got = M.direct(r)
    assert np.array_equal(got["c"][0], r.src_bank[7:307].astype(np.float64))
    assert np.array_equal(M.direct(r._replace(h=h))["speech"], M.direct(r._replace(h=None))["speech"])


def test_a_source_at_plus_300_db_changes_no_bit():
    src = M.Source(5, 400, -6, np.float32(300.0), M.rirs(1, 40, np.random.default_rng(4))[0])
    for form in (M.direct, M.as_kernel, M.direct_ld):
        a, b = form(_row()), form(_row(sources=[src]))
        assert b["g"][1] > 0.0 and b["P"][1] > 0.0
        for key in ("noisy", "target"):
            assert np.array_equal(a[key].astype(np.float32).view(np.uint32), b[key].astype(np.float32).view(np.uint32))


def test_invalid_segments_are_silence_and_gains_meet_their_snr():
    good = M.Source(5, 400, -6, np.float32(4.0), None)
    r = _row(sources=[good, good._replace(length=0), good._replace(start=-1), good._replace(start=2999, length=2)], peak=100.0)
    got = M.direct(r)
    assert [float(g) > 0 for g in got["g"]] == [True, True, False, False, False] and got["P"][2] == got["P"][3] == got["P"][4] == 0
    assert abs(10 * np.log10(got["Ps"] / (got["g"][1] ** 2 * got["P"][1])) - 4.0) < 1e-9
    assert np.array_equal(got["noisy"], M.direct(r._replace(sources=(good,)))["noisy"])


def test_the_three_forms_agree_and_the_long_double_is_wider():
    bt = M.make_batch(9, 1300, n_src=[4], src_K=[[40, 1, 300, 0]], src_len=[[7, 1, 1300, 5000]], src_off=[[-1, 5, 10 ** 9, -77]])
    r = M.row_of(bt, 0)
    ld, a, k = M.direct_ld(r), M.direct(r), M.as_kernel(r)
    assert ld["noisy"].dtype == np.longdouble and a["noisy"].dtype == k["noisy"].dtype == np.float64
    for key in ("noisy", "target"):
        assert float(np.max(np.abs(a[key] - ld[key]))) < 1e-13 and float(np.max(np.abs(k[key] - ld[key]))) < 1e-13
    if np.finfo(np.longdouble).eps < 1e-18:
        assert float(np.max(np.abs(a["noisy"] - ld["noisy"]))) > 0.0


def test_the_kernel_order_reductions_are_sums_and_maxima():
    rng = np.random.default_rng(5)
    for L in (1, 255, 1024, 1025, 5000, 300000):
        x = rng.standard_normal(L)
        assert abs(M._power_kernel(x) - float(np.mean(x * x))) <= 1e-13 * float(np.mean(x * x))
        assert M._max_kernel(x) == float(np.max(np.abs(x)))


def test_ulp32():
    for w in (1.0, 0.75, 0.5, 1.9999, 3e-5, -0.3, 1e-42, 0.0):
        want = float(np.spacing(np.float32(abs(w)))) if abs(w) >= 2.0 ** -126 else 2.0 ** -149
        assert float(M.ulp32(w)) == want, w


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
    assert rows > 30
    print(f"[scene] {rows} rows: largest E {top:.3e}, at most {tight:.2e} of the bound")


def test_the_registered_batches_cover_the_shapes():
    T = int(_lib.load().cmgan_mix_tile())
    bts = M.build_batches(T)
    assert [bts[f"tile-{L}"].clean.shape[1] for L in (1, T - 1, T, T + 1)] == [1, T - 1, T, T + 1]
    assert any(2.4 * T < bt.clean.shape[1] < 2.6 * T for bt in bts.values())
    for name in ("tile-1", f"tile-{T + 1}"):
        assert sorted(bts[name].n_src.tolist()) == [0, 1, 4, 4]
    ks = set(bts["chunk"].src_rir_len[0].tolist())
    assert ks == {M.KC - 1, M.KC, M.KC + 1, 2 * M.KC + 50}
    bt = bts[f"tile-{T}"]
    assert (bt.src_off < 0).any() and (bt.src_off > bt.src_len).any() and (bt.src_len == 1).any() and (bt.src_len == T).any()
    assert ((bt.src_len == 7) & (bt.src_rir_len == 40)).any() and (bt.src_len > T + 40).any()
    sb = lambda bt, b: min(max(int(bt.n_src[b]), 0), 4)
    bad = bts["bad"]
    assert sum(not M.segment_ok(bad.src_bank, int(bad.src_start[b, j]), int(bad.src_len[b, j]))
               for b in range(4) for j in range(sb(bad, b))) == 6
    assert bad.rir_index.min() < 0 and bad.rir_index.max() >= len(bad.rir) and bad.src_rir_len.max() > bad.rir.shape[1]
    assert all(float(M.case("peak", b)[1]["scale"]) < 1.0 for b in range(2))
    assert bts["located"].noise_bank is None


# ------------------------------------------------------------------ draw_sources
def test_draw_sources_keeps_the_room_and_places_sources_inside():
    gen = torch.Generator().manual_seed(3)
    sampler = RoomSampler(margin=0.4, generator=gen)
    rooms, n_taps = sampler.draw(6, 8000, 16000)
    state = gen.get_state()
    src = sampler.draw_sources(rooms, 3)
    assert src.shape == (6, 3, 15) and src.dtype == torch.float64 and src.is_contiguous()
    keep = [0, 1, 2, 6, 7, 8, 9, 10, 11, 12, 13, 14]
    assert torch.equal(src[:, :, keep], rooms[:, None, keep].expand(6, 3, 12))
    pos, size = src[:, :, 3:6], rooms[:, None, 0:3]
    assert bool((pos >= 0.4).all()) and bool((pos <= size - 0.4).all())
    assert not torch.equal(src[:, 0, 3:6], rooms[:, 3:6]) and not torch.equal(src[:, 0, 3:6], src[:, 1, 3:6])
    # from the sampler's generator, after the room draws: the same state gives the same positions
    assert not torch.equal(gen.get_state(), state)
    gen.set_state(state)
    assert torch.equal(sampler.draw_sources(rooms, 3), src)
    assert src.reshape(18, 15).shape == (18, 15)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            sampler.draw_sources(rooms, bad)
    with pytest.raises(ValueError):
        sampler.draw_sources(rooms[:, :14], 2)
    with pytest.raises(ValueError):
        sampler.draw_sources(rooms.to(torch.float32), 2)


# ------------------------------------------------------------------ the library without a GPU
def test_symbols_and_abi():
    lib = _lib.load()
    for name in ("cmgan_scene", "cmgan_scene_workspace_bytes", "cmgan_scene_max_sources", "cmgan_mix", "cmgan_mix_tile"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.cmgan_scene_max_sources() == SCENE_MAX_SOURCES == 4
    assert lib.cmgan_abi_version() == _lib.ABI_VERSION >= 13


def test_workspace_bytes():
    ws = _lib.load().cmgan_scene_workspace_bytes
    assert ws(None, 0, 100, 1, 0) == ws(None, 1, 0, 1, 0) == ws(None, 1, 100, 0, 0) == 0
    assert ws(None, 1, 100, 65537, 0) == ws(None, 65536, 100, 1, 0) == ws(None, 1, 100, 1, 5) == ws(None, 1, 100, 1, -1) == 0
    assert ws(None, 1, 2 ** 31 - 1, 1, 0) == 0
    base = ws(None, 4, 5000, 300, 2)
    assert base > 0 and base % 256 == 0
    assert base >= 4 * 5000 * 8 * 4                                       # speech, target and two sources in float64
    for B, L, K, S in ((5, 5000, 300, 2), (4, 5001, 300, 2), (4, 5000, 301, 2), (4, 5000, 300, 3), (4, 9000, 300, 2)):
        assert ws(None, B, L, K, S) >= base
    assert ws(None, 4, 5000, 300, 4) > ws(None, 4, 5000, 300, 0) == _lib.load().cmgan_mix_workspace_bytes(None, 4, 5000, 300)


def _native(**over):
    """cmgan_scene with a NULL handle and plausible (never dereferenced) pointers: every argument error comes first."""
    a = dict(clean=4096, B=2, L=100, ld=100, noise_bank=4096, bank_len=10, noise_start=4096, noise_len=4096, noise_off=4096,
             snr_db=4096, src_bank=4096, src_bank_len=10, S=2, n_src=4096, src_start=4096, src_len=4096, src_off=4096,
             src_snr_db=4096, rir_bank=4096, R=3, Kmax=40, rir_index=4096, rir_len=4096, src_rir_index=4096, src_rir_len=4096,
             peak=0.99, early=-1, noisy=4096, target=4096, ld_out=100, g=4096, p=4096, ps=4096, scale=4096, ws=4096,
             ws_bytes=1 << 30, stream=None)
    a.update(over)
    lib = _lib.load()
    rc = lib.cmgan_scene(None, *a.values())
    return rc, (lib.cmgan_last_error(None) or b"").decode()


def test_native_argument_errors_come_before_the_handle():
    rc, msg = _native()
    assert rc == BADARG and "null handle" in msg
    for over, code, word in (
            (dict(clean=None), BADARG, "null pointer"), (dict(noisy=None), BADARG, "null pointer"),
            (dict(g=None), BADARG, "null pointer"), (dict(p=None), BADARG, "null pointer"),
            (dict(noise_start=None), BADARG, "dry-noise bank needs"), (dict(snr_db=None), BADARG, "dry-noise bank needs"),
            (dict(S=5), BADARG, "located sources"), (dict(S=-1), BADARG, "located sources"),
            (dict(n_src=None), BADARG, "S > 0 needs"), (dict(src_bank=None), BADARG, "S > 0 needs"),
            (dict(src_off=None), BADARG, "S > 0 needs"),
            (dict(rir_len=None), BADARG, "RIR bank needs"), (dict(src_rir_index=None), BADARG, "src_rir_index"),
            (dict(clean=4098), BADARG, "4-byte"), (dict(n_src=4097), BADARG, "4-byte"), (dict(src_rir_len=4098), BADARG, "4-byte"),
            (dict(src_start=4100), BADARG, "8-byte"), (dict(p=4100), BADARG, "8-byte"),
            (dict(B=0), BADARG, "need 0 < B"), (dict(B=65536), BADARG, "need 0 < B"), (dict(L=0), BADARG, "need 0 < B"),
            (dict(ld=99), BADARG, "need 0 < B"), (dict(ld_out=99), BADARG, "need 0 < B"),
            (dict(bank_len=0), BADARG, "at least one sample"), (dict(src_bank_len=0), BADARG, "at least one sample"),
            (dict(peak=0.0), BADARG, "peak"), (dict(peak=float("inf")), BADARG, "peak"), (dict(peak=float("nan")), BADARG, "peak"),
            (dict(early=-2), BADARG, "early"), (dict(R=0), BADARG, "R >= 1"), (dict(Kmax=0), BADARG, "R >= 1"),
            (dict(Kmax=65537), UNSUPPORTED, "taps are supported"),
            (dict(L=2 ** 31 - 1, ld=2 ** 31, ld_out=2 ** 31), UNSUPPORTED, "samples are supported")):
        rc, msg = _native(**over)
        assert rc == code and msg.startswith("cmgan_scene: ") and word in msg, (over, rc, msg)
    # what may be absent: the dry noise, the sources (S = 0 ignores their pointers), the RIR bank
    for over in (dict(noise_bank=None, noise_start=None, noise_len=None, noise_off=None, snr_db=None, bank_len=0),
                 dict(S=0, src_bank=None, n_src=None, src_start=None, src_len=None, src_off=None, src_snr_db=None,
                      src_rir_index=None, src_rir_len=None, src_bank_len=0),
                 dict(rir_bank=None, rir_index=None, rir_len=None, src_rir_index=None, src_rir_len=None, R=0, Kmax=0)):
        rc, msg = _native(**over)
        assert rc == BADARG and "null handle" in msg, (over, msg)


class _NoNative:
    """An engine stand-in whose native side must never be reached."""
    device = CPU

    def __getattr__(self, name):
        raise AssertionError(f"the argument check let a call through to {name}")


def _args(B=3, L=50, S=2, R=4, K=20):
    f32, i64, i32 = torch.float32, torch.int64, torch.int32
    z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype)
    return dict(clean=z(B, L, dtype=f32), noise_bank=z(100, dtype=f32), noise_start=z(B, dtype=i64), noise_len=z(B, dtype=i64),
                noise_off=z(B, dtype=i64), snr_db=z(B, dtype=f32), n_src=z(B, dtype=i32), src_bank=z(200, dtype=f32),
                src_start=z(B, S, dtype=i64), src_len=z(B, S, dtype=i64), src_off=z(B, S, dtype=i64),
                src_snr_db=z(B, S, dtype=f32), rir_bank=z(R, K, dtype=f32), rir_index=z(B, dtype=i32), rir_len=z(B, dtype=i32),
                src_rir_index=z(B, S, dtype=i32), src_rir_len=z(B, S, dtype=i32))


def test_check_scene_args():
    a = _args()
    assert check_scene_args(CPU, **a) == (3, 50, 4, 20, 2)
    no_src = {k: (None if k.startswith("src_") or k == "n_src" else v) for k, v in a.items()}
    assert check_scene_args(CPU, **no_src) == (3, 50, 4, 20, 0)
    no_dry = {k: (None if k in ("noise_bank", "noise_start", "noise_len", "noise_off", "snr_db") else v) for k, v in a.items()}
    assert check_scene_args(CPU, **no_dry) == (3, 50, 4, 20, 2)
    no_rir = {k: (None if "rir" in k else v) for k, v in a.items()}
    assert check_scene_args(CPU, **no_rir) == (3, 50, 0, 0, 2)
    f32, i64, i32 = torch.float32, torch.int64, torch.int32
    z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype)
    cases = [
        (dict(clean=z(50, dtype=f32)), ValueError), (dict(clean=z(3, 50, dtype=torch.float64)), TypeError),
        (dict(clean=np.zeros((3, 50), dtype=np.float32)), TypeError), (dict(noise_start=None), ValueError),
        (dict(noise_bank=None), ValueError), (dict(snr_db=z(4, dtype=f32)), ValueError),
        (dict(n_src=z(3, dtype=i64)), TypeError), (dict(n_src=z(4, dtype=i32)), ValueError), (dict(n_src=None), ValueError),
        (dict(src_bank=None), ValueError), (dict(src_bank=z(2, 100, dtype=f32)), ValueError),
        (dict(src_start=z(3, 5, dtype=i64)), ValueError), (dict(src_start=z(3, 0, dtype=i64)), ValueError),
        (dict(src_start=z(3, dtype=i64)), ValueError), (dict(src_len=z(3, 3, dtype=i64)), ValueError),
        (dict(src_off=z(3, 2, dtype=i32)), TypeError), (dict(src_off=None), ValueError),
        (dict(src_snr_db=z(3, 2, dtype=torch.float64)), TypeError), (dict(src_snr_db=z(3, 4, dtype=f32)[:, ::2]), ValueError),
        (dict(src_rir_index=None), ValueError), (dict(src_rir_len=z(3, 2, dtype=i64)), TypeError),
        (dict(src_rir_index=z(2, 2, dtype=i32)), ValueError), (dict(rir_bank=None), ValueError),
        (dict(rir_bank=z(4, 65537, dtype=f32)), ValueError), (dict(rir_index=None), ValueError),
        (dict(peak=0.0), ValueError), (dict(peak=float("inf")), ValueError), (dict(early=-2), ValueError),
        (dict(early=1.5), ValueError)]
    if torch.cuda.is_available():
        cases.append((dict(src_bank=z(200, dtype=f32).cuda()), RuntimeError))
    for over, exc in cases:
        with pytest.raises(exc):
            check_scene_args(CPU, **{**a, **over})
    from cmgan_amd.engine import Engine
    for over, exc in cases:
        with pytest.raises(exc):
            Engine.scene.__wrapped__(_NoNative(), **{**a, **over})


def test_scene_draw_is_draw_with_trailing_fields_that_default_to_none():
    names = SceneDraw._fields
    assert names[:len(Draw._fields)] == Draw._fields and Draw._fields[-1] == "speed"
    assert names[len(Draw._fields):] == ("n_src", "src_start", "src_len", "src_off", "src_snr_db", "src_rir_index", "src_rir_len",
                                         "src_rooms")
    d = SceneDraw(*(torch.zeros(1),) * 6)
    assert all(getattr(d, n) is None for n in names[6:])


def test_dynamic_mixer_argument_errors():
    class Eng:
        device = CPU
    nb = NoiseBank.from_arrays([np.ones(10, dtype=np.float32)])
    for kw in (dict(sources=(0, 0)), dict(sources=(2, 1)), dict(sources=(-1, 2)), dict(sources=(1, 5)), dict(sources=3),
               dict(sources=(1.0, 2.0)), dict(sources=(True, 2)), dict(sources=(1, 2), source_snr_db=(5.0, 1.0)),
               dict(sources=(1, 2), source_snr_db=3.0), dict(source_bank=nb), dict(dry_noise=False)):
        with pytest.raises(ValueError):
            DynamicMixer(Eng(), nb, **kw)
    m = DynamicMixer(Eng(), nb, sources=(0, 4), dry_noise=False)
    assert m.sources == (0, 4) and m.source_bank is nb and m.dry_noise is False and m.source_snr_db == (0.0, 20.0)
    other = NoiseBank.from_arrays([np.ones(5, dtype=np.float32)])
    assert DynamicMixer(Eng(), nb, sources=(1, 1), source_bank=other).source_bank is other
    assert DynamicMixer(Eng(), nb).sources is None


def test_the_mixer_draws_sources_after_every_other_draw():
    """On the CPU generator: the leading fields of a draw with sources are the draw without them, bit for bit."""
    class Eng:
        device = CPU
    nb = NoiseBank.from_arrays([np.ones(n, dtype=np.float32) for n in (10, 300, 1)])
    sb = NoiseBank.from_arrays([np.ones(n, dtype=np.float32) for n in (50, 7)])
    draws = []
    for kw in ({}, dict(sources=(1, 3), source_bank=sb, source_snr_db=(-5.0, 5.0))):
        gen = torch.Generator().manual_seed(11)
        m = DynamicMixer(Eng(), nb, generator=gen, level_db=(-30.0, -20.0), speed=(0.9, 1.1), **kw)
        draws.append(m.draw(8))
    a, b = draws
    for name in Draw._fields[:10]:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or torch.equal(x, y), name
    assert type(a) is Draw and type(b) is SceneDraw and b.src_rir_index is None and b.src_rooms is None
    n = b.n_src
    assert n.dtype == torch.int32 and n.shape == (8,) and int(n.min()) >= 1 and int(n.max()) <= 3
    assert b.src_start.shape == b.src_len.shape == b.src_off.shape == b.src_snr_db.shape == (8, 3)
    assert set(b.src_len.flatten().tolist()) <= {50, 7} and set(b.src_start.flatten().tolist()) <= {0, 50}
    assert bool((b.src_off >= 0).all()) and bool((b.src_off < b.src_len).all())
    assert b.src_snr_db.dtype == torch.float32 and float(b.src_snr_db.min()) >= -5.0 and float(b.src_snr_db.max()) <= 5.0
    assert all(t.is_contiguous() for t in (b.src_start, b.src_len, b.src_off, b.src_snr_db))
