"""CPU side of the tempo and pitch perturbation (cmgan_amd/csrc/stretch.hip; include/cmgan_hip.h, "Tempo perturbation"): the
numpy model the GPU tests compare the kernel with (tests/stretch_model.py) against brute force and against the facts the
definition promises, the condition on E for every row the GPU tests judge, and every argument error of cmgan_stretch,
Engine.stretch, Engine.pitch_shift and DynamicMixer(tempo=, pitch=, ...), all of which are judged before a handle or a
GPU is needed."""
import inspect
import math

import numpy as np
import pytest
import torch

import stretch_model as M
from cmgan_amd import _lib
from cmgan_amd.engine import STRETCH_HOP, STRETCH_SEARCH, check_pitch_args, check_stretch_args
from cmgan_amd.mixing import Draw, DynamicMixer, NoiseBank, SceneDraw, StretchDraw, stretch_len, warp_len

BADARG = -1
CPU = torch.device("cpu")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ the model against facts that are not its own
@pytest.mark.parametrize("r", [0.25, 0.7, 1.0, 1.0371, 1.9, 4.0])
def test_model_agrees_with_brute_force(r):
    for seed, n, H, D in ((1, 150, 16, 5), (2, 97, 16, 0), (3, 200, 24, 30)):
        x = M.voiced(seed, n)
        q, c, s = M.positions(x, n, r, H, D)
        qb, cb, sb = M.positions_brute(x, n, r, H, D)
        assert np.array_equal(q, qb) and np.array_equal(c, cb) and np.array_equal(s, sb), (r, n, H, D)
        assert len(q) == -(-M.count(n, r) // H)


def test_brute_force_handles_non_finite_samples_like_the_model():
    x = M.voiced(4, 160)
    x[[40, 41, 90]] = [np.nan, np.inf, -np.inf]
    for r in (0.6, 1.7):
        q, _, s = M.positions(x, 160, r, 16, 6)
        qb, _, sb = M.positions_brute(x, 160, r, 16, 6)
        assert np.array_equal(q, qb) and np.array_equal(s, sb) and s.any()


def test_unit_rate_is_a_bitwise_copy_and_never_searches():
    x = M.voiced(5, 1000)
    for H, D in ((32, 20), (256, 160), (16, 0)):
        q, c, s = M.positions(x, 1000, 1.0, H, D)
        assert not s.any() and np.array_equal(q, np.arange(len(q)) * H) and np.array_equal(q, c)
        for form in (M.direct, M.direct_ld):
            y = form(x, 1000, 1.0, H, D)
            assert len(y) == 1000 and np.array_equal(_bits(y.astype(np.float32)), _bits(x))


def test_a_drift_copies_long_runs_and_splices_rarely():
    x = M.voiced(6, 20000)
    q, c, s = M.positions(x, 20000, 1.0001, 32, 20)
    assert int(s.sum()) == 0 and np.array_equal(q, c)                    # 2 samples of drift in all: within D
    q, c, s = M.positions(x, 20000, 1.01, 32, 20)
    assert 0 < int(s.sum()) < len(q) // 2
    y = M.direct(x, 20000, 1.01, 32, 20).astype(np.float32)
    k = int(np.flatnonzero(~s)[5])
    assert np.array_equal(_bits(y[k * 32:(k + 1) * 32]), _bits(x[q[k]:q[k] + 32]))


def test_ties_take_the_nominal_position():
    """Silence and an all-NaN row tie everywhere; a constant and an exact period that divides k H r tie (or match) wherever
    the windows lie inside the row: every searched frame there takes d = 0."""
    M.build_rows()
    nan_row = np.full(600, np.nan, dtype=np.float32)
    for x, n, r in ((M.ROWS["tie-silence"].x, 1000, 1.1), (nan_row, 600, 0.8)):
        q, _, s = M.positions(x, n, r, M.H_S, M.D_S)
        ks = np.flatnonzero(s)
        assert len(ks) > 3 and all(q[k] == M.nominal(k, r, M.H_S) for k in ks)
    for key in ("tie-constant", "tie-period"):
        row = M.ROWS[key]
        q, c, s = M.case(key)[0]
        ks = [k for k in np.flatnonzero(s)
              if M.nominal(k, row.r, row.H) + row.D + row.H <= row.n and c[k] + row.H <= row.n and M.nominal(k, row.r, row.H) >= row.D]
        assert len(ks) > 3 and all(q[k] == M.nominal(k, row.r, row.H) for k in ks), key


def test_the_constructed_rows_are_what_they_claim():
    M.build_rows()
    for key, sign in (("match-lo", -1), ("match-hi", +1)):
        row = M.ROWS[key]
        q, c, s = M.case(key)[0]
        assert s[1] and q[1] == M.nominal(1, row.r, row.H) + sign * row.D, (key, q[:3])
    row = M.ROWS["cut"]
    q, c, s = M.case("cut")[0]
    p = [M.nominal(k, row.r, row.H) for k in range(len(q))]
    assert s[1] and p[1] - row.D < 0                                      # candidates cut by q < 0
    late = [k for k in np.flatnonzero(s) if p[k] + row.D >= row.n]
    assert late and any(c[k] + row.H > row.n for k in late)               # cut by q >= n; the continuation runs past n
    for H, D in M.HOP_SEARCH:                                            # every (hop, search) edge searches at least once
        assert M.case(f"hd-{H}-{D}")[0][2].any(), (H, D)
    assert M.case("long")[0][2].sum() > 5 and M.ROWS["long"].N > 65536


def test_without_a_search_range_every_frame_sits_at_its_nominal_position():
    x = M.voiced(7, 2000)
    for r in (0.8, 1.0, 1.3):
        q, c, s = M.positions(x, 2000, r, 32, 0)
        p = np.array([M.nominal(k, r, 32) for k in range(len(q))])
        assert np.array_equal(q, p)
        assert np.array_equal(s[1:], c[1:] != p[1:])                     # searched (one candidate) except where c_k = p_k


def test_frame_counts_and_lengths_follow_count():
    x = M.voiced(8, 1000)
    for r in (0.25, 0.9, 1.0, 1.1, 4.0):
        for n in (0, 1, 31, 32, 33, 1000):
            q, _, _ = M.positions(x, n, r, 32, 20)
            assert len(q) == -(-M.count(n, r) // 32) and len(M.direct(x, n, r, 32, 20)) == M.count(n, r)
            assert len(M.positions(x, n, r, 32, 20, N=40)[0]) == -(-min(M.count(n, r), 40) // 32)
    assert M.order(2) == [0, -1, 1, -2, 2] and [M.rank(d) for d in M.order(3)] == list(range(7))
    f, g = M.fade(32)
    assert f[0] == 0.0 and g[0] == 1.0 and f[16] == 0.5 and np.all(np.diff(f) > 0) and np.array_equal(g, 1.0 - f)


def test_the_pitch_is_kept():
    """A 200 Hz harmonic tone at 16 kHz has its autocorrelation peak at lag 80 before and after the stretch."""
    t = np.arange(8000) / 16000.0
    x = sum(np.sin(2 * np.pi * 200.0 * h * t) / h for h in range(1, 6)).astype(np.float32) * 0.1
    for r in (0.8, 1.25):
        y = M.direct(x, 8000, r)
        w = y[1024:3072]
        ac = np.correlate(w, w, "full")[len(w) - 1:]
        assert abs(40 + int(np.argmax(ac[40:160])) - 80) <= 1 and abs(len(y) - 8000 / r) <= 1


def test_every_row_of_the_gpu_tests_respects_the_condition_on_E():
    """The rule |g - w| <= ulp32(w) / 2 + E may be used on a row only if E <= 2^-10 x ulp32(rms) / 2."""
    rows = M.build_rows()
    assert len(rows) > 50
    top, tight = 0.0, 0.0
    for key, row in rows.items():
        (q, c, s), E, w = M.case(key)
        bound = M.condition(E, w)
        assert len(w) == min(M.count(row.n, row.r), row.N) > 0 and np.all(np.isfinite(w.astype(np.float64))), key
        assert E <= bound, f"{key}: E = {E:.3e} above {bound:.3e}"
        top, tight = max(top, E), max(tight, E / bound)
    print(f"[stretch] {len(rows)} rows: largest E {top:.3e}, at most {tight:.2e} of the bound")


# ------------------------------------------------------------------ the library without a GPU
def test_symbols_and_constants():
    lib = _lib.load()
    for name in ("cmgan_stretch", "cmgan_stretch_max_hop", "cmgan_stretch_max_search"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.cmgan_stretch_max_hop() == STRETCH_HOP[1] == 1024 and STRETCH_HOP[0] == 16
    assert lib.cmgan_stretch_max_search() == STRETCH_SEARCH[1] == 1024 and STRETCH_SEARCH[0] == 0
    assert lib.cmgan_warp_max_rate() == M.MAX_RATE == 4.0
    assert lib.cmgan_abi_version() == _lib.ABI_VERSION >= 14
    for n, r in ((3000, 0.25), (3000, 1.0371), (70000, 1.03), (6000, 1.9)):   # stretch and warp agree on lengths
        assert int(lib.cmgan_warp_out_len(n, r)) == M.count(n, r)


def test_library_rejects_bad_arguments_before_it_needs_a_handle():
    lib = _lib.load()
    x = np.zeros(8192, dtype=np.float32)
    y = np.zeros(8192, dtype=np.float32)
    lengths = np.zeros(8, dtype=np.int32)
    out_len, status, searched = (np.full(8, 7, dtype=np.int32) for _ in range(3))
    pos = np.full(256, 7, dtype=np.int32)
    rate = np.ones(9, dtype=np.float64)
    px, py, pl, po, pt, pp, ps, pr = (a.ctypes.data for a in (x, y, lengths, out_len, status, pos, searched, rate))

    def call(x=px, B=2, L=1500, ldx=1500, lengths=pl, rate=pr, hop=256, search=160, y=py, N=1600, ldy=1600, out_len=po,
             status=pt, pos=pp, searched=ps):
        rc = lib.cmgan_stretch(None, x, B, L, ldx, lengths, rate, hop, search, y, N, ldy, out_len, status, pos, searched, None)
        return rc, (lib.cmgan_last_error(None) or b"").decode()

    cases = {
        "null pointer": [dict(x=None), dict(rate=None), dict(y=None)],
        "4-byte aligned": [dict(x=px + 2), dict(y=py + 1), dict(lengths=pl + 1), dict(out_len=po + 2), dict(status=pt + 3),
                           dict(pos=pp + 2), dict(searched=ps + 1)],
        "8-byte aligned": [dict(rate=pr + 4)],
        "need 1 <= B": [dict(B=0), dict(B=-3), dict(B=65536), dict(L=0), dict(L=-1), dict(N=0), dict(N=-2), dict(ldx=1499),
                        dict(ldy=1599)],
        "hop must lie": [dict(hop=15), dict(hop=1025), dict(hop=0), dict(hop=-256)],
        "search must lie": [dict(search=-1), dict(search=1025)],
        "overlap": [dict(y=px), dict(y=px + 4 * 1500), dict(y=px + 4 * 2999), dict(x=py + 4 * 100), dict(x=py + 4 * 3199)],
    }
    for text, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == BADARG and "cmgan_stretch" in msg and text in msg, (kw, rc, msg)
    # everything in order: only the handle is missing - nothing was enqueued, nothing was written
    for kw in (dict(), dict(lengths=None), dict(out_len=None), dict(status=None), dict(pos=None), dict(searched=None),
               dict(hop=16), dict(hop=1024), dict(search=0), dict(search=1024), dict(y=px + 4 * 3000),
               dict(x=py + 4 * 3200), dict(N=1, ldy=1), dict(B=1, L=1, ldx=1), dict(ldx=2000, ldy=2000)):
        rc, msg = call(**kw)
        assert rc == BADARG and "null handle" in msg, (kw, rc, msg)
    assert not y.any() and all((a == 7).all() for a in (status, out_len, pos, searched))


# ------------------------------------------------------------------ Engine.stretch's and Engine.pitch_shift's argument rules
def test_check_stretch_args():
    wav = torch.zeros(3, 2000)
    rate = torch.ones(3, dtype=torch.float64)
    i32 = lambda n=3: torch.zeros(n, dtype=torch.int32)
    assert check_stretch_args(CPU, wav, rate) == (3, 2000, None)
    assert check_stretch_args(CPU, wav, rate, 2200, i32(), 1024, 1024) == (3, 2000, 2200)
    assert check_stretch_args(CPU, wav, rate, hop=16, search=0) == (3, 2000, None)
    assert check_stretch_args(CPU, wav, rate, out=torch.zeros(3, 1800)) == (3, 2000, 1800)
    assert check_stretch_args(CPU, wav, rate, 1800, out=torch.zeros(3, 2500)[:, :1800]) == (3, 2000, 1800)
    assert check_stretch_args(CPU, torch.zeros(3, 2500)[:, :2000], rate, 1) == (3, 2000, 1)
    with pytest.raises(TypeError, match="wav: expected a torch.Tensor"):
        check_stretch_args(CPU, np.zeros((3, 2000), dtype=np.float32), rate)
    with pytest.raises(TypeError, match="wav: expected float32"):
        check_stretch_args(CPU, wav.double(), rate)
    with pytest.raises(RuntimeError, match="wav: tensor is on cpu"):
        check_stretch_args(torch.device("cuda:0"), wav, rate)
    for bad in (torch.zeros(2000), torch.zeros(1, 3, 2000), torch.zeros(0, 2000), torch.zeros(3, 0)):
        with pytest.raises(ValueError, match="wav: expected \\[B, L\\]"):
            check_stretch_args(CPU, bad, rate)
    with pytest.raises(ValueError, match="at most 65535 rows"):
        check_stretch_args(CPU, torch.zeros(1, 1).expand(65536, 1), rate)
    for bad in (torch.zeros(3, 4000)[:, ::2], torch.zeros(2000, 3).t(), torch.zeros(1, 2000).expand(3, 2000)):
        with pytest.raises(ValueError, match="wav: rows must be contiguous"):
            check_stretch_args(CPU, bad, rate)
    with pytest.raises(TypeError, match="rate: expected float64"):
        check_stretch_args(CPU, wav, rate.float())
    with pytest.raises(TypeError, match="rate: expected a torch.Tensor"):
        check_stretch_args(CPU, wav, 1.1)
    for bad in (torch.ones(2, dtype=torch.float64), torch.ones(3, 1, dtype=torch.float64)):
        with pytest.raises(ValueError, match="rate: expected \\[3\\]"):
            check_stretch_args(CPU, wav, bad)
    with pytest.raises(ValueError, match="rate: must be contiguous"):
        check_stretch_args(CPU, wav, torch.ones(6, dtype=torch.float64)[::2])
    with pytest.raises(TypeError, match="lengths: expected int32"):
        check_stretch_args(CPU, wav, rate, None, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="lengths: expected \\[3\\]"):
        check_stretch_args(CPU, wav, rate, None, i32(4))
    for bad in (0, -5, 2 ** 31, 100.5, True):
        with pytest.raises(ValueError, match="n_out must be"):
            check_stretch_args(CPU, wav, rate, bad)
    for bad in (15, 1025, 256.5, True):
        with pytest.raises(ValueError, match="hop must be"):
            check_stretch_args(CPU, wav, rate, hop=bad)
    for bad in (-1, 1025, 160.5, True):
        with pytest.raises(ValueError, match="search must be"):
            check_stretch_args(CPU, wav, rate, search=bad)
    with pytest.raises(TypeError, match="out: expected float32"):
        check_stretch_args(CPU, wav, rate, out=torch.zeros(3, 2000, dtype=torch.float64))
    with pytest.raises(ValueError, match="out: expected \\[3, 1800\\]"):
        check_stretch_args(CPU, wav, rate, 1800, out=torch.zeros(3, 1801))
    with pytest.raises(ValueError, match="out: expected \\[3, N\\]"):
        check_stretch_args(CPU, wav, rate, out=torch.zeros(2, 1800))
    with pytest.raises(ValueError, match="out: rows must be contiguous"):
        check_stretch_args(CPU, wav, rate, out=torch.zeros(3, 4000)[:, ::2])


def test_check_pitch_args():
    wav = torch.zeros(3, 2000)
    factor = torch.ones(3, dtype=torch.float64)
    assert check_pitch_args(CPU, wav, factor) == (3, 2000)
    assert check_pitch_args(CPU, wav, factor, 1900, 16, 0, 4, 0.5) == (3, 2000)
    with pytest.raises(TypeError, match="wav: expected float32"):
        check_pitch_args(CPU, wav.double(), factor)
    with pytest.raises(ValueError, match="wav: expected \\[B, L\\]"):
        check_pitch_args(CPU, torch.zeros(2000), factor)
    with pytest.raises(TypeError, match="factor: expected a torch.Tensor"):
        check_pitch_args(CPU, wav, 1.1)
    with pytest.raises(TypeError, match="factor: expected float64"):
        check_pitch_args(CPU, wav, factor.float())
    with pytest.raises(ValueError, match="factor: expected \\[3\\]"):
        check_pitch_args(CPU, wav, torch.ones(4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="wav: tensor is on cpu"):
        check_pitch_args(torch.device("cuda:0"), wav, factor)
    with pytest.raises(ValueError, match="n_out must be"):
        check_pitch_args(CPU, wav, factor, 0)
    with pytest.raises(ValueError, match="hop must be"):
        check_pitch_args(CPU, wav, factor, hop=8)
    with pytest.raises(ValueError, match="search must be"):
        check_pitch_args(CPU, wav, factor, search=2000)
    with pytest.raises(ValueError, match="zeros must be"):
        check_pitch_args(CPU, wav, factor, zeros=3)
    with pytest.raises(ValueError, match="rolloff must lie"):
        check_pitch_args(CPU, wav, factor, rolloff=1.5)


# ------------------------------------------------------------------ DynamicMixer's new arguments
class _NoEngine:
    device = CPU


def _bank():
    return NoiseBank.from_arrays([np.ones(100, dtype=np.float32), np.ones(50, dtype=np.float32)])


def test_mixer_rejects_bad_tempo_and_pitch_options():
    bank = _bank()
    mk = lambda **kw: DynamicMixer(_NoEngine(), bank, **kw)
    for bad in ((0.2, 1.0), (0.9, 4.5), (1.1, 0.9), (math.nan, 1.0), (0.9, math.inf)):
        with pytest.raises(ValueError, match="tempo must be \\(low, high\\) with"):
            mk(tempo=bad)
    for bad in (1.1, "fast", (0.9,), ("a", "b")):
        with pytest.raises(ValueError, match="tempo must be None or \\(low, high\\)"):
            mk(tempo=bad)
    for bad in ((-13, 0), (0, 12.5), (2, -2), (math.nan, 1.0)):
        with pytest.raises(ValueError, match="pitch must be \\(low, high\\) semitones"):
            mk(pitch=bad)
    for bad in (2, "up", (1,)):
        with pytest.raises(ValueError, match="pitch must be None or \\(low, high\\) in semitones"):
            mk(pitch=bad)
    for bad in (-0.1, 1.5, math.nan):
        with pytest.raises(ValueError, match="p_tempo must lie in"):
            mk(tempo=(0.9, 1.1), p_tempo=bad)
        with pytest.raises(ValueError, match="p_pitch must lie in"):
            mk(pitch=(-1, 1), p_pitch=bad)
    for bad in (15, 1025, 64.5, True):
        with pytest.raises(ValueError, match="stretch_hop must be"):
            mk(tempo=(0.9, 1.1), stretch_hop=bad)
    for bad in (-1, 1025, 0.5, True):
        with pytest.raises(ValueError, match="stretch_search must be"):
            mk(tempo=(0.9, 1.1), stretch_search=bad)
    # rates that can leave [1/4, 4]: t / p for the stretch, v p for the warp
    for kw in (dict(tempo=(0.3, 3.0), pitch=(-12, 12)), dict(tempo=(3.0, 3.5), pitch=(-6, 0)),
               dict(tempo=(0.3, 0.4), pitch=(0, 6))):
        with pytest.raises(ValueError, match="the stretch rates"):
            mk(**kw)
    for kw in (dict(speed=(0.3, 3.0), pitch=(-12, 12)), dict(speed=(3.0, 3.5), pitch=(0, 6)),
               dict(speed=(0.3, 0.4), pitch=(-6, 0))):
        with pytest.raises(ValueError, match="the warp rates"):
            mk(**kw)
    m = mk()
    assert m.tempo is None and m.pitch is None and m.p_tempo == 1.0 and m.p_pitch == 1.0
    assert (m.stretch_hop, m.stretch_search) == (256, 160) and m.last_stretch is None
    m = mk(tempo=(0.5, 2), pitch=(-12, 12), p_tempo=0.5, p_pitch=0.25, stretch_hop=16, stretch_search=0)
    assert m.tempo == (0.5, 2.0) and m.pitch == (-12.0, 12.0) and (m.p_tempo, m.p_pitch) == (0.5, 0.25)
    assert (m.stretch_hop, m.stretch_search) == (16, 0)


def test_stretch_len():
    f = lambda s: 2.0 ** (s / 12.0)
    assert stretch_len(32000) == 32000
    assert stretch_len(32000, tempo=(0.9, 1.1)) == warp_len(32000, 1.1)
    assert stretch_len(32000, pitch=(-2, 2)) == warp_len(warp_len(32000, 1.0 / f(-2)), f(2))
    assert stretch_len(32000, (0.9, 1.1), (-2, 3), (0.95, 1.05)) == warp_len(warp_len(32000, 1.1 / f(-2)), 1.05 * f(3))
    assert stretch_len(32000, speed=(0.95, 1.05)) == warp_len(32000, 1.05)
    # below probability 1 the rate 1.0 belongs to a range
    assert stretch_len(32000, tempo=(0.8, 0.9), p_tempo=0.5) == 32000 and stretch_len(32000, tempo=(0.8, 0.9)) > 32000
    assert stretch_len(32000, pitch=(1, 2), p_pitch=0.5) == warp_len(warp_len(32000, 1.0), f(2))
    bank = _bank()
    m = DynamicMixer(_NoEngine(), bank, tempo=(0.9, 1.1), pitch=(-2, 3), speed=(0.95, 1.05), p_pitch=0.5)
    assert m.stretch_len(32000) == stretch_len(32000, (0.9, 1.1), (-2, 3), (0.95, 1.05), p_pitch=0.5)
    assert DynamicMixer(_NoEngine(), bank).stretch_len(777) == 777
    assert DynamicMixer(_NoEngine(), bank, speed=(0.9, 1.1)).stretch_len(32000) == warp_len(32000, 1.1)
    with pytest.raises(ValueError, match="warp_len needs"):
        stretch_len(-1, tempo=(0.9, 1.1))


def test_defaults_leave_the_draws_as_they_are():
    """With the new arguments at their defaults: draw() has the signature it had, Draw and SceneDraw the fields they had,
    the same values come out and the generator ends in the same state; the new draws come after every other one."""
    assert list(inspect.signature(DynamicMixer.draw).parameters) == ["self", "B"]
    assert Draw._fields == ("noise_start", "noise_len", "noise_off", "snr_db", "rir_index", "rir_len", "rooms", "level_db",
                            "channel", "speed")
    assert SceneDraw._fields[:10] == Draw._fields and SceneDraw._fields[10:] == (
        "n_src", "src_start", "src_len", "src_off", "src_snr_db", "src_rir_index", "src_rir_len", "src_rooms")
    assert StretchDraw._fields == ("tempo", "pitch_factor", "stretch_rate", "warp_rate")
    bank = _bank()
    gen = lambda s=7: torch.Generator().manual_seed(s)
    for extra in (dict(), dict(sources=(1, 2))):
        g0, g1, g2 = gen(), gen(), gen()
        kw = dict(level_db=(-35, -15), speed=(0.9, 1.1), p_speed=0.5, **extra)
        m0 = DynamicMixer(_NoEngine(), bank, generator=g0, **kw)
        m1 = DynamicMixer(_NoEngine(), bank, generator=g1, tempo=None, p_tempo=0.3, pitch=None, p_pitch=0.3, stretch_hop=64,
                          stretch_search=7, **kw)
        m2 = DynamicMixer(_NoEngine(), bank, generator=g2, tempo=(0.9, 1.1), pitch=(-2, 2), **kw)
        d0, d1, d2 = m0.draw(500), m1.draw(500), m2.draw(500)
        assert type(d0) is type(d1) is type(d2) and len(d0) == len(d1) == len(d2)
        for a, b, c in zip(d0, d1, d2):
            assert (a is None and b is None and c is None) or (torch.equal(a, b) and torch.equal(a, c))
        assert m1.draw_stretch(500, d1.speed) is None
        assert torch.equal(g0.get_state(), g1.get_state()) and torch.equal(g0.get_state(), g2.get_state())
        s = m2.draw_stretch(500, d2.speed)
        assert not torch.equal(g0.get_state(), g2.get_state())
        for t in s:
            assert t.dtype == torch.float64 and tuple(t.shape) == (500,) and t.is_contiguous()
        lo, hi = 2.0 ** (-2 / 12.0), 2.0 ** (2 / 12.0)
        assert bool(((s.tempo >= 0.9) & (s.tempo <= 1.1)).all()) and bool(((s.pitch_factor >= lo) & (s.pitch_factor <= hi)).all())
        assert float(s.pitch_factor.min()) < lo * 1.01 and float(s.pitch_factor.max()) > hi / 1.01
        assert torch.equal(s.stretch_rate, s.tempo / s.pitch_factor) and torch.equal(s.warp_rate, d2.speed * s.pitch_factor)


def test_tempo_and_pitch_draws():
    bank = _bank()
    gen = lambda s=9: torch.Generator().manual_seed(s)
    s = DynamicMixer(_NoEngine(), bank, generator=gen(), tempo=(0.8, 1.2), p_tempo=0.5).draw_stretch(2000)
    ones = int((s.tempo == 1.0).sum())
    assert 850 < ones < 1150 and s.warp_rate is None                    # tempo alone: no warp
    assert bool((s.pitch_factor == 1.0).all()) and torch.equal(s.stretch_rate, s.tempo)
    s = DynamicMixer(_NoEngine(), bank, generator=gen(), pitch=(-3, 3), p_pitch=0.25).draw_stretch(2000)
    assert 1350 < int((s.pitch_factor == 1.0).sum()) < 1650 and bool((s.tempo == 1.0).all())
    assert torch.equal(s.warp_rate, s.pitch_factor) and torch.equal(s.stretch_rate, 1.0 / s.pitch_factor)
    s = DynamicMixer(_NoEngine(), bank, generator=gen(), tempo=(1.05, 1.05), pitch=(12, 12)).draw_stretch(50)
    assert bool((s.tempo == 1.05).all()) and bool((s.pitch_factor == 2.0).all())
    s = DynamicMixer(_NoEngine(), bank, generator=gen(), tempo=(0.5, 2.0), p_tempo=0.0, pitch=(-5, 5), p_pitch=0.0).draw_stretch(50)
    assert bool((s.stretch_rate == 1.0).all()) and bool((s.warp_rate == 1.0).all())
    s = DynamicMixer(_NoEngine(), bank, generator=gen(), tempo=(0.9, 1.1), speed=(0.9, 1.1)).draw_stretch(
        50, torch.full((50,), 1.07, dtype=torch.float64))
    assert bool((s.warp_rate == 1.07).all())                             # the speed stage's warp, folded in
