"""CPU side of the gain control (cmgan_amd/csrc/dynamics.hip; include/cmgan_hip.h, "Dynamics"): the float64 model the GPU
tests compare the kernels with (tests/dynamics_model.py) - its tiled scan against its serial loop and the long-double
loop, closed forms of the detector, E for every row the GPU tests use - then dynamics_params, what a DynamicsSampler
draws, the workspace formula, and every argument error of cmgan_dynamics, Engine.dynamics, DynamicsSampler and
DynamicMixer(dynamics=, dynamics_on=), all of which are judged before a handle or a GPU is needed."""
import math

import numpy as np
import pytest
import torch

import dynamics_model as M
from cmgan_amd import _lib
from cmgan_amd.engine import DYNAMICS_BLOCK, DYNAMICS_MAX_L, DYNAMICS_TILE, check_dynamics_args, dynamics_workspace_bytes
from cmgan_amd.mixing import Draw, DynamicMixer, DynamicsSampler, NoiseBank, PathDraw, SceneDraw, dynamics_params

BADARG = -1
CPU = torch.device("cpu")
FS = 16000


class _NoEngine:
    device = CPU


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("attack_ms, release_ms", [(5.0, 200.0), (30.0, 30.0), (20.0, 5.0), (0.0, 150.0), (10.0, 0.0)],
                         ids=["att<rel", "att=rel", "att>rel", "a_att=0", "a_rel=0"])
def test_tiled_scan_is_the_serial_loop(attack_ms, release_ms):
    n = 2577
    x = M.bursts(3, n)
    dyn = M.params(-28.0, 6.0, 6.0, attack_ms, release_ms, 2.0)
    for T in (M.TILE, 16):
        E, Ey = M.slack(x, None, n, dyn, T)
        (o, y), (ot, yt) = M.serial(x, None, n, dyn), M.tiled(x, None, n, dyn, T)
        print(f"T={T}: E={E:.3g} Ey={Ey:.3g}, tiled - serial: out {np.max(np.abs(ot - o)):.3g}, y {np.max(np.abs(yt - y)):.3g} dB, "
              f"peak reduction {y.max():.3g} dB")
        assert y.max() > 1.0                                            # the processor does something
        assert np.max(np.abs(ot - o)) <= E and np.max(np.abs(yt - y)) <= Ey
        assert Ey < 1e-11 and E < 1e-6 * 0.5 * M.ulp32(np.max(np.abs(o)))
        # the entry states are the serial loop's states at the tile edges
        c = M.want(x, *dyn[:3])
        inc = M.entry_states(c, dyn[3], dyn[4], T)
        assert inc[0] == 0.0 and np.max(np.abs(inc[1:] - y[T - 1:n - 1:T][:len(inc) - 1])) <= Ey


def test_long_double_loop_is_wider():
    x = M.bursts(4, 1500)
    dyn = M.params(-25.0, 4.0, 6.0, 5.0, 100.0)
    o, _ = M.serial(x, None, 1500, dyn, np.longdouble)
    assert o.dtype == np.longdouble
    if np.finfo(np.longdouble).eps < 1e-18:
        assert 0.0 < float(np.max(np.abs(M.serial(x, None, 1500, dyn)[0] - o))) < 1e-13


def test_static_curve_and_constant_key():
    thr, ratio, knee = -20.0, 4.0, 10.0
    slope = 1.0 - 1.0 / ratio
    level = lambda db: np.full(4000, 10.0 ** (db / 20.0), dtype=np.float32)
    for db, c in ((-40.0, 0.0), (-25.0 - 1e-3, 0.0), (-20.0, slope * 25.0 / 20.0), (-15.0, slope * 5.0), (-6.0, slope * 14.0)):
        x = level(db)
        xg = 20.0 * math.log10(float(x[0]))
        d = xg - thr
        exact = 0.0 if 2 * d < -knee else (slope * (d + knee / 2) ** 2 / (2 * knee) if 2 * abs(d) <= knee else slope * d)
        assert abs(exact - c) < 1e-2                                     # the table above is the textbook curve
        assert abs(float(M.want(x[:1], thr, slope, knee)[0]) - exact) < 1e-12
        _, y = M.serial(x, None, 4000, M.params(thr, ratio, knee, 5.0, 20.0))
        assert abs(y[-1] - exact) < 1e-9 * max(exact, 1.0) + exact * math.exp(-4000 / (0.005 * FS))   # converged to the static curve
        out, _ = M.serial(x, None, 4000, M.params(thr, ratio, knee, 5.0, 20.0, 3.0))
        assert abs(20.0 * math.log10(out[-1] / float(x[0])) - (3.0 - exact)) < 1e-6
    # the knee joins both branches continuously, and a hard knee has none
    for edge in (thr - knee / 2, thr + knee / 2):
        lo, hi = (float(M.want(np.float32([10.0 ** ((edge + s) / 20.0)]), thr, slope, knee)[0]) for s in (-1e-4, 1e-4))
        assert abs(hi - lo) < 1e-3
    assert float(M.want(np.float32([0.05]), -20.0, 1.0, 0.0)[0]) == 0.0
    assert float(M.want(np.float32([1.0]), -20.0, 1.0, 0.0)[0]) == 20.0
    # what is not finite counts as silence, and silence is floored at -120 dB
    assert M.want(np.float32([np.nan, np.inf, -np.inf]), -200.0, 1.0, 0.0).tolist() == [0.0, 0.0, 0.0]
    assert M.want(np.float32([0.0, 1e-9]), -200.0, 1.0, 0.0).tolist() == [80.0, 80.0]


def test_step_reaches_1_minus_1_over_e_after_the_attack_time():
    attack_ms, release_ms = 10.0, 300.0
    n_att, n_rel = int(attack_ms * FS / 1000), int(release_ms * FS / 1000)
    dyn = M.params(-20.0, np.inf, 0.0, attack_ms, release_ms)
    x = np.concatenate([np.full(1000, 10.0 ** (-40 / 20)), np.full(4000, 1.0), np.full(8000, 10.0 ** (-40 / 20))]).astype(np.float32)
    _, y = M.serial(x, None, len(x), dyn)
    assert np.all(y[:1000] == 0.0)
    assert abs(y[1000 + n_att - 1] / 20.0 - (1.0 - math.exp(-1.0))) < 1e-12      # n_att steps of y <- a y + (1 - a) 20
    top = y[4999]
    assert abs(y[4999 + n_rel] / top - math.exp(-1.0)) < 1e-12                   # and the release falls to 1 / e
    assert np.all(np.diff(y[1000:5000]) > 0) and np.all(np.diff(y[5000:]) < 0)


def test_identity_rows_and_non_finite_samples():
    x = M.bursts(5, 700)
    for dyn in (M.params(-30.0, 1.0, 6.0, 5.0, 100.0), M.params(10.0, 8.0, 4.0, 5.0, 100.0)):   # slope 0; all under the knee
        for f in (M.serial, M.tiled):
            out, y = f(x, None, 700, dyn)
            assert not y.any() and np.array_equal(out.astype(np.float32).view(np.uint32), x.view(np.uint32))
    bad = x.copy()
    bad[[10, 300, 650]] = [np.nan, np.inf, -np.inf]
    dyn = M.params(-30.0, 4.0, 6.0, 5.0, 100.0)
    out, _ = M.serial(bad, None, 700, dyn)
    assert np.isnan(out[10]) and out[300] == np.inf and out[650] == -np.inf and np.isfinite(np.delete(out, [10, 300, 650])).all()
    E, _ = M.slack(bad, None, 700, dyn)
    worst, same = M.excess(out.astype(np.float32), bad, None, 700, dyn, E)
    assert worst <= 0.0 and same
    moved = out.astype(np.float32)
    moved[10], moved[11] = moved[11], moved[10]
    assert M.excess(moved, bad, None, 700, dyn, E)[1] is False


def test_E_is_far_below_half_a_float32_ulp_for_every_gpu_row():
    """The acceptance rule rests on this: it is confirmed here, on the CPU, for the rows tests/test_gpu_dynamics.py uses."""
    worst = 0.0
    rows = [(name, M.bursts(20 + i, 2577), dyn) for i, (name, dyn) in enumerate(M.mix_rows().items())]
    rows += [(f"n={n}", M.bursts(40 + i, n), M.params(-28.0, 6.0, 6.0, 5.0, 120.0, 2.0)) for i, n in enumerate(M.edge_lengths())]
    rows.append(("257 tiles", M.bursts(9, 257 * M.TILE), M.params(-26.0, 5.0, 6.0, 5.0, 2000.0, 1.0)))
    for name, x, dyn in rows:
        n = len(x)
        E, Ey = M.slack(x, None, n, dyn)
        half = 0.5 * float(M.ulp32(np.max(np.abs(M.serial(x, None, n, dyn)[0]))))
        print(f"{name}: E = {E:.3g}, Ey = {Ey:.3g} dB, half a float32 ulp at the row's peak = {half:.3g}")
        worst = max(worst, E / half)
        assert Ey < 1e-11
    assert worst < 1e-5


# ------------------------------------------------------------------ dynamics_params and the sampler
def test_dynamics_params_against_scalar_formulas():
    t = dynamics_params(torch.tensor([-20.0, -30.0, -10.0]), torch.tensor([4.0, math.inf, 1.0]), torch.tensor([6.0, 0.0, 12.0]),
                        torch.tensor([5.0, 0.0, 30.0]), torch.tensor([100.0, 500.0, 50.0]), torch.tensor([3.0, 0.0, -1.0]), FS)
    assert t.dtype == torch.float64 and t.shape == (3, 6) and t.is_contiguous()
    for row, (thr, ratio, knee, att, rel, mk) in zip(t.tolist(), ((-20.0, 4.0, 6.0, 5.0, 100.0, 3.0), (-30.0, math.inf, 0.0, 0.0, 500.0, 0.0),
                                                                  (-10.0, 1.0, 12.0, 30.0, 50.0, -1.0))):
        want = [thr, 1.0 - 1.0 / ratio, knee, math.exp(-1.0 / (att / 1000 * FS)) if att else 0.0, math.exp(-1.0 / (rel / 1000 * FS)), mk]
        assert row == pytest.approx(want, rel=1e-15, abs=0.0)
        assert np.allclose(M.params(thr, ratio, knee, att, rel, mk), row, rtol=1e-15, atol=0.0)
    assert t[1, 1].item() == 1.0 and t[1, 3].item() == 0.0 and t[2, 1].item() == 0.0
    one = dynamics_params(-20.0, 4.0, 6.0, 5.0, 100.0, 0.0, 8000)          # scalars broadcast: one row
    assert one.shape == (6,) and one[3].item() == pytest.approx(math.exp(-1.0 / 40.0), rel=1e-15)
    assert dynamics_params(torch.zeros(4, 2), 2.0, 0.0, 1.0, 1.0, 0.0, FS).shape == (4, 2, 6)


def test_sampler_draws_stay_in_range_and_unchosen_rows_are_identities():
    gen = torch.Generator().manual_seed(5)
    s = DynamicsSampler(p=0.6, p_limiter=0.25, generator=gen)
    d = s.draw(4000, FS)
    assert d.dtype == torch.float64 and d.shape == (4000, 6) and d.is_contiguous()
    thr, slope, knee, a_att, a_rel, m = d.unbind(1)
    on = slope > 0
    assert 0.55 < on.double().mean().item() < 0.65
    assert (slope[~on] == 0).all() and (m[~on] == 0).all()                 # an unchosen row is copied
    lim = slope[on] == 1.0
    assert 0.2 < lim.double().mean().item() < 0.3
    rest = slope[on][~lim]
    assert rest.min().item() >= 1 - 1 / 2.0 and rest.max().item() <= 1 - 1 / 20.0
    assert thr.min().item() >= -30.0 and thr.max().item() <= -6.0
    assert knee.min().item() >= 0.0 and knee.max().item() <= 12.0
    coeff = lambda ms: math.exp(-1000.0 / (ms * FS))
    assert a_att.min().item() >= coeff(1.0) * (1 - 1e-12) and a_att.max().item() <= coeff(30.0) * (1 + 1e-12)
    assert a_rel.min().item() >= coeff(50.0) * (1 - 1e-12) and a_rel.max().item() <= coeff(500.0) * (1 + 1e-12)
    assert m[on].min().item() >= 0.0 and m[on].max().item() <= 1.0
    # log-uniform times: the median sits at the geometric mean
    t_att = -1000.0 / (FS * torch.log(a_att))
    assert math.sqrt(30.0) * 0.9 < t_att.median().item() < math.sqrt(30.0) * 1.1
    # the same seed draws the same table; p = 0 draws identities only, p = 1 none
    assert torch.equal(DynamicsSampler(p=0.6, p_limiter=0.25, generator=torch.Generator().manual_seed(5)).draw(4000, FS), d)
    assert (DynamicsSampler(p=0.0).draw(50, FS)[:, [1, 5]] == 0).all()
    assert (DynamicsSampler(p=1.0).draw(50, FS)[:, 1] > 0).all()


def test_sampler_table_places_the_threshold_under_the_rows_peak():
    drawn = torch.tensor([[-12.0, 0.75, 6.0, 0.9, 0.99, 0.5], [-20.0, 1.0, 0.0, 0.9, 0.99, 1.0], [-12.0, 0.0, 6.0, 0.9, 0.99, 0.0],
                          [-12.0, 0.75, 6.0, 0.9, 0.99, 0.5], [-12.0, 0.75, 6.0, 0.9, 0.99, 0.5]], dtype=torch.float64)
    wav = torch.tensor([[0.5, -0.1, 0.0], [0.01, 0.1, -0.05], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [0.1, math.nan, 0.2]])
    t = DynamicsSampler.table(drawn, wav)
    assert t.dtype == torch.float64 and t.shape == (5, 6)
    assert t[0].tolist() == pytest.approx([20 * math.log10(0.5) - 12.0, 0.75, 6.0, 0.9, 0.99, 0.5 * 0.75 * 12.0], rel=1e-7)   # the peak is a float32
    assert t[1].tolist() == pytest.approx([20 * math.log10(float(np.float32(0.1))) - 20.0, 1.0, 0.0, 0.9, 0.99, 20.0], rel=1e-12)
    assert t[2, 1].item() == 0.0 and t[2, 5].item() == 0.0
    for row in (3, 4):                                                      # silent, or not finite: copied
        assert t[row, 1].item() == 0.0 and t[row, 5].item() == 0.0 and torch.isfinite(t[row]).all()


def test_sampler_rejects_bad_options():
    for kw, text in ((dict(p=1.5), "p must lie"), (dict(p_limiter=-0.1), "p_limiter must lie"),
                     (dict(threshold_rel_db=(-6, -30)), "threshold_rel_db must be"), (dict(threshold_rel_db=(-math.inf, 0)), "threshold_rel_db must be"),
                     (dict(threshold_rel_db=-20), "threshold_rel_db must be"),
                     (dict(ratio=(0.5, 4)), "ratio must be"), (dict(ratio=(2, math.inf)), "ratio must be"), (dict(ratio=(8, 2)), "ratio must be"),
                     (dict(knee_db=(-1, 3)), "knee_db must be"), (dict(knee_db=(0, math.inf)), "knee_db must be"),
                     (dict(attack_ms=(0, 10)), "attack_ms must be"), (dict(release_ms=(100, 50)), "release_ms must be"),
                     (dict(release_ms="slow"), "release_ms must be"), (dict(makeup=(-0.1, 1)), "makeup must be"),
                     (dict(makeup=(0, math.inf)), "makeup must be")):
        with pytest.raises(ValueError, match=text):
            DynamicsSampler(**kw)
    s = DynamicsSampler()
    assert (s.p, s.p_limiter, s.threshold_rel_db, s.ratio, s.knee_db, s.attack_ms, s.release_ms, s.makeup) == \
        (0.5, 0.2, (-30.0, -6.0), (2.0, 20.0), (0.0, 12.0), (1.0, 30.0), (50.0, 500.0), (0.0, 1.0))


def test_mixer_rejects_bad_dynamics_options_and_keeps_its_draws():
    bank = NoiseBank.from_arrays([np.ones(100, dtype=np.float32), np.ones(50, dtype=np.float32)])
    for bad in ("clean", "target", None, ""):
        with pytest.raises(ValueError, match="dynamics_on must be 'noisy' or 'both'"):
            DynamicMixer(_NoEngine(), bank, dynamics_on=bad)
    with pytest.raises(TypeError, match="dynamics must be a DynamicsSampler"):
        DynamicMixer(_NoEngine(), bank, dynamics="agc")
    m = DynamicMixer(_NoEngine(), bank)
    assert m.dynamics is None and m.dynamics_on == "noisy" and m.last_dynamics is None
    assert DynamicMixer(_NoEngine(), bank, dynamics=DynamicsSampler(), dynamics_on="both").dynamics_on == "both"
    # the draws of the mixer's own generator are what they were, and the draws keep their fields
    gen = lambda s=7: torch.Generator().manual_seed(s)
    d0 = DynamicMixer(_NoEngine(), bank, generator=gen(), level_db=(-35, -15)).draw(6)
    d1 = DynamicMixer(_NoEngine(), bank, generator=gen(), level_db=(-35, -15), dynamics=DynamicsSampler(generator=gen(3))).draw(6)
    assert type(d0) is type(d1) is Draw and d0.dynamics is None and d1.dynamics is None
    for a, b in zip(d0, d1):
        assert (a is None and b is None) or torch.equal(a, b)
    for cls in (Draw, SceneDraw, PathDraw):
        assert "dynamics" not in cls._fields and cls.dynamics is None


# ------------------------------------------------------------------ the library without a GPU
def test_symbols_tile_and_abi():
    lib = _lib.load()
    for name in ("cmgan_dynamics", "cmgan_dynamics_workspace_bytes", "cmgan_dynamics_tile"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.cmgan_dynamics_tile() == DYNAMICS_TILE == M.TILE == 64 and DYNAMICS_BLOCK == 64 * DYNAMICS_TILE
    assert lib.cmgan_abi_version() == _lib.ABI_VERSION >= 20


def test_workspace_formula():
    lib = _lib.load()
    ws = lambda B, L: int(lib.cmgan_dynamics_workspace_bytes(B, L))
    T = DYNAMICS_TILE
    for B in (1, 2, 5, 32, 65535):
        for L in (1, T - 1, T, T + 1, DYNAMICS_BLOCK, DYNAMICS_BLOCK + 1, 32000, 160000, DYNAMICS_MAX_L):
            assert ws(B, L) == dynamics_workspace_bytes(B, L) > 0 and ws(B, L) % 256 == 0, (B, L)
    assert ws(3, 32000) <= ws(4, 32000) <= ws(4, 32001 + T)
    up = lambda v: (v + 255) & ~255
    assert ws(32, 32000) == up(32 * 500 * 65 * 8) + up(32 * 500 * 8) + up(32 * 8 * 8)
    for B, L in ((0, 100), (-1, 100), (65536, 100), (1, 0), (1, -5), (1, DYNAMICS_MAX_L + 1)):
        assert ws(B, L) == dynamics_workspace_bytes(B, L) == 0, (B, L)


def test_library_rejects_bad_arguments_before_it_needs_a_handle():
    lib = _lib.load()
    x = np.zeros(8192, dtype=np.float32)
    k = np.zeros(8192, dtype=np.float32)
    y = np.zeros(8192, dtype=np.float32)
    lengths = np.zeros(8, dtype=np.int32)
    status = np.full(8, 7, dtype=np.int32)
    dyn = np.zeros(8 * 6 + 1, dtype=np.float64)
    peak = np.full(9, 7.0, dtype=np.float64)
    raw = np.zeros(1 << 20, dtype=np.uint8)
    base = (raw.ctypes.data + 255) & ~255
    px, pk, py, pl, pt, pd, pp = (a.ctypes.data for a in (x, k, y, lengths, status, dyn, peak))

    def call(x=px, B=2, L=1500, ldw=1500, key=pk, ldk=1500, lengths=pl, dyn=pd, y=py, ldo=1500, status=pt, peak=pp, ws=base,
             ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = dynamics_workspace_bytes(B, L) if 1 <= B <= 8 and 1 <= L <= 4096 else 4096
        rc = lib.cmgan_dynamics(None, x, B, L, ldw, key, ldk, lengths, dyn, y, ldo, status, peak, ws, ws_bytes, None)
        return rc, (lib.cmgan_last_error(None) or b"").decode()

    need = dynamics_workspace_bytes(2, 1500)
    cases = {
        "null pointer": [dict(x=None), dict(dyn=None), dict(y=None)],
        "4-byte aligned": [dict(x=px + 2), dict(key=pk + 1), dict(y=py + 1), dict(lengths=pl + 1), dict(status=pt + 3)],
        "8-byte aligned": [dict(dyn=pd + 4), dict(peak=pp + 4)],
        "need 1 <= B": [dict(B=0), dict(B=-3), dict(B=65536), dict(L=0), dict(L=-1), dict(ldw=1499), dict(ldo=1499), dict(ldk=1499),
                        dict(ldk=0)],
        "rows of up to": [dict(L=DYNAMICS_MAX_L + 1, ldw=2 ** 31 - 1, ldo=2 ** 31 - 1, ldk=2 ** 31 - 1)],
        "wav and out overlap": [dict(y=px + 4), dict(y=px + 4 * 1500), dict(y=px, ldo=1501), dict(y=px + 4 * 2999), dict(x=py + 4 * 100)],
        "key and out overlap": [dict(y=pk + 4), dict(y=pk, ldo=1501), dict(key=py + 4 * 2999), dict(key=px + 4, y=px)],
        "workspace": [dict(ws=None), dict(ws=base + 64), dict(ws_bytes=need - 1), dict(ws_bytes=0)],
    }
    for text, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == BADARG and text in msg, (kw, rc, msg)
    # everything in order: only the handle is missing - nothing was enqueued, nothing was written
    for kw in (dict(), dict(key=None, ldk=0), dict(lengths=None), dict(status=None), dict(peak=None), dict(y=px), dict(y=pk),
               dict(y=px, key=px), dict(y=px, ldw=2000, ldo=2000), dict(y=px + 4 * 3000), dict(key=px), dict(B=1, L=1, ldw=1, ldk=1, ldo=1)):
        rc, msg = call(**kw)
        assert rc == BADARG and "null handle" in msg, (kw, rc, msg)
    assert not y.any() and (status == 7).all() and (peak == 7.0).all()


# ------------------------------------------------------------------ Engine.dynamics's argument rules
def test_check_dynamics_args():
    wav = torch.zeros(3, 2000)
    dyn = torch.zeros(3, 6, dtype=torch.float64)
    i32 = lambda n=3: torch.zeros(n, dtype=torch.int32)
    assert check_dynamics_args(CPU, wav, dyn) == (3, 2000)
    assert check_dynamics_args(CPU, wav, dyn, torch.zeros(3, 2000), i32(), torch.zeros(3, 2000)) == (3, 2000)
    assert check_dynamics_args(CPU, wav, dyn, out=wav) == (3, 2000)
    key = torch.zeros(3, 2000)
    assert check_dynamics_args(CPU, wav, dyn, key, out=key) == (3, 2000)    # the "both" order of the mixer, the other way round
    assert check_dynamics_args(CPU, wav, dyn, wav, out=wav) == (3, 2000)
    view = torch.zeros(3, 2500)[:, :2000]                                   # a row stride larger than L
    assert check_dynamics_args(CPU, view, dyn, view, out=view) == (3, 2000)
    assert check_dynamics_args(CPU, torch.zeros(1, 7), torch.zeros(1, 6, dtype=torch.float64)) == (1, 7)
    with pytest.raises(TypeError, match="wav: expected a torch.Tensor"):
        check_dynamics_args(CPU, np.zeros((3, 2000), dtype=np.float32), dyn)
    with pytest.raises(TypeError, match="wav: expected float32"):
        check_dynamics_args(CPU, wav.double(), dyn)
    with pytest.raises(RuntimeError, match="wav: tensor is on cpu"):
        check_dynamics_args(torch.device("cuda:0"), wav, dyn)
    for bad in (torch.zeros(2000), torch.zeros(1, 3, 2000), torch.zeros(0, 2000), torch.zeros(3, 0)):
        with pytest.raises(ValueError, match="wav: expected \\[B, L\\]"):
            check_dynamics_args(CPU, bad, dyn)
    with pytest.raises(ValueError, match="at most 65535 rows"):
        check_dynamics_args(CPU, torch.zeros(1, 1).expand(65536, 1), dyn)
    for bad in (torch.zeros(3, 4000)[:, ::2], torch.zeros(2000, 3).t(), torch.zeros(1, 2000).expand(3, 2000)):
        with pytest.raises(ValueError, match="wav: rows must be contiguous"):
            check_dynamics_args(CPU, bad, dyn)
    with pytest.raises(TypeError, match="dyn: expected float64"):
        check_dynamics_args(CPU, wav, dyn.float())
    for bad in (torch.zeros(3, 5), torch.zeros(2, 6), torch.zeros(3, 1, 6), torch.zeros(18)):
        with pytest.raises(ValueError, match="dyn: expected \\[3, 6\\]"):
            check_dynamics_args(CPU, wav, bad.double())
    with pytest.raises(ValueError, match="dyn: must be contiguous"):
        check_dynamics_args(CPU, wav, torch.zeros(3, 12, dtype=torch.float64)[:, ::2])
    with pytest.raises(TypeError, match="key: expected float32"):
        check_dynamics_args(CPU, wav, dyn, key.double())
    with pytest.raises(ValueError, match="key: expected \\[3, 2000\\]"):
        check_dynamics_args(CPU, wav, dyn, torch.zeros(3, 1999))
    with pytest.raises(ValueError, match="key: rows must be contiguous"):
        check_dynamics_args(CPU, wav, dyn, torch.zeros(3, 4000)[:, ::2])
    with pytest.raises(TypeError, match="lengths: expected int32"):
        check_dynamics_args(CPU, wav, dyn, None, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="lengths: expected \\[3\\]"):
        check_dynamics_args(CPU, wav, dyn, None, i32(4))
    with pytest.raises(ValueError, match="lengths: must be contiguous"):
        check_dynamics_args(CPU, wav, dyn, None, torch.zeros(6, dtype=torch.int32)[::2])
    with pytest.raises(TypeError, match="out: expected float32"):
        check_dynamics_args(CPU, wav, dyn, out=torch.zeros(3, 2000, dtype=torch.float64))
    with pytest.raises(ValueError, match="out: expected \\[3, 2000\\]"):
        check_dynamics_args(CPU, wav, dyn, out=torch.zeros(3, 2001))
    with pytest.raises(ValueError, match="out: rows must be contiguous"):
        check_dynamics_args(CPU, wav, dyn, out=torch.zeros(3, 4000)[:, ::2])
    both = torch.zeros(3, 4000)
    with pytest.raises(ValueError, match="out: overlaps wav"):
        check_dynamics_args(CPU, both[:, :2000], dyn, out=both[:, 1000:3000])
    with pytest.raises(ValueError, match="out: overlaps wav"):
        check_dynamics_args(CPU, both[:, :2000], dyn, out=both.view(-1)[:6000].view(3, 2000))   # the same start, another stride
    with pytest.raises(ValueError, match="out: overlaps key"):
        check_dynamics_args(CPU, wav, dyn, both[:, :2000], out=both[:, 1999:3999])
    with pytest.raises(ValueError, match="out: overlaps wav"):                   # spans are judged, as the library does: interleaved rows count
        check_dynamics_args(CPU, both[:, :2000], dyn, out=both[:, 2000:])
