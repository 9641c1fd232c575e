"""CPU side of the noise suppressor (cmgan_amd/csrc/suppress.hip; include/cmgan_hip.h, "Suppression"): the numpy model the
GPU tests compare the kernels with (tests/suppress_model.py) against the facts the definition promises, its two E1 against
scipy.special.exp1, the conditions on every row the GPU tests judge, the sampler's ranges, and every argument error of
cmgan_suppress, Engine.suppress, suppress_params, SuppressorSampler and DynamicMixer(suppressor=...), all of which are
judged before a handle or a GPU is needed."""
import math

import numpy as np
import pytest
import torch

import suppress_model as M
from cmgan_amd import _lib
from cmgan_amd.engine import (SUPPRESS_MAX_WINDOW, SUPPRESS_N_FFT, SUPPRESS_RULES, check_suppress_args, suppress_frames,
                              suppress_workspace_bytes)
from cmgan_amd.mixing import DynamicMixer, NoiseBank, SuppressDraw, SuppressorSampler, suppress_n_fft, suppress_params

BADARG = -1
CPU = torch.device("cpu")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ the model against the definition's promises
def test_a_gain_floor_of_one_reproduces_the_input():
    """w[k]^2 + w[k + h]^2 = 1: with every gain 1 the frames add up to the row."""
    for N in M.N_FFTS:
        x = M.noisy(3, 3 * N + 17)
        res = M.suppress(x, len(x), M.params(rule=M.LOGMMSE, g_min=1.0), N)
        E = M.slack(res)
        err = float(np.abs(res.w - x.astype(M.LD)).max())
        print(f"[suppress] g_min = 1, N = {N}: max |w - x| = {err:.3e}, E = {E:.3e}")
        assert (res.G == 1.0).all() and err <= E and E <= M.condition(res)
        assert np.array_equal(_bits(res.y), _bits(x))


def test_rule_0_is_a_bit_copy():
    x = M.noisy(4, 700).copy()
    x[13] = np.nan
    res = M.suppress(x, 700, M.params(rule=M.OFF), 256)
    assert np.array_equal(_bits(res.y), _bits(x)) and (res.G == 1.0).all() and res.G.shape == (M.n_frames(700, 256), 129)


def test_gains_on_stationary_noise_lie_between_the_floor_and_one_and_fall_with_the_bias():
    x = M.white(5, 16000)
    for rule in (M.WIENER, M.SPECSUB, M.LOGMMSE):
        means = []
        for bias in (0.5, 1.5, 4.0):
            res = M.suppress(x, len(x), M.params(rule=rule, bias=bias, g_min=0.05, D=30), 256)
            G = res.G.astype(np.float64)
            assert G.min() >= 0.05 and G.max() <= 1.0
            means.append(float(G[40:].mean()))
        print(f"[suppress] white noise, rule {rule}: mean gain at bias 0.5 / 1.5 / 4 = {means}")
        assert 0.05 < means[2] < means[1] < means[0] < 1.0


def test_gains_never_leave_the_floor_and_one():
    M.build_rows()
    for name, row in M.ROWS.items():
        res, _, _ = M.case(name)
        if res.G.size:
            g_min = 1.0 if int(row.p[0]) == M.OFF else row.p[5]
            for G in (res.G, res.G_d, res.G_d2):
                assert float(G.min()) >= g_min and float(G.max()) <= 1.0, name


def test_a_window_of_one_frame_tracks_the_periodogram():
    x = M.noisy(6, 1500)
    p = M.params(rule=M.WIENER, D=1, bias=2.0, a_n=0.7)
    res = M.suppress(x, 1500, p, 256)
    K = M.rfft(M.frames(x, 1500, 256, M.LD))
    A = K.real ** 2 + K.imag ** 2
    P, prev = np.empty_like(A), A[0]
    for t in range(len(A)):
        P[t] = prev = M.LD(0.7) * prev + (M.LD(1.0) - M.LD(0.7)) * A[t]
    assert np.array_equal(res.lam, np.maximum(M.LD(2.0) * P, M.LD(M.LAM_MIN)))


def _loop_model(x, n, p, N, T=np.float64):
    """The definition as plain Python loops over single frames and bins (a direct DFT sum per bin), float64."""
    h, F, Tb = N // 2, N // 2 + 1, M.n_frames(n, N)
    rule, a_dd, a_n, D, bias, g_min, xi_min = (float(v) for v in p)
    w = [math.sin(math.pi * k / N) for k in range(N)]
    xt = lambda i: float(x[i]) if 0 <= i < n else 0.0
    Y = [[sum(xt((t - 1) * h + k) * w[k] * complex(math.cos(2 * math.pi * ((f * k) % N) / N), -math.sin(2 * math.pi * ((f * k) % N) / N))
              for k in range(N)) for f in range(F)] for t in range(Tb)]
    G = [[0.0] * F for _ in range(Tb)]
    for f in range(F):
        P, Ps, Gp, gp = None, [], 0.0, 0.0
        for t in range(Tb):
            A = Y[t][f].real ** 2 + Y[t][f].imag ** 2
            P = a_n * (A if P is None else P) + (1.0 - a_n) * A
            Ps.append(P)
            lam = max(bias * min(Ps[max(0, t - int(D) + 1):]), M.LAM_MIN)
            gam = min(A / lam, M.GAMMA_MAX)
            xi = (1.0 - a_dd) * max(gam - 1.0, 0.0)
            if t > 0:
                xi = a_dd * (Gp * Gp) * gp + xi
            xi = max(xi, xi_min)
            q = xi / (1.0 + xi)
            g = q if rule == 1 else (math.sqrt(q) if rule == 2 else
                                     min(q * math.exp(float(M.e1_d(np.array([max(q * gam, M.V_MIN)]))[0]) / 2.0), 1.0))
            G[t][f] = Gp = max(g, g_min)
            gp = gam
    z = [[sum((1.0 if f in (0, h) else 2.0) * (G[t][f] * Y[t][f] * complex(math.cos(2 * math.pi * ((f * k) % N) / N),
                                                                          math.sin(2 * math.pi * ((f * k) % N) / N))).real
              for f in range(F)) / N for k in range(N)] for t in range(Tb)]
    y = [z[i // h][i % h + h] * w[i % h + h] + z[i // h + 1][i % h] * w[i % h] for i in range(n)]
    return np.array(y), np.array(G)


@pytest.mark.parametrize("rule", [M.WIENER, M.SPECSUB, M.LOGMMSE])
def test_model_agrees_with_plain_loops_on_a_tiny_case(rule):
    N, n = 256, 4 * 128 - 9                                              # 5 frames
    x = M.noisy(7 + rule, n)
    p = M.params(rule=rule, D=2, a_dd=0.9)
    assert M.n_frames(n, N) == 5
    res = M.suppress(x, n, p, N)
    y, G = _loop_model(x, n, p, N)
    E, EG = M.slack(res), M.gain_slack(res)
    err, err_g = float(np.abs(y.astype(M.LD) - res.w).max()), float(np.abs(G.astype(M.LD) - res.G).max())
    print(f"[suppress] loops against the model, rule {rule}: |y - w| = {err:.3e} (E = {E:.3e}), |G - G_w| = {err_g:.3e} (E_G = {EG:.3e})")
    assert err <= E and err_g <= EG


def test_e1_against_scipy():
    """Worst absolute error on a log grid of 40001 points over [2^-30, 45] and 2001 points across the split: the float64
    formulas 8.6e-16 against scipy, the long-double ones 3.6e-15 (scipy's own rounding at the small arguments, where E1 is
    about 20 and a float64 ulp 3.6e-15), the two against each other 2.7e-15.  The bound asserted is that ulp, 4e-15.  Only
    the absolute error reaches the gain; relative to E1 the two formulas differ by up to 1.8e-14 (just below the split,
    where the series cancels from 1.3 to 0.05)."""
    from scipy.special import exp1
    x = np.concatenate([np.exp(np.linspace(np.log(2.0 ** -30), np.log(45.0), 40001)), np.linspace(1.5, 2.5, 2001)])
    ref = exp1(x)
    d, w = M.e1_d(x), M.e1_w(x)
    err_d, err_w = float(np.abs(d - ref).max()), float(np.abs(w.astype(np.float64) - ref).max())
    err_dw = float(np.abs(d.astype(M.LD) - w).astype(np.float64).max())
    rel = float((np.abs(d.astype(M.LD) - w) / w).astype(np.float64).max())
    print(f"[suppress] E1: |d - scipy| = {err_d:.3e}, |w - scipy| = {err_w:.3e}, |d - w| = {err_dw:.3e}, relative {rel:.3e}")
    assert err_d <= 4e-15 and err_w <= 4e-15 and err_dw <= 4e-15
    c = M.e1_coefficients()
    assert len(c) == M.E1_TERMS == 26 and c[0] == 1.0 and c[1] == -0.25 and c[2] == 1.0 / 18.0 and M.E1_DEPTH == 40 and M.E1_SPLIT == 2.0


# ------------------------------------------------------------------ the conditions on every registered row
def test_every_registered_row_meets_the_conditions():
    M.build_rows()
    assert {f"len-{n}" for n in (1, 127, 128, 129, 256, 677, 2000, 0)} <= set(M.ROWS)
    worst_E = worst_G = 0.0
    for name, row in M.ROWS.items():
        res, E, EG = M.case(name)
        cap = M.condition(res)
        print(f"[suppress] {name}: n = {row.n}, N = {row.N}, rule {int(row.p[0])}, E = {E:.3e} (cap {cap:.3e}), E_G = {EG:.3e}")
        assert E <= cap, f"{name}: E = {E:.3e} above 2^-10 ulp32(rms) / 2 = {cap:.3e}"
        assert EG <= M.EG_MAX, f"{name}: E_G = {EG:.3e} above 2^-30"
        assert res.w.shape == (row.n,) and res.G.shape == (M.n_frames(row.n, row.N), row.N // 2 + 1)
        assert np.isfinite(res.w.astype(np.float64)).all()
        worst_E, worst_G = max(worst_E, E / cap if cap else 0.0), max(worst_G, EG)
    print(f"[suppress] the largest E / cap = {worst_E:.3e}, the largest E_G = {worst_G:.3e}")
    assert np.abs(M.ROWS["loud"].x).max() == 4.0
    assert not M.ROWS["silence-start"].x[:700].any() and not M.ROWS["silence-inside"].x[600:1300].any()


# ------------------------------------------------------------------ suppress_params and the sampler
def test_suppress_params():
    t = suppress_params("logmmse", fs=16000)
    assert t.dtype == torch.float64 and tuple(t.shape) == (7,)
    assert t.tolist() == [3.0, 0.98, 0.8, 62.0, 1.5, 10.0 ** -1.0, 10.0 ** -2.5]
    assert suppress_params("off")[0] == 0.0 and suppress_params("wiener")[0] == 1.0 and suppress_params("specsub")[0] == 2.0
    assert SUPPRESS_RULES == {"off": M.OFF, "wiener": M.WIENER, "specsub": M.SPECSUB, "logmmse": M.LOGMMSE}
    assert suppress_params("wiener", window_s=1.0, fs=48000)[3] == 94.0 and suppress_n_fft(48000) == 1024 and suppress_n_fft(31999) == 512
    assert suppress_params("wiener", window_s=100.0)[3] == 128.0 and suppress_params("wiener", window_s=0.0)[3] == 1.0
    assert suppress_params("wiener", window_s=1.0, fs=16000, n_fft=256)[3] == 125.0
    rows = suppress_params(torch.tensor([0.0, 1.0, 2.0]), floor_db=torch.tensor([-20.0, -6.0, 0.0]), bias=2.0)
    assert tuple(rows.shape) == (3, 7) and rows[:, 0].tolist() == [0.0, 1.0, 2.0] and rows[2, 5] == 1.0 and (rows[:, 4] == 2.0).all()
    assert np.array_equal(M.params(), suppress_params("logmmse", window_s=20 * 128 / 16000, n_fft=256).numpy())
    with pytest.raises(ValueError, match="rule must be one of"):
        suppress_params("mmse")
    for bad in (0, -16000, 16000.5, True):
        with pytest.raises(ValueError, match="fs must be"):
            suppress_params("wiener", fs=bad)
    for bad in (400, 2048, 0, True, 512.5):
        with pytest.raises(ValueError, match="n_fft must be one of"):
            suppress_params("wiener", n_fft=bad)


def test_sampler_ranges_and_options():
    gen = torch.Generator().manual_seed(3)
    s = SuppressorSampler(p=0.7, generator=gen)
    d = s.draw(4000, 16000)
    assert isinstance(d, SuppressDraw) and d.n_fft == 512 and d.table.dtype == torch.float64 and tuple(d.table.shape) == (4000, 7)
    assert d.table.is_contiguous()
    t = d.table.numpy()
    rule = t[:, 0]
    assert set(rule.tolist()) == {0.0, 1.0, 2.0, 3.0} and abs((rule == 0).mean() - 0.3) < 0.03
    for r in (1.0, 2.0, 3.0):
        assert abs((rule == r).mean() - 0.7 / 3) < 0.03
    for col, (lo, hi) in ((1, s.a_dd), (2, s.a_n), (4, s.bias)):
        assert t[:, col].min() >= lo and t[:, col].max() <= hi and t[:, col].max() - t[:, col].min() > 0.9 * (hi - lo)
    assert (t[:, 3] == np.floor(t[:, 3])).all() and t[:, 3].min() >= round(0.4 * 16000 / 256) and t[:, 3].max() <= round(1.5 * 16000 / 256)
    assert t[:, 5].min() >= 10 ** (-25 / 20) - 1e-15 and t[:, 5].max() <= 10 ** (-6 / 20) + 1e-15
    assert np.allclose(t[:, 6], 10 ** -2.5, rtol=1e-15)
    assert SuppressorSampler(p=0.0).draw(50, 16000).table[:, 0].eq(0).all()
    assert SuppressorSampler(p=1.0, p_wiener=0.0, p_specsub=0.0).draw(50, 48000).table[:, 0].eq(3).all()
    assert SuppressorSampler(p=1.0, p_wiener=1.0, p_specsub=0.0).draw(50, 48000).n_fft == 1024
    for bad in (-0.1, 1.5, math.nan):
        for name in ("p", "p_wiener", "p_specsub"):
            with pytest.raises(ValueError, match=f"{name} must lie in"):
                SuppressorSampler(**{name: bad})
    with pytest.raises(ValueError, match="p_wiener \\+ p_specsub must not exceed 1"):
        SuppressorSampler(p_wiener=0.6, p_specsub=0.6)
    for name, bads in (("floor_db", ((-10.0, 3.0), (-6.0, -10.0), (-math.inf, -6.0), -20.0, (math.nan, -6.0))),
                       ("bias", ((0.0, 2.0), (1.0, 17.0), (3.0, 2.0), 1.5)),
                       ("a_dd", ((0.5, 1.0), (-0.1, 0.5), (0.9, 0.8), 0.98)), ("a_n", ((0.5, 1.0), (-0.1, 0.5), (math.nan, 0.5))),
                       ("window_s", ((0.0, 1.0), (2.0, 1.0), (1.0, math.inf), 1.0))):
        for bad in bads:
            with pytest.raises(ValueError, match=f"{name} must be"):
                SuppressorSampler(**{name: bad})
    for bad in (1.0, math.inf, -math.inf, math.nan, True, "-25"):
        with pytest.raises(ValueError, match="xi_min_db must be"):
            SuppressorSampler(xi_min_db=bad)


# ------------------------------------------------------------------ the library without a GPU
def test_symbols_and_constants():
    lib = _lib.load()
    for name in ("cmgan_suppress", "cmgan_suppress_max_window", "cmgan_suppress_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.cmgan_suppress_max_window() == SUPPRESS_MAX_WINDOW == M.MAX_WINDOW == 128 and SUPPRESS_N_FFT == M.N_FFTS
    assert lib.cmgan_abi_version() == _lib.ABI_VERSION == 23
    import os
    import re
    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "cmgan_hip.h")).read()
    assert re.search(r"#define CMGAN_ABI_VERSION (\d+)", header).group(1) == "23"
    for B, L, N in ((1, 1, 256), (32, 32000, 512), (3, 2000, 1024), (65535, 100, 256), (2, 2 ** 31 - 1 - 2048, 1024)):
        T, F = suppress_frames(L, N), N // 2 + 1
        assert T == -(-L // (N // 2)) + 1
        assert lib.cmgan_suppress_workspace_bytes(B, L, N) == suppress_workspace_bytes(B, L, N) >= 24 * B * T * F
    for B, L, N in ((0, 100, 256), (65536, 100, 256), (1, 0, 256), (1, 2 ** 31 - 2047, 256), (1, 100, 400), (1, 100, 2048)):
        assert lib.cmgan_suppress_workspace_bytes(B, L, N) == suppress_workspace_bytes(B, L, N) == 0
    import cmgan_amd.mixing as mixing
    assert {"SuppressorSampler", "SuppressDraw", "suppress_params", "suppress_n_fft"} <= set(mixing.__all__)


def test_library_rejects_bad_arguments_before_it_needs_a_handle():
    lib = _lib.load()
    x, y, key = (np.zeros(8192, dtype=np.float32) for _ in range(3))
    lengths = np.zeros(8, dtype=np.int32)
    status = np.full(8, 7, dtype=np.int32)
    table = np.zeros(8 * 7, dtype=np.float64)
    gain = np.full(2 * 13 * 129, 7.0, dtype=np.float64)
    need = lib.cmgan_suppress_workspace_bytes(2, 1500, 256)
    raw = np.zeros(need + 512, dtype=np.uint8)
    pw = (raw.ctypes.data + 255) & ~255
    px, py, pk, pl, pt, pb, pg = (a.ctypes.data for a in (x, y, key, lengths, status, table, gain))

    def call(x=px, B=2, L=1500, ldx=1500, key=None, ldk=0, lengths=pl, table=pb, n_fft=256, y=py, ldy=1600, status=pt, gain=pg,
             ws=pw, ws_bytes=need):
        rc = lib.cmgan_suppress(None, x, B, L, ldx, key, ldk, lengths, table, n_fft, y, ldy, status, gain, ws, ws_bytes, None)
        return rc, (lib.cmgan_last_error(None) or b"").decode()

    cases = {
        "null pointer": [dict(x=None), dict(table=None), dict(y=None)],
        "4-byte aligned": [dict(x=px + 2), dict(y=py + 1), dict(key=pk + 2, ldk=1500), dict(lengths=pl + 1), dict(status=pt + 2)],
        "8-byte aligned": [dict(table=pb + 4), dict(gain=pg + 4)],
        "n_fft must be": [dict(n_fft=0), dict(n_fft=400), dict(n_fft=128), dict(n_fft=2048), dict(n_fft=-256)],
        "need 1 <= B": [dict(B=0), dict(B=-3), dict(B=65536), dict(L=0), dict(L=-1), dict(ldx=1499), dict(ldy=1499),
                        dict(key=pk, ldk=1499), dict(key=pk, ldk=0)],
        "samples are supported": [dict(B=1, L=2 ** 31 - 2047, ldx=2 ** 31, ldy=2 ** 31)],
        "x and y overlap": [dict(y=px + 4), dict(y=px + 4 * 1500), dict(y=px + 4 * 2999), dict(x=py + 4 * 100), dict(x=py + 4 * 3099),
                            dict(y=px, ldy=1500, ldx=1501), dict(y=px, ldy=1600)],
        "key and y overlap": [dict(key=py + 4, ldk=1500), dict(key=py, ldk=1500), dict(key=py + 4 * 3099, ldk=1500)],
        "workspace": [dict(ws=None), dict(ws=pw + 8), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(n_fft=512)],
    }
    for text, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == BADARG and "cmgan_suppress" in msg and text in msg, (kw, rc, msg)
    # everything in order: only the handle is missing - nothing was enqueued, nothing was written
    for kw in (dict(), dict(lengths=None), dict(status=None), dict(gain=None), dict(y=px, ldy=1500), dict(key=pk, ldk=1500),
               dict(key=pk, ldk=2000), dict(key=py, ldk=1600), dict(key=px, ldk=1500), dict(y=px + 4 * 3000), dict(x=py + 4 * 3100),
               dict(B=1, L=1, ldx=1, ldy=1), dict(ldx=2000, ldy=2000), dict(ws_bytes=need + 512)):
        rc, msg = call(**kw)
        assert rc == BADARG and "null handle" in msg, (kw, rc, msg)
    assert not y.any() and (status == 7).all() and (gain == 7.0).all()


# ------------------------------------------------------------------ Engine.suppress's argument rules
def test_check_suppress_args():
    wav = torch.zeros(3, 2000)
    tab = torch.zeros(3, 7, dtype=torch.float64)
    i32 = lambda n=3: torch.zeros(n, dtype=torch.int32)
    assert check_suppress_args(CPU, wav, tab) == (3, 2000)
    assert check_suppress_args(CPU, wav, tab, 256, i32(), torch.zeros(3, 2000), wav) == (3, 2000)
    assert check_suppress_args(CPU, torch.zeros(3, 2500)[:, :2000], tab, 1024, out=torch.zeros(3, 2500)[:, :2000]) == (3, 2000)
    key = torch.zeros(3, 2000)
    assert check_suppress_args(CPU, wav, tab, key=key, out=key) == (3, 2000)
    for bad in (400, 0, 2048, 512.5, True, None, "512"):
        with pytest.raises(ValueError, match="n_fft must be one of"):
            check_suppress_args(CPU, wav, tab, bad)
    with pytest.raises(TypeError, match="wav: expected a torch.Tensor"):
        check_suppress_args(CPU, np.zeros((3, 2000), dtype=np.float32), tab)
    with pytest.raises(TypeError, match="wav: expected float32"):
        check_suppress_args(CPU, wav.double(), tab)
    with pytest.raises(RuntimeError, match="wav: tensor is on cpu"):
        check_suppress_args(torch.device("cuda:0"), wav, tab)
    for bad in (torch.zeros(2000), torch.zeros(1, 3, 2000), torch.zeros(0, 2000), torch.zeros(3, 0)):
        with pytest.raises(ValueError, match="wav: expected \\[B, L\\]"):
            check_suppress_args(CPU, bad, tab)
    with pytest.raises(ValueError, match="at most 65535 rows"):
        check_suppress_args(CPU, torch.zeros(1, 1).expand(65536, 1), tab)
    for bad in (torch.zeros(3, 4000)[:, ::2], torch.zeros(2000, 3).t()):
        with pytest.raises(ValueError, match="wav: rows must be contiguous"):
            check_suppress_args(CPU, bad, tab)
    with pytest.raises(TypeError, match="table: expected a torch.Tensor"):
        check_suppress_args(CPU, wav, None)
    with pytest.raises(TypeError, match="table: expected float64"):
        check_suppress_args(CPU, wav, tab.float())
    for bad in (torch.zeros(3, 6, dtype=torch.float64), torch.zeros(2, 7, dtype=torch.float64), torch.zeros(21, dtype=torch.float64)):
        with pytest.raises(ValueError, match="table: expected \\[3, 7\\]"):
            check_suppress_args(CPU, wav, bad)
    with pytest.raises(ValueError, match="table: .*contiguous"):
        check_suppress_args(CPU, wav, torch.zeros(3, 14, dtype=torch.float64)[:, ::2])
    for bad, kind, text in ((torch.zeros(3, dtype=torch.int64), TypeError, "expected int32"), (2, TypeError, "expected a torch.Tensor"),
                            (i32(4), ValueError, "expected \\[3\\]"), (torch.zeros(6, dtype=torch.int32)[::2], ValueError, "contiguous")):
        with pytest.raises(kind, match=f"lengths: .*{text}"):
            check_suppress_args(CPU, wav, tab, lengths=bad)
    for name in ("key", "out"):
        with pytest.raises(TypeError, match=f"{name}: expected float32"):
            check_suppress_args(CPU, wav, tab, **{name: torch.zeros(3, 2000, dtype=torch.float64)})
        with pytest.raises(ValueError, match=f"{name}: expected \\[3, 2000\\]"):
            check_suppress_args(CPU, wav, tab, **{name: torch.zeros(3, 2001)})
        with pytest.raises(ValueError, match=f"{name}: rows must be contiguous"):
            check_suppress_args(CPU, wav, tab, **{name: torch.zeros(3, 4000)[:, ::2]})
    big = torch.zeros(3, 2600)
    with pytest.raises(ValueError, match="out: overlaps wav"):
        check_suppress_args(CPU, big[:, :2000], tab, out=big[:, 500:2500])
    with pytest.raises(ValueError, match="out: overlaps wav"):
        check_suppress_args(CPU, big[:, :2000], tab, out=big.view(-1)[:6000].view(3, 2000))
    with pytest.raises(ValueError, match="out: overlaps key"):
        check_suppress_args(CPU, wav, tab, key=big[:, :2000], out=big[:, 500:2500])


# ------------------------------------------------------------------ DynamicMixer's new arguments
class _NoEngine:
    device = CPU


def test_mixer_rejects_bad_suppressor_options():
    bank = NoiseBank.from_arrays([np.ones(100, dtype=np.float32), np.ones(50, dtype=np.float32)])
    mk = lambda **kw: DynamicMixer(_NoEngine(), bank, **kw)
    for bad in ("clean", "target", None, True):
        with pytest.raises(ValueError, match="suppressor_on must be 'noisy' or 'both'"):
            mk(suppressor_on=bad)
    for bad in (0.5, "wiener", (0.01, 0.2), SuppressorSampler):
        with pytest.raises(TypeError, match="suppressor must be a SuppressorSampler or None"):
            mk(suppressor=bad)
    m = mk()
    assert m.suppressor is None and m.suppressor_on == "noisy" and m.last_suppression is None
    s = SuppressorSampler()
    m = mk(suppressor=s, suppressor_on="both", sample_rate=48000)
    assert m.suppressor is s and m.suppressor_on == "both" and m.last_suppression is None
