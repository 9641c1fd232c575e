"""CPU side of the intelligibility loss (cmgan_amd/csrc/stoiloss.hip; include/cmgan_hip.h, "Intelligibility loss"): the numpy
model the GPU tests judge by (tests/stoiloss_model.py) against the host STOI of cmgan_amd.metrics, against float64 autograd
through a plain torch restatement and against central differences; the margins of every case; the settings object, the
argument rules and the library's own refusals.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import stoiloss_model as M
from cmgan_amd import _lib
from cmgan_amd import metrics as host_metrics
from cmgan_amd.engine import STOI_MIN_L, check_stoi_loss_args, check_stoi_settings, stoi_frames
from cmgan_amd.training import AuxLoss

CPU = torch.device("cpu")
BADARG, UNSUPPORTED = -1, -3
K = M.K_WEIGHT / 4
JUDGED = ("a", "b", "c", "d", "a16")        # the cases with a value
#: the worst |autograd - d| over the judged cases and both variants, relative to the row's largest gradient sample, was
#: measured here at 5.2e-13 (case a, extended; 2.6e-13 for case a as STOI, below 1e-14 elsewhere); the gate is ten times that
AUTOGRAD_GATE = 5.2e-12


# ------------------------------------------------------------------ the model against the host metric
@pytest.mark.parametrize("name", JUDGED)
def test_value_equals_the_host_stoi(name):
    est, ref = M.case(name)
    want = host_metrics.stoi(ref.astype(np.float64), est.astype(np.float64), M.FS)
    m = M.row_model(M.registered(name), False, K)
    print(f"case {name}: model = {float(m.value):.15f}, host = {want:.15f}, bound = {m.bound:.2e}")
    assert m.status == 0 and abs(float(m.value) - want) <= 1e-12
    assert abs(float(M._eval(name, False, K, "d").value) - want) <= 1e-12


# ------------------------------------------------------------------ the model against autograd
def torch_total(est, ref, extended, k):
    """The definitions restated in torch float64; (value, dA / de) of one row."""
    h, hann, bands = M.tables()
    e = torch.tensor(est, dtype=torch.float64, requires_grad=True)
    r = torch.tensor(ref, dtype=torch.float64)
    L = len(est)
    n10, nS = M.n10_of(L), M.frames_of(L)
    taps = torch.tensor(h[::-1].copy())[None, None, :]
    w = torch.tensor(hann)

    def resample(x):                                    # conv1d over the zero-stuffed signal: out[n] = sum_m u[m] h[8 (n + 11) - m]
        pad = torch.zeros(256, dtype=torch.float64)                     # 80 on the left, the rest never reached on the right
        u = torch.cat([pad[:80], torch.stack([x] + [torch.zeros_like(x)] * 4, dim=1).reshape(-1), pad])
        return torch.nn.functional.conv1d(u[None, None, :], taps, stride=8)[0, 0, :n10]
    e10, r10 = resample(e), resample(r)
    starts = torch.arange(nS) * M.HOP
    with torch.no_grad():
        idx = (starts[:, None] - 1 + torch.arange(M.N)[None, :]) % n10
        level = 20.0 * torch.log10((r10[idx] * w).pow(2).sum(1).sqrt() / 16.0)
        keep = torch.nonzero((level - level.max()) + M.DYN > 0)[:, 0]
    Kf = len(keep)
    grab = starts.index_select(0, keep)[:, None] + torch.arange(M.N)[None, :]

    def rebuild(x10):
        frames = x10[grab] * w                                          # [K, 256]
        out = torch.zeros((Kf + 1) * M.HOP, dtype=torch.float64)
        out = out.index_add(0, (starts[:Kf, None] + torch.arange(M.N)[None, :]).reshape(-1), frames.reshape(-1))
        fr = out.unfold(0, M.N, M.HOP)[:Kf - 1] * w
        p = (torch.fft.rfft(fr, M.NFFT, dim=1) / w.sum()).abs().pow(2)
        return torch.stack([p[:, lo:hi].sum(1).sqrt() for lo, hi in bands])   # [15, K - 1]
    X, Y = rebuild(r10), rebuild(e10)
    Xw, Yw = X.unfold(1, M.SEG, 1), Y.unfold(1, M.SEG, 1)               # [15, nW, 30]
    if not extended:
        alpha = (Xw.pow(2).sum(2, keepdim=True) / Yw.pow(2).sum(2, keepdim=True)).sqrt()
        yp = torch.minimum(Yw * alpha, Xw * (1.0 + 10.0 ** (15.0 / 20.0)))
        xn, yn = Xw - Xw.mean(2, keepdim=True), yp - yp.mean(2, keepdim=True)
        xn, yn = xn / xn.norm(dim=2, keepdim=True), yn / yn.norm(dim=2, keepdim=True)
        d = (xn * yn).sum((0, 2)) / M.J
    else:
        def twice(V):
            a = V - V.mean(2, keepdim=True)
            a = a / a.norm(dim=2, keepdim=True)
            c = a - a.mean(0, keepdim=True)
            return c / c.norm(dim=0, keepdim=True)
        d = (twice(Xw) * twice(Yw)).sum((0, 2)) / M.SEG
    value = d.mean()
    (-k * value).backward()
    return float(value.detach()), Kf, e.grad.numpy()


@pytest.mark.parametrize("extended", [False, True], ids=["stoi", "estoi"])
@pytest.mark.parametrize("name", JUDGED)
def test_analytic_gradient_matches_autograd(name, extended):
    est, ref = M.case(name)
    m = M.row_model(M.registered(name), extended, K)
    value, kept, g = torch_total(est, ref, extended, K)
    d = M._eval(name, extended, K, "d")
    scale = float(np.max(np.abs(m.g))) if name != "c" else float(np.max(np.abs(M.row_model(M.registered("a"), extended, K).g)))
    err = float(np.max(np.abs(g - d.g.astype(np.float64)))) / scale
    print(f"case {name} extended={extended}: |autograd - d| / max |g| = {err:.3e}; value diff = {abs(value - float(m.value)):.2e}")
    assert kept == m.kept and abs(value - float(m.value)) <= m.bound
    assert err <= AUTOGRAD_GATE


@pytest.mark.parametrize("extended", [False, True], ids=["stoi", "estoi"])
@pytest.mark.parametrize("name", ["a", "b"])
def test_gradient_matches_central_differences(name, extended):
    """<g, dir> against (A(e + t dir) - A(e - t dir)) / 2 t in long double along three random directions.  The step is 2^-20
    of the row's rms: the truncation error falls with its square (1e-7 .. 4e-7 of the value was seen at 2^-14, so about 1e-10
    here) and the rounding error is 2^-64 / 2^-20 of the value; the agreement is asked for at 1e-8, relatively."""
    est, ref = M.case(name)
    e = est.astype(M.LD)
    base = M.evaluate(e, ref, extended, K, M.LD)
    rms = float(np.sqrt(np.mean(est.astype(np.float64) ** 2)))
    g = np.random.Generator(np.random.PCG64(7 + len(name)))
    for trial in range(3):
        direction = g.standard_normal(len(est)).astype(M.LD)
        t = M.LD(rms * 2.0 ** -20)
        up, dn = M.evaluate(e + t * direction, ref, extended, K, M.LD), M.evaluate(e - t * direction, ref, extended, K, M.LD)
        assert up.kept == dn.kept == base.kept
        fd = (up.a - dn.a) / (2 * t)
        want = np.sum(base.g * direction)
        print(f"case {name} extended={extended} direction {trial}: fd = {float(fd):.12e}, <g, dir> = {float(want):.12e}")
        assert abs(fd - want) <= 1e-8 * abs(want)


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("extended", [False, True], ids=["stoi", "estoi"])
def test_cases_meet_the_conditions(extended):
    for name in ("a", "b", "c", "d", "e", "f", "a16"):
        c = M.conditions(M.registered(name), extended, K, scale_of=M.registered("a") if name == "c" else None)
        assert c["level_margin"] >= M.LEVEL_MARGIN and c["min_margin"] >= M.MIN_MARGIN, (name, c)
        assert c["E"] <= c["E_max"], (name, c)
    kept = {n: M.row_model(n, extended, K).kept for n in ("a", "b", "c", "d", "e", "f")}
    status = {n: M.row_model(n, extended, K).status for n in ("a", "b", "c", "d", "e", "f")}
    assert kept["d"] == 31 and kept["e"] == 30 and kept["a"] == kept["c"] == M.frames_of(M.L_SHORT) == 45
    assert kept["b"] < M.frames_of(M.L_LONG) - 15                      # the gap's frames are gone
    assert status == {"a": 0, "b": 0, "c": 0, "d": 0, "e": 1, "f": 2}
    if not extended:
        assert M.row_model("a", False, K).clipped > 0 and M.row_model("b", False, K).clipped > 0     # both branches of min
        assert abs(float(M.row_model("c", False, K).value) - 1.0) <= 1e-15
    for n in ("e", "f"):
        m = M.row_model(n, extended, K)
        assert np.isnan(float(m.value)) and m.a == 0 and not m.g.any()
    # kept frames straddle the gap of (b): a kept frame before it is followed by one after it
    est, ref = M.case("b")
    assert float(np.std(ref[M.GAP[0]:M.GAP[1]])) < 1e-2 * float(np.std(ref[:M.GAP[0]]))


# ------------------------------------------------------------------ settings and argument rules
def test_aux_loss_takes_the_stoi_settings():
    a = AuxLoss()
    assert a.w_stoi == 0.0 and a.stoi_extended is False
    a = AuxLoss(w_stoi=1, stoi_extended=True)
    assert isinstance(a.w_stoi, float) and a.w_stoi == 1.0 and a.stoi_extended is True and a.w_mr == 0.0 and a.w_si == 0.0
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="w_stoi: must be finite and >= 0"):
            AuxLoss(w_stoi=bad)
    for bad in (None, "1", True):
        with pytest.raises(TypeError, match="w_stoi: expected a number"):
            AuxLoss(w_stoi=bad)
    for bad in (1, None, "yes", 0.0):
        with pytest.raises(TypeError, match="stoi_extended: expected a bool"):
            AuxLoss(w_stoi=1.0, stoi_extended=bad)
    assert check_stoi_settings(np.float32(0.5), np.bool_(True)) == (0.5, True)


def test_check_stoi_loss_args():
    est, ref = torch.zeros(3, 9600), torch.zeros(3, 9600)
    assert check_stoi_loss_args(CPU, est, ref) == (3, 9600, 1.0, False)
    assert check_stoi_loss_args(CPU, est, ref, 0.5, True) == (3, 9600, 0.5, True)
    assert STOI_MIN_L == M.MIN_L and stoi_frames(STOI_MIN_L) == 31 and stoi_frames(STOI_MIN_L - 1) == 30
    assert stoi_frames(9600) == M.frames_of(9600) == 45
    short = torch.zeros(1, STOI_MIN_L - 1)
    with pytest.raises(ValueError, match="rows must hold at least 6554 samples"):
        check_stoi_loss_args(CPU, short, short)
    assert check_stoi_loss_args(CPU, torch.zeros(1, STOI_MIN_L), torch.zeros(1, STOI_MIN_L))[1] == STOI_MIN_L
    with pytest.raises(TypeError, match="est: expected a torch.Tensor"):
        check_stoi_loss_args(CPU, est.numpy(), ref)
    with pytest.raises(TypeError, match="ref: expected float32"):
        check_stoi_loss_args(CPU, est, ref.double())
    with pytest.raises(ValueError, match="ref: expected \\[3, 9600\\]"):
        check_stoi_loss_args(CPU, est, torch.zeros(3, 9601))
    with pytest.raises(ValueError, match="est: must be contiguous"):
        check_stoi_loss_args(CPU, torch.zeros(3, 19200)[:, ::2], ref)
    with pytest.raises(ValueError, match="w_stoi: must be finite"):
        check_stoi_loss_args(CPU, est, ref, -1.0)


# ------------------------------------------------------------------ the library without a GPU
def test_symbols_header_and_workspace():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "cmgan_hip.h")).read()
    assert "Intelligibility loss" in header
    for name in ("cmgan_stoi_loss", "cmgan_stoi_loss_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and re.search(rf"\b{name}\(", header), name
    query = lib.cmgan_stoi_loss_workspace_bytes
    for B, L in ((1, STOI_MIN_L), (4, 9600), (4, 16000), (32, 32000), (65535, 6600)):
        n10, nS = M.n10_of(L), M.frames_of(L)
        # at least: both 10 kHz signals, the estimate's 256 bins, the window gradients, the frame gradients and g10
        least = 8 * B * (3 * n10 + nS * (512 + 256) + (nS - 30) * 450)
        assert least <= query(None, B, L, 16000) <= 2 * least + 65536, (B, L)
    for B, L, fs in ((0, 9600, 16000), (65536, 9600, 16000), (1, STOI_MIN_L - 1, 16000), (1, 0, 16000), (1, -4, 16000),
                     (1, 9600, 8000), (1, 9600, 48000), (1, 2 ** 31 - 1, 16000)):
        assert query(None, B, L, fs) == 0, (B, L, fs)


def test_library_rejects_bad_arguments_before_it_needs_a_handle():
    lib = _lib.load()
    B, L = 2, 9600
    est, ref, g = (np.zeros(B * L + 8, dtype=np.float32) for _ in range(3))
    rows = np.full(B * 2 + 1, 7.0)
    total = np.full(2, 7.0, dtype=np.float32)
    status = np.full(B + 1, 7, dtype=np.int32)
    need = lib.cmgan_stoi_loss_workspace_bytes(None, B, L, 16000)
    raw = np.zeros(need + 512, dtype=np.uint8)
    pw = (raw.ctypes.data + 255) & ~255
    pe, pr, pg, prow, pt, ps = (a.ctypes.data for a in (est, ref, g, rows, total, status))

    def call(est=pe, ref=pr, B=B, L=L, fs=16000, extended=0, k=0.25, rows=prow, total=pt, status=ps, g=pg, ws=pw, ws_bytes=need):
        rc = lib.cmgan_stoi_loss(None, est, ref, B, L, fs, extended, k, rows, total, status, g, ws, ws_bytes, None)
        return rc, (lib.cmgan_last_error(None) or b"").decode()

    cases = {
        "null pointer": [dict(est=None), dict(ref=None), dict(rows=None), dict(total=None), dict(status=None)],
        "4-byte aligned": [dict(est=pe + 2), dict(ref=pr + 1), dict(total=pt + 2), dict(g=pg + 2), dict(status=ps + 2)],
        "8-byte aligned": [dict(rows=prow + 4)],
        "need 1 <= B": [dict(B=0), dict(B=-1), dict(B=65536)],
        "too short for 31 frames": [dict(L=STOI_MIN_L - 1), dict(L=1), dict(L=0), dict(L=-5)],
        "too long": [dict(L=2 ** 31 - 1)],
        "extended must be 0 or 1": [dict(extended=2), dict(extended=-1)],
        "k must be a number": [dict(k=float("nan"))],
        "g_audio overlaps": [dict(g=pe), dict(g=pr), dict(g=pe + 4 * (B * L - 1)), dict(est=pg + 4), dict(ref=pg + 4 * 7)],
        "workspace": [dict(ws=None), dict(ws=pw + 8), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(B=3)],
    }
    for text, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == BADARG and "cmgan_stoi_loss" in msg and text in msg, (kw, rc, msg)
    for fs in (8000, 10000, 48000, 0):
        rc, msg = call(fs=fs)
        assert rc == UNSUPPORTED and "fs must be 16000" in msg, (fs, rc, msg)
    # everything in order: only the handle is missing - nothing was enqueued, nothing was written
    for kw in (dict(), dict(g=None), dict(extended=1), dict(k=0.0), dict(L=STOI_MIN_L), dict(B=1), dict(ws_bytes=need + 512)):
        rc, msg = call(**kw)
        assert rc == BADARG and "null handle" in msg, (kw, rc, msg)
    assert not g.any() and (rows == 7.0).all() and (total == 7.0).all() and (status == 7).all()
