"""CPU side of the auxiliary losses (cmgan_amd/csrc/auxloss.hip; include/cmgan_hip.h, "Auxiliary losses"): the numpy model
the GPU tests judge by (tests/auxloss_model.py) against float64 autograd through torch.stft, the conditions of every
registered row, the settings object, the argument rules and the library's own refusals.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import auxloss_model as M
from cmgan_amd import _lib
from cmgan_amd.engine import (AUX_MAX_RESOLUTIONS, AUX_N_FFT, aux_loss_workspace_bytes, check_aux_loss_args,
                              check_aux_settings)
from cmgan_amd.training import AuxLoss, GraphedTrainStep, Trainer, adversarial_train_step, generator_train_step

CPU = torch.device("cpu")
BADARG = -1
ALL = tuple((L, b) for L in M.LENGTHS for b in range(M.B))


# ------------------------------------------------------------------ the model against autograd
def torch_total(est, ref, n_ffts, k_mr, k_si):
    """The definitions restated with torch.stft in float64; (A, dA / de) of one row."""
    e = torch.tensor(est, dtype=torch.float64, requires_grad=True)
    r = torch.tensor(ref, dtype=torch.float64)
    mr_sum = 0.0
    for n in n_ffts:
        win = torch.hann_window(n, periodic=True, dtype=torch.float64)
        mag = lambda x: torch.stft(x, n, hop_length=n // 4, window=win, center=True, pad_mode="reflect",
                                   return_complex=True).abs().pow(2).clamp(min=M.CLAMP).sqrt()
        me, mr = mag(e), mag(r)
        assert tuple(me.shape) == (n // 2 + 1, M.n_frames(len(est), n))
        sc = (mr - me).pow(2).sum().sqrt() / mr.pow(2).sum().sqrt()
        mr_sum = mr_sum + sc + (mr.log() - me.log()).abs().mean()
    ec, rc = e - e.mean(), r - r.mean()
    a = (ec * rc).sum() / ((rc * rc).sum() + M.EPS)
    s = a * rc
    q = ec - s
    si = 10.0 * torch.log10(((s * s).sum() + M.EPS) / ((q * q).sum() + M.EPS))
    A = k_mr * mr_sum / len(n_ffts) - k_si * si
    A.backward()
    return float(A.detach()), e.grad.numpy()


@pytest.mark.parametrize("L,b", ALL)
def test_analytic_gradient_matches_autograd(L, b):
    key = M.registered(L, b)
    est, ref = M.pair(L, b)
    for n_ffts in (M.N_FFT_SETS[0], M.N_FFT_SETS[3]):
        for w_mr, w_si in M.WEIGHTS:
            k_mr, k_si = w_mr / M.B, w_si / M.B
            m = M.row_model(key, n_ffts, k_mr, k_si)
            A, g = torch_total(est, ref, n_ffts, k_mr, k_si)
            err = float(np.max(np.abs(g.astype(M.LD) - m.g)))
            print(f"L={L} row={b} n_ffts={n_ffts} k=({k_mr:.3g}, {k_si:.3g}): |autograd - w| = {err:.3e}, E = {m.E:.3e}")
            assert err <= m.E
            assert abs(A - float(m.a)) <= 1e-12 * max(1.0, abs(A))


@pytest.mark.parametrize("L,b", ALL)
def test_registered_rows_meet_the_conditions(L, b):
    key = M.registered(L, b)
    for n_ffts in M.N_FFT_SETS:
        for w_mr, w_si in M.WEIGHTS:
            c = M.conditions(key, n_ffts, w_mr / M.B, w_si / M.B)
            assert c["E"] <= c["E_max"], (n_ffts, w_mr, w_si, c)
            assert not c["kink"] and not c["near_clamp"] and -20.0 <= c["si_sdr"] <= 40.0, (n_ffts, c)
        bounds = M.value_bounds(key, n_ffts)
        assert np.all(np.isfinite(bounds)) and np.all(bounds[:-1] < 1e-9) and bounds[-1] < 1e-7, bounds


def test_special_rows_of_the_model():
    est, ref = M.pair(1700, 0)
    same = M.register(("same", 1700), ref, ref)
    m = M.row_model(same, (256, 2048), 1.0, 0.0)
    assert np.all(m.rows[:-1] == 0) and np.all(m.g == 0) and m.E == 0.0
    zero = M.register(("zero", 1700), np.zeros_like(ref), ref)
    m = M.row_model(zero, (256, 2048), 1.0, 0.3)
    assert np.all(m.g == 0) and m.E == 0.0 and m.rows[-1] == 0 and np.all(m.rows[:-1] > 0)
    c = M.conditions(zero, (256, 2048), 1.0, 0.3)
    assert c["E"] <= c["E_max"] and not c["kink"] and not c["near_clamp"]


# ------------------------------------------------------------------ settings and argument rules
def test_aux_loss_settings():
    a = AuxLoss()
    assert a.n_ffts == (512, 1024, 2048) and a.w_mr == 0.0 and a.w_si == 0.0
    a = AuxLoss([256, np.int64(2048)], w_mr=1, w_si=0.5)
    assert a.n_ffts == (256, 2048) and isinstance(a.w_mr, float) and a.w_si == 0.5
    with pytest.raises(Exception):
        a.w_mr = 2.0
    for bad in ((), (256, 512, 1024, 2048, 256), (256, 512, 1024, 2048, 4096)):
        with pytest.raises(ValueError, match="need 1 to 4 resolutions"):
            AuxLoss(bad)
    for bad in ((400,), (128,), (4096,), (512.0,), (True,), ("512",), (512, None)):
        with pytest.raises(ValueError, match="a resolution must be one of"):
            AuxLoss(bad)
    with pytest.raises(ValueError, match="must be distinct"):
        AuxLoss((512, 1024, 512))
    with pytest.raises(TypeError, match="n_ffts: expected a sequence"):
        AuxLoss(512)
    for name in ("w_mr", "w_si"):
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=f"{name}: must be finite and >= 0"):
                AuxLoss(**{name: bad})
        for bad in (None, "1", True):
            with pytest.raises(TypeError, match=f"{name}: expected a number"):
                AuxLoss(**{name: bad})
    assert check_aux_settings((2048, 256), 1, 0) == ((2048, 256), 1.0, 0.0)
    assert AUX_N_FFT == M.N_FFTS and AUX_MAX_RESOLUTIONS == 4


def test_training_entry_points_take_aux():
    import inspect
    for fn in (generator_train_step, adversarial_train_step, GraphedTrainStep.__init__, Trainer.__init__):
        p = inspect.signature(fn).parameters
        assert "aux" in p and p["aux"].default is None, fn
    for fn, args in ((generator_train_step, (None,) * 4), (adversarial_train_step, (None,) * 7)):
        with pytest.raises(TypeError, match="aux: expected an AuxLoss or None"):
            fn(*args, aux=(512, 1024))


def test_check_aux_loss_args():
    est, ref = torch.zeros(3, 1100), torch.zeros(3, 1100)
    assert check_aux_loss_args(CPU, est, ref) == (3, 1100, (512, 1024, 2048), 1.0, 0.0)
    assert check_aux_loss_args(CPU, est, ref, (256,), 0, 2) == (3, 1100, (256,), 0.0, 2.0)
    with pytest.raises(ValueError, match="rows must hold more than 1024 samples"):
        check_aux_loss_args(CPU, est[:, :1024].contiguous(), ref[:, :1024].contiguous())
    assert check_aux_loss_args(CPU, est[:, :1025].contiguous(), ref[:, :1025].contiguous())[1] == 1025
    assert check_aux_loss_args(CPU, torch.zeros(1, 129), torch.zeros(1, 129), (256,))[1] == 129
    with pytest.raises(TypeError, match="est: expected a torch.Tensor"):
        check_aux_loss_args(CPU, est.numpy(), ref)
    with pytest.raises(TypeError, match="ref: expected float32"):
        check_aux_loss_args(CPU, est, ref.double())
    with pytest.raises(RuntimeError, match="est: tensor is on cpu"):
        check_aux_loss_args(torch.device("cuda:0"), est, ref)
    for bad in (torch.zeros(1100), torch.zeros(1, 3, 1100), torch.zeros(0, 1100)):
        with pytest.raises(ValueError, match="est: expected \\[B, L\\]"):
            check_aux_loss_args(CPU, bad, ref)
    with pytest.raises(ValueError, match="ref: expected \\[3, 1100\\]"):
        check_aux_loss_args(CPU, est, torch.zeros(3, 1101))
    with pytest.raises(ValueError, match="est: must be contiguous"):
        check_aux_loss_args(CPU, torch.zeros(3, 2200)[:, ::2], ref)
    with pytest.raises(ValueError, match="ref: must be contiguous"):
        check_aux_loss_args(CPU, est, torch.zeros(3, 2200)[:, :1100])
    with pytest.raises(ValueError, match="at most 65535 rows"):
        check_aux_loss_args(CPU, torch.zeros(65536, 129), torch.zeros(65536, 129), (256,))
    with pytest.raises(ValueError, match="must be distinct"):
        check_aux_loss_args(CPU, est, ref, (256, 256))
    with pytest.raises(ValueError, match="w_si: must be finite"):
        check_aux_loss_args(CPU, est, ref, (256,), 1.0, -0.1)


# ------------------------------------------------------------------ the library without a GPU
def test_symbols_header_and_workspace():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "cmgan_hip.h")).read()
    assert "Auxiliary losses" in header
    for name in ("cmgan_aux_loss", "cmgan_aux_loss_max_resolutions", "cmgan_aux_loss_workspace_bytes", "cmgan_loss_backward_aux"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and re.search(rf"\b{name}\(", header), name
    assert len(_lib.SIGNATURES["cmgan_loss_backward_aux"][1]) == len(_lib.SIGNATURES["cmgan_loss_backward"][1]) + 1
    assert lib.cmgan_aux_loss_max_resolutions() == AUX_MAX_RESOLUTIONS

    def native(B, L, res):
        arr = (np.ctypeslib.ctypes.c_int * len(res))(*res)
        return lib.cmgan_aux_loss_workspace_bytes(None, B, L, len(res), arr)

    for B, L, res in ((1, 129, (256,)), (3, 1100, (2048,)), (3, 1700, (256, 512, 1024, 2048)), (32, 32000, (512, 1024, 2048)),
                      (65535, 1025, (2048, 256)), (2, 2 ** 31 - 1 - 4096, (1024,))):
        cells = sum(B * M.n_frames(L, n) * (n // 2 + 1) for n in res)
        assert native(B, L, res) == aux_loss_workspace_bytes(B, L, res) >= 24 * cells
    for B, L, res in ((0, 2000, (256,)), (65536, 2000, (256,)), (1, 128, (256,)), (1, 1024, (256, 2048)), (1, 2000, (400,)),
                      (1, 2000, (256, 256)), (1, 2000, ()), (1, 3000, (256, 512, 1024, 2048, 256)), (1, 2 ** 31 - 4096, (256,))):
        assert native(B, L, res) == aux_loss_workspace_bytes(B, L, res) == 0, (B, L, res)


def test_library_rejects_bad_arguments_before_it_needs_a_handle():
    lib = _lib.load()
    ctypes = np.ctypeslib.ctypes
    B, L = 2, 1100
    est, ref, g = (np.zeros(B * L + 8, dtype=np.float32) for _ in range(3))
    rows = np.full(B * 9, 7.0)
    total = np.full(3, 7.0, dtype=np.float32)
    res = (512, 1024, 2048)
    arr = (ctypes.c_int * 4)(*res, 256)
    need = lib.cmgan_aux_loss_workspace_bytes(None, B, L, 3, arr)
    raw = np.zeros(need + 512, dtype=np.uint8)
    pw = (raw.ctypes.data + 255) & ~255
    pe, pr, pg, prow, pt = (a.ctypes.data for a in (est, ref, g, rows, total))

    def call(est=pe, ref=pr, B=B, L=L, n_res=3, n_fft=arr, k_mr=0.5, k_si=0.1, rows=prow, total=pt, g=pg, ws=pw, ws_bytes=need):
        rc = lib.cmgan_aux_loss(None, est, ref, B, L, n_res, n_fft, k_mr, k_si, rows, total, g, ws, ws_bytes, None)
        return rc, (lib.cmgan_last_error(None) or b"").decode()

    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    cases = {
        "null pointer": [dict(est=None), dict(ref=None), dict(rows=None), dict(total=None)],
        "4-byte aligned": [dict(est=pe + 2), dict(ref=pr + 1), dict(total=pt + 2), dict(g=pg + 2)],
        "8-byte aligned": [dict(rows=prow + 4)],
        "need 1 <= B": [dict(B=0), dict(B=-1), dict(B=65536)],
        "1 to 4 resolutions": [dict(n_res=0), dict(n_res=5), dict(n_res=-1), dict(n_fft=None)],
        "must be 256, 512, 1024 or 2048": [dict(n_fft=ints(512, 400, 2048)), dict(n_fft=ints(128, 512, 1024)),
                                           dict(n_fft=ints(512, 1024, 4096)), dict(n_fft=ints(0, 512, 1024))],
        "must be distinct": [dict(n_fft=ints(512, 1024, 512)), dict(n_fft=ints(2048, 2048, 512))],
        "L must exceed half": [dict(L=1024), dict(L=1), dict(L=0), dict(L=-5), dict(L=128, n_res=1, n_fft=ints(256))],
        "too long": [dict(L=2 ** 31 - 4096)],
        "must be numbers": [dict(k_mr=float("nan")), dict(k_si=float("nan"))],
        "g_audio overlaps": [dict(g=pe), dict(g=pr), dict(g=pe + 4 * (B * L - 1)), dict(est=pg + 4), dict(ref=pg + 4 * 7)],
        "workspace": [dict(ws=None), dict(ws=pw + 8), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(n_res=4)],
    }
    for text, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == BADARG and "cmgan_aux_loss" in msg and text in msg, (kw, rc, msg)
    # everything in order: only the handle is missing - nothing was enqueued, nothing was written
    for kw in (dict(), dict(g=None), dict(k_mr=0.0), dict(k_si=0.0), dict(L=1025), dict(n_res=1), dict(ws_bytes=need + 512),
               dict(B=1), dict(n_res=2, n_fft=ints(2048, 256))):
        rc, msg = call(**kw)
        assert rc == BADARG and "null handle" in msg, (kw, rc, msg)
    assert not g.any() and (rows == 7.0).all() and (total == 7.0).all()
