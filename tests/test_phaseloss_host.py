"""CPU side of the phase loss (cmgan_amd/csrc/phaseloss.hip; include/cmgan_hip.h, "Phase loss"): the numpy model the GPU tests
judge by (tests/phaseloss_model.py) against float64 autograd through torch.atan2 and a plain restatement, against central
differences in long double, and against a loop that counts the terms; the margins of every GPU case; the settings object, the
argument rules and the library's own refusals.  No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

import phaseloss_model as M
from cmgan_amd import _lib
from cmgan_amd.engine import PHASE_MAX_F, PHASE_MAX_T, check_phase_loss_args, check_phase_settings
from cmgan_amd.training import AuxLoss

CPU = torch.device("cpu")
BADARG = -1
K3 = tuple(w / 3 for w in M.K_WEIGHTS)                  # k = w / B at B = 3
#: the worst |autograd - d| over the cases below, relative to the row's largest gradient sample, was measured here at 2.2e-16
#: (the nan row at T = 3; 4e-17 .. 2.1e-16 elsewhere: autograd runs the same few operations in another order); the gate is
#: ten times that
AUTOGRAD_GATE = 2.2e-15
JUDGED = (("rand", 17, 201, 0.0), ("zeros", 17, 201, 0.0), ("zeros", 1, 201, 0.0), ("floor", 17, 201, M.FLOOR), ("rand", 2, 601, 0.0),
          ("nan", 3, 201, 0.0))


# ------------------------------------------------------------------ the model against autograd
def torch_total(er, ei, cr, ci, k3, floor):
    """The definitions restated plainly in torch float64: (values [3], counts [3], dA / d est_real, dA / d est_imag)."""
    a = torch.tensor(er.astype(np.float64))
    b = torch.tensor(ei.astype(np.float64))
    c, d = torch.tensor(cr.astype(np.float64)), torch.tensor(ci.astype(np.float64))
    ok = torch.isfinite(a) & torch.isfinite(b) & torch.isfinite(c) & torch.isfinite(d)
    a, b, c, d = (torch.where(ok, x, torch.ones_like(x)) for x in (a, b, c, d))
    me, mc = a * a + b * b, c * c + d * d
    ok = ok & (me > 0) & (mc > 0) & ~(me < floor * floor) & ~(mc < floor * floor)
    a, b = (torch.where(ok, x, torch.ones_like(x)).requires_grad_(True) for x in (a, b))
    p, q = torch.atan2(b, a), torch.atan2(d, c)

    def aw(x):
        return (x - M.TWO_PI * torch.round(x / M.TWO_PI)).abs()
    terms = ((aw(p - q), ok),
             (aw((p[:, 1:] - p[:, :-1]) - (q[:, 1:] - q[:, :-1])), ok[:, 1:] & ok[:, :-1]),
             (aw((p[1:] - p[:-1]) - (q[1:] - q[:-1])), ok[1:] & ok[:-1]))
    total, values, counts = torch.zeros((), dtype=torch.float64), [], []
    for k, (x, v) in zip(k3, terms):
        n = int(v.sum())
        value = x[v].sum() / n if n else torch.zeros((), dtype=torch.float64)
        total = total + k * value
        values.append(float(value.detach()))
        counts.append(n)
    if total.requires_grad:
        total.backward()
    zero = torch.zeros_like(a)
    ga, gb = (zero if x.grad is None else x.grad for x in (a, b))
    return values, counts, torch.where(ok, ga, zero).numpy(), torch.where(ok, gb, zero).numpy()


@pytest.mark.parametrize("kind,nT,nF,floor", JUDGED)
def test_analytic_gradient_matches_autograd(kind, nT, nF, floor):
    values, counts, ga, gb = torch_total(*M.row(kind, nT, nF), K3, floor)
    d = M.row_model(kind, nT, nF, K3, floor, "d")
    w = M.row_model(kind, nT, nF, K3, floor, "w")
    assert counts == list(d.counts) == list(w.counts)
    assert np.max(np.abs(np.array(values) - d.values)) <= 64 * M.U * np.pi
    scale = max(float(np.max(np.abs(d.g_real))), float(np.max(np.abs(d.g_imag))))
    err = max(float(np.max(np.abs(ga - d.g_real))), float(np.max(np.abs(gb - d.g_imag)))) / scale
    print(f"[phaseloss] {kind} T={nT} F={nF}: |autograd - d| / max |g| = {err:.3e}")
    assert err <= AUTOGRAD_GATE
    assert not ga[d.void].any() and not d.g_real[d.void].any() and not d.g_imag[d.void].any()


@pytest.mark.parametrize("kind,nT,nF,floor", [("floor", 17, 201, M.FLOOR), ("floor2", 3, 201, M.FLOOR)])
def test_gradient_matches_central_differences(kind, nT, nF, floor):
    """<g, dir> against (A(e + h dir) - A(e - h dir)) / 2 h in long double along three random directions, on the rows with a
    floor, where no judged |z| is below 1e-2.  A is linear in the angles as long as no r changes sign or wraps, and the angle
    is smooth in e: with h = 2^-24 the truncation is about (h / |z|)^2 <= 4e-11 of a term and the rounding 2^-64 / h = 1e-12
    of the value; the agreement is asked for at 1e-8, relatively (seen: 1e-12 .. 2e-10).  A term within h / |z| = 6e-6 of a
    kink would break that by orders of magnitude; the seeded directions meet none."""
    est_real, est_imag, cr, ci = M.row(kind, nT, nF)
    base = M.evaluate(est_real, est_imag, cr, ci, K3, floor, M.LD)
    g = np.random.Generator(np.random.PCG64(11 + nT))
    h = M.LD(2.0 ** -24)
    for trial in range(3):
        da, db = g.standard_normal((nT, nF)).astype(M.LD), g.standard_normal((nT, nF)).astype(M.LD)
        up = M.evaluate(est_real, est_imag, cr, ci, K3, floor, M.LD, shift=(h * da, h * db))
        dn = M.evaluate(est_real, est_imag, cr, ci, K3, floor, M.LD, shift=(-h * da, -h * db))
        fd = (up.a - dn.a) / (2 * h)
        want = np.sum(base.g_real * da) + np.sum(base.g_imag * db)
        print(f"[phaseloss] {kind} direction {trial}: fd = {float(fd):.12e}, <g, dir> = {float(want):.12e}")
        assert abs(fd - want) <= 1e-8 * abs(want)


# ------------------------------------------------------------------ the cases
def _loop_counts(void):
    nT, nF = void.shape
    n = [0, 0, 0]
    for t in range(nT):
        for f in range(nF):
            if void[t, f]:
                continue
            n[0] += 1
            n[1] += f >= 1 and not void[t, f - 1]
            n[2] += t >= 1 and not void[t - 1, f]
    return n


@pytest.mark.parametrize("nT,nF", M.SHAPES)
def test_cases_meet_the_conditions(nT, nF):
    for name, (kinds, floor) in M.BATCHES.items():
        k3 = tuple(w / len(kinds) for w in M.K_WEIGHTS)
        for kind in kinds:
            w, d = M.row_model(kind, nT, nF, k3, floor, "w"), M.row_model(kind, nT, nF, k3, floor, "d")
            assert w.branch_margin >= M.BRANCH_MARGIN and w.floor_margin >= M.FLOOR_MARGIN, (name, kind, w.branch_margin, w.floor_margin)
            assert list(w.counts) == list(d.counts) == _loop_counts(w.void) and w.status == d.status, (name, kind)
            # the float64 evaluation lies inside the slack the roundings allow, and inside the values' bound
            for gd, gw, E in ((d.g_real, w.g_real, w.E_real), (d.g_imag, w.g_imag, w.E_imag)):
                assert np.all(np.abs(gd.astype(M.LD) - gw) <= E), (name, kind)
                # the slack hides nothing: at most 2^-10 of half an ulp of the sample it belongs to (stoiloss_model's condition)
                assert np.all(E <= 2.0 ** -10 * M.ulp32(gw.astype(np.float64)) / 2 + (gw == 0) * 1.0), (name, kind)
            assert np.max(np.abs(d.values.astype(M.LD) - w.values)) <= M.value_bound(nT, nF) <= M.VALUE_CAP, (name, kind)
            if kind in ("same", "double"):
                assert not w.values.any() and not w.g_real.any() and not w.g_imag.any() and w.branch_margin == np.inf
                assert not d.values.any() and not d.g_real.any() and not d.g_imag.any()
            if kind == "void":
                assert w.status == 7 and not w.counts.any() and not w.values.any() and not w.g_real.any() and w.a == 0
            elif nT == 1:
                assert w.status == 4 and w.counts[2] == 0 and w.values[2] == 0
            else:
                assert w.status == 0
    ze, zc = M.zero_cells(nT, nF)
    w = M.row_model("zeros", nT, nF, K3, 0.0, "w")
    cells = set(ze) | set(zc)
    assert int(w.void.sum()) == len(cells) and all(w.void[t, f] for t, f in cells) and w.counts[0] == nT * nF - len(cells)
    assert w.counts[1] < nT * (nF - 1) - len(cells) + 3          # neighbours share a pair
    void, _ = M.void_map(*M.row("floor", nT, nF), M.FLOOR)
    assert 0.15 <= void.mean() <= 0.25                            # a tenth of each spectrum below the floor
    assert int(M.row_model("nan", nT, nF, K3, 0.0, "w").void.sum()) == len({(nT // 2, 5), (0, nF - 2), (nT - 1, 77)})


def test_remainder_is_the_ieee_operation():
    x = np.array([0.0, 1.0, -1.0, 3.2, -3.2, 6.0, -6.0, 6.5, 9.0, -9.0, 9.5, -9.5, 12.0, 3.0, -3.0])
    want = [math.remainder(float(v), M.TWO_PI) for v in x]              # every value is exact in both precisions
    assert [float(v) for v in M.remainder(x, np.float64)] == want
    assert [float(v) for v in M.remainder(x.astype(M.LD), M.LD)] == want


# ------------------------------------------------------------------ settings and argument rules
def test_aux_loss_takes_the_phase_settings():
    a = AuxLoss()
    assert (a.w_ip, a.w_gd, a.w_iaf, a.phase_floor) == (0.0, 0.0, 0.0, 0.0) and not a.phase and a.audio
    a = AuxLoss(w_ip=1, w_iaf=np.float32(0.5), phase_floor=1e-3)
    assert all(isinstance(v, float) for v in (a.w_ip, a.w_gd, a.w_iaf, a.phase_floor))
    assert (a.w_ip, a.w_gd, a.w_iaf, a.phase_floor) == (1.0, 0.0, 0.5, 1e-3) and a.phase and not a.audio
    assert a.w_mr == a.w_si == a.w_stoi == 0.0 and a.n_ffts == (512, 1024, 2048)
    assert AuxLoss(w_gd=1.0, w_si=0.1).audio and AuxLoss(w_gd=1.0, w_stoi=0.1).audio and AuxLoss(w_gd=1.0, w_mr=0.1).audio
    assert AuxLoss(phase_floor=0.5).phase is False
    for name in ("w_ip", "w_gd", "w_iaf", "phase_floor"):
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=f"{name}: must be finite and >= 0"):
                AuxLoss(**{name: bad})
        for bad in (None, "1", True):
            with pytest.raises(TypeError, match=f"{name}: expected a number"):
                AuxLoss(**{name: bad})
    assert check_phase_settings(np.float32(0.5), 1, 0, np.float64(2.0)) == (0.5, 1.0, 0.0, 2.0)


def test_check_phase_loss_args():
    F = 201
    er, ei, cs = torch.zeros(3, 1, 5, F), torch.zeros(3, 1, 5, F), torch.zeros(3, 2, 5, F)
    assert check_phase_loss_args(CPU, F, er, ei, cs) == (3, 5, 1.0, 1.0, 1.0, 0.0)
    assert check_phase_loss_args(CPU, F, er[:, 0], ei[:, 0], cs, 0.5, 0, 2, 1e-2) == (3, 5, 0.5, 0.0, 2.0, 1e-2)
    assert check_phase_loss_args(CPU, F, er[:, :, :1].contiguous(), ei[:, :, :1].contiguous(), cs[:, :, :1].contiguous())[1] == 1
    with pytest.raises(TypeError, match="est_real: expected a torch.Tensor"):
        check_phase_loss_args(CPU, F, er.numpy(), ei, cs)
    with pytest.raises(TypeError, match="est_imag: expected float32"):
        check_phase_loss_args(CPU, F, er, ei.double(), cs)
    with pytest.raises(ValueError, match="est_real: expected \\[B, T, 201\\] or \\[B, 1, T, 201\\]"):
        check_phase_loss_args(CPU, F, torch.zeros(3, 1, 5, 200), ei, cs)
    with pytest.raises(ValueError, match="est_real: expected"):
        check_phase_loss_args(CPU, F, torch.zeros(3, 2, 5, F), ei, cs)
    with pytest.raises(ValueError, match="est_imag: expected \\[3, 1, 5, 201\\]"):
        check_phase_loss_args(CPU, F, er, ei[:, 0], cs)
    with pytest.raises(ValueError, match="clean_spec: expected \\[3, 2, 5, 201\\]"):
        check_phase_loss_args(CPU, F, er, ei, torch.zeros(3, 2, 6, F))
    with pytest.raises(ValueError, match="clean_spec: must be contiguous"):
        check_phase_loss_args(CPU, F, er, ei, torch.zeros(3, 2, 5, 2 * F)[..., ::2])
    with pytest.raises(ValueError, match="w_gd: must be finite"):
        check_phase_loss_args(CPU, F, er, ei, cs, 1.0, -1.0)
    with pytest.raises(ValueError, match="phase_floor: must be finite"):
        check_phase_loss_args(CPU, F, er, ei, cs, floor=float("nan"))
    with pytest.raises(ValueError, match="at most 1024 bins"):
        check_phase_loss_args(CPU, 1025, torch.zeros(1, 1, 1025), torch.zeros(1, 1, 1025), torch.zeros(1, 2, 1, 1025))
    assert (PHASE_MAX_T, PHASE_MAX_F) == (1000000, 1024)


# ------------------------------------------------------------------ the library without a GPU
def test_symbols_header_and_workspace():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "cmgan_hip.h")).read()
    assert "Phase loss" in header and "boundary" in header
    for name in ("cmgan_phase_loss", "cmgan_phase_loss_workspace_bytes", "cmgan_phase_loss_tile_frames"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and re.search(rf"\b{name}\(", header), name
    assert lib.cmgan_phase_loss_tile_frames() == M.TILE_FRAMES
    query = lib.cmgan_phase_loss_workspace_bytes
    for B, T in ((1, 1), (3, 17), (32, 321), (65535, 8), (1, PHASE_MAX_T)):
        least = B * -(-T // M.TILE_FRAMES) * 6 * 8                      # six float64 per tile
        assert least <= query(None, B, T) <= least + 255 and query(None, B, T) % 256 == 0, (B, T)
    for B, T in ((0, 5), (-1, 5), (65536, 5), (1, 0), (1, -3), (1, PHASE_MAX_T + 1), (1, 2 ** 31 - 1)):
        assert query(None, B, T) == 0, (B, T)


def test_library_rejects_bad_arguments_before_it_needs_a_handle():
    lib = _lib.load()
    B, T, F = 2, 9, 201
    n = B * T * F
    er, ei, gr, gi = (np.zeros(n + 8, dtype=np.float32) for _ in range(4))
    cs = np.zeros(2 * n + 8, dtype=np.float32)
    rows = np.full(3 * B + 1, 7.0)
    counts, status = np.full(3 * B + 2, 7, dtype=np.int32), np.full(B + 2, 7, dtype=np.int32)
    total = np.full(6, 7.0, dtype=np.float32)
    need = lib.cmgan_phase_loss_workspace_bytes(None, B, T)
    raw = np.zeros(need + 512, dtype=np.uint8)
    pw = (raw.ctypes.data + 255) & ~255
    per, pei, pcs, pgr, pgi, prow, pcnt, pt, ps = (a.ctypes.data for a in (er, ei, cs, gr, gi, rows, counts, total, status))

    def call(er=per, ei=pei, cs=pcs, B=B, T=T, k=(0.3, 0.3, 0.3), floor=0.0, rows=prow, counts=pcnt, total=pt, status=ps, gr=pgr,
             gi=pgi, ws=pw, ws_bytes=need):
        rc = lib.cmgan_phase_loss(None, er, ei, cs, B, T, *k, floor, rows, counts, total, status, gr, gi, ws, ws_bytes, None)
        return rc, (lib.cmgan_last_error(None) or b"").decode()

    nan = float("nan")
    cases = {
        "null pointer": [dict(er=None), dict(ei=None), dict(cs=None), dict(rows=None), dict(counts=None), dict(total=None),
                         dict(status=None)],
        "4-byte aligned": [dict(er=per + 2), dict(ei=pei + 1), dict(cs=pcs + 2), dict(total=pt + 2), dict(gr=pgr + 2), dict(gi=pgi + 1),
                           dict(status=ps + 2), dict(counts=pcnt + 2)],
        "8-byte aligned": [dict(rows=prow + 4)],
        "need 1 <= B": [dict(B=0), dict(B=-1), dict(B=65536)],
        "need 1 <= T": [dict(T=0), dict(T=-5), dict(T=PHASE_MAX_T + 1)],
        "must be numbers": [dict(k=(nan, 0.3, 0.3)), dict(k=(0.3, nan, 0.3)), dict(k=(0.3, 0.3, nan))],
        "floor must be a number >= 0": [dict(floor=nan), dict(floor=-1e-3), dict(floor=-float("inf"))],
        "needs both g_real and g_imag": [dict(gr=None), dict(gi=None)],
        "workspace": [dict(ws=None), dict(ws=pw + 8), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(B=3, T=16)],
    }
    for text, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == BADARG and "cmgan_phase_loss" in msg and text in msg, (kw, rc, msg)
    # everything in order: only the handle is missing - nothing was enqueued, nothing was written
    for kw in (dict(), dict(gr=None, gi=None), dict(k=(0.0, 0.0, 0.0)), dict(floor=1e-2), dict(T=1), dict(B=1), dict(ws_bytes=need + 512)):
        rc, msg = call(**kw)
        assert rc == BADARG and "null handle" in msg, (kw, rc, msg)
    assert not gr.any() and not gi.any() and (rows == 7.0).all() and (total == 7.0).all() and (status == 7).all() and (counts == 7).all()
