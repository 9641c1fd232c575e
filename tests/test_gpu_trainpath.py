"""The TRAINING conv path - DenseBlockTrain, DenseEncoderTrain, DecoderTrain (mask and complex): train.hip, train_x3.hip and
the training instantiations of conv_x3.hip - against torch autograd through the project's oracle in FLOAT64
(tests/trainpath_model.py), at the plane widths, clip lengths, grid sizes and position counts where the kernels' tilings
change.  Per case: the forward, dL/dx (the encoder has none) and every parameter gradient; all misses of a case are collected
and named together.

Bars are those of test_gpu_training.py: GRAD_TOL = 1e-4 max-norm relative for the forward, dL/dx and every parameter
gradient tensor (relative to its own maximum), plus assert_close(rtol 1e-3, atol_rel 2e-4) for the forward and dL/dx; a conv
bias directly in front of an InstanceNorm (zero gradient in exact arithmetic) stays below 1e-4 of the norm-bias gradient's
maximum.  tests/test_trainpath_model.py asserts the arithmetic each case is named for and that fp32 torch autograd meets
these bars at every shape.  Slopes are the kink-free twin's except in the default-slope cases (trainpath_model's header).

Measured worst figures per group (MI355X, the default split-f16 mode; bar 1e-4 in every column; "zero bias" = the largest
such bias gradient over the norm-bias gradient's maximum).  All 87 cases pass; none of the newly covered edges was wrong.

    group                     forward    dL/dx      parameters   zero bias
    plane widths              2.28e-06   1.09e-05   2.39e-05     4.26e-06
    time edges                2.72e-06   1.52e-05   7.29e-05     7.20e-06    (mask-3x1x63 dense_block.norm4.bias: 63 positions)
    grid sizes                1.86e-06   6.98e-06   5.95e-06     6.44e-06
    finalize passes           2.22e-06   1.24e-05   4.10e-05     5.16e-05    (dense-1x322x201: norm1.bias, conv4.bias)
    weight-gradient walk      1.57e-06   1.09e-05   1.04e-05     6.49e-06
    persistent second trip    1.57e-06   1.38e-05   5.28e-05     4.90e-05    (encoder-2x245x201: conv_1.1.bias, conv_1.0.bias)
    gradient magnitude        2.28e-06   1.09e-05   2.39e-05     4.26e-06    (2^-40 and 2^+20: the unscaled figures)
    offset statistics         8.64e-06   -          2.89e-05     7.71e-06
    default slopes            2.52e-06   1.59e-06   7.84e-06     3.09e-06

Sensitivity, checked once on the GPU with two deliberately wrong builds of the loops these cases are named for:
db_stats_finalize_tiles_kernel cut to one pass fails dense-1x322x201 alone (forward 2.7e-4, norm1.bias 6.8e-4);
rc_dgrad_x3_kernel cut to one trip fails the three second-trip cases alone (dL/dx 6 .. 7, encoder gradients 3 .. 10e-2).
"""
import pytest
import torch

import convpath_model as M
import trainpath_model as TM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_ENGINE, _MODS, _WORST = [], {}, {}


def _engine():
    if not _ENGINE:
        from cmgan_amd.engine import Engine
        _ENGINE.append(Engine(device=DEV))
    return _ENGINE[0]


def _module(c, st=None, tag=""):
    """the *Train wrapper of the case's module on the shared engine, one per (module, slopes, mask width, state tag)"""
    key = (c.module, c.slopes, c.F if c.module == "mask" else 0, tag)
    if key not in _MODS:
        from cmgan_amd.training import DecoderTrain, DenseBlockTrain, DenseEncoderTrain
        rel = TM.relative(c, TM.module_state(c) if st is None else st)
        if c.module == "dense":
            _MODS[key] = DenseBlockTrain(rel, engine=_engine())
        elif c.module == "encoder":
            _MODS[key] = DenseEncoderTrain(rel, engine=_engine())
        else:
            _MODS[key] = DecoderTrain(c.module, rel, num_features=2 * c.F - 1, engine=_engine())
    return _MODS[key]


def _to_gpu(c, x, dy):
    """NCHW float32 on the host -> the channels-last tensors the wrappers take"""
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    dyd = (dy[:, 0] if c.module == "mask" else dy.permute(0, 2, 3, 1)).contiguous().to(DEV)
    return xd, dyd


def _step(c, mod, xd, dyd):
    """forward + backward; (y, dx or None, {key: gradient}) as the wrapper returns them, gradients cloned out of the bucket"""
    y = mod.forward(xd)
    if c.module == "dense":
        dx, grads = mod.backward(xd, dyd)
    elif c.module == "encoder":
        dx, grads = None, mod.backward(dyd)
    else:
        dx, grads = mod.backward(dyd)
    return y, dx, {k: v.clone() for k, v in grads.items()}


def _nchw(c, y, dx, grads):
    """the same in the reference's layout, on the host"""
    y = y.unsqueeze(1) if c.module == "mask" else y.permute(0, 3, 1, 2)
    return {"y": y.cpu(), "dx": None if dx is None else dx.permute(0, 3, 1, 2).cpu(), "grads": {k: v.cpu() for k, v in grads.items()}}


def _run(group, c, ref=None, st=None, xdy=None, tag="", k=1.0):
    """one case against its float64 reference (k: dy scaled by it on both sides); returns the GPU result"""
    x, dy = TM.inputs(c)[:2] if xdy is None else xdy
    ref = TM.reference64(c) if ref is None else ref
    if k != 1.0:
        dy, ref = dy * k, TM.scaled(ref, k)
    got = _nchw(c, *_step(c, _module(c, st, tag), *_to_gpu(c, x, dy)))
    ck = TM.Checks(f"trainpath[{TM.case_id(c)}{tag}]")
    ck.compare(c, got, ref)
    w = _WORST.setdefault(group, {})
    for name, v in ck.worst.items():
        w[name] = max(w.get(name, 0.0), v)
    print(f"[worst] {group}: " + ", ".join(f"{n} {v:.2e}" for n, v in sorted(w.items())))
    ck.done()
    return got


@pytest.mark.parametrize("c", TM.WIDTHS, ids=TM.case_id)
def test_plane_widths(c):
    """B = 2, T = 11; 62 / 63 the widest fallback and the narrowest walkable plane of the 64-channel kernels."""
    assert TM.dense_kernel(c.F) == TM.WIDTH_KERNELS[c.module][c.F]
    if c.module == "encoder":
        assert TM.out_plane(c) == TM.ENCODER_OUT[c.F]
    _run("plane widths", c)


@pytest.mark.parametrize("c", TM.TIME_EDGES, ids=TM.case_id)
def test_time_edges(c):
    """T <= dil: every t - dil tap of the forward and every t + dil tap of the data gradient (the time-reversed
    instantiation) is padding; T = dil + 1: one row is not.  B = 3."""
    assert TM.dense_kernel(c.F) == "x3" and c.B == 3
    _run("time edges", c)


@pytest.mark.parametrize("c", TM.GRID_CASES, ids=TM.case_id)
def test_grid_sizes_of_the_xcd_remap_on_the_data_gradient(c):
    assert TM.dense_kernel(c.F) == "x3" and c.B * TM.dense_tiles(c.T, c.F) == TM.GRIDS[(c.B, c.T)]
    assert sorted(TM.GRIDS.values()) == [1, 3, 7, 8, 9, 17]
    _run("grid sizes", c)


@pytest.mark.parametrize("c", TM.FINALIZE_CASES, ids=TM.case_id)
def test_tile_finalize_passes(c):
    """1, 256 and 257 tiles per clip: the last is the first shape where db_stats_finalize_tiles_kernel's loop runs twice."""
    nt = TM.dense_tiles(c.T, c.F)
    assert nt == TM.FINALIZE[c.T] and TM.finalize_passes(nt) == (2 if c.T == 322 else 1)
    _run("finalize passes", c)


@pytest.mark.parametrize("c", TM.WGRAD_CASES, ids=TM.case_id)
def test_weight_gradient_walk_and_splits(c):
    steps, per, counts = TM.wgrad_splits(c.B * c.T * c.F)
    want = {(1, 1, 5): (1, 1, 1), (9, 1, 9): (3, 1, 3), (5, 1, 63): (10, 1, 10), (2, 64, 64): (256, 1, 256),
            (2, 41, 100): (257, 2, 129)}[c[1:4]]
    assert (steps, per, sum(1 for n in counts if n)) == want
    assert all(n == 0 for n in counts[want[2]:])                  # the empty splits trail
    _run("weight-gradient walk", c)


@pytest.mark.parametrize("c", TM.PERSISTENT_CASES, ids=TM.case_id)
def test_persistent_row_conv_data_gradient_second_trip(c):
    ng = 1 if c.module == "encoder" else 2
    tiles, grid, trips = TM.rc_dgrad_geometry(c.B * c.T * c.F, ng)
    assert tiles > TM.RCD_TILES * TM.RCD_CAP[ng] and grid == TM.RCD_CAP[ng] and trips == 2
    _run("persistent second trip", c)


@pytest.mark.parametrize("k", TM.MAGNITUDE_SCALES, ids=["2^-40", "2^+20"])
@pytest.mark.parametrize("c", TM.MAGNITUDE_CASES, ids=TM.case_id)
def test_gradient_magnitude(c, k):
    """dy scaled by 2^-40 and 2^+20: every error is relative and the float64 reference scales exactly, so the same bars
    hold; every output is finite and dL/dx is not flushed to zero.  (Bit-identity with the unscaled run is not asked: the
    InstanceNorm backward is not written to promise it.)"""
    got = _run("gradient magnitude", c, k=k, tag=f" x {k:g}")
    assert torch.isfinite(got["y"]).all() and all(torch.isfinite(g).all() for g in got["grads"].values())
    if got["dx"] is not None:
        assert torch.isfinite(got["dx"]).all() and float(got["dx"].abs().max()) > 0.0


def test_offset_statistics():
    """Every pre-norm channel of the encoder 8 .. 16 standard deviations from zero: the training forward's variance comes
    from fp32 tile partials (E[x^2] - mean^2), as in inference; the gradients go through the same mean and rstd."""
    st, xdy, ref, ratios = TM.offset_case()
    assert set(ratios) == set(M.ENC_KEYS)
    for key, r in ratios.items():
        assert 8.0 <= float(r.min()) and float(r.max()) <= 16.0, key
    _run("offset statistics", TM.OFFSET_CASE, ref=ref, st=st, xdy=xdy, tag=" offset")


@pytest.mark.parametrize("c", TM.DEFAULT_CASES, ids=TM.case_id)
def test_default_slopes_on_a_wide_plane(c):
    """The state dict's own PReLU slopes (~0.25) on the split-f16 kernels; the input seed keeps every float64 pre-activation
    KINK_MARGIN from zero (asserted on the host), so the gradient is as well defined as the twin's."""
    assert c.slopes == "default" and TM.dense_kernel(c.F) == "x3"
    _run("default slopes", c)


@pytest.mark.parametrize("c", TM.WORKSPACE_CASES, ids=TM.case_id)
def test_determinism_and_exact_size_workspace(c):
    """Two forward + backward runs are bit-identical; and inside a workspace of EXACTLY the advertised size, with a 64 KB
    0xA5 guard band behind it in the same allocation, the band stays intact and every result equals the roomy run's."""
    mod, eng = _module(c), _engine()
    if c.module == "dense":
        need = eng.lib.cmgan_dense_train_workspace_bytes(eng._h, c.B, c.T, c.F)
    elif c.module == "encoder":
        need = eng.lib.cmgan_encoder_train_workspace_bytes(eng._h, c.B, c.T, c.F)
    else:
        need = eng.lib.cmgan_decoder_train_workspace_bytes(eng._h, c.B, c.T, c.F)
    xd, dyd = _to_gpu(c, *TM.inputs(c)[:2])

    def same(a, b):
        return torch.equal(a[0], b[0]) and (a[1] is None or torch.equal(a[1], b[1])) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])

    try:
        mod._ws = torch.zeros(need + (1 << 22), dtype=torch.uint8, device=DEV)
        first = _step(c, mod, xd, dyd)
        first = (first[0].clone(), None if first[1] is None else first[1].clone(), first[2])
        assert same(first, _step(c, mod, xd, dyd)), "two runs differ"
        buf = torch.empty(need + TM.GUARD_BYTES, dtype=torch.uint8, device=DEV)
        buf[need:].fill_(0xA5)
        mod._ws = buf[:need]                                       # the library is told `need` bytes, the guard follows
        tight = _step(c, mod, xd, dyd)
        torch.cuda.synchronize()
        assert mod._ws.data_ptr() == buf.data_ptr() and mod._ws.numel() == need, "the wrapper replaced the workspace"
        assert bool((buf[need:] == 0xA5).all()), "the workspace was overrun"
        assert same(first, tight), "the exact-size workspace changes the result"
    finally:
        mod._ws = None
        mod._shape = None
