"""The inference conv path - dense encoder, mask / complex decoders, their InstanceNorm statistics (conv.hip, conv_x3.hip,
in_running.hip) - against the project's oracle in FLOAT64 (tests/convpath_model.py), at the plane widths, clip lengths
and grid sizes where the tilings change.  The GPU sees random spectrograms [B, 2, T, F] directly; no STFT is involved.

Per case and matrix mode:
  encoder     the `encoder` tap of forward_with_taps vs dense_encoder;
  decoders    the GPU's own tscb4 tap fed to the float64 decoders (so the conformers are not part of the comparison) vs the
              `mask` / `complex` taps and the recombined out_real / out_imag;
  statistics  every norm's (scale, shift) [B][64] and the mask head's pair from the blob of tscnet_forward_stats on the same
              input, one by one, vs gamma / sqrt(var + eps), beta - mean * scale of the float64 pass;
  frozen      stream_encoder / stream_decoder on a blob built from those float64 statistics (the decoder on an arbitrary
              random x [B, T, F', 64]) vs the oracle replaying the same statistics: conv arithmetic without reductions;
  running     stream_*_running with hist = 0 on zeroed sums vs the float64 own-statistics result and pairs: in_running.hip.

Tolerances are the suite's (test_gpu_parity): STAGE = 2e-4 max-norm plus assert_close(rtol 1e-3, atol_rel 2e-5) for f32 and
f16x3; a statistics vector is held to STAGE relative to its own max; f16x1 (widths only, final outputs only) to GATE.
Tile counts the cases are named for are computed from the tile sizes and asserted, so a tile change cannot move them."""
import numpy as np
import pytest
import torch

import convpath_model as M
from conftest import assert_close, rel_err
from oracle.weights import make_state_dict

pytestmark = pytest.mark.gpu

GATE = 1e-3
STAGE = 2e-4
DEV = "cuda:0"

_MODELS, _SD, _REF = {}, {}, {}


def _sd(n_fft):
    if n_fft not in _SD:
        sd = make_state_dict(seed=0, num_features=n_fft // 2 + 1)
        _SD[n_fft] = (sd, M.to64(sd))
    return _SD[n_fft]


def _model(n_fft, mode, sd=None, tag=""):
    key = (n_fft, mode, tag)
    if key not in _MODELS:
        from cmgan_amd import TSCNet
        m = TSCNet(num_channel=64, num_features=n_fft // 2 + 1, mfma_mode=mode).cuda()
        _MODELS[key] = m.load_state_dict(sd if sd is not None else _sd(n_fft)[0]).eval()
        assert _MODELS[key].engine.mfma_mode == mode
    return _MODELS[key]


def _inputs(n_fft, B, T):
    """(spec [B,2,T,F], x [B,T,F',64]) float32, seeded by the shape"""
    F = n_fft // 2 + 1
    rng = np.random.Generator(np.random.PCG64(7000 + 131 * n_fft + 17 * T + B))
    spec = torch.from_numpy(rng.standard_normal((B, 2, T, F)).astype(np.float32))
    x = torch.from_numpy(rng.standard_normal((B, T, (F + 1) // 2, 64)).astype(np.float32))
    return spec, x


def _shared_ref(n_fft, B, T, sd64, tag, spec, x):
    """What does not depend on the matrix mode, computed once per shape: the float64 encoder and its statistics, and
    the float64 decoders on the arbitrary x with their own statistics."""
    key = (n_fft, B, T, tag)
    if key not in _REF:
        enc, st_enc = M.encoder(sd64, spec.double())
        own, st_x = M.decoders(sd64, x.double().permute(0, 3, 1, 2), spec.double())
        _REF[key] = {"enc": enc, "st_enc": st_enc, "own": own, "st_x": st_x}
    return _REF[key]


class _Checks:
    """Runs every comparison of a case, prints each figure in the suite's `[parity]` style and fails at the end with the
    names of all that missed, so that one run shows the whole picture and a wrong norm is named."""

    def __init__(self, case):
        self.case, self.failed = case, []

    def report(self, name, err, bar):
        print(f"[parity] {self.case} {name}: rel_err = {err:.3e}")
        if not err < bar:
            self.failed.append(f"{name}: {err:.3e} >= {bar:g}")

    def close(self, name, got, want, gate=STAGE):
        """test_gpu_parity._check: max-norm relative error under `gate` and the elementwise rtol / atol_rel bound"""
        self.report(name, rel_err(got, want), gate)
        try:
            assert_close(got, want, rtol=1e-3, atol_rel=2e-5, name=name)
        except AssertionError as e:
            self.failed.append(str(e))

    def pairs(self, tag, got: dict, want: dict):
        """per norm: scale and shift, each relative to the max of its float64 counterpart"""
        assert set(got) == set(want)
        for k in want:
            for what, g, w in (("scale", got[k][0], want[k][0]), ("shift", got[k][1], want[k][1])):
                self.report(f"{tag} {k}.{what}", rel_err(g, w), STAGE)

    def done(self):
        assert not self.failed, f"{self.case}: " + "; ".join(self.failed)


def _run_case(n_fft, B, T, mode, sd=None, sd64=None, tag="", final_only=False, x=None):
    """Every comparison of the module header for one shape and mode.  Returns the float64 statistics of the two passes:
    (the GPU-tap pass, the arbitrary-x pass)."""
    if sd64 is None:
        sd, sd64 = _sd(n_fft)
    model = _model(n_fft, mode, sd, tag)
    eng = model.engine
    spec, x_rand = _inputs(n_fft, B, T)
    x = x_rand if x is None else x
    ref = _shared_ref(n_fft, B, T, sd64, tag, spec, x)
    ck = _Checks(f"convpath[n_fft={n_fft} B={B} T={T} {mode}{tag}]")
    spec_d, x_d = spec.to(DEV), x.to(DEV)

    # ---- own statistics: taps, the decoders on the GPU's own TSCB output ----------------------------------------
    real, imag, taps = model.forward_with_taps(spec_d)
    h = taps["tscb4"].double().cpu()
    dec, st_dec = M.decoders(sd64, h, spec.double())
    if final_only:                                   # f16x1: the one claim the project makes for that mode
        ck.report("out_real", rel_err(real, dec["real"]), GATE)
        ck.report("out_imag", rel_err(imag, dec["imag"]), GATE)
        ck.done()
        return None
    ck.close("encoder", taps["encoder"], ref["enc"])
    ck.close("mask", taps["mask"], dec["mask"])
    ck.close("complex", taps["complex"], dec["complex"])
    ck.close("out_real", real, dec["real"])
    ck.close("out_imag", imag, dec["imag"])

    # ---- statistics, norm by norm ---------------------------------------------------------------------------------
    r2, i2, blob = eng.tscnet_forward_stats(spec_d)
    assert torch.equal(r2, real) and torch.equal(i2, imag), "the forward is not bit-reproducible"
    st_all = dict(ref["st_enc"])
    st_all.update(st_dec)
    assert set(st_all) == set(M.NORM_KEYS + [M.MASK_KEY])
    ck.pairs("stats", M.parse_blob(blob, sd64, B), M.pairs(sd64, st_all))

    # ---- frozen: the float64 statistics replayed on both sides ------------------------------------------------------
    frozen = M.build_blob(st_all, sd64, B).to(DEV)
    xe = eng.stream_encoder(spec_d, frozen)                                     # [B,T,F',64]
    ck.close("frozen encoder", xe.permute(0, 3, 1, 2), M.encoder(sd64, spec.double(), replay=ref["st_enc"])[0])
    fr, fi = eng.stream_decoder(x_d, spec_d, frozen)
    want = M.decoders(sd64, x.double().permute(0, 3, 1, 2), spec.double(), replay=st_dec)[0]
    ck.close("frozen out_real", fr, want["real"])
    ck.close("frozen out_imag", fi, want["imag"])

    # ---- running statistics from zeroed sums = own statistics --------------------------------------------------------
    sums = torch.zeros(eng.stream_sums_doubles(B), dtype=torch.float64, device=DEV)
    used = torch.zeros(eng.stats_floats(B), device=DEV)
    xr = eng.stream_encoder_running(spec_d, 0, sums, stats_out=used)
    ck.close("running encoder", xr.permute(0, 3, 1, 2), ref["enc"])
    rr, ri = eng.stream_decoder_running(x_d, spec_d, 0, sums, stats_out=used)
    ck.close("running out_real", rr, ref["own"]["real"])
    ck.close("running out_imag", ri, ref["own"]["imag"])
    st_run = dict(ref["st_enc"])
    st_run.update(ref["st_x"])
    ck.pairs("running", M.parse_blob(used, sd64, B), M.pairs(sd64, st_run))
    ck.done()
    return st_all, st_run


MODES = ["f32", "f16x3"]

# n_fft -> (F, F'): 16 below the epilogue's 16-step; 64; 128 encoder wide / decoders narrow; 240 one below the limit in
# the decoders; 256 the narrowest plane on the x3 kernels; 512; 400 the anchor
WIDTHS = {16: (9, 5), 64: (33, 17), 128: (65, 33), 240: (121, 61), 256: (129, 65), 400: (201, 101), 512: (257, 129)}


@pytest.mark.parametrize("mode", MODES + ["f16x1"])
@pytest.mark.parametrize("n_fft", sorted(WIDTHS))
def test_plane_widths(n_fft, mode):
    F, F2 = WIDTHS[n_fft]
    assert (F, F2) == (n_fft // 2 + 1, n_fft // 4 + 1)
    # which kernel each conv of the case runs on in the split-f16 modes (f32 mode: always the fp32 kernel)
    kernels = [M.dense_ntiles("f16x3", 11, F, 64)[0], M.dense_ntiles("f16x3", 11, F2, 64)[0], M.dense_ntiles("f16x3", 11, F2, 128)[0]]
    assert kernels == {16: ["f32"] * 3, 64: ["f32"] * 3, 128: ["x3", "f32", "x3"], 240: ["x3", "f32", "x3"],
                       256: ["x3"] * 3, 400: ["x3"] * 3, 512: ["x3"] * 3}[n_fft]
    _run_case(n_fft, 2, 11, mode, final_only=mode == "f16x1")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", [1, 2, 3, 8, 9, 17])
@pytest.mark.parametrize("n_fft", [256, 400])
def test_time_edges(n_fft, T, mode):
    """T < dil: every t - dil tap of a dense layer (dil 1, 2, 4, 8) is padding; T = dil + 1: one row of it is not.
    B = 3, so the clip offsets of every kernel matter."""
    _run_case(n_fft, 3, T, mode)


# (B, T) -> B * ntiles of the x3 dense conv on the encoder plane of n_fft 256 (F 129): xcd_contiguous_block()'s remap with
# fewer blocks than XCDs, one more / one less than a multiple of 8, and a remainder
GRIDS = {(1, 1): 1, (3, 1): 3, (7, 1): 7, (2, 7): 8, (3, 5): 9, (1, 33): 17}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,T", sorted(GRIDS))
def test_grid_sizes_of_the_xcd_remap(B, T, mode):
    kernel, nt = M.dense_ntiles("f16x3", T, 129, 64)
    assert kernel == "x3" and B * nt == GRIDS[(B, T)]
    assert sorted(GRIDS.values()) == [1, 3, 7, 8, 9, 17]
    _run_case(256, B, T, mode)


# mode -> {T: tiles per clip of the dense conv the case is named for} at n_fft 256, B = 1: in_finalize_kernel walks the
# tiles 16 ways x 8 loads, so 1, < 16, 16, 17, 128 (one full pass), 129 and 145 (a second pass of 1 and of 17 tiles).  The
# encoder plane (F 129) has 130 positions per frame, more than an fp32 tile: its one-tile case is the decoders' plane.
FINALIZE = {"f32": {1: 1, 14: 15, 15: 16, 16: 17, 126: 128, 127: 129, 142: 145},
            "f16x3": {1: 1, 28: 15, 30: 16, 32: 17, 249: 128, 251: 129, 282: 145}}


@pytest.mark.parametrize("mode,T", [(m, T) for m in MODES for T in sorted(FINALIZE[m])])
def test_finalize_loop_edges(mode, T):
    want = FINALIZE[mode][T]
    assert sorted(FINALIZE[mode].values()) == [1, 15, 16, 17, 128, 129, 145]
    plane = 65 if (mode == "f32" and T == 1) else 129
    assert M.dense_ntiles(mode, T, plane, 64) == ("f32" if mode == "f32" else "x3", want)
    assert want <= M.INF_NP * M.INF_LOADS or want - M.INF_NP * M.INF_LOADS in (1, 17)
    _run_case(256, 1, T, mode)


@pytest.mark.parametrize("mode", MODES)
def test_offset_statistics(mode):
    """Every pre-norm channel 8 .. 16 standard deviations from zero (conv biases raised, convpath_model.offset_state_dict):
    E[x^2] - mean^2 from fp32 tile partials loses about (1 + r^2) 2^-24 of the variance, 2e-5 at r = 16 - inside STAGE.
    Guards against moving the partials to a narrower type or a longer fp32 chain.
    The ratio is a property of biases AND input, so the arbitrary x of the frozen / running decoder checks is here a
    TSCB-like tensor (the TSCB output the biases were aimed with, plus a quarter of its deviation in white noise): unit
    white noise, a ninth of a TSCB output's deviation, would sit 60 .. 120 deviations out, which is not this case."""
    n_fft, B, T = 256, 2, 33
    if "offset" not in _SD:
        sd, sd64 = _sd(n_fft)
        spec, x = _inputs(n_fft, B, T)
        # the decoders' biases are aimed with the split-f16 model's TSCB output; the ratio is asserted below on what each
        # mode's own run recorded
        h = _model(n_fft, "f16x3").forward_with_taps(spec.to(DEV))[2]["tscb4"].cpu()
        off = M.offset_state_dict(sd, spec, h)
        _SD["offset"] = (off, M.to64(off), (h.permute(0, 2, 3, 1) + 0.25 * h.std() * x).contiguous())
    sd, sd64, x = _SD["offset"]
    for which, st in zip(("own", "running"), _run_case(n_fft, B, T, mode, sd, sd64, tag=" offset", x=x)):
        ratios = M.offset_ratios(st)
        assert set(ratios) == set(M.NORM_KEYS + [M.MASK_KEY])
        for k, r in ratios.items():
            print(f"[offset] {which} {k}: |mean| / std in [{float(r.min()):.2f}, {float(r.max()):.2f}]")
            assert 8.0 <= float(r.min()) and float(r.max()) <= 16.0, (which, k)
