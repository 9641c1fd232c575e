"""The mask decoder's head (conv.hip, mask_head_kernel): sub_pixel (1,3) conv 64 -> 128, pixel shuffle and conv_1 (1,2)
64 -> 1 evaluated as one linear map whose weights the library folds at load time (api.hip, build_mask_head).

  1. the folded table against the same sums in numpy float64 from the state dict;
  2. the kernel alone against the UNFOLDED chain in float64 at the shapes where it can go wrong;
  3. the whole network on the smallest real case against the oracle, in both fp32-class matrix modes (the `complex`
     tap covers the complex decoder's reuse of the mask decoder's slot-0 image)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle import cmgan_oracle as O
from oracle.weights import make_state_dict, synthetic_clips
from test_gpu_parity import STAGE, _report

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P = "mask_decoder"


def _model(sd, mode):
    from cmgan_amd import TSCNet
    return TSCNet(num_channel=64, num_features=201, mfma_mode=mode).cuda().load_state_dict(sd).eval()


def _fold64(sd):
    """G[k][ci][r][kf], g0[r][kf] in float64; sub-pixel output channel o = r * 64 + c (generator.py:112-119)."""
    wsp = sd[P + ".sub_pixel.conv.weight"].double().numpy()[:, :, 0, :].reshape(2, 64, 64, 3)     # [r, c, ci, k]
    bsp = sd[P + ".sub_pixel.conv.bias"].double().numpy().reshape(2, 64)                           # [r, c]
    w1 = sd[P + ".conv_1.weight"].double().numpy()[0, :, 0, :]                                     # [c, kf]
    return np.einsum("cf,rcik->kirf", w1, wsp), np.einsum("cf,rc->rf", w1, bsp)


@pytest.fixture(scope="module")
def sd0():
    return make_state_dict(seed=0, num_features=201)


@pytest.fixture(scope="module")
def model0(sd0):
    return _model(sd0, "f32")          # the kernel and the fold do not depend on the matrix mode


@pytest.mark.parametrize("seed", [0, 5])
def test_fold_matches_float64(seed, sd0, model0):
    """One fp32 rounding of an exact double sum plus one ulp of slack: |diff| <= 2^-23 |value| elementwise.  A mistake
    in the r / c channel order misses this by orders of magnitude."""
    sd = sd0 if seed == 0 else make_state_dict(seed=seed, num_features=201)
    m = model0 if seed == 0 else _model(sd, "f16x3")
    G, g0 = m.engine.mask_head_weights()
    G64, g64 = _fold64(sd)
    assert G.shape == G64.shape and g0.shape == g64.shape
    for name, got, want in (("G", G, G64), ("g0", g0, g64)):
        ratio = np.abs(got.astype(np.float64) - want) / np.abs(want)
        _report(f"mask head fold seed {seed}: {name} worst |diff| / |value| (gate 2^-23 = {2.0 ** -23:.3e})", float(ratio.max()))
        assert np.all(np.abs(got.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want)), name
    assert float(np.abs(G64).max()) > 0 and float(np.abs(g64).max()) > 0


def _reference(sd, y, scale, shift):
    """The unfolded chain in float64: norm -> PReLU -> zero pad -> (1,3) conv 64 -> 128 + bias -> pixel shuffle -> the two
    conv_1 taps kept separate (the dm layout), and the bound's sum |g0| + sum |G| |v| in the same model."""
    alpha = sd[P + ".dense_block.prelu4.weight"].double()
    v = scale.double()[:, None, None, :] * y.double() + shift.double()[:, None, None, :]
    v = torch.where(v >= 0, v, alpha * v)                                     # [B, T, Fe, 64]
    x = v.permute(0, 3, 1, 2)                                                 # NCHW
    sp = F.conv2d(F.pad(x, (1, 1, 0, 0)), sd[P + ".sub_pixel.conv.weight"].double(), sd[P + ".sub_pixel.conv.bias"].double())
    b, ch, t, w = sp.shape
    sp = sp.reshape(b, 2, ch // 2, t, w).permute(0, 2, 3, 4, 1).reshape(b, ch // 2, t, w * 2)     # [B, 64, T, 2Fe]
    w1 = sd[P + ".conv_1.weight"].double()[0, :, 0, :]                                            # [c, kf]
    dm = torch.einsum("bctw,cf->btwf", sp, w1)                                                    # [B, T, 2Fe, 2]
    G64, g64 = _fold64(sd)
    Ga = torch.from_numpy(np.abs(G64))                                                            # [k, ci, r, kf]
    va = F.pad(v.abs(), (0, 0, 1, 1))                                                             # [B, T, Fe + 2, 64]
    fe = v.shape[2]
    mag = sum(torch.einsum("btfi,irk->btfrk", va[:, :, k:k + fe], Ga[k]) for k in range(3))       # [B, T, Fe, r, kf]
    mag = mag + torch.from_numpy(np.abs(g64))
    return dm, mag.reshape(b, t, 2 * fe, 2)


# the last case is not one of the issue's: 574 positions, more than the 512 one workgroup covers
@pytest.mark.parametrize("T,Fe", [(t, f) for t in (1, 3) for f in (1, 2, 5, 17, 33)] + [(7, 41)])
def test_kernel_matches_unfolded_float64(T, Fe, sd0, model0):
    """|err| <= 200 * 2^-24 * (|g0| + sum |G| |v|): 193 fp32 accumulations, the fp32 normalise and PReLU of the inputs
    and the fold's own rounding, with slack to 200.  Every element: both r, both kf, the first and last f' (Fe = 1: both
    neighbours are padding, 2: one each), a 16-position wave boundary and a ragged last wave (17, 33); entries 2 and 3
    of every row are zero."""
    B = 2
    gen = torch.Generator().manual_seed(1000 * T + Fe)
    y = torch.randn(B, T, Fe, 64, generator=gen)
    scale = torch.tensor([[0.7], [-1.3]]) * (0.5 + torch.rand(B, 64, generator=gen))      # a different pair per clip
    shift = torch.tensor([[0.4], [-0.2]]) + 0.3 * torch.randn(B, 64, generator=gen)
    want, mag = _reference(sd0, y, scale, shift)
    dm = model0.engine.mask_head(y.to(DEV), scale.to(DEV), shift.to(DEV)).cpu()
    assert dm.shape == (B, T, 2 * Fe, 4)
    assert torch.all(dm[..., 2:] == 0)
    err = (dm[..., :2].double() - want).abs()
    bound = 200 * 2.0 ** -24 * mag
    _report(f"mask head [{B}x{T}x{Fe}] worst |err| / bound", float((err / bound).max()))
    _report(f"mask head [{B}x{T}x{Fe}] vs float64", rel_err(dm[..., :2], want))
    assert torch.all(err <= bound)
    assert float(want.abs().max()) > 1e-2 and bool((y < 0).any()) and bool((y > 0).any())


def test_head_rejects_bad_shapes(model0):
    from cmgan_amd._lib import CmganError
    with pytest.raises(CmganError):
        model0.engine.mask_head(torch.zeros(1, 1, 0, 64, device=DEV), torch.zeros(1, 64, device=DEV), torch.zeros(1, 64, device=DEV))


_ORACLE = {}


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
def test_smallest_real_case_matches_oracle(mode, sd0):
    """One 0.3 s clip (T = 49) through the whole network: the `mask` tap, the `complex` tap (its dense block reads the
    slot-0 image the mask decoder's block wrote) and the outputs against the oracle, at test_gpu_parity's STAGE gate."""
    wav = synthetic_clips(1, 4800, seed=12)
    x = O.stft_compress(wav * O.rms_scale(wav)[:, None])
    if not _ORACLE:
        st = {}
        wr, wi = O.tscnet_forward(sd0, x, st)
        _ORACLE.update(st=st, real=wr, imag=wi)
    real, imag, got = _model(sd0, mode).forward_with_taps(x.to(DEV))
    for name in ("mask", "complex"):
        assert _report(f"tscnet[1x49 {mode}].{name}", rel_err(got[name], _ORACLE["st"][name])) < STAGE, name
    assert _report(f"tscnet[1x49 {mode}].real", rel_err(real, _ORACLE["real"])) < STAGE
    assert _report(f"tscnet[1x49 {mode}].imag", rel_err(imag, _ORACLE["imag"])) < STAGE
