"""CPU checks of tests/convpath_model.py, the float64 reference tests/test_gpu_convpath.py holds the conv path to: the
statistics blob round-trips, float64 is the fp32 oracle up to fp32 rounding, the offset state dict does what its name
says, and the GPU file's case tables reach the tile counts they are named for."""
import torch

import convpath_model as M
import test_gpu_convpath as G
from conftest import rel_err
from oracle import cmgan_oracle as O
from oracle.weights import make_state_dict


def _case(n_fft=64, B=2, T=5):
    sd = make_state_dict(seed=0, num_features=n_fft // 2 + 1)
    spec, x = G._inputs(n_fft, B, T)
    return sd, M.to64(sd), spec, x


def test_blob_builder_and_its_inverse_round_trip():
    sd, sd64, spec, x = _case()
    B = spec.size(0)
    _, st = M.encoder(sd64, spec.double())
    st.update(M.decoders(sd64, x.double().permute(0, 3, 1, 2), spec.double())[1])
    assert list(st) == M.ENC_KEYS + M.DEC_KEYS[:4] + [M.MASK_KEY] + M.DEC_KEYS[4:] and len(M.NORM_KEYS) == 15
    blob = M.build_blob(st, sd64, B)
    assert blob.dtype == torch.float32 and blob.numel() == M.stats_floats(B) == 16 * 2 * B * 64 + 2 * B
    got, want = M.parse_blob(blob, sd64, B), M.pairs(sd64, st)
    assert set(got) == set(want) == set(M.NORM_KEYS + [M.MASK_KEY])
    for k in want:
        assert got[k][0].shape == want[k][0].shape == (B, 1 if k == M.MASK_KEY else 64)
        assert rel_err(got[k][0], want[k][0]) < 1e-7 and rel_err(got[k][1], want[k][1]) < 2e-7, k
    # slot 15 is unused, the encoder-only blob leaves the decoders' slots zero
    assert not blob[15 * 2 * B * 64:16 * 2 * B * 64].any()
    enc_only = M.build_blob({k: st[k] for k in M.ENC_KEYS}, sd64, B)
    assert torch.equal(enc_only[:6 * 2 * B * 64], blob[:6 * 2 * B * 64]) and not enc_only[6 * 2 * B * 64:].any()


def test_float64_reference_is_the_fp32_oracle_up_to_fp32_rounding():
    sd, sd64, spec, x = _case(n_fft=64, B=2, T=9)
    enc32 = O.dense_encoder(sd, M._model_in(spec))
    enc64, st = M.encoder(sd64, spec.double())
    assert enc64.dtype == torch.float64 and rel_err(enc32, enc64) < 2e-5
    h = x.permute(0, 3, 1, 2)
    dec64, st_dec = M.decoders(sd64, h.double(), spec.double())
    assert rel_err(O.mask_decoder(sd, h), dec64["mask"]) < 2e-5
    assert rel_err(O.complex_decoder(sd, h), dec64["complex"]) < 2e-5
    # recombination: mask * (re, im) is the reference's mask * mag * (cos, sin)(phase)
    re, im = spec[:, 0:1].double(), spec[:, 1:2].double()
    mag, ph = torch.sqrt(re * re + im * im), torch.atan2(im, re)
    assert rel_err(dec64["real"], dec64["mask"] * mag * torch.cos(ph) + dec64["complex"][:, 0:1]) < 1e-14
    assert rel_err(dec64["imag"], dec64["mask"] * mag * torch.sin(ph) + dec64["complex"][:, 1:2]) < 1e-14
    # replaying a pass's own statistics is that pass
    assert rel_err(M.encoder(sd64, spec.double(), replay=st)[0], enc64) < 1e-13
    assert rel_err(M.decoders(sd64, h.double(), spec.double(), replay=st_dec)[0]["real"], dec64["real"]) < 1e-13


def test_offset_state_dict_puts_every_norm_input_8_to_16_deviations_from_zero():
    n_fft, B, T = 256, 2, 33                                   # the GPU case
    sd, sd64, spec, _ = _case(n_fft, B, T)
    enc, st0 = M.encoder(sd64, spec.double())
    h = enc
    for b in range(1, 5):
        h = O.tscb(sd64, f"TSCB_{b}", h)
    off = M.offset_state_dict(sd, spec, h)
    changed = sorted(k for k in sd if not torch.equal(sd[k], off[k]))
    assert changed == sorted(M.BIAS_OF.values()) and len(changed) == 16
    off64 = M.to64(off)
    enc1, st = M.encoder(off64, spec.double())
    assert rel_err(enc1, enc) < 1e-6                           # a bias in front of an InstanceNorm changes nothing behind it
    st.update(M.decoders(off64, h, spec.double())[1])
    ratios = M.offset_ratios(st)
    assert set(ratios) == set(M.NORM_KEYS + [M.MASK_KEY])
    for k, r in ratios.items():
        assert 8.0 <= float(r.min()) and float(r.max()) <= 16.0, (k, float(r.min()), float(r.max()))
    assert max(float(r.max()) for r in M.offset_ratios(st0).values()) < 8.0     # the plain state dict is nowhere near


def test_gpu_case_tables_reach_the_tile_counts_they_are_named_for():
    for n_fft, (F, F2) in G.WIDTHS.items():
        assert (F, F2) == (n_fft // 2 + 1, n_fft // 4 + 1) and n_fft % 16 == 0 and (n_fft // 4) % 4 == 0
    assert [M.conv3x_walkable(G.WIDTHS[n][1], 64) for n in (240, 256)] == [False, True]
    for (B, T), grid in G.GRIDS.items():
        assert B * M.dense_ntiles("f16x3", T, 129, 64)[1] == grid
    for mode, table in G.FINALIZE.items():
        for T, nt in table.items():
            plane = 65 if (mode == "f32" and T == 1) else 129
            assert M.dense_ntiles(mode, T, plane, 64)[1] == nt, (mode, T)
    assert max(max(t) for t in G.FINALIZE.values()) < 300
