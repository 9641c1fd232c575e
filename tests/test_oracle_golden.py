"""Pins the oracle (oracle/cmgan_oracle.py) against fixtures produced by the
reference's own modules (tests/golden/make_golden.py).  CPU only."""
import json
import os
import re

import pytest
import torch

from conftest import GOLDEN, assert_close, load_golden, rel_err
from oracle import cmgan_oracle as O
from oracle.weights import conformer_state_dict, make_state_dict, synthetic_clips

TOL = 2e-5   # fp32 re-association noise between two CPU formulations of the same sums


@pytest.fixture(scope="module")
def sd():
    return make_state_dict(seed=0, num_features=201)


def test_state_dict_manifest_matches_reference():
    with open(os.path.join(GOLDEN, "state_dict_manifest.json")) as f:
        manifest = json.load(f)
    sd = make_state_dict(0, 201)
    assert len(manifest) == 359
    assert set(manifest) == set(sd)
    for k, shape in manifest.items():
        assert list(sd[k].shape) == shape, k


def test_weights_are_deterministic():
    a, b = make_state_dict(7), make_state_dict(7)
    assert all(torch.equal(a[k], b[k]) for k in a)
    c = make_state_dict(8)
    assert not torch.equal(a["dense_encoder.conv_1.0.weight"], c["dense_encoder.conv_1.0.weight"])


def test_stft_compress_uncompress_istft():
    g = load_golden("stft.npz")
    spec = O.stft(g["wav"])
    assert rel_err(spec, g["spec"]) < 1e-6
    comp = O.power_compress(spec)
    assert rel_err(comp, g["compressed"]) < 1e-6
    unc = O.power_uncompress(comp[:, 0:1], comp[:, 1:2])
    assert rel_err(unc, g["uncompressed"]) < 1e-6
    assert rel_err(O.istft(unc.squeeze(1)), g["istft"]) < 1e-6
    # round trip through the model-layout helpers
    x = O.stft_compress(g["wav"])
    assert x.shape == (2, 2, 9, 201)
    back = O.uncompress_istft(x[:, 0:1], x[:, 1:2])
    assert rel_err(back, g["wav"]) < 1e-5


def test_conformer_block_stages():
    g = load_golden("conformer.npz")
    csd = conformer_state_dict(seed=3)
    stages = {}
    out = O.conformer_block(csd, "", g["x"], stages)
    for name in ("ff1", "attn", "conv", "ff2"):
        assert rel_err(stages[name], g[name]) < TOL, name
    assert rel_err(out, g["out"]) < TOL


def test_attention_rel_pos_clamp_beyond_512():
    g = load_golden("attention_long.npz")
    csd = conformer_state_dict(seed=3)
    out = O.attention(csd, "attn", g["x"])
    assert rel_err(out, g["out"]) < TOL


def test_tscnet_stages_and_output(sd):
    g = load_golden("tscnet.npz")
    stages = {}
    real, imag = O.tscnet_forward(sd, g["x"], stages)
    assert rel_err(stages["encoder"], g["encoder"]) < TOL
    assert rel_err(stages["tscb1"], g["tscb1"]) < TOL
    assert rel_err(stages["tscb4"], g["tscb4"]) < TOL
    assert rel_err(stages["mask"], g["mask"]) < TOL
    assert rel_err(stages["complex"], g["complex"]) < TOL
    assert rel_err(real, g["real"]) < TOL
    assert rel_err(imag, g["imag"]) < TOL


def test_tscnet_48k_variant():
    g = load_golden("tscnet48.npz")
    sd48 = make_state_dict(seed=5, num_features=601)
    real, imag = O.tscnet_forward(sd48, g["x"])
    assert rel_err(real, g["real"]) < TOL
    assert rel_err(imag, g["imag"]) < TOL


def test_pipeline_ragged_and_chunked(sd):
    g = load_golden("pipeline.npz")
    out = O.enhance(sd, g["noisy"])
    assert out.shape == (2350,)
    assert rel_err(out, g["enhanced"]) < 5e-5
    out_c = O.enhance(sd, g["noisy"], cut_len=int(g["cut_len_chunked"]))
    assert rel_err(out_c, g["enhanced_chunked"]) < 5e-5


def test_pipeline_48k_variant_ragged_chunked_and_short_output():
    """configs[3]: n_fft 1200 / hop 300 wav -> wav through the reference's own enhance_one_track glue, incl. the
    reference quirk that a 100-sample padding which is not a multiple of hop returns a SHORTER track."""
    g = load_golden("pipeline48.npz")
    sd48 = make_state_dict(seed=5, num_features=601)
    out = O.enhance(sd48, g["noisy"], cut_len=48000 * 16, n_fft=1200, hop=300)
    assert out.shape == (4150,) and rel_err(out, g["enhanced"]) < 5e-5
    out_c = O.enhance(sd48, g["noisy"], cut_len=int(g["cut_len_chunked"]), n_fft=1200, hop=300)
    assert rel_err(out_c, g["enhanced_chunked"]) < 5e-5
    out_s = O.enhance(sd48, g["noisy_short"], cut_len=48000 * 16, n_fft=1200, hop=300)
    assert out_s.shape == (2400,) == tuple(g["enhanced_short"].shape)
    assert rel_err(out_s, g["enhanced_short"]) < 5e-5


@pytest.mark.parametrize("tag", ["a", "b", "silence"])
def test_real_recordings_match_the_reference(sd, tag):
    """AudioSamples tracks (and one with gated digital silence) enhanced by the reference modules."""
    g = load_golden("tracks.npz")
    noisy = (g[f"pcm_{tag}"].float() / 32768.0)[None, :]
    out = O.enhance(sd, noisy)
    assert rel_err(out, g[f"enhanced_{tag}"]) < 5e-5
    assert_close(out, g[f"enhanced_{tag}"], rtol=1e-3, atol_rel=1e-4, name=f"track {tag}")


FFN_KEYS = ("fn.norm.weight", "fn.norm.bias", "fn.fn.net.0.weight", "fn.fn.net.0.bias", "fn.fn.net.3.weight",
            "fn.fn.net.3.bias")


@pytest.mark.parametrize("masked", [True, False])
def test_train_mode_feed_forward_and_its_gradients(masked):
    """The gradient oracle (autograd through O.feed_forward_train) against the reference module's own autograd."""
    g = load_golden("ffn_train.npz")
    csd = conformer_state_dict(seed=3)
    leaf = {"ff1." + k: csd["ff1." + k].clone().requires_grad_(True) for k in FFN_KEYS}
    x = g["x"].clone().requires_grad_(True)
    with torch.enable_grad():
        y = O.feed_forward_train(leaf, "ff1", x, g["mask1"] if masked else None, g["mask2"] if masked else None)
        y.backward(g["dy"])
    pre = "" if masked else "nomask_"
    assert rel_err(y, g["y" if masked else "y_nomask"]) < TOL
    assert rel_err(x.grad, g["dx" if masked else "dx_nomask"]) < TOL
    for k in FFN_KEYS:
        assert rel_err(leaf["ff1." + k].grad, g[pre + k.replace(".", "_")]) < TOL, k


CM_KEYS = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.conv.weight", "net.4.conv.bias",
           "net.5.weight", "net.5.bias", "net.7.weight", "net.7.bias")


def test_train_mode_conv_module_and_its_gradients():
    """BatchNorm1d on batch statistics (+ running-stat update) and every gradient vs the reference module's autograd."""
    g = load_golden("convmod_train.npz")
    csd = conformer_state_dict(seed=3)
    leaf = {"conv." + k: csd["conv." + k].clone().requires_grad_(True) for k in CM_KEYS}
    running = {"mean": csd["conv.net.5.running_mean"].clone(), "var": csd["conv.net.5.running_var"].clone()}
    x = g["x"].clone().requires_grad_(True)
    with torch.enable_grad():
        y = O.conv_module_train(leaf, "conv", x, running)
        y.backward(g["dy"])
    assert rel_err(y, g["y"]) < TOL and rel_err(x.grad, g["dx"]) < TOL
    assert rel_err(running["mean"], g["running_mean"]) < 1e-6 and rel_err(running["var"], g["running_var"]) < 1e-6
    for k in CM_KEYS:
        assert rel_err(leaf["conv." + k].grad, g["grad_" + k.replace(".", "_")]) < TOL, k


AT_KEYS = ("norm.weight", "norm.bias", "fn.to_q.weight", "fn.to_kv.weight", "fn.to_out.weight", "fn.to_out.bias",
           "fn.rel_pos_emb.weight")


def test_train_mode_attention_and_its_gradients():
    g = load_golden("attn_train.npz")
    csd = conformer_state_dict(seed=3)
    leaf = {"attn." + k: csd["attn." + k].clone().requires_grad_(True) for k in AT_KEYS}
    x = g["x"].clone().requires_grad_(True)
    with torch.enable_grad():
        y = O.attention_train(leaf, "attn", x, g["mask"])
        y.backward(g["dy"])
    assert rel_err(y, g["y"]) < TOL and rel_err(x.grad, g["dx"]) < TOL
    for k in AT_KEYS:
        assert rel_err(leaf["attn." + k].grad, g["grad_" + k.replace(".", "_")]) < TOL, k


def test_train_mode_conformer_block_and_all_its_gradients():
    g = load_golden("block_train.npz")
    csd = conformer_state_dict(seed=3)
    leaf = {k: v.clone().requires_grad_(True) for k, v in csd.items() if v.dtype == torch.float32 and "running" not in k}
    sdx = dict(csd)
    sdx.update(leaf)
    masks = {k[5:]: g[k] for k in g if k.startswith("mask_")}
    x = g["x"].clone().requires_grad_(True)
    with torch.enable_grad():
        y = O.conformer_block_train(sdx, "", x, masks)
        y.backward(g["dy"])
    assert rel_err(y, g["y"]) < TOL and rel_err(x.grad, g["dx"]) < TOL
    for k, v in leaf.items():
        want = g["grad_" + k.replace(".", "_")]
        if k == "conv.net.4.conv.bias":          # exactly zero behind a batch-statistics BatchNorm: rounding noise only
            assert float(v.grad.abs().max()) < 1e-4 * float(g["grad_conv_net_5_bias"].abs().max())
            continue
        assert rel_err(v.grad, want) < 5e-5, k


def test_train_mode_tscb(sd):
    g = load_golden("tscb_train.npz")
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items()
            if k.startswith("TSCB_1.") and v.dtype == torch.float32 and "running" not in k}
    sdx = dict(sd)
    sdx.update(leaf)
    mt = {k[len("mask_time_"):]: g[k] for k in g if k.startswith("mask_time_")}
    mf = {k[len("mask_freq_"):]: g[k] for k in g if k.startswith("mask_freq_")}
    x = g["x"].clone().requires_grad_(True)
    with torch.enable_grad():
        y = O.tscb_train(sdx, "TSCB_1", x, mt, mf)
        y.backward(g["dy"])
    assert rel_err(y, g["y"]) < TOL and rel_err(x.grad, g["dx"]) < TOL
    for k in g:
        if k.startswith("grad_"):
            name = next(n for n in leaf if n[len("TSCB_1."):].replace(".", "_") == k[5:])
            assert rel_err(leaf[name].grad, g[k]) < 5e-5, k


def test_dense_block_gradients(sd):
    """autograd through the oracle's dense_block (the gradient oracle of cmgan_amd.training.DenseBlockTrain)."""
    g = load_golden("dense_train.npz")
    pre = "dense_encoder.dilated_dense."
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith(pre)}
    sdx = dict(sd)
    sdx.update(leaf)
    x = g["x"].clone().requires_grad_(True)
    with torch.enable_grad():
        y = O.dense_block(sdx, pre[:-1], x)
        y.backward(g["dy"])
    assert rel_err(y, g["y"]) < TOL and rel_err(x.grad, g["dx"]) < TOL
    for k, v in leaf.items():
        want = g["grad_" + k[len(pre):].replace(".", "_")]
        if ".conv" in k and k.endswith(".bias"):     # a bias in front of an InstanceNorm: exactly zero gradient
            assert float(v.grad.abs().max()) < 1e-4 * float(g["grad_norm1_bias"].abs().max())
            continue
        assert rel_err(v.grad, want) < 5e-5, k


def test_dense_encoder_gradients(sd):
    g = load_golden("encoder_train.npz")
    pre = "dense_encoder."
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith(pre)}
    sdx = dict(sd)
    sdx.update(leaf)
    with torch.enable_grad():
        y = O.dense_encoder(sdx, g["x"])
        y.backward(g["dy"])
    assert rel_err(y, g["y"]) < TOL
    for k, v in leaf.items():
        want = g["grad_" + k[len(pre):].replace(".", "_")]
        if k.endswith(".0.bias") or re.search(r"\.conv\d\.bias$", k):          # conv biases in front of an InstanceNorm
            assert float(v.grad.abs().max()) < 1e-4 * float(g["grad_conv_1_1_bias"].abs().max())
            continue
        assert rel_err(v.grad, want) < 5e-5, k


def _decoder_case(sd, fixture, pre, fn, num_features=None):
    g = load_golden(fixture)
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith(pre)}
    if num_features is not None:
        leaf[pre + "prelu_out.weight"] = sd[pre + "prelu_out.weight"][:num_features].clone().requires_grad_(True)
    sdx = dict(sd)
    sdx.update(leaf)
    x = g["x"].clone().requires_grad_(True)
    with torch.enable_grad():
        y = fn(sdx, x)
        y.backward(g["dy"])
    assert rel_err(y, g["y"]) < TOL
    assert rel_err(x.grad, g["dx"]) < 5e-5
    ref_scale = float(g["grad_norm_bias"].abs().max())
    for k, v in leaf.items():
        want = g["grad_" + k[len(pre):].replace(".", "_")]
        zero = [r"\.conv\d\.bias$", r"sub_pixel\.conv\.bias$"] if "complex" in pre else [r"\.conv\d\.bias$", r"conv_1\.bias$"]
        if any(re.search(z, k) for z in zero):
            # a bias in front of an InstanceNorm: exactly zero gradient (rounding noise in both implementations)
            assert float((v.grad - want).abs().max()) < 1e-4 * max(ref_scale, float(want.abs().max())), k
            continue
        assert rel_err(v.grad, want) < 5e-5, k


def test_mask_decoder_gradients(sd):
    _decoder_case(sd, "maskdec_train.npz", "mask_decoder.", O.mask_decoder, num_features=21)


def test_complex_decoder_gradients(sd):
    _decoder_case(sd, "complexdec_train.npz", "complex_decoder.", O.complex_decoder)


def test_generator_step_gradients(sd):
    """One generator optimisation step of the reference trainer minus the discriminator: loss terms, the gradients at
    the network output and the digests of all 335 parameter gradients."""
    from cmgan_amd.synth import sample_indices, synthetic_dropout_masks
    g = load_golden("generator_step.npz")
    masks = [tuple({k: torch.from_numpy(v) for k, v in d.items()} for d in pair)
             for pair in synthetic_dropout_masks(77, 2, 9, 101)]
    out = O.generator_step_gradients(sd, g["clean"], g["noisy"], masks)
    assert abs(float(out["loss"]) - float(g["loss"])) < 2e-5 * abs(float(g["loss"]))
    assert rel_err(out["terms"], g["terms"]) < 2e-5
    assert rel_err(out["est_real"], g["est_real"]) < 5e-5 and rel_err(out["est_imag"], g["est_imag"]) < 5e-5
    assert rel_err(out["d_real"], g["d_real"]) < 5e-5 and rel_err(out["d_imag"], g["d_imag"]) < 5e-5
    keys = [k[len("gsmp_"):] for k in g if k.startswith("gsmp_")]
    assert len(keys) == 335 and set(keys) == set(out["grads"])
    scale = max(float(g["gl2_" + k]) for k in keys)
    for k in keys:
        got = out["grads"][k].reshape(-1)
        l2 = float(g["gl2_" + k])
        smp = got[torch.from_numpy(sample_indices(got.numel()))]
        tol = 1e-4 * l2 + 1e-7 * scale                                  # zero-gradient biases: absolute floor
        assert float((smp - g["gsmp_" + k]).abs().max()) < tol + 1e-4 * float(g["gsmp_" + k].abs().max()), k
        assert abs(float(got.double().norm()) - l2) < 1e-4 * l2 + 1e-7 * scale, k


def test_generator_gradient_noise_floor(sd):
    """How well-defined the whole-network gradient is: the same step through the oracle in fp64.  PReLU and |.| kinks
    make single elements jump, so fp32 autograd (the reference's and any re-implementation) agrees with fp64 only to
    ~2e-4 (median over tensors, relative to the tensor's max) and ~1e-2 (worst tensor) on this fixture; the GPU test
    of the whole step uses this measured floor as its bar, the per-module tests stay at 1e-6."""
    from cmgan_amd.synth import synthetic_dropout_masks
    g = load_golden("generator_step.npz")
    masks = [tuple({k: torch.from_numpy(v) for k, v in d.items()} for d in pair)
             for pair in synthetic_dropout_masks(77, 2, 9, 101)]
    o32 = O.generator_step_gradients(sd, g["clean"], g["noisy"], masks)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    m64 = [tuple({k: v.double() for k, v in d.items()} for d in pair) for pair in masks]
    o64 = O.generator_step_gradients(sd64, g["clean"].double(), g["noisy"].double(), m64)
    scale = max(float(v.abs().max()) for v in o64["grads"].values())
    errs = []
    for k, v64 in o64["grads"].items():
        den = float(v64.abs().max())
        if den > 1e-6 * scale:
            errs.append(float((o32["grads"][k].double() - v64).abs().max()) / den)
    errs = sorted(errs)
    print(f"[noise floor] fp32 vs fp64 autograd: median {errs[len(errs) // 2]:.2e}, worst {errs[-1]:.2e}")
    assert 1e-5 < errs[len(errs) // 2] < 1e-3 and errs[-1] < 5e-2


def test_gradient_noise_floor_disappears_in_the_kink_free_twin(sd):
    """The same measurement with every PReLU slope at 1 - 1e-3 i / n (cmgan_amd.synth.kink_free_twin): fp32 and fp64
    autograd now agree to rounding on EVERY tensor (measured: median 1e-6, worst 1e-5), i.e. the 1e-2 above is the
    kinks and nothing else.  The whole-step GPU tests use this twin to hold every gradient of the full pipeline to
    the 1e-3 gate (tests/test_gpu_training.py)."""
    from cmgan_amd.synth import kink_free_twin, synthetic_dropout_masks
    g = load_golden("generator_step.npz")
    tw = kink_free_twin(sd)
    assert sum(1 for k in sd if not torch.equal(sd[k], tw[k])) == 17           # the 17 PReLU modules of TSCNet
    masks = [tuple({k: torch.from_numpy(v) for k, v in d.items()} for d in pair)
             for pair in synthetic_dropout_masks(77, 2, 9, 101)]
    o32 = O.generator_step_gradients(tw, g["clean"], g["noisy"], masks)
    tw64 = {k: (v.double() if v.is_floating_point() else v) for k, v in tw.items()}
    m64 = [tuple({k: v.double() for k, v in d.items()} for d in pair) for pair in masks]
    o64 = O.generator_step_gradients(tw64, g["clean"].double(), g["noisy"].double(), m64)
    scale = max(float(v.abs().max()) for v in o64["grads"].values())
    errs = sorted(float((o32["grads"][k].double() - v).abs().max()) / float(v.abs().max())
                  for k, v in o64["grads"].items() if float(v.abs().max()) > 1e-6 * scale)
    print(f"[noise floor, kink-free twin] fp32 vs fp64 autograd: median {errs[len(errs) // 2]:.2e}, worst {errs[-1]:.2e}")
    assert errs[-1] < 1e-4


def test_discriminator_forward_and_gradients():
    """Metric discriminator in train mode: one spectral-norm power iteration, dropout mask, autograd vs the reference
    module; then the eval-mode score with the updated u / v."""
    from cmgan_amd.synth import discriminator_state_dict
    g = load_golden("disc_train.npz")
    dsd = discriminator_state_dict(0)
    leaf = {k: v.clone().requires_grad_(True) for k, v in dsd.items() if not (k.endswith("_u") or k.endswith("_v"))}
    sdx = dict(dsd)
    sdx.update(leaf)
    x, y = g["x"].clone().requires_grad_(True), g["y"].clone().requires_grad_(True)
    with torch.enable_grad():
        score, new = O.discriminator(sdx, x, y, g["mask"], train=True)
        score.backward(g["dscore"])
    assert rel_err(score, g["score"]) < TOL
    assert rel_err(x.grad, g["dx"]) < 5e-5 and rel_err(y.grad, g["dy"]) < 5e-5
    for k, v in leaf.items():
        assert rel_err(v.grad, g["grad_" + k.replace(".", "_")]) < 5e-5, k
    for k, v in new.items():
        assert rel_err(v, g["new_" + k.replace(".", "_")]) < TOL, k
    sde = dict(dsd)
    sde.update(new)
    score_eval, _ = O.discriminator(sde, g["x"], g["y"], None, train=False)
    assert rel_err(score_eval, g["score_eval"]) < TOL


def test_adversarial_generator_gradients(sd):
    """The generator half of the reference's full train step (loss incl. 0.05 x gen_loss_GAN through the metric
    discriminator) at T = 33: loss, GAN term and the digests of all 335 parameter gradients."""
    import numpy as np
    from cmgan_amd.synth import discriminator_state_dict, sample_indices, synthetic_dropout_masks
    g = load_golden("adversarial_step.npz")
    masks = [tuple({k: torch.from_numpy(v) for k, v in d.items()} for d in pair)
             for pair in synthetic_dropout_masks(78, 2, 33, 101)]
    dmask = torch.from_numpy((np.random.RandomState(79).random_sample((2, 64)) >= 0.3).astype(np.float32) / np.float32(0.7))
    out = O.adversarial_generator_gradients(sd, discriminator_state_dict(0), g["clean"], g["noisy"], masks, dmask)
    assert abs(float(out["loss"]) - float(g["loss"])) < 2e-5 * float(g["loss"])
    assert abs(float(out["gan"]) - float(g["gan"])) < 2e-5 * float(g["gan"])
    errs = []
    scale = max(float(g["gl2_" + k]) for k in out["grads"])
    for k, v in out["grads"].items():
        want = g["gsmp_" + k]
        if float(g["gl2_" + k]) > 1e-4 * scale:
            smp = v.reshape(-1)[torch.from_numpy(sample_indices(v.numel()))]
            errs.append(float((smp - want).abs().max()) / float(want.abs().max()))
    errs.sort()
    assert errs[len(errs) // 2] < 2e-5 and errs[-1] < 3e-2


def test_conformer_block_with_attention_mask():
    """ConformerBlock.forward(x, mask): the [b, n] bool mask of conformer.py:113-126 (ragged lengths and an arbitrary
    pattern incl. fully masked query rows)."""
    g = load_golden("conformer_mask.npz")
    csd = conformer_state_dict(seed=3)
    out = O.conformer_block(csd, "", g["x"], mask=g["mask"].bool())
    assert rel_err(out, g["out"]) < TOL


def test_validation_step_losses_match_the_reference(sd):
    """Generator half of Trainer.test_step: forward_generator_step + the three non-adversarial loss terms."""
    g = load_golden("valstep.npz")
    out = O.forward_generator_step(sd, g["clean"], g["noisy"])
    assert rel_err(out["est_audio"], g["est_audio"]) < 5e-5
    loss, l_ri, l_mag, l_time = O.generator_loss(out, g["clean"])
    for got, key in ((loss, "loss"), (l_ri, "loss_ri"), (l_mag, "loss_mag"), (l_time, "time_loss")):
        assert abs(float(got) - float(g[key])) < 2e-5 * abs(float(g[key])), key


def test_chunk_rows_rule():
    # evaluation.py:30-34: smallest divisor of 100 that is >= ceil(len / cut_len)
    assert O.chunk_rows(2400, 1000) == 4
    assert O.chunk_rows(256000, 256000) == 1
    assert O.chunk_rows(256100, 256000) == 2
    assert O.chunk_rows(3 * 256000, 256000) == 4      # 3 does not divide 100
    assert O.chunk_rows(6 * 256000 + 100, 256000) == 10


# ------------------------------------------------------------------ oracle/_ref: the reference's own modules
def _ref_runner():
    from oracle import ref_runner                     # oracle/_ref is a build() product (oracle/make_ref.py)
    if not ref_runner.available():
        pytest.skip("oracle/_ref not built (build() found no reference tree to compile it from)")
    return ref_runner


def test_ref_modules_reproduce_the_committed_goldens_bit_for_bit(sd):
    """oracle/_ref is the bytecode of /root/reference/src/models/{generator,conformer}.py + utils.py: run on the
    golden inputs it must return the golden outputs EXACTLY (the fixtures were made by the same modules), and the
    oracle port must agree with it at fp32 rounding level on a fresh input."""
    R = _ref_runner()
    g = load_golden("tscnet.npz")
    model = R.tscnet(sd)
    real, imag = model(g["x"])
    assert torch.equal(real, g["real"]) and torch.equal(imag, g["imag"])
    wav = synthetic_clips(1, 3200, seed=21)
    got = O.enhance_batch(sd, wav)
    want = R.enhance_batch(model, wav)
    assert rel_err(got, want) < 2e-5


def test_ref_enhance_glue_matches_the_pipeline_golden(sd):
    """ref_runner.enhance = src/evaluation.py:21-53 around the reference modules: the ragged clip and the > cut_len
    chunked form of the committed golden, bit for bit."""
    R = _ref_runner()
    g = load_golden("pipeline.npz")
    model = R.tscnet(sd)
    assert torch.equal(R.enhance(model, g["noisy"]), g["enhanced"])
    assert torch.equal(R.enhance(model, g["noisy"], cut_len=int(g["cut_len_chunked"])), g["enhanced_chunked"])
