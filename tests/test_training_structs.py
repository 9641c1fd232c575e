"""The ctypes parameter structs of cmgan_amd.training, field by field: every pointer is the `data_ptr()` of the tensor
the kernels expect there.  CPU tensors, no Engine, no library: a swapped table entry shows up as a named field here
instead of as a wrong gradient on the GPU.  The expected keys are written out independently of the tables under test."""
import collections
import ctypes

import pytest
import torch

from cmgan_amd import training as T
from cmgan_amd._lib import (AttnParams, ConvModParams, DecoderParams, DenseParams, DiscParams, EncoderParams,
                            FfnParams)


class Tensors(dict):
    """One distinct small CPU tensor per key of a shape table; counts how often each key is read."""

    def __init__(self, keys):
        super().__init__({k: torch.zeros(2) for k in keys})
        self.reads = collections.Counter()
        assert len({t.data_ptr() for t in self.values()}) == len(self)

    def __getitem__(self, key):
        self.reads[key] += 1
        return super().__getitem__(key)

    def assert_each_read_once(self):
        assert dict(self.reads) == {k: 1 for k in self}


def pointers(s, path=""):
    """{field path: pointer or None} over every pointer of a struct, sub-structs and arrays included."""
    out = {}
    for name, ctype in s._fields_:
        value = getattr(s, name)
        if issubclass(ctype, ctypes.Structure):
            out.update(pointers(value, f"{path}{name}."))
        elif issubclass(ctype, ctypes.Array):
            out.update({f"{path}{name}[{i}]": v for i, v in enumerate(value)})
        else:
            out[path + name] = value
    return out


def check(s, struct_type, expected, *sources):
    """`expected`: {field path: key}; the key is looked up in `sources` (tensor dicts with disjoint keys).  Every other
    pointer of the struct must be null, every key of every source read exactly once."""
    assert type(s) is struct_type
    got = pointers(s)
    assert set(expected) <= set(got)
    lookup = {k: dict.__getitem__(src, k) for src in sources for k in src}
    for field, value in got.items():
        if field in expected:
            assert value == lookup[expected[field]].data_ptr(), f"{field} does not point at {expected[field]}"
        else:
            assert not value, f"{field} must stay null"
    for src in sources:
        src.assert_each_read_once()


def dense_expected(field_prefix="", key_prefix=""):
    exp = {}
    for i in range(4):
        exp[f"{field_prefix}conv_weight[{i}]"] = f"{key_prefix}conv{i + 1}.weight"
        exp[f"{field_prefix}conv_bias[{i}]"] = f"{key_prefix}conv{i + 1}.bias"
        exp[f"{field_prefix}norm_weight[{i}]"] = f"{key_prefix}norm{i + 1}.weight"
        exp[f"{field_prefix}norm_bias[{i}]"] = f"{key_prefix}norm{i + 1}.bias"
        exp[f"{field_prefix}prelu_weight[{i}]"] = f"{key_prefix}prelu{i + 1}.weight"
    return exp


def test_feed_forward_struct():
    t = Tensors(T.FeedForwardTrain.SHAPES)
    check(T._fill(FfnParams(), T._FFN_TABLE, t), FfnParams,
          {"ln_weight": "fn.norm.weight", "ln_bias": "fn.norm.bias", "w1": "fn.fn.net.0.weight",
           "b1": "fn.fn.net.0.bias", "w2": "fn.fn.net.3.weight", "b2": "fn.fn.net.3.bias"}, t)


def test_conv_module_struct():
    t = Tensors(T.ConvModuleTrain.SHAPES)
    check(T._fill(ConvModParams(), T._CM_TABLE, t), ConvModParams,
          {"ln_weight": "net.0.weight", "ln_bias": "net.0.bias", "pw1_weight": "net.2.weight",
           "pw1_bias": "net.2.bias", "dw_weight": "net.4.conv.weight", "dw_bias": "net.4.conv.bias",
           "bn_weight": "net.5.weight", "bn_bias": "net.5.bias", "pw2_weight": "net.7.weight",
           "pw2_bias": "net.7.bias"}, t)


def test_attention_struct():
    t = Tensors(T.AttentionTrain.shapes())
    check(T._fill(AttnParams(), T._AT_TABLE, t), AttnParams,
          {"ln_weight": "norm.weight", "ln_bias": "norm.bias", "to_q_weight": "fn.to_q.weight",
           "to_kv_weight": "fn.to_kv.weight", "to_out_weight": "fn.to_out.weight", "to_out_bias": "fn.to_out.bias",
           "rel_pos_emb": "fn.rel_pos_emb.weight"}, t)


@pytest.mark.parametrize("prefix", ["", "dilated_dense.", "dense_block."])
def test_dense_block_struct(prefix):
    t = Tensors(prefix + k for k in T.DenseBlockTrain.SHAPES)
    s = T._dense_struct(t, prefix) if prefix else T._dense_struct(t)
    check(s, DenseParams, dense_expected(key_prefix=prefix), t)


def test_encoder_struct():
    t = Tensors(T.DenseEncoderTrain.SHAPES)
    exp = dense_expected("dense.", "dilated_dense.")
    for i, pre in ((1, "conv_1"), (2, "conv_2")):
        exp[f"conv{i}_weight"] = pre + ".0.weight"
        exp[f"conv{i}_bias"] = pre + ".0.bias"
        exp[f"norm{i}_weight"] = pre + ".1.weight"
        exp[f"norm{i}_bias"] = pre + ".1.bias"
        exp[f"prelu{i}_weight"] = pre + ".2.weight"
    check(T._encoder_struct(t), EncoderParams, exp, t)


def test_mask_decoder_struct():
    t = Tensors(T.DecoderTrain.shapes("mask", 201))
    exp = dense_expected("dense.", "dense_block.")
    exp.update({"sub_pixel_weight": "sub_pixel.conv.weight", "sub_pixel_bias": "sub_pixel.conv.bias",
                "conv_weight": "conv_1.weight", "conv_bias": "conv_1.bias", "norm_weight": "norm.weight",
                "norm_bias": "norm.bias", "prelu_weight": "prelu.weight", "final_weight": "final_conv.weight",
                "final_bias": "final_conv.bias", "prelu_out_weight": "prelu_out.weight"})
    check(T._decoder_struct(t, "mask"), DecoderParams, exp, t)


def test_complex_decoder_struct_leaves_the_mask_head_null():
    t = Tensors(T.DecoderTrain.shapes("complex", 201))
    exp = dense_expected("dense.", "dense_block.")
    exp.update({"sub_pixel_weight": "sub_pixel.conv.weight", "sub_pixel_bias": "sub_pixel.conv.bias",
                "conv_weight": "conv.weight", "conv_bias": "conv.bias", "norm_weight": "norm.weight",
                "norm_bias": "norm.bias", "prelu_weight": "prelu.weight"})
    s = T._decoder_struct(t, "complex")
    check(s, DecoderParams, exp, t)
    assert s.final_weight is None and s.final_bias is None and s.prelu_out_weight is None


def disc_expected(with_buffers):
    exp = {}
    for i in range(4):
        exp[f"conv_weight_orig[{i}]"] = f"layers.{3 * i}.weight_orig"
        exp[f"norm_weight[{i}]"] = f"layers.{3 * i + 1}.weight"
        exp[f"norm_bias[{i}]"] = f"layers.{3 * i + 1}.bias"
        exp[f"prelu_weight[{i}]"] = f"layers.{3 * i + 2}.weight"
        if with_buffers:
            exp[f"conv_u[{i}]"] = f"layers.{3 * i}.weight_u"
            exp[f"conv_v[{i}]"] = f"layers.{3 * i}.weight_v"
    exp.update({"fc1_weight_orig": "layers.14.weight_orig", "fc1_bias": "layers.14.bias",
                "prelu5_weight": "layers.16.weight", "fc2_weight_orig": "layers.17.weight_orig",
                "fc2_bias": "layers.17.bias", "slope": "layers.18.slope"})
    if with_buffers:
        exp.update({"fc1_u": "layers.14.weight_u", "fc1_v": "layers.14.weight_v", "fc2_u": "layers.17.weight_u",
                    "fc2_v": "layers.17.weight_v"})
    return exp


def test_discriminator_struct_with_buffers():
    t = Tensors(T.DiscriminatorTrain.shapes())
    buffers = Tensors(f"{p}.{s}" for p in ("layers.0", "layers.3", "layers.6", "layers.9", "layers.14", "layers.17")
                      for s in ("weight_u", "weight_v"))
    check(T._disc_struct(t, buffers), DiscParams, disc_expected(True), t, buffers)


def test_discriminator_gradient_struct_leaves_u_and_v_null():
    t = Tensors(T.DiscriminatorTrain.shapes())
    s = T._disc_struct(t)
    check(s, DiscParams, disc_expected(False), t)
    assert all(v is None for a in (s.conv_u, s.conv_v) for v in a)
    assert s.fc1_u is None and s.fc1_v is None and s.fc2_u is None and s.fc2_v is None
