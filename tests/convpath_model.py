"""Float64 reference of the inference conv path (cmgan_amd/csrc/conv.hip, conv_x3.hip, in_running.hip) for
tests/test_gpu_convpath.py, plus the host mirrors of the tilings those kernels use.  TEST INFRASTRUCTURE ONLY.

The reference is the project's own oracle (oracle/cmgan_oracle.py: dense_encoder, mask_decoder, complex_decoder,
norm_stats) run on a float64 copy of the state dict; nothing here restates a kernel.  What this file adds:

* `encoder` / `decoders`: the two halves around the TSCBs in float64, with the InstanceNorm statistics they used
  (`norm_stats("record")`) or were given (`"replay"`);
* `pairs`: the (scale, shift) a norm's consumer applies, gamma / sqrt(var + eps) and beta - mean * scale, in float64;
* `build_blob` / `parse_blob`: the statistics blob of include/cmgan_hip.h ("Streaming") from / to those pairs;
* `conv3_ntiles`, `conv3x_ntiles`, `conv3x_walkable`, `dense_ntiles`: how many tiles a conv of a plane has and which
  kernel the library picks for it - mirrors of the host code, pinned to its text by tests/test_conv_x3_tile_model.py;
* `offset_state_dict`: the state dict with conv biases raised until every pre-norm channel sits 8 .. 16 standard
  deviations from zero.

Statistics blob (cmgan_stats_floats(B) floats; tscnet_impl in api.hip writes it in this order):

    norm j = 0 .. 15 at float offset j * 2 * B * 64:  scale [B][64], then shift [B][64]
        0        dense_encoder.conv_1.1                       (input of the encoder's dense block)
        1 .. 4   dense_encoder.dilated_dense.norm1 .. norm4
        5        dense_encoder.conv_2.1                       (the encoder's output norm, plane F')
        6 .. 9   mask_decoder.dense_block.norm1 .. norm4
        10 .. 13 complex_decoder.dense_block.norm1 .. norm4
        14       complex_decoder.norm                         (over the pixel-shuffled [B, 64, T, 2F'] tensor)
        15       unused
    then [B][2] = {mean, 1 / sqrt(var + eps)} of mask_decoder.norm's one channel (final_combine_kernel's layout)
"""
from __future__ import annotations

import torch

from oracle import cmgan_oracle as O

EPS = O.EPS

# ---- tilings (conv.hip, conv_x3.hip; pinned by tests/test_conv_x3_tile_model.py) ---------------------------------
CONV_TILE = 128                                    # conv3_kernel: outputs per tile
CX_NPB64, CX_NWV64 = 2, 8                          # conv3x_kernel, 64 output channels: position blocks per wave, waves
CX_NPB128, CX_NWV128 = 2, 4                        # 128 output channels (the sub-pixel conv)
EPI_STEP = 16                                      # CX_EPILOGUE: positions between a wave's position blocks
INF_NP, INF_LOADS = 16, 8                          # in_finalize_kernel: partial sums per channel, loads in flight


def x3_rows(cout: int) -> int:
    """staged rows = MFMA positions of a conv3x_kernel tile"""
    return 16 * (CX_NPB128 * CX_NWV128 if cout == 128 else CX_NPB64 * CX_NWV64)


def x3_rstep(cout: int) -> int:
    """rows between two staging loads of one thread (8 threads per row)"""
    return 8 * (CX_NWV128 if cout == 128 else CX_NWV64)


def x3_npb(cout: int) -> int:
    return CX_NPB128 if cout == 128 else CX_NPB64


def conv3_ntiles(T: int, F: int) -> int:
    return (T * (F + 1) + CONV_TILE - 1) // CONV_TILE


def conv3x_ntiles(T: int, F: int, cout: int) -> int:
    tile = x3_rows(cout) - 2
    return (T * (F + 1) + tile - 1) // tile


def conv3x_walkable(F: int, cout: int) -> bool:
    """conv_x3.hip's predicate of the same name: the plane is wide enough for the kernel's row walk"""
    return F + 1 >= max(x3_rstep(cout), EPI_STEP)


def dense_ntiles(mode: str, T: int, F: int, cout: int = 64) -> tuple:
    """(kernel, tiles per clip) of a conv of plane width F in matrix mode `mode`, as tscnet_impl chooses"""
    if mode != "f32" and conv3x_walkable(F, cout):
        return "x3", conv3x_ntiles(T, F, cout)
    return "f32", conv3_ntiles(T, F)


# ---- norms -----------------------------------------------------------------------------------------------------------
def _block(p):
    return [f"{p}.norm{i}" for i in range(1, 5)]


ENC_KEYS = ["dense_encoder.conv_1.1"] + _block("dense_encoder.dilated_dense") + ["dense_encoder.conv_2.1"]
DEC_KEYS = _block("mask_decoder.dense_block") + _block("complex_decoder.dense_block") + ["complex_decoder.norm"]
NORM_KEYS = ENC_KEYS + DEC_KEYS                    # blob slots 0 .. 14
MASK_KEY = "mask_decoder.norm"
N_SLOTS = 16

# the conv whose bias moves the mean of a norm's input
BIAS_OF = {"dense_encoder.conv_1.1": "dense_encoder.conv_1.0.bias", "dense_encoder.conv_2.1": "dense_encoder.conv_2.0.bias",
           "complex_decoder.norm": "complex_decoder.sub_pixel.conv.bias", MASK_KEY: "mask_decoder.conv_1.bias"}
for _p in ("dense_encoder.dilated_dense", "mask_decoder.dense_block", "complex_decoder.dense_block"):
    for _i in range(1, 5):
        BIAS_OF[f"{_p}.norm{_i}"] = f"{_p}.conv{_i}.bias"


def stats_floats(B: int) -> int:
    return N_SLOTS * 2 * B * 64 + 2 * B


def to64(sd: dict) -> dict:
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def _model_in(spec):
    re, im = spec[:, 0:1], spec[:, 1:2]
    return torch.cat([torch.sqrt(re * re + im * im), spec], dim=1)


@torch.no_grad()
def encoder(sd, spec, replay: dict | None = None):
    """spec [B,2,T,F] -> (dense_encoder output [B,64,T,F'], the statistics used {key: (mean, var) [B,C,1,1]})."""
    st = {} if replay is None else replay
    with O.norm_stats("record" if replay is None else "replay", st):
        y = O.dense_encoder(sd, _model_in(spec))
    return y, st


@torch.no_grad()
def decoders(sd, h, spec, replay: dict | None = None):
    """h [B,64,T,F'], spec [B,2,T,F] -> ({mask, complex, real, imag}, statistics): both decoders and the recombination
    of TSCNet.forward (generator.py:187-194; mask * mag * (cos, sin)(phase) is mask * (re, im))."""
    st = {} if replay is None else replay
    with O.norm_stats("record" if replay is None else "replay", st):
        mask = O.mask_decoder(sd, h)
        cplx = O.complex_decoder(sd, h)
    out = {"mask": mask, "complex": cplx, "real": mask * spec[:, 0:1] + cplx[:, 0:1],
           "imag": mask * spec[:, 1:2] + cplx[:, 1:2]}
    return out, st


def pairs(sd, stats: dict) -> dict:
    """{key: (scale [B,C], shift [B,C])} for the keys of `stats`: what the norm's consumer multiplies and adds."""
    out = {}
    for k, (mean, var) in stats.items():
        mean, var = mean.double().flatten(1), var.double().flatten(1)
        scale = sd[k + ".weight"].double() / torch.sqrt(var + EPS)
        out[k] = (scale, sd[k + ".bias"].double() - mean * scale)
    return out


def build_blob(stats: dict, sd, B: int) -> torch.Tensor:
    """float32 statistics blob from recorded float64 (mean, var); norms missing from `stats` stay zero."""
    blob = torch.zeros(stats_floats(B), dtype=torch.float64)
    ns = blob[:N_SLOTS * 2 * B * 64].view(N_SLOTS, 2, B, 64)
    for k, (scale, shift) in pairs(sd, {k: v for k, v in stats.items() if k != MASK_KEY}).items():
        j = NORM_KEYS.index(k)
        ns[j, 0], ns[j, 1] = scale, shift
    if MASK_KEY in stats:
        mean, var = stats[MASK_KEY]
        m = blob[N_SLOTS * 2 * B * 64:].view(B, 2)
        m[:, 0], m[:, 1] = mean.double().flatten(), 1.0 / torch.sqrt(var.double().flatten() + EPS)
    return blob.float()


def parse_blob(blob: torch.Tensor, sd, B: int, keys=None) -> dict:
    """The inverse: {key: (scale [B,C], shift [B,C])} in float64 for `keys` (default: all 15 norms and the mask head's).
    The mask head's {mean, rstd} becomes the same kind of pair through its one gamma / beta."""
    blob = blob.detach().double().cpu()
    assert blob.numel() == stats_floats(B)
    ns = blob[:N_SLOTS * 2 * B * 64].view(N_SLOTS, 2, B, 64)
    out = {}
    for k in (NORM_KEYS + [MASK_KEY]) if keys is None else keys:
        if k == MASK_KEY:
            m = blob[N_SLOTS * 2 * B * 64:].view(B, 2)
            scale = sd[k + ".weight"].double() * m[:, 1:2]
            out[k] = (scale, sd[k + ".bias"].double() - m[:, 0:1] * scale)
        else:
            j = NORM_KEYS.index(k)
            out[k] = (ns[j, 0].clone(), ns[j, 1].clone())
    return out


# ---- offset statistics -----------------------------------------------------------------------------------------------
OFFSET_RATIO = 12.0                                # aimed |mean| / std, the middle of the asserted 8 .. 16


@torch.no_grad()
def offset_state_dict(sd, spec, h=None):
    """A copy of `sd` (float32) whose conv biases put every norm input about OFFSET_RATIO standard deviations from zero.
    InstanceNorm removes a per-channel constant exactly, so a bias changes no tensor downstream of its norm: the
    statistics of ONE pass with the original biases give every new bias at once, bias_c += ratio * std_c - mean_c
    (clip average).  The sub-pixel conv's norm channel c pools conv channels c and c + 64: both get the same step.
    `h` [B,64,T,F'] (optional): the decoders' input; without it only the encoder's biases move."""
    sd64 = to64(sd)
    _, st = encoder(sd64, spec.double())
    if h is not None:
        st.update(decoders(sd64, h.double(), spec.double())[1])
    out = dict(sd)
    for k, (mean, var) in st.items():
        step = (OFFSET_RATIO * torch.sqrt(var) - mean).mean(dim=0).flatten()
        b = sd[BIAS_OF[k]].double()
        out[BIAS_OF[k]] = (b + (step.repeat(2) if b.numel() == 2 * step.numel() else step)).float()
    return out


def offset_ratios(stats: dict) -> dict:
    """{key: |mean| / std [B,C]} of recorded statistics"""
    return {k: (mean.abs() / torch.sqrt(var)).flatten(1) for k, (mean, var) in stats.items()}
