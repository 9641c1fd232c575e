"""The running-statistics streaming contract on the CPU model (tests/stream_running_model.py), its published costs
(tests/golden/stream_running_cost.json) and the argument errors of its C ABI that need no GPU.  CPU only."""
import ctypes
import json
import os
import sys

import pytest
import torch

from conftest import GOLDEN, rel_err
from oracle import cmgan_oracle as O
from oracle import stream_oracle as S
from oracle.weights import make_state_dict, synthetic_clips

import stream_running_model as R

sys.path.insert(0, GOLDEN)
import make_stream_running_cost as MC  # noqa: E402


@pytest.fixture(scope="module")
def sd():
    return make_state_dict(seed=0, num_features=201)


@pytest.fixture(scope="module")
def spec():
    wav = synthetic_clips(1, 6000, seed=31)                  # T = 61 frames
    return O.stft_compress(wav * O.rms_scale(wav)[:, None])


def test_one_step_covering_the_clip_is_the_reference_forward(sd, spec):
    """window >= T: one step on fresh sums = the reference arithmetic on the whole clip."""
    sums = {}
    got = R.stream_forward(sd, spec, window=64, context=8, lookahead=8, sums=sums)
    want = O.tscnet_forward(sd, spec)
    assert rel_err(got[0], want[0]) < 1e-6 and rel_err(got[1], want[1]) < 1e-6
    assert len(sums) == 16                                   # encoder 2 + 4, each decoder 4 + 1
    assert all(n == 61 * (101 if "dense_encoder.conv_2" in k or "_decoder.dense" in k else 201)
               for k, (n, _, _) in sums.items() if "sub_pixel" not in k and k != "complex_decoder.norm")
    assert sums["complex_decoder.norm"][0] == 61 * 202       # the pixel-shuffled width 2 F'
    assert sums["mask_decoder.norm"][0] == 61 * 201 and sums["mask_decoder.norm"][1].shape == (1, 1)


def test_running_and_frozen_agree_on_the_first_step_calibrated_on_its_frames(sd, spec):
    """Step 0 of a running stream sees frames [0, W + La) and nothing before: its encoder output is the frozen
    encoder's under statistics calibrated on exactly those frames (fp64 sums vs torch's fp32 mean / var)."""
    e1 = 24
    part = spec[:, :, :e1]
    frozen = S.encoder_frozen(sd, part, S.calibrate(sd, part))
    running = R.encoder_step(sd, part, 0, {})
    assert rel_err(running, frozen) < 2e-6
    # and the running statistics are NOT the first window's afterwards: step 1 counts its new frames only
    sums = {}
    R.encoder_step(sd, part, 0, sums)
    n0 = sums["dense_encoder.conv_1.1"][0]
    R.encoder_step(sd, spec[:, :, e1 - S.HIST:e1 + 10], S.HIST, sums)
    assert sums["dense_encoder.conv_1.1"][0] == n0 + 10 * 201


def test_short_windows_with_carried_sums_stay_close_to_the_whole_clip(sd, spec):
    want = O.tscnet_forward(sd, spec)
    got = R.stream_forward(sd, spec, window=16, context=8, lookahead=4)           # 4 steps
    assert 1e-4 < rel_err(got[0], want[0]) < 0.5
    assert torch.isfinite(got[0]).all() and got[0].shape == want[0].shape
    # the model leaves the oracle as it found it
    assert O._instance_norm.__module__ == O.__name__ and S._encoder.__module__ == S.__name__


def test_published_running_costs_are_recomputed_by_the_model():
    """tests/golden/stream_running_cost.json (tests/golden/make_stream_running_cost.py) against the model, on the
    recordings where the frozen blob does worst; and the go / no-go entry: running beats frozen on track_silence
    with 100-frame windows and no look-ahead."""
    costs = json.load(open(os.path.join(GOLDEN, "stream_running_cost.json")))
    frozen = json.load(open(os.path.join(GOLDEN, "stream_cost_oracle.json")))
    assert set(costs) == set(frozen)
    sd = make_state_dict(seed=0)
    for name, pcm in MC.tracks():
        if name == "b":
            continue
        whole = O.enhance_batch(sd, pcm)[0]
        for la in ((0, 40) if name == "silence" else (0,)):
            key = f"track_{name}_w100_c40_l{la}"
            got = MC.cost(R.enhance_stream(sd, pcm, window=100, context=40, lookahead=la)[0], whole)
            want = costs[key]
            assert abs(got["rel_max"] - want["rel_max"]) < 1e-4, key
            assert abs(got["rel_rms"] - want["rel_rms"]) < 1e-4, key
            assert abs(got["ssnr"] - want["ssnr"]) < 0.02, key
            assert abs(got["stoi"] - want["stoi"]) < 1e-5, key
    gate = "track_silence_w100_c40_l0"
    assert costs[gate]["rel_max"] < frozen[gate]["rel_max"] and costs[gate]["ssnr"] > frozen[gate]["ssnr"]
    for name in ("a", "b", "silence"):                       # one window covers a recording: no cost
        assert costs[f"track_{name}_w400_c40_l40"]["rel_max"] < 2e-6


def test_running_abi_argument_errors_without_gpu():
    from cmgan_amd import _lib
    lib = _lib.load()
    BADARG = -1
    assert lib.cmgan_stream_encoder_running(None, None, 1, 8, 0, None, None, None, None, 0, None) == BADARG
    assert lib.cmgan_stream_decoder_running(None, None, None, 1, 8, 0, None, None, None, None, None, 0, None) == BADARG
    assert lib.cmgan_stream_sums_doubles(None, 1) == 0
    # the size needs no device state, only a non-null handle (never dereferenced here) and B > 0
    fake = ctypes.create_string_buffer(64)
    h = ctypes.cast(fake, ctypes.c_void_p)
    assert lib.cmgan_stream_sums_doubles(h, 0) == 0
    assert lib.cmgan_stream_sums_doubles(h, -3) == 0
    assert lib.cmgan_stream_sums_doubles(h, 2) == (15 * 64 + 1) * 3 * 2
