"""CPU checks of tests/disc_model.py, the float64 reference tests/test_gpu_disc.py holds csrc/disc.hip to: the reference
reproduces the reference module's own output (tests/golden/disc_train.npz), every GPU case reaches the branch of
disc.hip it is named for (by the plan mirrors), and the seeded inputs sit away from the two places where the network
is not differentiable - a tie of the max pool, a PReLU input at zero - by more than fp32 noise."""
import os
import re

import pytest
import torch

import disc_model as M
from conftest import ROOT, load_golden

BY_ID = {M.case_id(c): c for c in M.CASES}
CHUNKED = ("chunked_B9_T177-default", "chunked_B9_T177-spread")


def test_float64_reference_reproduces_the_reference_modules_fp32_golden():
    """disc_train.npz is Discriminator(ndf=16) itself in fp32 (tests/golden/make_golden.py, section 20).  Bar per
    quantity: 8 x the error of this file's own graph in fp32 against float64 at the same shape, at least 2e-6."""
    from cmgan_amd.synth import discriminator_state_dict
    g = load_golden("disc_train.npz")
    xy = torch.stack([g["x"][:, 0].permute(0, 2, 1), g["y"][:, 0].permute(0, 2, 1)], dim=-1).contiguous()
    args = (discriminator_state_dict(0), xy, g["mask"], g["dscore"][:, 0])
    want = M.reference(*args)
    golden = {"score": g["score"][:, 0], "score_eval": g["score_eval"][:, 0],
              "dxy": torch.stack([g["dx"][:, 0].permute(0, 2, 1), g["dy"][:, 0].permute(0, 2, 1)], dim=-1),
              "buffers": {k: g["new_" + k.replace(".", "_")] for k in want["buffers"]},
              "grads": {k: g["grad_" + k.replace(".", "_")] for k in want["grads"]}}
    assert len(golden["buffers"]) == 12 and len(golden["grads"]) == 22
    floor = M.errors(M.reference(*args, dtype=torch.float32), want)
    err = M.errors(golden, want)
    assert set(err) == set(floor) and len(err) == 5 + 12 + 22
    for k, e in err.items():
        print(f"[golden] {k}: rel_err = {e:.3e} (fp32 floor {floor[k]:.1e})")
        assert e < M.bar(floor[k]), (k, e, floor[k])


def test_plan_mirrors_name_the_constants_of_the_kernel_file():
    """The mirrors restate host arithmetic; this pins the constants they share with csrc/disc.hip by its text."""
    src = open(os.path.join(ROOT, "cmgan_amd", "csrc", "disc.hip")).read()
    assert int(re.search(r"#define DC_SPLIT (\d+)", src).group(1)) == M.DC_SPLIT
    assert int(re.search(r"#define DW_TP (\d+)", src).group(1)) == M.DW_TP
    assert "int ns = 1024 / groups;" in src and "const long cap = ((long)DC_SPLIT * 16 * 64 * 128) / nw;" in src
    assert "G = 1024 / C;" in src
    assert src.count("(total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096") == 2
    assert "bool disc_shape_ok(int T, int F) { return T >= 16 && F >= 16; }" in src
    assert M.shape_ok(16, 201) and not M.shape_ok(15, 201) and not M.shape_ok(16, 15)


def test_the_golden_shape_never_leaves_the_one_tile_per_chunk_path():
    """What the existing fixtures (B = 2, T = 33, F = 201) reach: one tile per chunk, one finalize step, one grid
    pass - the reason for the cases below."""
    for L in M.wgrad_plan(2, 33, 201):
        assert L["ns"] == L["tiles_total"] and L["tpc"] == 1 and L["empty_chunks"] == 0 and not L["cap_binds"]
    for L in M.norm_plan(2, 33, 201):
        assert L["finalize_steps"] == 1 and L["stride_iters"] == 1
    assert [d[0] for d in M.layer_dims(33, 201)] == [33, 16, 8, 4]


@pytest.mark.parametrize("cid", CHUNKED)
def test_chunked_case_reaches_the_multi_tile_loop_the_cap_and_the_empty_chunks(cid):
    _, B, T, F_, _, _ = BY_ID[cid]
    plan = M.wgrad_plan(B, T, F_)
    assert [L["tiles_total"] for L in plan] == [2475, 619, 155, 38]
    assert [L["ns"] for L in plan] == [1024, 512, 128, 32]
    assert [L["tpc"] for L in plan] == [3, 2, 2, 2]
    assert all(L["tpc"] >= 2 for L in plan)
    assert plan[0]["empty_chunks"] == 1024 - 825 and any(L["empty_chunks"] > 0 for L in plan)
    assert [L["cap_binds"] for L in plan] == [False, True, True, True]
    assert all(L["ns"] * L["nw"] <= M.DC_SPLIT * 16 * 64 * 128 for L in plan)      # the slabs fit the workspace
    norm = M.norm_plan(B, T, F_)
    assert B > norm[3]["G"] == 8 and norm[3]["finalize_steps"] == 2
    assert norm[0]["total"] == 1267200 > 4096 * 256 and norm[0]["stride_iters"] == 2 and norm[0]["grid"] == 4096


def test_large_batch_case_steps_the_finalize_loop_on_every_layer():
    _, B, T, F_, _, _ = BY_ID["batch65_T16-spread"]
    norm = M.norm_plan(B, T, F_)
    assert [L["G"] for L in norm] == [64, 32, 16, 8]
    assert all(B > L["G"] and L["finalize_steps"] >= 2 for L in norm)
    assert norm[0]["finalize_steps"] == 2 and norm[3]["finalize_steps"] == 9


def test_small_cases_reach_the_time_chains_and_parity_classes_they_name():
    assert [(d[0], d[3]) for d in M.layer_dims(16, 201)] == [(16, 8), (8, 4), (4, 2), (2, 1)]       # 1-row plane
    assert not M.shape_ok(15, 201)                                                                # 16 is the smallest
    assert [d[0] for d in M.layer_dims(31, 201)] + [M.layer_dims(31, 201)[3][3]] == [31, 15, 7, 3, 1]
    for cls in M.dgrad_classes(3, 31, 201)[:3]:          # odd Ti, odd Fi (201, 25) or even (100, 50): rt = 1 is smaller
        assert cls[2] < cls[0] and cls[3] < cls[1]
    assert len(set(M.dgrad_classes(3, 31, 201)[0])) == 4                                          # all four differ
    assert [d[0] for d in M.layer_dims(46, 201)] + [M.layer_dims(46, 201)[3][3]] == [46, 23, 11, 5, 2]
    assert [d[1] for d in M.layer_dims(33, 601)] + [M.layer_dims(33, 601)[3][4]] == [601, 300, 150, 75, 37]
    plan = M.wgrad_plan(4, 321, 201)
    assert plan[0]["tiles_total"] == 2000 and plan[0]["ns"] == 1024 and plan[0]["tpc"] == 2


def test_every_case_of_the_issue_is_present_once_per_weight_set_it_names():
    shapes = {c[1:4] for c in M.CASES}
    assert shapes == {(2, 16, 201), (3, 31, 201), (1, 46, 201), (9, 177, 201), (65, 16, 201), (4, 321, 201), (2, 33, 601)}
    assert {c[1:4] for c in M.CASES if c[4] == "spread"} == shapes          # every shape runs the spread weights
    assert len({M.case_id(c) for c in M.CASES}) == len(M.CASES)
    st = M.states()
    for i in (2, 5, 8, 11, 16):                                             # PReLU slopes far from 0.25, both signs
        w = st["spread"][f"layers.{i}.weight"]
        assert float(w.min()) < 0.0 and float(w.max()) > 0.6
    for i in (1, 4, 7, 10):                                                 # gains far from 1, both signs
        w = st["spread"][f"layers.{i}.weight"]
        assert float(w.min()) < -0.4 and float(w.max()) > 1.4 and float(w.abs().min()) >= 0.4


POOL_MARGIN = 1e-4       # of the plane's max: fp32 noise (1e-6) cannot flip the argmax
KINK_RATIO = 2.0         # nearest PReLU input to zero / largest fp32 error seen among the inputs within 1e-3 of zero


@pytest.mark.parametrize("cid", sorted(BY_ID))
def test_inputs_of_every_gpu_case_sit_off_the_pool_ties_and_prelu_kinks(cid):
    """Asserted on the reference alone.  An argmax that flips, or one PReLU input that lands on the other side of
    zero, changes dL/dxy by 1e-4 .. 1e-3 of its max in ANY fp32 evaluation (measured with this file's fp32 graph: 7e-4
    for one flipped layer-2 input at B = 9 x T = 177) - the seeds of disc_model.CASES were searched for inputs where
    neither can happen, and this holds them to it."""
    case = BY_ID[cid]
    want = M.case_reference(case)
    pm = M.pool_margin(want["taps"]["a4"])
    ratios = M.kink_ratios(want["taps"], M.case_taps32(case))
    print(f"[inputs] {cid}: pool margin {pm:.2e}, kink ratios " + " ".join(f"{r:.1f}" for r in ratios))
    assert pm > POOL_MARGIN
    assert min(ratios) > KINK_RATIO, ratios
    xy, mask, dscore = M.inputs(case)
    assert 0.5 < float(xy.mean()) < 1.1 and float(xy.min()) >= 0.0          # |randn|: O(1) magnitudes
    assert set(mask.unique().tolist()) == {0.0, float(torch.tensor(1.0) / torch.tensor(0.7))}


def test_zero_row_case_has_a_silent_clip_and_a_finite_reference():
    xy, _, _ = M.inputs(M.ZERO_ROW)
    assert float(xy[1].abs().max()) == 0.0 and float(xy[0].min()) >= 0.0 and float(xy[2].max()) > 1.0
    want = M.case_reference(M.ZERO_ROW)
    assert bool(torch.isfinite(want["score"]).all()) and bool(torch.isfinite(want["dxy"]).all())
