"""Host side of tests/test_gpu_trainpath.py (runs anywhere): the mirrors of tests/trainpath_model.py pinned to the text of
train.hip / train_x3.hip, the arithmetic every case of the GPU file is named for, the margin condition of the default-slope
seeds, and the check that the bars are reachable - torch's own fp32 autograd through the oracle stays inside them against
the float64 reference at every shape the GPU file uses (so no kink sits in the inputs either)."""
import os
import re

import pytest
import torch

import convpath_model as M
import trainpath_model as TM
from conftest import ROOT
from trainpath_model import Case


def _src(name):
    return open(os.path.join(ROOT, "cmgan_amd", "csrc", name)).read()


def _body(text, start, end):
    """the text from `start` up to the next `end`"""
    i = text.index(start)
    return text[i:text.index(end, i)]


def test_mirrors_name_the_constants_of_the_kernel_files():
    tr, x3 = _src("train.hip"), _src("train_x3.hip")
    for name in ("DB_WG_SPLIT", "RC_WG_SPLIT", "DB_NCH", "MT_NCH", "DB_MAXBLK"):
        assert int(re.search(rf"#define {name} (\d+)", tr).group(1)) == getattr(TM, name), name
    assert TM.GRAD_TOL == 1e-4

    # the dense weight gradient: steps, splits and the walk of one lane
    wg = _body(x3, "void db_conv_wgrad_x3_kernel(", "void launch_db_conv_wgrad_x3(")
    assert f"const unsigned steps = (M + {TM.WG_STEP - 1}) / {TM.WG_STEP}, per = (steps + nsplit - 1) / nsplit;" in wg
    assert "const unsigned st0 = s * per, st1 = st0 + per < steps ? st0 + per : steps;" in wg
    assert f"unsigned m0 = (st0 + wv) * {TM.WG_STEP} + 8 * g;" in wg
    assert f"for (unsigned st = st0 + wv; st < st1; st += {TM.WG_WAVES})" in wg
    assert "__global__ __launch_bounds__(256) void db_conv_wgrad_x3_kernel(" in x3         # four waves
    adv = TM.WG_STEP * TM.WG_WAVES
    assert f"const int adv_t = {adv} / F, adv_f = {adv} - adv_t * F;" in wg and f"m0 += {adv}u;" in wg
    assert "if (f >= F) { f -= F; ++t; }" in wg and "while (t >= T) { t -= T; ++bb; }" in wg
    assert "const bool interior = m0 + 7u < M && f + df >= 0 && f + 7 + df < F && f + 7 < F && ts0 >= 0 && ts0 < T;" in wg
    assert "launch_db_conv_wgrad_x3(ctx, g, aslot(s), B, T, F, dil, DB_WG_SPLIT, ws + pl.wpart" in tr
    assert "if ((long)M * 256 < (1L << 32)) {" in tr                      # every plane below 4 GB takes that kernel
    rw = _body(x3, "void rc_wgrad_x3_kernel(", "Row-conv data gradient")
    assert f"const unsigned steps = (Mo + {TM.WG_STEP - 1}) / {TM.WG_STEP}, per = (steps + nsplit - 1) / nsplit;" in rw
    assert "launch_rc_wgrad_x3(ctx, NG, dz, in, gm, RC_WG_SPLIT, wpart" in tr

    # the persistent row-conv data gradient
    rd = _body(x3, "void rc_dgrad_x3_kernel(", "void launch_rc_wgrad_x3(")
    assert f"const unsigned m = (unsigned)tile * {TM.RCD_POS}u + (unsigned)c;" in rd
    assert f"for (int tile = blockIdx.x * {TM.RCD_TILES} + wv; tile < ntiles; tile += gridDim.x * {TM.RCD_TILES})" in rd
    assert f"const int ntiles = (int)((Mi + {TM.RCD_POS - 1}) / {TM.RCD_POS});" in rd
    assert (f"const int want = (ntiles + {TM.RCD_TILES - 1}) / {TM.RCD_TILES}, cap = ng == 1 ? {TM.RCD_CAP[1]} : "
            f"{TM.RCD_CAP[2]};") in rd
    assert "const int grid = want < cap ? (want > 0 ? want : 1) : cap;" in rd
    assert "__global__ __launch_bounds__(512) void rc_dgrad_x3_kernel(" in x3              # eight waves
    assert "if (!rc_dgrad_x3(ctx, 1, dz2, p.c2_w, g2, ws + pl.d))" in tr and "if (!rc_dgrad_x3(ctx, 2, g, p.sp_w, gs, ws + pl.d))" in tr

    # which kernel a width takes, the tile partials and their finalize pass, the data gradient's scratch
    assert "static bool db_x3_forward(int F) { return conv3x_walkable(F, 64); }" in tr
    assert "return k_on && gm.KW == 3 && gm.PL == 1 && conv3x_walkable(gm.Fi, 64) &&" in tr
    assert "const bool x3d = db_x3_forward(F);" in tr
    fin = _body(tr, "void db_stats_finalize_tiles_kernel(", "// a = PReLU(InstanceNorm(z))")
    assert f"for (int t = k; t < ntiles; t += {TM.FINALIZE_THREADS})" in fin
    assert (f"db_stats_finalize_tiles_kernel<<<B * 64, {TM.FINALIZE_THREADS}, 0, st>>>(\n"
            "                                               ws + pl.part, conv3x_ntiles(T, F, 64), (double)P, mean, rstd)") in tr
    assert "const size_t chunks = (size_t)B * DB_NCH * 64 * 3, tiles = (size_t)B * conv3x_ntiles(T, F, 64) * 128;" in tr
    assert "p.part = take(chunks > tiles ? chunks : tiles);" in tr
    assert "const float* slots = sc + 256 + 2 * B * 64;" in tr
    assert "for (int k = threadIdx.x; k < DB_MAXBLK; k += 256) m = fmaxf(m, slots[k]);" in tr
    assert "db_in_bwd_kernel<<<DB_MAXBLK, 256, 0, st>>>" in tr


def test_plane_width_cases_take_the_kernels_they_are_named_for():
    assert all((c.B, c.T) == (2, 11) for c in TM.WIDTHS)
    for c in TM.WIDTHS:
        assert TM.dense_kernel(c.F) == TM.WIDTH_KERNELS[c.module][c.F], c
    assert sorted(c.F for c in TM.WIDTHS if c.module == "dense") == [5, 9, 62, 63, 64, 101, 201]
    assert {c.F: TM.out_plane(c) for c in TM.WIDTHS if c.module == "encoder"} == TM.ENCODER_OUT \
        == {61: 31, 63: 32, 64: 32, 125: 63, 127: 64, 201: 101}
    for k in TM.DECODERS:
        assert sorted(c.F for c in TM.WIDTHS if c.module == k) == [31, 62, 63, 64, 101]
    # 62 the widest fallback plane, 63 the narrowest walkable one: its row (with the virtual zero column) is the staging step
    assert not M.conv3x_walkable(62, 64) and M.conv3x_walkable(63, 64) and 63 + 1 == M.x3_rstep(64)
    assert TM.dense_kernel(TM.out_plane(Case("encoder", 2, 11, 125))) == "x3" and TM.dense_kernel(TM.out_plane(Case("encoder", 2, 11, 123))) == "f32"
    # an even input width: the stride-2 conv reads no right padding (its last tap 2 (F' - 1) - 1 + 2 is the last column), and
    # in the data gradient the last column's tap 0 points at output fo = (F - 1 + 1 - 0) / 2 = F', one past the edge
    Fo = TM.out_plane(Case("encoder", 2, 11, 64))
    assert 2 * (Fo - 1) - 1 + 2 == 64 - 1 and (64 - 1 + 1 - 0) % 2 == 0 and (64 - 1 + 1 - 0) // 2 == Fo
    assert 2 * (TM.out_plane(Case("encoder", 2, 11, 63)) - 1) - 1 + 2 == 63          # an odd width does read it
    # the mask head's per-bin slopes are cut to the output width
    assert TM.module_state(Case("mask", 2, 11, 31))["mask_decoder.prelu_out.weight"].numel() == 61
    # the data gradient's scratch fits the partial-sum area it is carved from, at every shape
    for c in TM.all_cases():
        assert TM.dgrad_scratch_floats(c.B) <= TM.partial_area_floats(c.B, c.T, c.F), c


def test_time_edge_cases_sit_on_the_dilations():
    dils = (1, 2, 4, 8)
    assert set(TM.TIME_TS) == {1, 2, 3, 8, 9, 17}
    for T in TM.TIME_TS:
        assert T in dils or T - 1 in dils or T == 2 * 8 + 1       # T <= dil for some layer, or one row past a dilation
    assert {(c.module, c.F) for c in TM.TIME_EDGES} == {("dense", 63), ("dense", 101), ("encoder", 125), ("mask", 63), ("complex", 63)}
    assert all(c.B == 3 and TM.dense_kernel(c.F) == "x3" for c in TM.TIME_EDGES)
    assert sorted(c.T for c in TM.TIME_EDGES if c.module == "encoder") == [1, 2, 9]


def test_grid_and_finalize_cases_have_the_tile_counts_they_are_named_for():
    assert sorted(c.B * TM.dense_tiles(c.T, c.F) for c in TM.GRID_CASES) == [1, 3, 7, 8, 9, 17]
    for c in TM.GRID_CASES:
        assert c.F == 129 and c.B * TM.dense_tiles(c.T, c.F) == TM.GRIDS[(c.B, c.T)]
    assert {c.T: TM.dense_tiles(c.T, c.F) for c in TM.FINALIZE_CASES} == TM.FINALIZE == {1: 1, 321: 256, 322: 257}
    assert [TM.finalize_passes(n) for n in (1, 256, 257)] == [1, 1, 2]
    assert all(c.B == 1 and c.F == 201 for c in TM.FINALIZE_CASES)
    # the whole-step tests' B = 1 x T = 321 plane stops at exactly one pass
    assert TM.finalize_passes(TM.dense_tiles(321, 201)) == 1 and TM.dense_tiles(321, 201) == TM.FINALIZE_THREADS


def test_weight_gradient_cases_hit_the_walks_and_splits_they_are_named_for():
    by = {(c.B, c.T, c.F): c for c in TM.WGRAD_CASES}
    assert set(by) == {(1, 1, 5), (9, 1, 9), (5, 1, 63), (2, 64, 64), (2, 41, 100)}

    def split(B, T, F):
        return TM.wgrad_splits(B * T * F)

    # (1,1,5): one ragged step, F < 8 (a lane's eight positions never lie in one row: never interior)
    steps, per, counts = split(1, 1, 5)
    assert (steps, per) == (1, 1) and counts[0] == 1 and sum(counts) == 1 and 5 < TM.WG_STEP and 5 < 8
    # (9,1,9): T F = 9, one advance of 128 positions crosses fourteen clips
    assert TM.wgrad_clips_per_advance(1, 9) == 14 and split(9, 1, 9)[0] == 3
    # (5,1,63): two clips per advance, on a wide plane
    assert TM.wgrad_clips_per_advance(1, 63) == 2 and TM.dense_kernel(63) == "x3" and split(5, 1, 63)[0] == 10
    # (2,64,64): exactly one full step in each of the 256 splits
    steps, per, counts = split(2, 64, 64)
    assert 2 * 64 * 64 == 8192 and (steps, per) == (256, 1) and counts == [1] * 256 and 8192 % TM.WG_STEP == 0
    # (2,41,100): 257 steps, two per split, split 128 holds one ragged step, 129 .. 255 are empty
    steps, per, counts = split(2, 41, 100)
    assert 2 * 41 * 100 == 8200 and (steps, per) == (257, 2)
    assert counts[:128] == [2] * 128 and counts[128] == 1 and counts[129:] == [0] * 127 and 8200 - 256 * TM.WG_STEP == 8


def test_persistent_cases_need_a_second_trip():
    want = {"encoder": (1, 2 * 245 * 201, 98490, 6156), "mask": (2, 2 * 165 * 101, 33330, 2084), "complex": (2, 2 * 165 * 101, 33330, 2084)}
    for c in TM.PERSISTENT_CASES:
        ng, pos, pos_, tiles_ = want[c.module]
        assert pos == pos_ == c.B * c.T * c.F                      # input positions of conv_2 / the sub-pixel conv
        tiles, grid, trips = TM.rc_dgrad_geometry(pos, ng)
        assert tiles == tiles_ and tiles > TM.RCD_TILES * TM.RCD_CAP[ng] and grid == TM.RCD_CAP[ng] and trips == 2
    # what the whole-step tests reach at B = 1 x T = 321: one trip
    assert TM.rc_dgrad_geometry(321 * 201, 1)[2] == 1 and TM.rc_dgrad_geometry(321 * 101, 2)[2] == 1
    assert 321 * 201 == 64521 and 321 * 101 == 32421


def test_magnitude_workspace_and_default_cases_are_wide_planes():
    for c in TM.MAGNITUDE_CASES + TM.WORKSPACE_CASES + TM.DEFAULT_CASES + [TM.OFFSET_CASE]:
        assert TM.dense_kernel(c.F) == "x3" and TM.dense_kernel(TM.out_plane(c)) == "x3", c
    assert {(c.module, TM.out_plane(c)) for c in TM.MAGNITUDE_CASES} == {(m, F) for m in TM.MODULES for F in (63, 101)}
    assert all((c.B, c.T, TM.out_plane(c), c.slopes) == (1, 3, 63, "default") for c in TM.DEFAULT_CASES)
    assert [c.module for c in TM.DEFAULT_CASES] == list(TM.MODULES)
    assert all((c.B, c.T, TM.out_plane(c)) == (3, 9, 63) for c in TM.WORKSPACE_CASES[:4])
    assert TM.dense_tiles(*TM.WORKSPACE_CASES[4][2:4]) == 257
    assert TM.MAGNITUDE_SCALES == (2.0 ** -40, 2.0 ** 20)


@pytest.mark.parametrize("c", TM.DEFAULT_CASES, ids=TM.case_id)
def test_default_slope_seeds_keep_every_pre_activation_off_the_kink(c):
    """The condition the default-slope cases rest on: no float64 PReLU input within KINK_MARGIN of zero."""
    margin = TM.kink_margin(c)
    print(f"[kink] {TM.case_id(c)} seed {TM.DEFAULT_SEEDS[c.module]}: min |PReLU input| = {margin:.3e}")
    assert margin >= TM.KINK_MARGIN == 2e-5
    assert TM.find_default_seed(c) == TM.DEFAULT_SEEDS[c.module]
    sd = TM.module_state(c)
    slopes = torch.cat([v.flatten() for k, v in sd.items() if "prelu" in k or k.endswith(".2.weight")])
    assert float(slopes.abs().max()) < 0.6                        # the state dict's own slopes, not the twin's


# Where torch's fp32 autograd is no witness: a conv bias in front of an InstanceNorm has gradient sum(dz) = 0, which is as
# exact as the means the norm's backward subtracts.  torch's CPU kernel adds a plane's means in one fp32 chain, error about
# 2^-24 sqrt(P) rstd gamma of the norm-bias gradient: 0.6 .. 1.1e-4 at P = 49 245 .. 64 722 positions per clip (1.09e-4 at
# dense-1x322x201, 1.01e-4 at encoder-2x245x201), on either side of the 1e-4 bar by the draw.  The kernels add chunk
# partials in fp64 and ARE held to the bar at those shapes (tests/test_gpu_trainpath.py); here the figure is printed above
# 2^15 positions per clip and held at and below.  Forward, dL/dx and every other gradient are held at every shape.
TORCH_SUM_LIMIT = 1 << 15


def _fp32_stays_inside_the_bars(c, ref, st=None, xdy=None, tag="", k=1.0):
    if k != 1.0:
        x, dy = TM.inputs(c)[:2]
        xdy, ref = (x, dy * k), TM.scaled(ref, k)
    ck = TM.Checks(f"fp32 autograd {TM.case_id(c)}{tag}")
    ck.compare(c, TM.reference(c, torch.float32, st=st, xdy=xdy), ref, hold_zero_bias=c.T * c.F <= TORCH_SUM_LIMIT)
    ck.done()


@pytest.mark.parametrize("c", TM.all_cases(), ids=TM.case_id)
def test_fp32_autograd_through_the_oracle_meets_every_bar(c):
    _fp32_stays_inside_the_bars(c, TM.reference64(c))


@pytest.mark.parametrize("k", TM.MAGNITUDE_SCALES, ids=["2^-40", "2^+20"])
@pytest.mark.parametrize("c", TM.MAGNITUDE_CASES, ids=TM.case_id)
def test_fp32_autograd_meets_every_bar_on_scaled_gradients(c, k):
    _fp32_stays_inside_the_bars(c, TM.reference64(c), tag=f" x {k:g}", k=k)


def test_offset_case_sits_8_to_16_deviations_out_and_fp32_meets_the_bars():
    st, xdy, ref, ratios = TM.offset_case()
    assert set(ratios) == set(M.ENC_KEYS)
    for key, r in ratios.items():
        print(f"[offset] {key}: |mean| / std in [{float(r.min()):.2f}, {float(r.max()):.2f}]")
        assert 8.0 <= float(r.min()) and float(r.max()) <= 16.0, key
    _fp32_stays_inside_the_bars(TM.OFFSET_CASE, ref, st=st, xdy=xdy, tag=" offset")
