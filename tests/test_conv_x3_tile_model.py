"""CPU model of how conv3x_kernel (cmgan_amd/csrc/conv_x3.hip) finds the (t, f) of its rows: the staging map of CX_SETUP
(one division per thread, then RSTEP-row steps with ONE wrap each) and the store map of CX_EPILOGUE (one division per
lane, then 16-position steps with one wrap), against exact divmod over every tile of a plane.

The single wrap is exact only while a plane row (F + 1 positions with the virtual zero column) is at least as long as
the step.  Below that the walk drifts: rows that hold data are staged as zero padding, outputs that exist are not
stored - wrong numbers, no fault (every address the drifted walk produces is still a valid (t < T, f < F) of the clip).
conv3x_walkable (conv_x3.hip, mirrored in tests/convpath_model.py) is the limit callers obey; this file pins it to the
walks from both sides, and pins the mirrors' constants to the kernel file's text, so that whoever changes NWV / NPB
meets the limit here."""
import os
import re

import numpy as np
import pytest

import convpath_model as M
from conftest import ROOT

TS = (1, 2, 3, 5, 9, 17, 33)                       # frames: one row of the plane .. several tiles of the widest plane
COUTS = (64, 128)                                  # (RSTEP, rows) = (64, 256) and (32, 128)
FPS = range(2, 141)                                # F + 1


def staging_rows(T, F, cout, tile, walk):
    """What CX_SETUP stages as row p = 0 .. rows - 1 of `tile`: [rows][2] = (t, f) of the t-plane element, (-1, -1) for
    zero padding.  walk=False: the same by exact division."""
    Fp, rows, rstep = F + 1, M.x3_rows(cout), M.x3_rstep(cout)
    q0 = tile * (rows - 2)
    out = np.full((rows, 2), -1)
    first = q0 - 1 + np.arange(rstep)              # tid >> 3 = 0 .. RSTEP - 1
    if walk:
        tt = np.maximum(first, 0) // Fp
        ff = first - tt * Fp                       # q = -1 -> (0, -1): padding
        for e in range(rows // rstep):
            ok = (ff >= 0) & (ff < F) & (tt < T)
            out[np.arange(rstep)[ok] + rstep * e] = np.stack([tt[ok], ff[ok]], 1)
            ff = ff + rstep
            wrap = ff >= Fp
            ff, tt = np.where(wrap, ff - Fp, ff), tt + wrap
    else:
        q = q0 - 1 + np.arange(rows)
        t, f = np.divmod(np.maximum(q, 0), Fp)
        ok = (q >= 0) & (f < F) & (t < T)
        out[ok] = np.stack([t[ok], f[ok]], 1)
    return out


def stored_outputs(T, F, cout, tile, walk):
    """What CX_EPILOGUE stores for MFMA position p of `tile`: [rows][2] = (t, f), (-1, -1) where nothing is stored."""
    Fp, rows, npb = F + 1, M.x3_rows(cout), M.x3_npb(cout)
    q0 = tile * (rows - 2)
    out = np.full((rows, 2), -1)
    wv, c = np.divmod(np.arange(rows // npb), 16)  # one (wave, lane & 15) per entry
    base = 16 * npb * wv + c
    if walk:
        t, f = np.divmod(q0 + base, Fp)
        for tb in range(npb):
            if tb > 0:
                f = f + M.EPI_STEP
                wrap = f >= Fp
                f, t = np.where(wrap, f - Fp, f), t + wrap
            p = base + 16 * tb
            ok = (t < T) & (f < F) & (p < rows - 2)
            out[p[ok]] = np.stack([t[ok], f[ok]], 1)
    else:
        p = np.arange(rows)
        t, f = np.divmod(q0 + p, Fp)
        ok = (t < T) & (f < F) & (p < rows - 2)
        out[ok] = np.stack([t[ok], f[ok]], 1)
    return out


def walks_exact(F, cout, Ts=TS):
    for T in Ts:
        for tile in range(M.conv3x_ntiles(T, F, cout)):
            if not np.array_equal(staging_rows(T, F, cout, tile, True), staging_rows(T, F, cout, tile, False)):
                return False
            if not np.array_equal(stored_outputs(T, F, cout, tile, True), stored_outputs(T, F, cout, tile, False)):
                return False
    return True


@pytest.mark.parametrize("cout", COUTS)
def test_predicate_admits_exactly_the_widths_the_walks_are_exact_for(cout):
    """No narrower: every admitted width walks exactly.  Not needlessly wider: every refused width has a tile where the
    walk goes wrong (so the fp32 kernel is taken only where it is needed)."""
    exact = {Fp: walks_exact(Fp - 1, cout) for Fp in FPS}
    admitted = {Fp: M.conv3x_walkable(Fp - 1, cout) for Fp in FPS}
    assert exact == admitted, [Fp for Fp in FPS if exact[Fp] != admitted[Fp]]
    limit = min(Fp for Fp in FPS if admitted[Fp])
    assert limit == M.x3_rstep(cout) == {64: 64, 128: 32}[cout]
    assert all(admitted[Fp] == (Fp >= limit) for Fp in FPS)


def test_every_width_the_library_hands_to_the_x3_kernels_walks_exactly():
    """tscnet_impl's choice (convpath_model.dense_ntiles) over every n_fft cmgan_create accepts up to the 48 kHz model:
    the encoder plane F = n_fft / 2 + 1 and the decoder plane F' = (F + 1) / 2, 64- and 128-channel kernels."""
    seen = set()
    for n_fft in range(16, 1201, 16):
        F = n_fft // 2 + 1
        for plane, cout in ((F, 64), ((F + 1) // 2, 64), ((F + 1) // 2, 128)):
            for mode in ("f16x3", "f16x1"):
                if M.dense_ntiles(mode, 3, plane, cout)[0] == "x3":
                    seen.add((plane, cout))
            assert M.dense_ntiles("f32", 3, plane, cout) == ("f32", M.conv3_ntiles(3, plane))
    assert (201, 64) in seen and (101, 64) in seen and (101, 128) in seen and (601, 64) in seen and (301, 128) in seen
    assert (65, 64) in seen and (33, 128) in seen and (33, 64) not in seen and (61, 64) not in seen and (5, 128) not in seen
    for plane, cout in sorted(seen):
        assert M.conv3x_walkable(plane, cout)
        if plane + 1 not in FPS:                   # the narrow ones are covered exhaustively above
            assert walks_exact(plane, cout, Ts=(2, 9)), (plane, cout)


def test_narrow_planes_the_library_used_to_run_are_the_ones_that_drift():
    """The widths of the gap: n_fft 16 .. 240 in the split-f16 modes.  At n_fft 128 the encoder plane (65) walks, the
    decoders' (33) does not; 240 is one step below the limit in the decoders, 256 the first width that is right."""
    assert not walks_exact(9, 64) and not walks_exact(5, 64) and not walks_exact(5, 128)
    assert walks_exact(65, 64) and not walks_exact(33, 64) and walks_exact(33, 128)
    assert walks_exact(121, 64) and not walks_exact(61, 64) and walks_exact(61, 128)
    assert walks_exact(129, 64) and walks_exact(65, 128)


@pytest.mark.parametrize("cout", COUTS)
def test_a_drifted_walk_never_leaves_the_clip(cout):
    """Why the gap was wrong numbers and not a fault: whatever (t, f) the drifted walks produce passes the kernel's own
    t < T, 0 <= f < F test before it is used as an address (staging_rows / stored_outputs apply that test); the
    t - dil plane is read only where that test passed and t >= dil."""
    for Fp in range(2, M.x3_rstep(cout)):
        for T in (1, 3, 17):
            for tile in range(M.conv3x_ntiles(T, Fp - 1, cout)):
                for rows in (staging_rows(T, Fp - 1, cout, tile, True), stored_outputs(T, Fp - 1, cout, tile, True)):
                    used = rows[rows[:, 0] >= 0]
                    assert (used[:, 0] < T).all() and (used[:, 1] >= 0).all() and (used[:, 1] < Fp - 1).all()


@pytest.mark.parametrize("cout,F", [(64, 63), (64, 64), (64, 65), (64, 101), (64, 129),
                                    (128, 31), (128, 32), (128, 63), (128, 65), (128, 101)])
def test_tiles_cover_the_plane_once_and_stage_their_halo(cout, F):
    """On a walkable plane: every (t, f) is stored by exactly one tile, and MFMA position p reads rows p, p + 1, p + 2 =
    the f - 1, f, f + 1 neighbours (the virtual zero column is the padding between two rows of the plane)."""
    assert M.conv3x_walkable(F, cout)
    T = 9
    count = np.zeros((T, F), int)
    for tile in range(M.conv3x_ntiles(T, F, cout)):
        st, out = staging_rows(T, F, cout, tile, True), stored_outputs(T, F, cout, tile, True)
        for p in np.nonzero(out[:, 0] >= 0)[0]:
            t, f = out[p]
            count[t, f] += 1
            assert tuple(st[p + 1]) == (t, f)
            assert tuple(st[p]) == ((t, f - 1) if f > 0 else (-1, -1))
            assert tuple(st[p + 2]) == ((t, f + 1) if f + 1 < F else (-1, -1))
    assert (count == 1).all()


def test_mirrors_name_the_constants_of_the_kernel_files():
    """convpath_model restates host arithmetic; this pins what it shares with the sources by their text."""
    def src(name):
        return open(os.path.join(ROOT, "cmgan_amd", "csrc", name)).read()

    x3, cv, api, tr = src("conv_x3.hip"), src("conv.hip"), src("api.hip"), src("train.hip")
    for name in ("CX_NPB64", "CX_NWV64", "CX_NPB128", "CX_NWV128"):
        assert int(re.search(rf"#define {name} (\d+)", x3).group(1)) == getattr(M, name)
    assert int(re.search(r"#define CONV_TILE (\d+)", cv).group(1)) == M.CONV_TILE
    assert int(re.search(r"#define INF_NP (\d+)", cv).group(1)) == M.INF_NP
    assert f"t0 += INF_NP * {M.INF_LOADS}" in cv
    assert "constexpr int RSTEP = NTHR / 8;" in x3 and "constexpr int CX_ROWS = 16 * NPB * NWV;" in x3
    assert "constexpr int CX_TILE = CX_ROWS - 2;" in x3
    assert "ff_ += RSTEP;" in x3 and "if (ff_ >= Fp) { ff_ -= Fp; ++tt_; }" in x3
    assert f"if (tb > 0) {{ f += {M.EPI_STEP}; if (f >= Fp) {{ f -= Fp; ++t; }} }}" in x3
    assert "const int rstep = 8 * (cout == 128 ? CX_NWV128 : CX_NWV64);" in x3
    assert f"return F + 1 >= (rstep > {M.EPI_STEP} ? rstep : {M.EPI_STEP});" in x3
    assert "int conv3_ntiles(int T, int F) { return (T * (F + 1) + CONV_TILE - 1) / CONV_TILE; }" in cv
    # the callers: per plane width and kernel in the forward, the same predicate on the training side
    assert "x3e = x3 && conv3x_walkable(F, 64), x3d = x3 && conv3x_walkable(F2, 64), x3s = x3 && conv3x_walkable(F2, 128);" in api
    assert "static bool db_x3_forward(int F) { return conv3x_walkable(F, 64); }" in tr
    assert M.conv3x_ntiles(33, 129, 64) == 17 and M.conv3x_ntiles(33, 65, 128) == 18 and M.conv3_ntiles(33, 129) == 34
