"""Float64 references of the TRAINING conv path (cmgan_amd/csrc/train.hip, train_x3.hip, conv_x3.hip: DenseBlockTrain,
DenseEncoderTrain, DecoderTrain) for tests/test_gpu_trainpath.py, the cases of that file with the arithmetic they are named
for, and the host mirrors of the tilings the training kernels use.  TEST INFRASTRUCTURE ONLY.

The reference is torch autograd through the project's own oracle (oracle/cmgan_oracle.py: dense_block, dense_encoder,
mask_decoder, complex_decoder) on a float64 copy of the state dict; nothing here restates a kernel.  What this file adds:

* `Case` (module, B, T, F, slopes): F is the width of the module's INPUT plane - the plane of its dilated dense block (the
  encoder's output and the decoders' input plane is F' = (F - 1) // 2 + 1; a decoder's output is 2 F - 1 wide);
* `inputs` / `reference`: seeded inputs of a case and {y, dx, grads} of the oracle in a given dtype, NCHW;
* `Checks.compare`: the bars of tests/test_gpu_training.py applied to such a result, shared by the GPU file and by the host
  file's check that fp32 torch autograd stays inside them;
* the case groups of tests/test_gpu_trainpath.py and mirrors of the host arithmetic they are named for (weight-gradient
  steps and splits, the persistent row-conv data gradient's trips, tile counts via convpath_model) - pinned to the text of
  the kernel files by tests/test_trainpath_model.py.

PReLU slopes: "twin" = cmgan_amd.synth.kink_free_twin (slopes 1 - 1e-3 i / n), as in the whole-step tests and for the same
reason: with the default slopes one of 10^5 .. 10^7 pre-activations landing on the other side of zero moves every upstream
gradient far beyond rounding.  "default" = the state dict's own slopes (~0.25), on a small wide plane, with an input seed
chosen so that no float64 pre-activation lies within KINK_MARGIN of zero (DEFAULT_SEEDS; asserted by the host file)."""
from __future__ import annotations

import re
from collections import namedtuple

import numpy as np
import torch

import convpath_model as M
from conftest import assert_close, rel_err
from oracle import cmgan_oracle as O
from test_gpu_convpath import GRIDS                # (B, T) -> B * tiles of a 64-channel x3 conv on a plane of width 129
from test_gpu_training import GRAD_TOL             # the suite's bar of a training gradient: 1e-4 of the tensor's maximum

# ---- tilings of the training kernels (train.hip, train_x3.hip; pinned by tests/test_trainpath_model.py) ----------------
WG_STEP = 32                                       # db_conv_wgrad_x3_kernel / rc_wgrad_x3_kernel: positions per step
WG_WAVES = 4                                       # waves of a block: one lane advances WG_STEP * WG_WAVES positions per trip
DB_WG_SPLIT = 256                                  # position ranges (blocks per tap) of the dense weight gradient
RC_WG_SPLIT = 256                                  # ... of the row convs'
RCD_POS = 16                                       # rc_dgrad_x3_kernel: input positions per tile
RCD_TILES = 8                                      # tiles per block and trip (one per wave)
RCD_CAP = {1: 768, 2: 256}                         # most blocks of the persistent grid, by NG (64 NG output channels)
DB_NCH = 256                                       # position chunks per clip of the per-(b, c) reductions
MT_NCH = 32                                        # ... of the single-channel mask head
DB_MAXBLK = 2048                                   # blocks of db_in_bwd_kernel = |dz| maxima left for the dgrad scale
FINALIZE_THREADS = 256                             # db_stats_finalize_tiles_kernel: tiles added per pass


def ceil_div(a: int, b: int) -> int:
    return (a + b - 1) // b


def dense_kernel(F: int) -> str:
    """which forward / data-gradient kernel a 64 -> 64 conv of a plane of width F takes in training (db_x3_forward,
    rc_x3_forward: both conv3x_walkable(F, 64))"""
    return "x3" if M.conv3x_walkable(F, 64) else "f32"


def dense_tiles(T: int, F: int) -> int:
    """tiles per clip of the dense block's conv (forward partials, data gradient) on a walkable plane"""
    assert M.conv3x_walkable(F, 64)
    return M.conv3x_ntiles(T, F, 64)


def finalize_passes(ntiles: int) -> int:
    return ceil_div(ntiles, FINALIZE_THREADS)


def wgrad_splits(positions: int, nsplit: int = DB_WG_SPLIT):
    """(steps, steps per split, [steps of split s]) of a weight gradient over `positions`"""
    steps = ceil_div(positions, WG_STEP)
    per = ceil_div(steps, nsplit)
    return steps, per, [max(0, min((s + 1) * per, steps) - s * per) for s in range(nsplit)]


def wgrad_clips_per_advance(T: int, F: int) -> int:
    """clips a lane of the dense weight gradient moves on by in one trip (the `while (t >= T)` wraps), at the least"""
    return (WG_STEP * WG_WAVES) // (T * F)


def rc_dgrad_geometry(positions: int, ng: int):
    """(tiles, blocks, trips of the busiest block) of rc_dgrad_x3_kernel over `positions` input positions"""
    tiles = ceil_div(positions, RCD_POS)
    grid = min(max(ceil_div(tiles, RCD_TILES), 1), RCD_CAP[ng])
    return tiles, grid, ceil_div(tiles, RCD_TILES * grid)


def dgrad_scratch_floats(B: int) -> int:
    """db_dgrad_setup_kernel's scratch inside the partial-sum area: 256, scale and zeros per (b, c), the block maxima"""
    return 256 + 2 * B * 64 + DB_MAXBLK


def partial_area_floats(B: int, T: int, F: int) -> int:
    """db_plan's `part`: the chunk partials or, when larger, the conv kernel's per-(clip, tile) partials"""
    return max(B * DB_NCH * 64 * 3, B * M.conv3x_ntiles(T, F, 64) * 128)


# ---- modules ---------------------------------------------------------------------------------------------------------
MODULES = ("dense", "encoder", "mask", "complex")
PREFIX = {"dense": "dense_encoder.dilated_dense", "encoder": "dense_encoder", "mask": "mask_decoder",
          "complex": "complex_decoder"}
# conv biases directly in front of an InstanceNorm (exactly zero gradient) and the norm bias whose gradient scales their bar
ZERO_BIAS = {"dense": [r"^conv\d\.bias$"], "encoder": [r"\.0\.bias$", r"\.conv\d\.bias$"],
             "mask": [r"\.conv\d\.bias$", r"^conv_1\.bias$"], "complex": [r"\.conv\d\.bias$"]}
SCALE_KEY = {"dense": "norm1.bias", "encoder": "conv_1.1.bias", "mask": "norm.bias", "complex": "norm.bias"}
KINK_MARGIN = 2e-5

Case = namedtuple("Case", "module B T F slopes", defaults=("twin",))


def case_id(c: Case) -> str:
    return f"{c.module}-{c.B}x{c.T}x{c.F}" + ("" if c.slopes == "twin" else "-" + c.slopes)


def out_plane(c: Case) -> int:
    """F' of the encoder; the other modules keep their plane"""
    return (c.F - 1) // 2 + 1 if c.module == "encoder" else c.F


_STATE = {}


def full_state(slopes: str) -> dict:
    """the generator state dict (seed 0, 201 features) with the given slopes, float32"""
    if slopes not in _STATE:
        from cmgan_amd.synth import kink_free_twin, make_state_dict
        sd = make_state_dict(seed=0)
        _STATE[slopes] = kink_free_twin(sd) if slopes == "twin" else sd
    return _STATE[slopes]


def module_state(c: Case, sd: dict | None = None) -> dict:
    """the module's slice of the state dict under its full keys; the mask head's per-bin slopes cut to 2 F - 1 bins"""
    sd = full_state(c.slopes) if sd is None else sd
    p = PREFIX[c.module] + "."
    st = {k: v for k, v in sd.items() if k.startswith(p)}
    if c.module == "mask":
        assert 2 * c.F - 1 <= st[p + "prelu_out.weight"].numel()
        st[p + "prelu_out.weight"] = st[p + "prelu_out.weight"][:2 * c.F - 1].clone()
    return st


def relative(c: Case, st: dict) -> dict:
    """the same under the keys relative to the module, as the *Train wrappers take them"""
    n = len(PREFIX[c.module]) + 1
    return {k[n:]: v for k, v in st.items()}


# input seeds of the default-slope cases (B = 1, T = 3, F' = 63): the first seeds from 0 whose float64 pass keeps every
# PReLU input at least KINK_MARGIN from zero (find_default_seed; about half of all seeds do at 5e4 pre-activations)
DEFAULT_SEEDS = {"dense": 0, "encoder": 3, "mask": 1, "complex": 2}


def inputs(c: Case, seed: int | None = None):
    """(x, dy, spec) float32 NCHW, seeded by the case: x the module's input ([B,64,T,F]; encoder: [B,3,T,F] = (|spec|, re,
    im) of `spec` [B,2,T,F], else spec is None), dy the gradient at its output."""
    if seed is None:
        seed = DEFAULT_SEEDS[c.module] if c.slopes == "default" else 0
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([7200, MODULES.index(c.module), c.B, c.T, c.F, seed])))

    def draw(*shape):
        return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))

    spec = None
    if c.module == "encoder":
        spec = draw(c.B, 2, c.T, c.F)
        x = M._model_in(spec)
        dy = draw(c.B, 64, c.T, out_plane(c))
    else:
        x = draw(c.B, 64, c.T, c.F)
        dy = draw(c.B, 64, c.T, c.F) if c.module == "dense" else draw(c.B, 1 if c.module == "mask" else 2, c.T, 2 * c.F - 1)
    return x, dy, spec


def oracle_forward(c: Case, sd: dict, x: torch.Tensor) -> torch.Tensor:
    if c.module == "dense":
        return O.dense_block(sd, PREFIX["dense"], x)
    return {"encoder": O.dense_encoder, "mask": O.mask_decoder, "complex": O.complex_decoder}[c.module](sd, x)


def reference(c: Case, dtype=torch.float64, st: dict | None = None, xdy=None, kinks: dict | None = None) -> dict:
    """{y, dx (None: the encoder's input carries no gradient), grads {relative key: dL/dparam}} of torch autograd through
    the oracle in `dtype`, NCHW.  `st`: the module's state (default module_state(c)); `xdy`: (x, dy) (default inputs(c));
    `kinks`: filled with min |PReLU input| per PReLU."""
    st = module_state(c) if st is None else st
    x, dy = inputs(c)[:2] if xdy is None else xdy
    leaf = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in st.items()}
    xr = x.to(dtype).clone().requires_grad_(c.module != "encoder")
    with torch.enable_grad(), O.prelu_inputs({} if kinks is None else kinks):
        y = oracle_forward(c, leaf, xr)
        y.backward(dy.to(dtype))
    return {"y": y.detach(), "dx": xr.grad, "grads": {k: v.grad for k, v in relative(c, leaf).items()}}


_REF = {}


def reference64(c: Case) -> dict:
    """the float64 reference of the case's own state and inputs, computed once and left unchanged"""
    if c not in _REF:
        _REF[c] = reference(c)
    return _REF[c]


def scaled(ref: dict, k: float) -> dict:
    """the reference of k * dy: the backward is linear in dy (k a power of two: exact in float64)"""
    return {"y": ref["y"], "dx": None if ref["dx"] is None else ref["dx"] * k, "grads": {n: g * k for n, g in ref["grads"].items()}}


def kink_margin(c: Case, seed: int | None = None) -> float:
    """min |PReLU input| over every PReLU of the case's float64 forward"""
    kinks = {}
    with torch.no_grad(), O.prelu_inputs(kinks):
        oracle_forward(c, M.to64(module_state(c)), inputs(c, seed)[0].double())
    assert kinks
    return min(kinks.values())


def find_default_seed(c: Case, tries: int = 64) -> int:
    """how DEFAULT_SEEDS was chosen: the first seed whose margin is at least KINK_MARGIN"""
    return next(s for s in range(tries) if kink_margin(c, s) >= KINK_MARGIN)


# ---- the bars (tests/test_gpu_training.py) ------------------------------------------------------------------------------
class Checks:
    """Runs every comparison of a case, prints each figure in the suite's `[parity]` style and fails at the end with the
    names of all that missed.  `worst` keeps the largest figure per group (forward, dL/dx, parameter gradients, and the
    zero-gradient biases relative to their bar's scale) for the GPU file's docstring."""

    def __init__(self, case: str):
        self.case, self.failed, self.worst = case, [], {}

    def report(self, group, name, err, bar):
        print(f"[parity] {self.case} {name}: rel_err = {err:.3e}")
        self.worst[group] = max(self.worst.get(group, 0.0), err)
        if not err < bar:
            self.failed.append(f"{name}: {err:.3e} >= {bar:g}")

    def close(self, group, name, got, want):
        """forward and dL/dx: GRAD_TOL max-norm relative plus the elementwise rtol / atol_rel bound"""
        self.report(group, name, rel_err(got, want), GRAD_TOL)
        try:
            assert_close(got, want, rtol=1e-3, atol_rel=2e-4, name=name)
        except AssertionError as e:
            self.failed.append(str(e))

    def compare(self, c: Case, got: dict, ref: dict, hold_zero_bias: bool = True):
        """got / ref: {y, dx, grads} in the reference's layout.  hold_zero_bias=False (only for the host file's fp32 torch
        witness on its largest planes): the zero-gradient biases are printed, not held."""
        self.close("forward", "forward", got["y"], ref["y"])
        assert (got["dx"] is None) == (ref["dx"] is None) == (c.module == "encoder")
        if ref["dx"] is not None:
            self.close("dL/dx", "dL/dx", got["dx"], ref["dx"])
        assert set(got["grads"]) == set(ref["grads"])
        scale = float(ref["grads"][SCALE_KEY[c.module]].abs().max())
        for k, want in ref["grads"].items():
            g = got["grads"][k]
            assert g.shape == want.shape, k
            if any(re.search(z, k) for z in ZERO_BIAS[c.module]):
                # in front of an InstanceNorm: zero in exact arithmetic (the float64 value is rounding noise)
                self.report("zero bias / scale", f"|dL/d[{k}]| / max|dL/d[{SCALE_KEY[c.module]}]|",
                            float(g.detach().double().abs().max()) / scale, 1e-4 if hold_zero_bias else float("inf"))
            else:
                self.report("parameters", f"dL/d[{k}]", rel_err(g, want), GRAD_TOL)

    def done(self):
        assert not self.failed, f"{self.case}: " + "; ".join(self.failed)


# ---- the cases of tests/test_gpu_trainpath.py -------------------------------------------------------------------------
DECODERS = ("mask", "complex")

# plane widths, B = 2, T = 11.  Dense block: 62 the widest fallback plane, 63 the narrowest walkable one (a row of 64 = the
# staging step).  Encoder: F' = 31, 32, 32, 63, 64, 101; 64 an even width (the stride-2 conv's last tap hangs over the
# edge), 125 -> conv_2's output plane is the narrowest walkable one.  Decoders: F'.
WIDTHS = ([Case("dense", 2, 11, F) for F in (5, 9, 62, 63, 64, 101, 201)]
          + [Case("encoder", 2, 11, F) for F in (61, 63, 64, 125, 127, 201)]
          + [Case(k, 2, 11, F) for k in DECODERS for F in (31, 62, 63, 64, 101)])
WIDTH_KERNELS = {"dense": {5: "f32", 9: "f32", 62: "f32", 63: "x3", 64: "x3", 101: "x3", 201: "x3"},
                 "encoder": {61: "f32", 63: "x3", 64: "x3", 125: "x3", 127: "x3", 201: "x3"},
                 "mask": {31: "f32", 62: "f32", 63: "x3", 64: "x3", 101: "x3"},
                 "complex": {31: "f32", 62: "f32", 63: "x3", 64: "x3", 101: "x3"}}
ENCODER_OUT = {61: 31, 63: 32, 64: 32, 125: 63, 127: 64, 201: 101}

# T <= dil: every t - dil tap (forward) and every t + dil tap (data gradient, revt) of a layer is padding; T = dil + 1:
# exactly one row is not.  B = 3: the clip offsets of every kernel matter.
TIME_TS = (1, 2, 3, 8, 9, 17)
TIME_EDGES = ([Case("dense", 3, T, F) for F in (63, 101) for T in TIME_TS]
              + [Case("encoder", 3, T, 125) for T in (1, 2, 9)]
              + [Case(k, 3, T, 63) for k in DECODERS for T in (1, 2, 9)])

# grid sizes of the XCD remap on the data-gradient instantiation: B * tiles in {1, 3, 7, 8, 9, 17} at F = 129
GRID_CASES = [Case("dense", B, T, 129) for B, T in sorted(GRIDS)]

# tiles per clip -> passes of db_stats_finalize_tiles_kernel: 257 is the first shape that takes the second
FINALIZE = {1: 1, 321: 256, 322: 257}
FINALIZE_CASES = [Case("dense", 1, T, 201) for T in sorted(FINALIZE)]

# the dense weight gradient's walk and splits
WGRAD_CASES = [Case("dense", 1, 1, 5),             # one ragged step, F < 8, never interior
               Case("dense", 9, 1, 9),             # T F = 9: one advance crosses fourteen clips
               Case("dense", 5, 1, 63),            # T F = 63: two clips per advance, on a wide plane
               Case("dense", 2, 64, 64),           # 8192 positions: exactly one full step in each of the 256 splits
               Case("dense", 2, 41, 100)]          # 8200: 257 steps, two per split, split 128 one ragged step, 129 .. empty

# the persistent row-conv data gradient's second trip: more tiles than 8 x the block cap
PERSISTENT_CASES = [Case("encoder", 2, 245, 201), Case("mask", 2, 165, 101), Case("complex", 2, 165, 101)]

# gradient magnitude: dy scaled by 2^-40 and 2^+20, planes 63 and 101 (the encoder's output plane: F = 125 and 201)
MAGNITUDE_SCALES = (2.0 ** -40, 2.0 ** 20)
MAGNITUDE_CASES = ([Case(k, 2, 11, F) for k in ("dense",) + DECODERS for F in (63, 101)]
                   + [Case("encoder", 2, 11, F) for F in (125, 201)])

# conv biases raised until every pre-norm channel sits 8 .. 16 standard deviations from zero
OFFSET_CASE = Case("encoder", 2, 33, 125)

# default slopes on a wide plane, B = 1, T = 3, F' = 63
DEFAULT_CASES = [Case("dense", 1, 3, 63, "default"), Case("encoder", 1, 3, 125, "default"),
                 Case("mask", 1, 3, 63, "default"), Case("complex", 1, 3, 63, "default")]

# determinism and exact-size workspaces: one wide case per module and the dense block's 257-tile case
WORKSPACE_CASES = [Case("dense", 3, 9, 63), Case("encoder", 3, 9, 125), Case("mask", 3, 9, 63), Case("complex", 3, 9, 63),
                   Case("dense", 1, 322, 201)]
GUARD_BYTES = 65536


def all_cases() -> list:
    """every distinct (module, shape, slopes) the GPU file runs, in a fixed order"""
    seen = []
    for c in (WIDTHS + TIME_EDGES + GRID_CASES + FINALIZE_CASES + WGRAD_CASES + PERSISTENT_CASES + MAGNITUDE_CASES
              + [OFFSET_CASE] + DEFAULT_CASES + WORKSPACE_CASES):
        if c not in seen:
            seen.append(c)
    return seen


_OFFSET = {}


def offset_case():
    """(module state with raised biases, (x, dy), its float64 reference, |mean| / std per norm of the float64 pass)"""
    if not _OFFSET:
        c = OFFSET_CASE
        x, dy, spec = inputs(c)
        sd = M.offset_state_dict(full_state(c.slopes), spec)
        st = module_state(c, sd)
        stats = M.encoder(M.to64(sd), spec.double())[1]
        _OFFSET["v"] = (st, (x, dy), reference(c, st=st, xdy=(x, dy)), M.offset_ratios(stats))
    return _OFFSET["v"]
