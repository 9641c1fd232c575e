"""float64 CPU reference of the metric discriminator (cmgan_amd/csrc/disc.hip), no GPU import.

`reference()` mirrors oracle/cmgan_oracle.py::discriminator with every tensor in one dtype (float64 for the reference,
float32 for the round-off floor the GPU bars are derived from) and returns, through autograd, everything
`DiscriminatorTrain` produces: the score, the six updated u / v pairs, dL/dxy, the 22 parameter gradients under the
keys of `DiscriminatorTrain.grads`, and the eval-mode score with the updated buffers.  The pool is
F.adaptive_max_pool2d like the reference module (amax differs in backward on ties).

`wgrad_plan()` / `norm_plan()` are Python MIRRORS of host arithmetic in csrc/disc.hip - keep them in sync with it.

`CASES`, `states()` and `inputs()` are the shapes, weights and seeded inputs tests/test_disc_model.py (CPU: the input
conditions, the branch each case reaches) and tests/test_gpu_disc.py (the kernels) share.

    python tests/disc_model.py          prints the fp32 floors and bars of every case (the table in test_gpu_disc.py)
"""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.cmgan_oracle import EPS, spectral_normed  # noqa: E402

CH = (2, 16, 32, 64, 128)
SN = ("layers.0", "layers.3", "layers.6", "layers.9", "layers.14", "layers.17")


# ---- mirrors of the host code of csrc/disc.hip: KEEP IN SYNC ------------------------------------------------------------
DC_SPLIT, DW_TP = 32, 32           # disc.hip: #define DC_SPLIT / DW_TP
NORM_GRID_CAP, NORM_BLOCK = 4096, 256


def layer_dims(T, F_):
    """dc_plan(): [(Ti, Fi, Ci, To, Fo, Co)] of the four convolutions."""
    out, t, f = [], T, F_
    for i in range(4):
        out.append((t, f, CH[i], t // 2, f // 2, CH[i + 1]))
        t, f = t // 2, f // 2
    return out


def shape_ok(T, F_):
    """disc_shape_ok()."""
    return T >= 16 and F_ >= 16


def wgrad_plan(B, T, F_):
    """launch_disc_backward(): the split-K launch shape of dc_conv_wgrad_kernel per layer - MIRROR, line for line."""
    plan = []
    for (Ti, Fi, Ci, To, Fo, Co) in layer_dims(T, F_):
        P = To * Fo
        nw = 16 * Ci * Co
        Mtot = 16 * Ci
        MB = Mtot if Mtot < 8192 // Co else 8192 // Co
        groups = Mtot // MB
        tiles_total = (B * P + DW_TP - 1) // DW_TP
        ns = 1024 // groups
        want = ns                                  # what the block budget alone would launch
        cap = (DC_SPLIT * 16 * 64 * 128) // nw
        if ns > cap:
            ns = cap
        if ns > tiles_total:
            ns = tiles_total
        tpc = (tiles_total + ns - 1) // ns
        used = (tiles_total + tpc - 1) // tpc      # chunks with t_begin < tiles_total
        plan.append(dict(tiles_total=tiles_total, MB=MB, groups=groups, cap=cap, ns=ns, tpc=tpc, empty_chunks=ns - used,
                         cap_binds=cap < min(want, tiles_total), nw=nw))
    return plan


def norm_plan(B, T, F_):
    """gin_bwd_finalize_kernel's G = 1024 / C clip groups and the 4096-block cap of gin_norm_prelu_kernel /
    gin_in_bwd_kernel per layer - MIRROR."""
    plan = []
    for (Ti, Fi, Ci, To, Fo, Co) in layer_dims(T, F_):
        total = B * To * Fo * Co
        blocks = (total + NORM_BLOCK - 1) // NORM_BLOCK
        grid = blocks if blocks < NORM_GRID_CAP else NORM_GRID_CAP
        G = 1024 // Co
        plan.append(dict(C=Co, G=G, finalize_steps=(B + G - 1) // G, total=total, grid=grid,
                         stride_iters=(total + grid * NORM_BLOCK - 1) // (grid * NORM_BLOCK)))
    return plan


def dgrad_classes(B, T, F_):
    """dc_conv_gemm_kernel<1>: positions of the four parity classes (rt, rf) per layer; the grid is sized by the first."""
    return [[B * ((Ti - rt + 1) // 2) * ((Fi - rf + 1) // 2) for rt in (0, 1) for rf in (0, 1)]
            for (Ti, Fi, *_r) in layer_dims(T, F_)]


# ---- the reference -------------------------------------------------------------------------------------------------------
def _forward(dsd, h, mask, train, taps=None):
    """oracle.cmgan_oracle.discriminator with adaptive_max_pool2d; h [B,2,F,T].  `taps` collects what the input
    conditions look at: the PReLU inputs and the pooled plane."""
    new = {}
    for i in range(4):
        p = f"layers.{3 * i}"
        w, u, v = spectral_normed(dsd[p + ".weight_orig"], dsd[p + ".weight_u"], dsd[p + ".weight_v"], train)
        new[p + ".weight_u"], new[p + ".weight_v"] = u, v
        h = F.conv2d(h, w, None, stride=(2, 2), padding=(1, 1))
        h = F.instance_norm(h, weight=dsd[f"layers.{3 * i + 1}.weight"], bias=dsd[f"layers.{3 * i + 1}.bias"], eps=EPS)
        if taps is not None:
            taps[f"n{i + 1}"] = h.detach()
        h = F.prelu(h, dsd[f"layers.{3 * i + 2}.weight"])
    if taps is not None:
        taps["a4"] = h.detach()
    h = F.adaptive_max_pool2d(h, 1).flatten(1)
    w, u, v = spectral_normed(dsd["layers.14.weight_orig"], dsd["layers.14.weight_u"], dsd["layers.14.weight_v"], train)
    new["layers.14.weight_u"], new["layers.14.weight_v"] = u, v
    h = F.linear(h, w, dsd["layers.14.bias"])
    if mask is not None:
        h = h * mask
    if taps is not None:
        taps["n5"] = h.detach()
    h = F.prelu(h, dsd["layers.16.weight"])
    w, u, v = spectral_normed(dsd["layers.17.weight_orig"], dsd["layers.17.weight_u"], dsd["layers.17.weight_v"], train)
    new["layers.17.weight_u"], new["layers.17.weight_v"] = u, v
    h = F.linear(h, w, dsd["layers.17.bias"])
    return torch.sigmoid(dsd["layers.18.slope"] * h), new


def reference(state, xy, mask, dscore, dtype=torch.float64):
    """One train-mode forward + backward and the eval-mode forward after it.  state: the module's state dict (34
    entries); xy [B,T,F,2]; mask [B,64] keep-mask (0 or 1/0.7) or None; dscore [B].  Returns a dict: score [B], buffers
    {key: new u / v}, dxy [B,T,F,2], grads {key: gradient} (22), score_eval [B], taps (PReLU inputs, pooled plane)."""
    sd = {k: v.detach().to(dtype).clone() for k, v in state.items()}
    leaf = {k: sd[k].requires_grad_(True) for k in sd if not k.endswith(("weight_u", "weight_v"))}
    assert len(leaf) == 22
    x = xy.detach().to(dtype).clone().requires_grad_(True)
    m = None if mask is None else mask.detach().to(dtype)
    taps = {}
    with torch.enable_grad():
        score, new = _forward(sd, x.permute(0, 3, 2, 1), m, True, taps)
        score.backward(dscore.detach().to(dtype).reshape(-1, 1))
    with torch.no_grad():
        sde = dict(sd)
        sde.update(new)
        score_eval, _ = _forward(sde, x.detach().permute(0, 3, 2, 1), None, False)
    return {"score": score.detach()[:, 0], "buffers": {k: v.detach() for k, v in new.items()}, "dxy": x.grad.detach(),
            "grads": {k: v.grad.detach() for k, v in leaf.items()}, "score_eval": score_eval[:, 0], "taps": taps}


def pool_margin(a4):
    """Smallest (largest - second largest) / max|plane| over the (b, c) planes the max pool reduces."""
    flat = a4.flatten(2)
    top = flat.topk(2, dim=2).values
    return float(((top[..., 0] - top[..., 1]) / flat.abs().amax(dim=2)).min())


def kink_ratios(taps, taps32):
    """Per PReLU: the smallest |input| of the reference over the largest fp32 error among the inputs within 1e-3 of
    zero (`taps32` = the same forward in fp32).  A masked-out head unit is exactly zero in every arithmetic and both
    sides use the derivative of d5 >= 0 there: not counted."""
    out = []
    for i in range(1, 6):
        n, a = taps[f"n{i}"], taps[f"n{i}"].abs()
        near = (a < 1e-3) & (a > 0)
        err = float((taps32[f"n{i}"].double() - n).abs()[near].max()) if bool(near.any()) else 0.0
        out.append(float(a[a > 0].min()) / max(err, 1e-7))
    return out


# ---- the shared cases ----------------------------------------------------------------------------------------------------
# (id, B, T, F, weights, input seed): weights "default" = discriminator_state_dict(0), "spread" = states()["spread"].
# The seeds were searched (a few thousand per large case) for inputs that meet the conditions
# tests/test_disc_model.py asserts: no pooled plane near a tie, no PReLU input within fp32 noise of zero.
CASES = [
    ("min_T16", 2, 16, 201, "default", 1581),
    ("min_T16", 2, 16, 201, "spread", 1532),
    ("odd_T31", 3, 31, 201, "spread", 1173),
    ("b1_T46", 1, 46, 201, "spread", 1234),
    ("chunked_B9_T177", 9, 177, 201, "default", 43685),
    ("chunked_B9_T177", 9, 177, 201, "spread", 39596),
    ("batch65_T16", 65, 16, 201, "spread", 28827),
    ("trainer_B4_T321", 4, 321, 201, "spread", 47988),
    ("F601_T33", 2, 33, 601, "spread", 1049),
]
CHUNKED = CASES[5]
ZERO_ROW = ("zero_row_T31", 3, 31, 201, "spread", 310)      # row 1 of the batch is all zeros


def case_id(case):
    return f"{case[0]}-{case[4]}"


@functools.lru_cache(maxsize=None)
def states():
    """"default": cmgan_amd.synth.discriminator_state_dict(0) (slopes 0.25 +- 0.05, gains 1 +- 0.1).  "spread": seed 1
    with PReLU slopes in [-0.3, 0.9], InstanceNorm gains in +-[0.4, 1.8] and biases in [-0.6, 0.6], far from the initial
    values where dalpha / dgamma / dbeta have special cases (slope sign, gain sign, bias 0)."""
    from cmgan_amd.synth import discriminator_state_dict
    spread = dict(discriminator_state_dict(1))
    rng = np.random.Generator(np.random.PCG64(4242))
    for i in range(4):
        c = CH[i + 1]
        gain = rng.uniform(0.4, 1.8, c) * np.where(rng.uniform(size=c) < 0.25, -1.0, 1.0)
        spread[f"layers.{3 * i + 1}.weight"] = torch.from_numpy(gain.astype(np.float32))
        spread[f"layers.{3 * i + 1}.bias"] = torch.from_numpy(rng.uniform(-0.6, 0.6, c).astype(np.float32))
        spread[f"layers.{3 * i + 2}.weight"] = torch.from_numpy(rng.uniform(-0.3, 0.9, c).astype(np.float32))
    spread["layers.16.weight"] = torch.from_numpy(rng.uniform(-0.3, 0.9, 64).astype(np.float32))
    return {"default": dict(discriminator_state_dict(0)), "spread": spread}


def inputs(case):
    """(xy [B,T,F,2] = |N(0,1)|, keep-mask [B,64] in {0, 1/0.7}, dscore [B] ~ N(0,1)), float32, from the case's seed."""
    _, B, T, F_, _, seed = case
    rng = np.random.Generator(np.random.PCG64(seed))
    xy = np.abs(rng.standard_normal((B, T, F_, 2))).astype(np.float32)
    mask = ((rng.uniform(size=(B, 64)) >= 0.3).astype(np.float32) / np.float32(0.7)).astype(np.float32)
    dscore = rng.standard_normal(B).astype(np.float32)
    if case[0].startswith("zero_row"):
        xy[1] = 0.0
    return torch.from_numpy(xy), torch.from_numpy(mask), torch.from_numpy(dscore)


def case_taps32(case):
    """The PReLU inputs of the case's train-mode forward in fp32 (forward only)."""
    st = {k: v.detach().clone() for k, v in states()[case[4]].items()}
    xy, mask, _ = inputs(case)
    taps = {}
    with torch.no_grad():
        _forward(st, xy.permute(0, 3, 2, 1), mask, True, taps)
    return taps


@functools.lru_cache(maxsize=None)
def case_reference(case, dtype=torch.float64):
    """reference() of a case: computed once per process, shared by every test that needs it, never modified."""
    return reference(states()[case[4]], *inputs(case), dtype=dtype)


# ---- the quantities every comparison looks at ----------------------------------------------------------------------------
def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def border(dxy):
    """dxy [B,T,F,2] at t in {0, T-1} or f in {0, F-1}, as one vector."""
    T, F_ = dxy.shape[1], dxy.shape[2]
    m = torch.zeros(T, F_, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return dxy[:, m]


def errors(got, want):
    """{quantity: max|got - want| / max|want|} of two reference()-shaped results."""
    e = {"score": rel(got["score"], want["score"]), "score_eval": rel(got["score_eval"], want["score_eval"]),
         "dx": rel(got["dxy"][..., 0], want["dxy"][..., 0]), "dy": rel(got["dxy"][..., 1], want["dxy"][..., 1]),
         "border": rel(border(got["dxy"].cpu()), border(want["dxy"].cpu()))}
    for k, v in want["buffers"].items():
        e[k] = rel(got["buffers"][k], v)
    for k, v in want["grads"].items():
        e["grad " + k] = rel(got["grads"][k], v)
    return e


FLOOR_FACTOR, BAR_MIN = 8.0, 2e-6


def bar(floor):
    """8 x the fp32 floor (a different but equally long summation order), no tighter than 2e-6."""
    return max(FLOOR_FACTOR * floor, BAR_MIN)


def main():
    """The fp32 floors: the same graph in fp32 torch on the CPU against the float64 reference, per case and quantity."""
    torch.manual_seed(0)
    print("FLOORS = {")
    for case in CASES + [ZERO_ROW]:
        want = case_reference(case)
        e = errors(case_reference(case, torch.float32), want)
        if case is ZERO_ROW:
            e = {k: e[k] for k in ("score", "score_eval")}
        worst = max(e.values())
        print(f"    # {case_id(case)}: B, T, F = {case[1:4]}, seed {case[5]}, pool margin "
              f"{pool_margin(want['taps']['a4']):.1e}, kink ratio {min(kink_ratios(want['taps'], case_taps32(case))):.1f},")
        print(f"    # worst floor {worst:.1e} ({max(e, key=e.get)}) -> bar {bar(worst):.1e}")
        print(f"    {case_id(case)!r}: {{")
        items = [f"{k!r}: {v:.2e}" for k, v in e.items()]
        for i in range(0, len(items), 3):
            print("        " + ", ".join(items[i:i + 3]) + ",")
        print("    },")
    print("}")


if __name__ == "__main__":
    main()
