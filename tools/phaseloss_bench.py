"""The phase loss on the GPU against the bytes it has to move, beside the auxiliary losses and the training step it joins
(cmgan_phase_loss / Engine.phase_loss; Engine.aux_loss in the same session; generator_train_step with and without the phase
weights).

    python tools/phaseloss_bench.py [--batch 32] [--seconds 2] [--iters 20] [--repeats 7] [--step-iters 2] [--limit 400] [--out PATH]

Prints one JSON line (and writes it to --out when one is given: profiles/r31_phaseloss_bench.json was written by passing
--out).  Two cases at 16 kHz, each isolated under --limit seconds with its calls timed alternately (tools/benchlib.py):
"phase": the compressed spectra of --batch pairs of --seconds s (the clips of tools/stretch_bench.py, the estimate with white
noise at 10 dB SNR, its spectrum turned by 0.1 rad; T = 321 frames of F = 201 bins at 2 s): device ms per Engine.phase_loss
call with the gradient and for the values alone, and per Engine.aux_loss call with the gradient at (512, 1024, 2048) on the waveforms; every kernel's time in the
call with a gradient from the library's own event pairs (median of 9 calls); the bytes the call has to move - 16 in and 8 out
per cell, 16 in for the values alone - against the 6.3 TB/s a streaming kernel reaches on this part, as a fraction; and the
device's gradient of pair 0 against the long-double model of tests/phaseloss_model.py by its acceptance rule.  "step":
generator_train_step (eager, dropout drawn, optimiser included) at the same batch without aux and with the three phase weights,
alternately."""
import argparse
import os
import statistics
import sys

import benchlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS = 16000
FULL = (512, 1024, 2048)
KERNELS = ("pl_terms", "pl_fold", "pl_total", "pl_grad")
WEIGHTS = (0.3, 0.2, 0.1)
FLOOR = 1e-3
HBM_TBPS = 6.3                     # what a streaming kernel reaches on an MI355X (of 8.0 on paper)


def _pairs(B, L, seconds):
    import numpy as np
    from stretch_bench import clips
    ref = clips(B, L, seconds).astype(np.float32)
    noise = np.random.default_rng(seconds).standard_normal((B, L))
    noise *= np.sqrt(np.mean(ref.astype(np.float64) ** 2, axis=1, keepdims=True)) * 10.0 ** (-10.0 / 20.0)
    return (ref + noise).astype(np.float32), ref


def case_phase(B, seconds, iters, repeats):
    import numpy as np
    import torch
    import phaseloss_model as M
    from cmgan_amd.engine import Engine

    eng = Engine()
    dev = eng.device
    L = seconds * FS
    e, r = _pairs(B, L, seconds)
    noisy, clean = torch.from_numpy(e).to(dev), torch.from_numpy(r).to(dev)
    c = eng.rms_scale(noisy)
    est_spec, clean_spec = eng.stft_compress(noisy, c), eng.stft_compress(clean, c)
    # a stand-in for the network's output: the noisy spectrum turned by 0.1 rad, so that bins 0 and F - 1, which are real in
    # any STFT, are not real in the estimate (an angle difference of exactly pi is a tie of the wrap, where a long-double model
    # and a float64 kernel may differ and the model's margin is 0; the clean spectrum keeps its real bins)
    co, si = float(np.cos(0.1)), float(np.sin(0.1))
    est_real = (co * est_spec[:, 0:1] - si * est_spec[:, 1:2]).contiguous()
    est_imag = (si * est_spec[:, 0:1] + co * est_spec[:, 1:2]).contiguous()
    T, F = int(clean_spec.shape[2]), int(clean_spec.shape[3])
    est_audio, target = noisy * c[:, None], clean * c[:, None]
    calls = {"phase_grad": lambda: eng.phase_loss(est_real, est_imag, clean_spec, *WEIGHTS, FLOOR),
             "phase_values": lambda: eng.phase_loss(est_real, est_imag, clean_spec, *WEIGHTS, FLOOR, grad=False),
             "aux_grad_512_1024_2048": lambda: eng.aux_loss(est_audio, target, FULL, 1.0, 0.05)}
    ms = benchlib.alternate(calls, iters, repeats, warmup=3)
    cells = B * T * F
    row = {"case": "phase", "shape": f"{B}x{seconds}s", "frames": T, "bins": F, "cells": cells,
           "workspace_kb": round(int(eng.lib.cmgan_phase_loss_workspace_bytes(None, B, T)) / 1024, 1)}
    for k in calls:
        s = benchlib.summary(ms[k])
        row.update({f"{k}_ms_per_call": s[0], f"{k}_ms_min": s[1], f"{k}_ms_max": s[2]})
    seen = {k: [] for k in KERNELS}
    for _ in range(9):
        eng.set_profiling(True)
        calls["phase_grad"]()
        once = {k: 0.0 for k in KERNELS}
        for name, t in eng.profile():
            if name in once:
                once[name] += t
        for k in KERNELS:
            seen[k].append(once[k])
    eng.set_profiling(False)
    kern = {k: statistics.median(v) for k, v in seen.items()}
    row["kernel_ms"] = {k: round(v, 4) for k, v in kern.items()}
    # the yardstick: the bytes that have to move, at the rate a streaming kernel reaches
    for name, per_cell, t_ms in (("phase_grad", 24, statistics.median(ms["phase_grad"])),
                                 ("phase_values", 16, statistics.median(ms["phase_values"])),
                                 ("pl_terms_kernel", 16, kern["pl_terms"]), ("pl_grad_kernel", 24, kern["pl_grad"])):
        floor_ms = cells * per_cell / (HBM_TBPS * 1e12) * 1e3
        row[f"{name}_bytes_floor_ms"] = round(floor_ms, 4)
        row[f"{name}_fraction_of_hbm_rate"] = round(floor_ms / t_ms, 3) if t_ms > 0 else None
    row["atan2_per_s_e9"] = round(2 * cells * (9 / 8 + 10 / 8) / ((kern["pl_terms"] + kern["pl_grad"]) * 1e-3) / 1e9, 1)
    out = calls["phase_grad"]()
    k3 = tuple(w / B for w in WEIGHTS)
    rows0 = [x.cpu().numpy() for x in (est_real[0, 0], est_imag[0, 0], clean_spec[0, 0], clean_spec[0, 1])]
    m = M.evaluate(*rows0, k3, FLOOR, M.LD)
    ok, frac = M.accept(out.g_real[0, 0].cpu().numpy(), out.g_imag[0, 0].cpu().numpy(), m)
    row.update({"pair0_gradient_accepted": ok, "pair0_worst_excess_over_half_ulp_in_E": round(frac, 4),
                "pair0_values": [round(float(v), 6) for v in out.rows[0]], "pair0_counts": [int(v) for v in out.counts[0]],
                "pair0_counts_equal_model": [int(v) for v in out.counts[0]] == [int(v) for v in m.counts],
                "pair0_value_error_u_pi": round(float(np.max(np.abs(out.rows[0].cpu().numpy().astype(M.LD) - m.values)))
                                                / (M.U * np.pi), 3),
                "pair0_branch_margin": float(m.branch_margin), "pair0_floor_margin": float(m.floor_margin),
                "rows_with_a_status": int(np.count_nonzero(out.status.cpu().numpy())),
                "mcells_per_s": round(cells / (statistics.median(ms["phase_grad"]) * 1e-3) / 1e6, 1),
                "device": torch.cuda.get_device_name(0)})
    return row


def case_step(B, seconds, iters, repeats):
    import torch
    from cmgan_amd.training import AdamW, AuxLoss, GeneratorTrain, generator_train_step
    from cmgan_amd.synth import make_state_dict

    L = seconds * FS
    gen = GeneratorTrain(make_state_dict(seed=0), device="cuda:0")
    opt = AdamW(gen.engine, gen.param_bucket, gen.grad_bucket, lr=5e-4)
    e, r = _pairs(B, L, seconds)
    noisy, clean = torch.from_numpy(e).to(gen.engine.device), torch.from_numpy(r).to(gen.engine.device)
    aux = AuxLoss(w_ip=WEIGHTS[0], w_gd=WEIGHTS[1], w_iaf=WEIGHTS[2], phase_floor=FLOOR)
    tgen = torch.Generator(device=gen.engine.device).manual_seed(1)
    calls = {"step": lambda: generator_train_step(gen, opt, clean, noisy, generator=tgen),
             "step_phase": lambda: generator_train_step(gen, opt, clean, noisy, generator=tgen, aux=aux)}
    ms = benchlib.alternate(calls, iters, repeats, warmup=2)
    row = {"case": "step", "shape": f"{B}x{seconds}s"}
    for k in calls:
        s = benchlib.summary(ms[k])
        row.update({f"{k}_ms": s[0], f"{k}_ms_min": s[1], f"{k}_ms_max": s[2]})
    row["phase_adds_ms"] = round(statistics.median(ms["step_phase"]) - statistics.median(ms["step"]), 3)
    row["phase_adds_share"] = round(row["phase_adds_ms"] / statistics.median(ms["step"]), 4)
    row["device"] = torch.cuda.get_device_name(0)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step-iters", type=int, default=2)
    ap.add_argument("--limit", type=float, default=400.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, choices=("phase", "step"), help="(internal) run one case")
    a = ap.parse_args()
    if a.case == "phase":
        return benchlib.print_case(case_phase(a.batch, a.seconds, a.iters, a.repeats))
    if a.case == "step":
        return benchlib.print_case(case_step(a.batch, a.seconds, a.step_iters, a.repeats))
    rows, stopped = benchlib.run_cases(__file__, benchlib.flags(a, "batch", "seconds", "iters", "repeats", "step_iters"),
                                       [("phase", ("phase",)), ("step", ("step",))], a.limit)
    device, = benchlib.lift(rows, "device")
    line = {"metric": "phase_loss", "batch": a.batch, "fs": FS, "seconds": a.seconds, "weights": list(WEIGHTS), "floor": FLOOR,
            "aux_n_ffts": list(FULL), "hbm_rate_tb_per_s": HBM_TBPS, "iters": a.iters, "step_iters": a.step_iters,
            "repeats": a.repeats, "limit_s_per_case": a.limit, "device": device, "cases": rows, "stopped": stopped}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
