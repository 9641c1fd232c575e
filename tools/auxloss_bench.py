"""The auxiliary losses on the GPU vs the host, and beside the training step they join (cmgan_aux_loss / Engine.aux_loss vs
the float64 numpy model of tests/auxloss_model.py on one host thread; generator_train_step with and without aux=).

    python tools/auxloss_bench.py [--batch 32] [--seconds 2] [--iters 20] [--repeats 7] [--step-iters 2] [--limit 400] [--out PATH]

Prints one JSON line (and writes it to --out when one is given: profiles/r29_auxloss_bench.json was written by passing
--out).  Two cases at 16 kHz, each isolated under --limit seconds with its calls timed alternately (tools/benchlib.py):
"aux": --batch pairs of --seconds s (the clips of tools/stretch_bench.py, the estimate with white noise at 10 dB SNR): device ms
per Engine.aux_loss call with the gradient at (512, 1024, 2048) and at (1024,), and for the values alone; every kernel's
share of the first from the library's own event pairs (median of 9 calls); the seconds the host takes per pair for the
float64 model of the same call, and the device's gradient of that pair against it in units of the model's E.  "step":
generator_train_step (eager, dropout drawn, optimiser included) at the same batch without aux and with
AuxLoss((512, 1024, 2048), w_mr=1, w_si=0.05), alternately."""
import argparse
import os
import statistics
import sys
import time

import benchlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS = 16000
FULL = (512, 1024, 2048)
KERNELS = ("aux_spectra", "aux_si_part", "aux_fold", "aux_total", "aux_grad", "aux_join")
W_MR, W_SI = 1.0, 0.05


def _pairs(B, L, seconds):
    import numpy as np
    from stretch_bench import clips
    ref = clips(B, L, seconds).astype(np.float32)
    noise = np.random.default_rng(seconds).standard_normal((B, L))
    noise *= np.sqrt(np.mean(ref.astype(np.float64) ** 2, axis=1, keepdims=True)) * 10.0 ** (-10.0 / 20.0)
    return (ref + noise).astype(np.float32), ref


def case_aux(B, seconds, iters, repeats):
    import numpy as np
    import torch
    import auxloss_model as M
    from cmgan_amd.engine import Engine, aux_loss_workspace_bytes

    eng = Engine()
    dev = eng.device
    L = seconds * FS
    e, r = _pairs(B, L, seconds)
    est, ref = torch.from_numpy(e).to(dev), torch.from_numpy(r).to(dev)
    calls = {"grad_512_1024_2048": lambda: eng.aux_loss(est, ref, FULL, W_MR, W_SI),
             "grad_1024": lambda: eng.aux_loss(est, ref, (1024,), W_MR, W_SI),
             "values_512_1024_2048": lambda: eng.aux_loss(est, ref, FULL, W_MR, W_SI, grad=False)}
    ms = benchlib.alternate(calls, iters, repeats, warmup=3)
    row = {"case": "aux", "shape": f"{B}x{seconds}s", "samples_per_clip": L,
           "workspace_mb": round(aux_loss_workspace_bytes(B, L, FULL) / 2 ** 20, 1)}
    for k in calls:
        s = benchlib.summary(ms[k])
        row.update({f"{k}_ms_per_call": s[0], f"{k}_ms_min": s[1], f"{k}_ms_max": s[2]})
    seen = {k: [] for k in KERNELS}
    for _ in range(9):
        eng.set_profiling(True)
        calls["grad_512_1024_2048"]()
        once = {k: 0.0 for k in KERNELS}
        for name, t in eng.profile():
            if name in once:
                once[name] += t                                         # (a launch per resolution)
        for k in KERNELS:
            seen[k].append(once[k])
    eng.set_profiling(False)
    kern = {k: statistics.median(v) for k, v in seen.items()}
    row["kernel_ms"] = {k: round(v, 4) for k, v in kern.items()}
    row["kernel_share"] = {k: round(v / sum(kern.values()), 3) for k, v in kern.items()}
    # the host: the float64 model (scipy.fft) of pair 0 on one thread, and the device's gradient of that pair against it
    key = M.register(("bench", B, L), e[0], r[0])
    M.resolution(e[0][:4096], r[0][:4096], 512)                          # (imports, first-use costs)
    t0 = time.perf_counter()
    for n in FULL:
        M.resolution(e[0], r[0], n)
    M.si_sdr(e[0], r[0])
    row["host_model_s_per_pair"] = round(time.perf_counter() - t0, 4)
    med = statistics.median(ms["grad_512_1024_2048"])
    row["speedup_vs_host"] = round(row["host_model_s_per_pair"] * B * 1000.0 / med, 1)
    m = M.row_model(key, FULL, W_MR / B, W_SI / B)
    out = calls["grad_512_1024_2048"]()
    ok, frac = M.accept(out.grad[0].cpu().numpy(), m)
    row.update({"pair0_gradient_accepted": ok, "pair0_worst_excess_over_half_ulp_in_E": round(frac, 4),
                "pair0_si_sdr_db": round(float(out.rows[0, -1]), 3), "msamples_per_s": round(B * L / (med * 1e-3) / 1e6, 1),
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
    aux = AuxLoss(FULL, w_mr=W_MR, w_si=W_SI)
    tgen = torch.Generator(device=gen.engine.device).manual_seed(1)
    calls = {"step": lambda: generator_train_step(gen, opt, clean, noisy, generator=tgen),
             "step_aux": lambda: generator_train_step(gen, opt, clean, noisy, generator=tgen, aux=aux)}
    ms = benchlib.alternate(calls, iters, repeats, warmup=2)
    row = {"case": "step", "shape": f"{B}x{seconds}s"}
    for k in calls:
        s = benchlib.summary(ms[k])
        row.update({f"{k}_ms": s[0], f"{k}_ms_min": s[1], f"{k}_ms_max": s[2]})
    row["aux_adds_ms"] = round(statistics.median(ms["step_aux"]) - statistics.median(ms["step"]), 3)
    row["aux_adds_share"] = round(row["aux_adds_ms"] / statistics.median(ms["step"]), 4)
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
    ap.add_argument("--case", default=None, choices=("aux", "step"), help="(internal) run one case")
    a = ap.parse_args()
    if a.case == "aux":
        return benchlib.print_case(case_aux(a.batch, a.seconds, a.iters, a.repeats))
    if a.case == "step":
        return benchlib.print_case(case_step(a.batch, a.seconds, a.step_iters, a.repeats))
    rows, stopped = benchlib.run_cases(__file__, benchlib.flags(a, "batch", "seconds", "iters", "repeats", "step_iters"),
                                       [("aux", ("aux",)), ("step", ("step",))], a.limit)
    device, = benchlib.lift(rows, "device")
    line = {"metric": "aux_loss", "batch": a.batch, "fs": FS, "seconds": a.seconds, "n_ffts": list(FULL), "w_mr": W_MR, "w_si": W_SI,
            "iters": a.iters, "step_iters": a.step_iters, "repeats": a.repeats, "limit_s_per_case": a.limit, "device": device,
            "cases": rows, "stopped": stopped, "host_threads": 1, "host_cpus_available": benchlib.host_cpus()}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
