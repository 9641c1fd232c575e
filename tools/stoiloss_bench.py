"""The intelligibility loss on the GPU vs the host, beside the auxiliary losses and the training step it joins
(cmgan_stoi_loss / Engine.stoi_loss vs the float64 numpy model of tests/stoiloss_model.py on one host thread; Engine.aux_loss in
the same session; generator_train_step with and without w_stoi).

    python tools/stoiloss_bench.py [--batch 32] [--seconds 2] [--iters 20] [--repeats 7] [--step-iters 2] [--limit 400] [--out PATH]

Prints one JSON line (and writes it to --out when one is given: profiles/r30_stoiloss_bench.json was written by passing
--out).  Two cases at 16 kHz, each isolated under --limit seconds with its calls timed alternately (tools/benchlib.py):
"stoi": --batch pairs of --seconds s (the clips of tools/stretch_bench.py, the estimate with white noise at 10 dB SNR): device ms
per Engine.stoi_loss call for STOI and ESTOI, with the gradient and for the values alone, and per Engine.aux_loss call with the
gradient at (512, 1024, 2048); every kernel's share of the STOI call with a gradient from the library's own event pairs (median
of 9 calls); the seconds the host takes per pair for the float64 model of that call, and the device's gradient of pair 0 against
the long-double model in units of the model's E.  "step": generator_train_step (eager, dropout drawn, optimiser included) at the
same batch without aux and with AuxLoss(w_stoi=0.5), alternately."""
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
KERNELS = ("sl_tables", "sl_resample", "sl_level", "sl_keep", "sl_env", "sl_corr", "sl_finalize", "sl_total", "sl_env_grad",
           "sl_ola_grad", "sl_resample_grad")
W_STOI = 0.5


def _pairs(B, L, seconds):
    import numpy as np
    from stretch_bench import clips
    ref = clips(B, L, seconds).astype(np.float32)
    noise = np.random.default_rng(seconds).standard_normal((B, L))
    noise *= np.sqrt(np.mean(ref.astype(np.float64) ** 2, axis=1, keepdims=True)) * 10.0 ** (-10.0 / 20.0)
    return (ref + noise).astype(np.float32), ref


def case_stoi(B, seconds, iters, repeats):
    import numpy as np
    import torch
    import stoiloss_model as M
    from cmgan_amd.engine import Engine

    eng = Engine()
    dev = eng.device
    L = seconds * FS
    e, r = _pairs(B, L, seconds)
    est, ref = torch.from_numpy(e).to(dev), torch.from_numpy(r).to(dev)
    calls = {"stoi_grad": lambda: eng.stoi_loss(est, ref, W_STOI, False),
             "stoi_values": lambda: eng.stoi_loss(est, ref, W_STOI, False, grad=False),
             "estoi_grad": lambda: eng.stoi_loss(est, ref, W_STOI, True),
             "estoi_values": lambda: eng.stoi_loss(est, ref, W_STOI, True, grad=False),
             "aux_grad_512_1024_2048": lambda: eng.aux_loss(est, ref, FULL, 1.0, 0.05)}
    ms = benchlib.alternate(calls, iters, repeats, warmup=3)
    row = {"case": "stoi", "shape": f"{B}x{seconds}s", "samples_per_clip": L,
           "workspace_mb": round(int(eng.lib.cmgan_stoi_loss_workspace_bytes(None, B, L, FS)) / 2 ** 20, 1)}
    for k in calls:
        s = benchlib.summary(ms[k])
        row.update({f"{k}_ms_per_call": s[0], f"{k}_ms_min": s[1], f"{k}_ms_max": s[2]})
    seen = {k: [] for k in KERNELS}
    for _ in range(9):
        eng.set_profiling(True)
        calls["stoi_grad"]()
        once = {k: 0.0 for k in KERNELS}
        for name, t in eng.profile():
            if name in once:
                once[name] += t
        for k in KERNELS:
            seen[k].append(once[k])
    eng.set_profiling(False)
    kern = {k: statistics.median(v) for k, v in seen.items()}
    row["kernel_ms"] = {k: round(v, 4) for k, v in kern.items()}
    row["kernel_share"] = {k: round(v / sum(kern.values()), 3) for k, v in kern.items()}
    # the host: the float64 model (scipy.fft) of pair 0 on one thread, and the device's gradient of that pair against it
    key = M.register(("bench", B, L), e[0], r[0])
    M.evaluate(e[0][:8000], r[0][:8000], False, W_STOI / B)              # (imports, first-use costs)
    for name, extended in (("stoi", False), ("estoi", True)):
        t0 = time.perf_counter()
        M.evaluate(e[0], r[0], extended, W_STOI / B)
        row[f"host_model_{name}_s_per_pair"] = round(time.perf_counter() - t0, 4)
    med = statistics.median(ms["stoi_grad"])
    row["speedup_vs_host"] = round(row["host_model_stoi_s_per_pair"] * B * 1000.0 / med, 1)
    out = calls["stoi_grad"]()
    status = out.status.cpu().numpy()
    row["rows_with_a_status"] = int(np.count_nonzero(status))
    m = M.row_model(key, False, W_STOI / B)
    ok, frac = M.accept(out.grad[0].cpu().numpy(), m)
    row.update({"pair0_gradient_accepted": ok, "pair0_worst_excess_over_half_ulp_in_E": round(frac, 4),
                "pair0_stoi": round(float(out.rows[0, 0]), 6), "pair0_kept_frames": int(out.rows[0, 1]),
                "pair0_level_margin_db": round(m.level_margin, 6), "pair0_min_margin": float(m.min_margin),
                "msamples_per_s": round(B * L / (med * 1e-3) / 1e6, 1), "device": torch.cuda.get_device_name(0)})
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
    aux = AuxLoss(w_stoi=W_STOI)
    tgen = torch.Generator(device=gen.engine.device).manual_seed(1)
    calls = {"step": lambda: generator_train_step(gen, opt, clean, noisy, generator=tgen),
             "step_stoi": lambda: generator_train_step(gen, opt, clean, noisy, generator=tgen, aux=aux)}
    ms = benchlib.alternate(calls, iters, repeats, warmup=2)
    row = {"case": "step", "shape": f"{B}x{seconds}s"}
    for k in calls:
        s = benchlib.summary(ms[k])
        row.update({f"{k}_ms": s[0], f"{k}_ms_min": s[1], f"{k}_ms_max": s[2]})
    row["stoi_adds_ms"] = round(statistics.median(ms["step_stoi"]) - statistics.median(ms["step"]), 3)
    row["stoi_adds_share"] = round(row["stoi_adds_ms"] / statistics.median(ms["step"]), 4)
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
    ap.add_argument("--case", default=None, choices=("stoi", "step"), help="(internal) run one case")
    a = ap.parse_args()
    if a.case == "stoi":
        return benchlib.print_case(case_stoi(a.batch, a.seconds, a.iters, a.repeats))
    if a.case == "step":
        return benchlib.print_case(case_step(a.batch, a.seconds, a.step_iters, a.repeats))
    rows, stopped = benchlib.run_cases(__file__, benchlib.flags(a, "batch", "seconds", "iters", "repeats", "step_iters"),
                                       [("stoi", ("stoi",)), ("step", ("step",))], a.limit)
    device, = benchlib.lift(rows, "device")
    line = {"metric": "stoi_loss", "batch": a.batch, "fs": FS, "seconds": a.seconds, "w_stoi": W_STOI, "aux_n_ffts": list(FULL),
            "iters": a.iters, "step_iters": a.step_iters, "repeats": a.repeats, "limit_s_per_case": a.limit, "device": device,
            "cases": rows, "stopped": stopped, "host_threads": 1, "host_cpus_available": benchlib.host_cpus()}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
