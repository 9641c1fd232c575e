"""The noise suppressor on the GPU vs the host, and beside the calls around it (cmgan_suppress / Engine.suppress vs the
float64 numpy model of tests/suppress_model.py on one host thread; Engine.mix without a RIR; Engine.channel at 4 sections,
which it follows in DynamicMixer).

    python tools/suppress_bench.py [--batch 32] [--iters 50] [--repeats 7] [--host-clips 1] [--limit 300] [--out PATH]

Prints one JSON line (and writes it to --out when one is given: profiles/r28_suppress_bench.json was written by passing
--out).  Two cases at 16 kHz: --batch clips of 2 s and of 10 s (the clips of tools/stretch_bench.py plus white noise at
-26 dB), n_fft 512, a minimum window of 1 s (62 frames), floor -20 dB, bias 1.5, a_dd 0.98, a_n 0.8.  Every case runs isolated
under --limit seconds and the calls are timed alternately (tools/benchlib.py).  Per case: device ms per Engine.suppress
call for each rule without and with a key (the median and the spread of `repeats` measurements of `iters` calls; a call is
its three launches), Engine.mix without a RIR and Engine.channel with 4 sections per row on the same batch, the three
kernels of a call of each rule from the library's own event pairs (median of 9 calls), what a step of the gain chain costs
and how much of it is E1 (the log-MMSE chain minus the Wiener chain, per frame), the DynamicMixer call without and with
suppressor=SuppressorSampler(p=1), the seconds the host takes per clip for the float64 model (timed on the first
--host-clips clips), and a check of those clips: the samples in float32 ulps of the model's."""
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
N_FFT = 512
RULES = ("wiener", "specsub", "logmmse")
KERNELS = ("suppress_analyse", "suppress_gain", "suppress_synth")


def run_case(B, seconds, iters, repeats, host_clips):
    import numpy as np
    import torch
    import suppress_model as M
    from dynamics_bench import sections
    from stretch_bench import clips
    from cmgan_amd.engine import Engine, suppress_frames
    from cmgan_amd.mixing import DynamicMixer, NoiseBank, SuppressorSampler, suppress_params

    if not torch.cuda.is_available():
        raise SystemExit("suppress_bench needs the GPU")
    eng = Engine()
    dev = eng.device
    L = seconds * FS
    T = suppress_frames(L, N_FFT)
    rng = np.random.default_rng(seconds)
    x = (clips(B, L, seconds) + 0.05 * rng.standard_normal((B, L))).astype(np.float32)
    wav = torch.from_numpy(x).to(dev)
    key = torch.from_numpy((x + 0.01 * rng.standard_normal((B, L))).astype(np.float32)).to(dev)
    table = {r: suppress_params(r, fs=FS, n_fft=N_FFT).reshape(1, 7).repeat(B, 1).contiguous().to(dev) for r in RULES}
    sos = torch.from_numpy(sections(B)).to(dev)
    out = torch.empty_like(wav)
    beside = benchlib.mix_beside(rng, B, dev)
    calls = {}
    for r in RULES:
        calls[r] = lambda r=r: eng.suppress(wav, table[r], N_FFT, out=out)
        calls[r + "_key"] = lambda r=r: eng.suppress(wav, table[r], N_FFT, key=key, out=out)
    calls["mix"] = lambda: eng.mix(wav, *beside)
    calls["channel"] = lambda: eng.channel(wav, sos, out=out)
    ms = benchlib.alternate(calls, iters, repeats, warmup=3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    row = {"case": f"{B}x{seconds}s", "samples_per_clip": L, "frames_per_clip": T, "bins": N_FFT // 2 + 1,
           "window_frames": int(table["wiener"][0, 3].item()), "gain_threads": B * (N_FFT // 2 + 1)}
    for k in calls:
        s = benchlib.summary(ms[k])
        row.update({f"{k}_ms_per_call": s[0], f"{k}_ms_min": s[1], f"{k}_ms_max": s[2],
                    f"{k}_spread": round((max(ms[k]) - min(ms[k])) / statistics.median(ms[k]), 4)})
    # the three kernels, from the library's own event pairs
    kernel = {}
    for r in RULES:
        seen = {k: [] for k in KERNELS}
        for _ in range(9):
            eng.set_profiling(True)
            eng.suppress(wav, table[r], N_FFT, out=out)
            for name, t in eng.profile():
                if name in seen:
                    seen[name].append(t)
        eng.set_profiling(False)
        kernel[r] = {k: round(statistics.median(v), 4) for k, v in seen.items()}
        row.update({f"{r}_{k}_ms": v for k, v in kernel[r].items()})
    chain = {r: kernel[r]["suppress_gain"] * 1e3 / T for r in RULES}
    row.update({"gain_us_per_frame_" + r: round(chain[r], 4) for r in RULES})
    row["e1_us_per_frame"] = round(chain["logmmse"] - chain["wiener"], 4)
    row["e1_share_of_the_logmmse_step"] = round((chain["logmmse"] - chain["wiener"]) / chain["logmmse"], 3)
    row["dominant_kernel_logmmse"] = max(KERNELS, key=lambda k: kernel["logmmse"][k])
    # the mixer call without and with the stage at p = 1 (host wall clock inside HIP events: the call's own tensor work included)
    bank = NoiseBank.from_arrays([(0.1 * rng.standard_normal(10 * FS)).astype(np.float32)], device=dev)
    clean = torch.from_numpy(clips(B, L, seconds)).to(dev)
    mixers = {"mixer_plain": DynamicMixer(eng, bank, None, early_ms=None),
              "mixer_suppressor": DynamicMixer(eng, bank, None, early_ms=None, suppressor=SuppressorSampler(p=1.0))}
    mm = benchlib.alternate({k: (lambda m=m: m(clean)) for k, m in mixers.items()}, max(iters // 5, 5), repeats, warmup=3)
    for k in mixers:
        s = benchlib.summary(mm[k])
        row.update({f"{k}_ms_per_call": s[0], f"{k}_ms_min": s[1], f"{k}_ms_max": s[2]})
    row["mixer_rules_drawn"] = sorted(set(mixers["mixer_suppressor"].last_suppression.table[:, 0].tolist()))
    # the host: the float64 model (scipy.fft) per clip on one thread, and the device's samples against it
    n_host = max(0, min(host_clips, B))
    host_s, ulps = {}, 0.0
    M._one(x[0, :3000], None, 3000, table["logmmse"][0].cpu().numpy(), N_FFT, np.float64, M.e1_d)     # (imports, first-use costs)
    for r in RULES:
        p = table[r][0].cpu().numpy()
        got = eng.suppress(wav, table[r], N_FFT).cpu().numpy()
        t0 = time.perf_counter()
        want = [M._one(x[b], None, L, p, N_FFT, np.float64, M.e1_d)[0] for b in range(n_host)]
        host_s[r] = round((time.perf_counter() - t0) / n_host, 5) if n_host else None
        for b, d in enumerate(want):
            y = d.astype(np.float32)
            err = np.abs(got[b].astype(np.float64) - y.astype(np.float64)) / np.spacing(np.maximum(np.abs(y), np.float32(1e-30)))
            ulps = max(ulps, float(np.max(err)))
    row.update({"suppress_over_mix": round(med["logmmse"] / med["mix"], 2), "suppress_over_channel": round(med["logmmse"] / med["channel"], 2),
                "msamples_per_s_logmmse": round(B * L / (med["logmmse"] * 1e-3) / 1e6, 1),
                "host_model_s_per_clip": host_s, "host_clips_timed": n_host,
                "speedup_vs_host_logmmse": None if not n_host else round(host_s["logmmse"] * B * 1000.0 / med["logmmse"], 1),
                "max_ulps_vs_f32_of_the_float64_model": ulps, "device": torch.cuda.get_device_name(0)})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-clips", type=int, default=1)
    ap.add_argument("--limit", type=float, default=300.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", type=int, default=None, metavar="SECONDS", help="(internal) run one case")
    a = ap.parse_args()
    if a.case is not None:
        return benchlib.print_case(run_case(a.batch, a.case, a.iters, a.repeats, a.host_clips))
    rows, stopped = benchlib.run_cases(__file__, benchlib.flags(a, "batch", "iters", "repeats", "host_clips"),
                                       [(f"{sec}s", (sec,)) for sec in (2, 10)], a.limit)
    device, = benchlib.lift(rows, "device")
    line = {"metric": "suppress", "batch": a.batch, "fs": FS, "n_fft": N_FFT, "rules": list(RULES), "window_s": 1.0, "floor_db": -20.0,
            "bias": 1.5, "a_dd": 0.98, "a_n": 0.8, "launches_per_call": 3, "iters": a.iters, "repeats": a.repeats,
            "limit_s_per_case": a.limit, "device": device, "cases": rows, "stopped": stopped, "host_threads": 1,
            "host_cpus_available": benchlib.host_cpus()}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
