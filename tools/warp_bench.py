"""Speed perturbation on the GPU vs the host, and beside the call it precedes (cmgan_warp / Engine.warp vs
scipy.signal.resample_poly on one host thread; Engine.mix without a RIR).

    python tools/warp_bench.py [--batch 32] [--iters 100] [--repeats 7] [--host-clips 4] [--limit 120] [--out PATH]

Prints one JSON line (and writes it to --out when one is given: profiles/r14_warp_bench.json was written by passing
--out).  Two cases at 16 kHz: --batch clips of ceil(32000 x 1.1) samples warped to 32000 (2 s batches) and of
ceil(160000 x 1.1) warped to 160000 (10 s), one rate per row, uniform in 0.9 .. 1.1, zeros = 24, rolloff = 0.95.  Every
case runs isolated under --limit seconds and the calls are timed alternately (tools/benchlib.py).  Per case: device ms
per Engine.warp call (one launch) and per Engine.mix call without a RIR on the warped batch (the median and the spread of
`repeats` measurements of `iters` calls), the same warp with every rate at 1.0 and at 1.1 (the tap count follows the
rate), the seconds the host takes per clip for scipy.signal.resample_poly(x, 10, 11) in float64 - ONE fixed ratio, the
nearest thing the host has (timed on the first --host-clips clips) -, the taps per output, and a check of 256 outputs of
one row against the definition written out in float64 numpy (np.sinc, np.cos), in float32 ulps.

A/B of the tap recurrence against sinpi / cospi at every tap: build the other form side by side,
`cmgan_amd.build.build(variant="direct", extra_flags=["-DWARP_DIRECT_TRIG"])`, and run this tool alternately with and
without `CMGAN_HIP_LIB=cmgan_amd/lib/variants/direct/libcmgan_hip.so` in one session."""
import argparse
import math
import os
import statistics
import sys
import time

import benchlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS = 16000
HI = 1.1
ZEROS, ROLLOFF = 24, 0.95


def host_outputs(x, r, ns):
    """y[i] for the outputs ns of one row by the definition, float64 numpy (float64 [len(ns)])."""
    import numpy as np
    fc = ROLLOFF * (1.0 / r if r > 1.0 else 1.0)
    W = ZEROS / fc
    out = np.zeros(len(ns))
    for j, i in enumerate(ns):
        t = float(i) * r
        k = np.arange(max(0, int(math.floor(t - W)) - 1), min(len(x), int(math.ceil(t + W)) + 2))
        d = t - k
        h = np.where(np.abs(d) < W, fc * np.sinc(fc * d) * (0.5 + 0.5 * np.cos(np.pi * d / W)), 0.0)
        out[j] = float(np.sum(x[k].astype(np.float64) * h))
    return out


def run_case(B, seconds, iters, repeats, host_clips):
    import numpy as np
    import torch
    from scipy.signal import resample_poly
    from cmgan_amd import _lib
    from cmgan_amd.engine import Engine
    from cmgan_amd.mixing import warp_len

    if not torch.cuda.is_available():
        raise SystemExit("warp_bench needs the GPU")
    eng = Engine()
    dev = eng.device
    tile = int(_lib.load().cmgan_warp_tile())
    L = math.ceil(seconds * FS * HI)
    N = warp_len(L, HI)
    rng = np.random.default_rng(seconds)
    x = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    rate_np = rng.uniform(0.9, 1.1, B)
    wav = torch.from_numpy(x).to(dev)
    rate = torch.from_numpy(rate_np).to(dev)
    ones = torch.ones(B, dtype=torch.float64, device=dev)
    fast = torch.full((B,), HI, dtype=torch.float64, device=dev)
    out = torch.empty(B, N, dtype=torch.float32, device=dev)
    scratch = torch.empty_like(out)
    beside = benchlib.mix_beside(rng, B, dev)
    calls = {"warp": lambda: eng.warp(wav, rate, N, zeros=ZEROS, rolloff=ROLLOFF, out=out),
             "warp_rate_1": lambda: eng.warp(wav, ones, N, zeros=ZEROS, rolloff=ROLLOFF, out=scratch),
             "warp_rate_1p1": lambda: eng.warp(wav, fast, N, zeros=ZEROS, rolloff=ROLLOFF, out=scratch),
             "mix": lambda: eng.mix(out, *beside)}
    ms = benchlib.alternate(calls, iters, repeats, warmup=3)
    got, n_out, status = (t.cpu().numpy() for t in eng.warp(wav, rate, N, zeros=ZEROS, rolloff=ROLLOFF, info=True))
    n_host = max(1, min(host_clips, B))
    resample_poly(x[0, :2000].astype(np.float64), 10, 11)             # (imports, first-use costs)
    t0 = time.perf_counter()
    for b in range(n_host):
        resample_poly(x[b].astype(np.float64), 10, 11)
    host_s = (time.perf_counter() - t0) / n_host
    ns = np.arange(N // 2, N // 2 + 256)
    want = host_outputs(x[0], float(rate_np[0]), ns).astype(np.float32)
    ulps = float(np.max(np.abs(got[0, ns].astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want))))
    med = {k: statistics.median(v) for k, v in ms.items()}
    wp, mx = benchlib.summary(ms["warp"]), benchlib.summary(ms["mix"])
    fc = ROLLOFF / np.maximum(rate_np, 1.0)
    taps = float(np.mean(2.0 * ZEROS / fc))
    return {"case": f"{B}x{seconds}s", "samples_in_per_clip": L, "samples_out_per_clip": N, "tiles_per_clip": -(-N // tile),
            "warp_ms_per_call": wp[0], "warp_ms_min": wp[1], "warp_ms_max": wp[2],
            "warp_rate_1_ms_per_call": benchlib.summary(ms["warp_rate_1"])[0],
            "warp_rate_1p1_ms_per_call": benchlib.summary(ms["warp_rate_1p1"])[0],
            "mix_no_rir_ms_per_call": mx[0], "mix_ms_min": mx[1], "mix_ms_max": mx[2],
            "warp_over_mix": round(med["warp"] / med["mix"], 3),
            "msamples_out_per_s": round(B * N / (med["warp"] * 1e-3) / 1e6, 1), "mean_taps_per_output": round(taps, 1),
            "gtaps_per_s": round(B * N * taps / (med["warp"] * 1e-3) / 1e9, 1),
            "host_resample_poly_s_per_clip": round(host_s, 5), "host_clips_timed": n_host,
            "host_ms_per_batch": round(host_s * B * 1000.0, 2), "speedup_vs_host": round(host_s * B * 1000.0 / med["warp"], 1),
            "rows_full": bool((n_out == N).all()), "rows_valid": bool((status == 0).all()),
            "max_ulps_vs_f32_of_host_definition": ulps, "device": torch.cuda.get_device_name(0), "tile": tile}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-clips", type=int, default=4)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", type=int, default=None, metavar="SECONDS", help="(internal) run one case")
    a = ap.parse_args()
    if a.case is not None:
        return benchlib.print_case(run_case(a.batch, a.case, a.iters, a.repeats, a.host_clips))
    rows, stopped = benchlib.run_cases(__file__, benchlib.flags(a, "batch", "iters", "repeats", "host_clips"),
                                       [(f"{sec}s", (sec,)) for sec in (2, 10)], a.limit)
    line = {"metric": "warp", "batch": a.batch, "fs": FS, "rates": [0.9, 1.1], "zeros": ZEROS, "rolloff": ROLLOFF,
            "launches_per_call": 1, "iters": a.iters, "repeats": a.repeats, "limit_s_per_case": a.limit, "cases": rows,
            "stopped": stopped, "host_threads": 1, "host_cpus_available": benchlib.host_cpus()}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
