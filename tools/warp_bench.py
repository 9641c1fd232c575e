"""Speed perturbation on the GPU vs the host, and beside the call it precedes (cmgan_warp / Engine.warp vs
scipy.signal.resample_poly on one host thread; Engine.mix without a RIR).

    python tools/warp_bench.py [--batch 32] [--iters 100] [--repeats 7] [--host-clips 4] [--limit 120] [--out PATH]

Prints one JSON line (and writes it to --out, default profiles/r14_warp_bench.json).  Two cases at 16 kHz: --batch clips
of ceil(32000 x 1.1) samples warped to 32000 (2 s batches) and of ceil(160000 x 1.1) warped to 160000 (10 s), one rate
per row, uniform in 0.9 .. 1.1, zeros = 24, rolloff = 0.95.  Every case runs in a process of its own under a time limit
of --limit seconds; after a case that fails or runs out of time no further case is started.  Per case: device ms per
Engine.warp call (one launch) and per Engine.mix call without a RIR on the warped batch (HIP events around `iters` calls
after a warm-up; the two are measured alternately, `repeats` times each, and the median and the spread are reported), the
same warp with every rate at 1.0 and at 1.1 (the tap count follows the rate), the seconds the host takes per clip for
scipy.signal.resample_poly(x, 10, 11) in float64 - ONE fixed ratio, the nearest thing the host has (timed on the first
--host-clips clips) -, the taps per output, and a check of 256 outputs of one row against the definition written out in
float64 numpy (np.sinc, np.cos), in float32 ulps.

A/B of the tap recurrence against sinpi / cospi at every tap: build the other form side by side,
`cmgan_amd.build.build(variant="direct", extra_flags=["-DWARP_DIRECT_TRIG"])`, and run this tool alternately with and
without `CMGAN_HIP_LIB=cmgan_amd/lib/variants/direct/libcmgan_hip.so` in one session."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

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
    bank = torch.from_numpy((0.1 * rng.standard_normal(10 * FS)).astype(np.float32)).to(dev)
    start = torch.zeros(B, dtype=torch.int64, device=dev)
    length = torch.full((B,), bank.numel(), dtype=torch.int64, device=dev)
    off = torch.arange(B, dtype=torch.int64, device=dev) * 977
    snr = torch.linspace(0.0, 20.0, B, dtype=torch.float32, device=dev)
    calls = {"warp": lambda: eng.warp(wav, rate, N, zeros=ZEROS, rolloff=ROLLOFF, out=out),
             "warp_rate_1": lambda: eng.warp(wav, ones, N, zeros=ZEROS, rolloff=ROLLOFF, out=scratch),
             "warp_rate_1p1": lambda: eng.warp(wav, fast, N, zeros=ZEROS, rolloff=ROLLOFF, out=scratch),
             "mix": lambda: eng.mix(out, bank, start, length, off, snr)}

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for _ in range(3):
        for c in calls.values():
            c()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(repeats):                                          # alternately: all see the same machine
        for k, c in calls.items():
            ms[k].append(timed(c))
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
    fc = ROLLOFF / np.maximum(rate_np, 1.0)
    taps = float(np.mean(2.0 * ZEROS / fc))
    return {"case": f"{B}x{seconds}s", "samples_in_per_clip": L, "samples_out_per_clip": N, "tiles_per_clip": -(-N // tile),
            "warp_ms_per_call": round(med["warp"], 4), "warp_ms_min": round(min(ms["warp"]), 4),
            "warp_ms_max": round(max(ms["warp"]), 4), "warp_rate_1_ms_per_call": round(med["warp_rate_1"], 4),
            "warp_rate_1p1_ms_per_call": round(med["warp_rate_1p1"], 4),
            "mix_no_rir_ms_per_call": round(med["mix"], 4), "mix_ms_min": round(min(ms["mix"]), 4),
            "mix_ms_max": round(max(ms["mix"]), 4), "warp_over_mix": round(med["warp"] / med["mix"], 3),
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_warp_bench.json"))
    ap.add_argument("--case", type=int, default=None, metavar="SECONDS", help="(internal) run one case")
    a = ap.parse_args()
    if a.case is not None:
        print("CASE " + json.dumps(run_case(a.batch, a.case, a.iters, a.repeats, a.host_clips)))
        return
    rows, stopped = [], None
    for seconds in (2, 10):
        cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--iters", str(a.iters), "--repeats",
               str(a.repeats), "--host-clips", str(a.host_clips), "--case", str(seconds)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            stopped = f"{seconds}s: no result within {a.limit} s"
            break
        line = next((l for l in r.stdout.splitlines() if l.startswith("CASE ")), None)
        if r.returncode != 0 or line is None:
            stopped = f"{seconds}s: exit status {r.returncode}: {r.stderr.strip()[-400:]}"
            break
        rows.append(json.loads(line[5:]))
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    line = {"metric": "warp", "batch": a.batch, "fs": FS, "rates": [0.9, 1.1], "zeros": ZEROS, "rolloff": ROLLOFF,
            "launches_per_call": 1, "iters": a.iters, "repeats": a.repeats, "limit_s_per_case": a.limit, "cases": rows,
            "stopped": stopped, "host_threads": 1, "host_cpus_available": cpus}
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")
    if stopped:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
