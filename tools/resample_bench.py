"""Sample-rate conversion on the GPU vs the host (cmgan_resample / Engine.resample vs scipy.signal.resample_poly).

    python tools/resample_bench.py [--batch 32] [--seconds 2] [--iters 200] [--out PATH]

Prints one JSON line (and writes it to --out): for 48 k -> 16 k, 44.1 k -> 16 k and 16 k -> 44.1 k on B clips of the given
length, device ms per Engine.resample call (HIP events around `iters` calls after warm-up; a call is the table kernel
plus the resampling kernel), the bytes the algorithm must move (input once + output once, float32) over that time as a
fraction of the 8 TB/s HBM peak, and the host's resample_poly seconds on the float64 copy of the same clips."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12            # bytes / s (spec)
PAIRS = [(48000, 16000), (44100, 16000), (16000, 44100)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scipy import signal as sig
    from cmgan_amd.engine import Engine
    from cmgan_amd.resample import geometry

    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs the GPU")
    eng = Engine()
    rows = []
    for fs_in, fs_out in PAIRS:
        B, L = a.batch, int(fs_in * a.seconds)
        up, down, n_taps, _ = geometry(fs_in, fs_out)
        x = np.random.default_rng(fs_in).standard_normal((B, L)).astype(np.float32)
        xd = torch.from_numpy(x).cuda()
        for _ in range(5):
            y = eng.resample(xd, fs_in, fs_out)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            y = eng.resample(xd, fs_in, fs_out)
        e1.record()
        torch.cuda.synchronize()
        dev_ms = e0.elapsed_time(e1) / a.iters
        x64 = x.astype(np.float64)
        sig.resample_poly(x64[:1], up, down, axis=-1)                                   # (builds scipy's taps once)
        t0 = time.perf_counter()
        want = sig.resample_poly(x64, up, down, axis=-1)
        host_s = time.perf_counter() - t0
        nbytes = 4 * (x.size + y.numel())
        err = float(np.max(np.abs(y.cpu().numpy().astype(np.float64) - want)) / np.max(np.abs(want)))
        rows.append({"fs_in": fs_in, "fs_out": fs_out, "up": up, "down": down, "taps_per_output": -(-n_taps // up),
                     "device_ms_per_call": round(dev_ms, 4), "bytes_moved": nbytes,
                     "fraction_of_hbm_peak": round(nbytes / (dev_ms * 1e-3) / HBM_PEAK, 4),
                     "host_resample_poly_s": round(host_s, 4), "speedup_vs_host": round(host_s * 1000.0 / dev_ms, 1),
                     "max_err_over_peak_vs_host": err})
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    line = {"metric": "resample", "batch": a.batch, "clip_s": a.seconds, "iters": a.iters, "hbm_peak_bytes_per_s": HBM_PEAK,
            "pairs": rows, "host_cpus": cpus, "device": torch.cuda.get_device_name(0)}
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
