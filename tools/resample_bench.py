"""Sample-rate conversion on the GPU vs the host (cmgan_resample / Engine.resample vs scipy.signal.resample_poly).

    python tools/resample_bench.py [--batch 32] [--seconds 2] [--iters 200] [--limit 120] [--out PATH]

Prints one JSON line (and writes it to --out): for 48 k -> 16 k, 44.1 k -> 16 k and 16 k -> 44.1 k on B clips of the given
length, each pair an isolated case under --limit seconds (tools/benchlib.py), device ms per Engine.resample call (one
measurement of `iters` calls after warm-up; a call is the table kernel plus the resampling kernel), the bytes the algorithm must move (input once + output once, float32) over that time as a
fraction of the 8 TB/s HBM peak, and the host's resample_poly seconds on the float64 copy of the same clips."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import benchlib  # noqa: E402

HBM_PEAK = 8.0e12            # bytes / s (spec)
PAIRS = [(48000, 16000), (44100, 16000), (16000, 44100)]


def run_case(B, seconds, iters, fs_in, fs_out):
    import numpy as np
    import torch
    from scipy import signal as sig
    from cmgan_amd.engine import Engine
    from cmgan_amd.resample import geometry

    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs the GPU")
    eng = Engine()
    L = int(fs_in * seconds)
    up, down, n_taps, _ = geometry(fs_in, fs_out)
    x = np.random.default_rng(fs_in).standard_normal((B, L)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    call = lambda: eng.resample(xd, fs_in, fs_out)
    dev_ms, = benchlib.alternate({"resample": call}, iters, 1, warmup=5)["resample"]
    y = call()
    x64 = x.astype(np.float64)
    sig.resample_poly(x64[:1], up, down, axis=-1)                                   # (builds scipy's taps once)
    t0 = time.perf_counter()
    want = sig.resample_poly(x64, up, down, axis=-1)
    host_s = time.perf_counter() - t0
    nbytes = 4 * (x.size + y.numel())
    err = float(np.max(np.abs(y.cpu().numpy().astype(np.float64) - want)) / np.max(np.abs(want)))
    return {"fs_in": fs_in, "fs_out": fs_out, "up": up, "down": down, "taps_per_output": -(-n_taps // up),
            "device_ms_per_call": benchlib.summary([dev_ms])[0], "bytes_moved": nbytes,
            "fraction_of_hbm_peak": round(nbytes / (dev_ms * 1e-3) / HBM_PEAK, 4),
            "host_resample_poly_s": round(host_s, 4), "speedup_vs_host": round(host_s * 1000.0 / dev_ms, 1),
            "max_err_over_peak_vs_host": err, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", nargs=2, type=int, default=None, metavar=("FS_IN", "FS_OUT"), help="(internal) run one case")
    a = ap.parse_args()
    if a.case is not None:
        return benchlib.print_case(run_case(a.batch, a.seconds, a.iters, *a.case))
    rows, stopped = benchlib.run_cases(__file__, benchlib.flags(a, "batch", "seconds", "iters"),
                                       [(f"{i} -> {o}", (i, o)) for i, o in PAIRS], a.limit)
    device, = benchlib.lift(rows, "device")
    line = {"metric": "resample", "batch": a.batch, "clip_s": a.seconds, "iters": a.iters, "hbm_peak_bytes_per_s": HBM_PEAK,
            "limit_s_per_case": a.limit, "pairs": rows, "stopped": stopped, "host_cpus": benchlib.host_cpus(), "device": device}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
