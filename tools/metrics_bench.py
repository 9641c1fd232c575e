"""Objective-metric scoring on the GPU vs the host (cmgan_metrics / Engine.metrics vs cmgan_amd.metrics).

    python tools/metrics_bench.py [--batch 32] [--seconds 2] [--iters 20] [--tracks 32] [--limit 120] [--out PATH]

Prints one JSON line, measured in one isolated case under --limit seconds (tools/benchlib.py): device ms per
Engine.metrics call on B clips of the given length at 16 kHz (one measurement of `iters` calls after warm-up), host compute_metrics seconds for the same clips (with the CPU count this process may use), and the wall time
of evaluation() on `tracks` synthetic wav pairs (random-init weights; a constant stub PESQ)."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import benchlib  # noqa: E402


FS = 16000


def clips(B, L, seed=0):
    """speech-like int16-scale clean clips and noisy / processed versions of them."""
    g = np.random.default_rng(seed)
    t = np.arange(L) / 16000.0
    clean = np.zeros((B, L))
    for b in range(B):
        f0 = g.uniform(90, 220)
        env = np.clip(np.sin(2 * np.pi * g.uniform(1.5, 4.0) * t + g.uniform(0, 6.28)), 0, None) ** 2
        clean[b] = sum(np.sin(2 * np.pi * k * f0 * t) / k for k in range(1, 20)) * env * 6000.0
    clean += g.standard_normal((B, L)) * 4.0
    proc = 0.95 * clean + g.standard_normal((B, L)) * 60.0
    return clean.astype(np.float32), proc.astype(np.float32)


def run_case(a):
    import torch
    from cmgan_amd import TSCNet
    from cmgan_amd import metrics as M
    from cmgan_amd.engine import Engine
    from cmgan_amd.evaluation import evaluation
    from cmgan_amd.synth import make_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs the GPU")
    B, L = a.batch, int(FS * a.seconds)
    clean, proc = clips(B, L)
    eng = Engine()
    xc, xp = torch.from_numpy(clean).cuda(), torch.from_numpy(proc).cuda()
    call = lambda: eng.metrics(xc, xp, FS, pesq_mos=2.5)
    dev_ms, = benchlib.alternate({"metrics": call}, a.iters, 1, warmup=3)["metrics"]
    dev_scores = call()

    t0 = time.perf_counter()
    host = [M.compute_metrics(clean[b], proc[b], FS, 0, pesq_mos=2.5) for b in range(B)]
    host_s = time.perf_counter() - t0
    got = torch.stack(tuple(dev_scores[:6]), 1).cpu().numpy()
    max_dev = float(np.max(np.abs(got - np.array(host)) / (1.0 + np.abs(np.array(host)))))

    model = TSCNet(64, 201).cuda().load_state_dict(make_state_dict(seed=0)).eval()
    from scipy.io import wavfile
    with tempfile.TemporaryDirectory() as d:
        nd, cd = os.path.join(d, "noisy"), os.path.join(d, "clean")
        os.makedirs(nd)
        os.makedirs(cd)
        tc, tp = clips(a.tracks, L, seed=1)
        for i in range(a.tracks):
            wavfile.write(os.path.join(nd, f"t_{i}.wav"), FS, np.round(tp[i]).astype(np.int16))
            wavfile.write(os.path.join(cd, f"t_{i}.wav"), FS, np.round(tc[i]).astype(np.int16))
        evaluation(model, nd, cd, pesq_fn=lambda f, x, y: 2.5, verbose=False)           # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        evaluation(model, nd, cd, pesq_fn=None, allow_missing_pesq=True, verbose=False)
        torch.cuda.synchronize()
        eval_s = time.perf_counter() - t0
    return {"device_ms_per_call": benchlib.summary([dev_ms], 3)[0], "host_compute_metrics_s": round(host_s, 3),
            "host_cpus": benchlib.host_cpus(), "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
            "speedup_vs_host": round(host_s * 1000.0 / dev_ms, 1), "max_rel_diff_vs_host": max_dev,
            "evaluation_tracks": a.tracks, "evaluation_wall_s": round(eval_s, 3), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tracks", type=int, default=32)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", action="store_const", const=(), default=None, help="(internal) run the case")
    a = ap.parse_args()
    if a.case is not None:
        return benchlib.print_case(run_case(a))
    rows, stopped = benchlib.run_cases(__file__, benchlib.flags(a, "batch", "seconds", "iters", "tracks"),
                                       [("metrics", ())], a.limit)
    line = {"metric": "objective_metrics", "batch": a.batch, "clip_s": a.seconds, "fs": FS, **(rows[0] if rows else {}),
            "limit_s_per_case": a.limit, "stopped": stopped}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
