"""Objective-metric scoring on the GPU vs the host (cmgan_metrics / Engine.metrics vs cmgan_amd.metrics).

    python tools/metrics_bench.py [--batch 32] [--seconds 2] [--iters 20] [--tracks 32] [--out PATH]

Prints one JSON line: device ms per Engine.metrics call on B clips of the given length at 16 kHz (HIP events, after
warm-up), host compute_metrics seconds for the same clips (with the CPU count this process may use), and the wall time
of evaluation() on `tracks` synthetic wav pairs (random-init weights; a constant stub PESQ)."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tracks", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cmgan_amd import TSCNet
    from cmgan_amd import metrics as M
    from cmgan_amd.engine import Engine
    from cmgan_amd.evaluation import evaluation
    from cmgan_amd.synth import make_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs the GPU")
    B, L, fs = a.batch, int(16000 * a.seconds), 16000
    clean, proc = clips(B, L)
    eng = Engine()
    xc, xp = torch.from_numpy(clean).cuda(), torch.from_numpy(proc).cuda()
    for _ in range(3):
        eng.metrics(xc, xp, fs, pesq_mos=2.5)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        dev_scores = eng.metrics(xc, xp, fs, pesq_mos=2.5)
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / a.iters

    t0 = time.perf_counter()
    host = [M.compute_metrics(clean[b], proc[b], fs, 0, pesq_mos=2.5) for b in range(B)]
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
            wavfile.write(os.path.join(nd, f"t_{i}.wav"), fs, np.round(tp[i]).astype(np.int16))
            wavfile.write(os.path.join(cd, f"t_{i}.wav"), fs, np.round(tc[i]).astype(np.int16))
        evaluation(model, nd, cd, pesq_fn=lambda f, x, y: 2.5, verbose=False)           # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        evaluation(model, nd, cd, pesq_fn=None, allow_missing_pesq=True, verbose=False)
        torch.cuda.synchronize()
        eval_s = time.perf_counter() - t0

    cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    line = {"metric": "objective_metrics", "batch": B, "clip_s": a.seconds, "fs": fs,
            "device_ms_per_call": round(dev_ms, 3), "host_compute_metrics_s": round(host_s, 3),
            "host_cpus": cpus, "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
            "speedup_vs_host": round(host_s * 1000.0 / dev_ms, 1), "max_rel_diff_vs_host": max_dev,
            "evaluation_tracks": a.tracks, "evaluation_wall_s": round(eval_s, 3),
            "device": torch.cuda.get_device_name(0)}
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
