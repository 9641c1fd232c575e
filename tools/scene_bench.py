"""Scenes on the GPU beside the call they extend, and vs the host (cmgan_scene / Engine.scene vs Engine.mix with the same
talker response; a float64 scipy.signal.fftconvolve chain on one host thread).

    python tools/scene_bench.py [--batch 32] [--seconds 2] [--rir-seconds 0.5] [--iters 20] [--repeats 7]
                                [--host-clips 2] [--limit 180] [--out PATH]

Prints one JSON line (and writes it to --out when one is given: profiles/r15_scene_bench.json was written by passing
--out).  One case per source count S = 0, 1, 2, 4 at 16 kHz: --batch clips of --seconds, every response (the talker's and
each source's) --rir-seconds long, every row with all S sources, segments of 3 s looping from a random offset, a dry noise
as well.  Every case runs isolated under --limit seconds and the two calls are timed alternately (tools/benchlib.py).
Per case: device ms per Engine.scene call and per Engine.mix call on the same clean batch, dry noise and talker responses
(the median and the spread of `repeats` measurements of `iters` calls), their ratio, the seconds the host takes per clip
for the same scene in float64 (fftconvolve of the clip and of each looped segment, powers, gains, sum and peak guard;
timed on the first --host-clips clips), and the largest difference of those clips' noisy rows from the host's, in float32
ulps of the row's peak.

cmgan_mix is the S = 0 case of cmgan_scene and runs the same kernels (cmgan_amd/csrc/scene.hip), so the S = 0 row times
one code path twice and its `same_bits_as_mix` holds by construction; profiles/r15_scene_bench.json was measured when
Engine.mix still had kernels of its own."""
import argparse
import os
import statistics
import sys
import time

import benchlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS = 16000
SOURCES = (0, 1, 2, 4)
PEAK, EARLY = 0.99, 800


def host_scene(clean, h, n0, snr0, segs, hs, snrs):
    """One row by the definition in float64: (noisy, seconds)."""
    import numpy as np
    from scipy.signal import fftconvolve
    t0 = time.perf_counter()
    L = len(clean)
    d = int(np.argmax(np.abs(h)))
    speech = fftconvolve(clean.astype(np.float64), h.astype(np.float64))[d:d + L]
    ps = float(np.mean(speech * speech))
    n0 = n0.astype(np.float64)
    v = speech + np.sqrt(ps / (float(np.mean(n0 * n0)) * 10.0 ** (snr0 / 10.0))) * n0
    for seg, hj, snr in zip(segs, hs, snrs):
        c = fftconvolve(seg.astype(np.float64), hj.astype(np.float64), mode="valid")          # seg holds m = -(K - 1) .. L - 1
        v = v + np.sqrt(ps / (float(np.mean(c * c)) * 10.0 ** (snr / 10.0))) * c
    m = float(np.max(np.abs(v)))
    pk = float(np.float32(PEAK))
    return v * (pk / m if m > pk else 1.0), time.perf_counter() - t0


def run_case(B, seconds, rir_seconds, S, iters, repeats, host_clips):
    import numpy as np
    import torch
    from cmgan_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("scene_bench needs the GPU")
    eng = Engine()
    dev = eng.device
    L, K, Sc = int(seconds * FS), int(rir_seconds * FS), max(S, 1)
    rng = np.random.default_rng(15)
    x = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    rir_np = (rng.standard_normal((B * (1 + Sc), K)) * np.exp(-np.arange(K) / (0.15 * K))).astype(np.float32)
    rir_np[:, 40] = 2.0                                                   # a direct path behind a short onset
    bank_np = (0.1 * rng.standard_normal(10 * FS)).astype(np.float32)
    seg_len = 3 * FS
    start_np = rng.integers(0, len(bank_np) - seg_len, (B, Sc))
    off_np = rng.integers(0, seg_len, (B, Sc))
    snr_np = rng.uniform(0.0, 10.0, (B, Sc)).astype(np.float32)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    clean, rir, bank = t(x, torch.float32), t(rir_np, torch.float32), t(bank_np, torch.float32)
    n_start = torch.zeros(B, dtype=torch.int64, device=dev)
    n_len = torch.full((B,), bank.numel(), dtype=torch.int64, device=dev)
    n_off = torch.arange(B, dtype=torch.int64, device=dev) * 977
    snr = torch.full((B,), 10.0, dtype=torch.float32, device=dev)
    idx = torch.arange(B, dtype=torch.int32, device=dev)
    rlen = torch.full((B,), K, dtype=torch.int32, device=dev)
    src = [None] * 6
    s_idx = s_rlen = None
    if S:
        src = [torch.full((B,), S, dtype=torch.int32, device=dev), bank, t(start_np, torch.int64),
               torch.full((B, S), seg_len, dtype=torch.int64, device=dev), t(off_np, torch.int64), t(snr_np, torch.float32)]
        s_idx = (B + torch.arange(B * S, dtype=torch.int32, device=dev)).reshape(B, S)
        s_rlen = torch.full((B, S), K, dtype=torch.int32, device=dev)
    calls = {"scene": lambda: eng.scene(clean, bank, n_start, n_len, n_off, snr, *src, rir, idx, rlen, s_idx, s_rlen, peak=PEAK,
                                        early=EARLY),
             "mix": lambda: eng.mix(clean, bank, n_start, n_len, n_off, snr, rir, idx, rlen, peak=PEAK, early=EARLY)}
    ms = benchlib.alternate(calls, iters, repeats, warmup=2)
    got = calls["scene"]()[0].cpu().numpy()
    same_as_mix = bool(torch.equal(calls["scene"]()[0], calls["mix"]()[0])) if S == 0 else None
    n_host = max(1, min(host_clips, B))
    host_s, ulps = [], 0.0
    for b in range(n_host):
        n0 = bank_np[(977 * b + np.arange(L)) % len(bank_np)]
        segs = [bank_np[start_np[b, j] + (off_np[b, j] + np.arange(-(K - 1), L)) % seg_len] for j in range(S)]
        want, s = host_scene(x[b], rir_np[b], n0, 10.0, segs, [rir_np[B + b * S + j] for j in range(S)],
                             [float(snr_np[b, j]) for j in range(S)])
        host_s.append(s)
        ulps = max(ulps, float(np.max(np.abs(got[b] - want)) / np.spacing(np.float32(np.max(np.abs(want))))))
    med = {k: statistics.median(v) for k, v in ms.items()}
    sc, mx = benchlib.summary(ms["scene"]), benchlib.summary(ms["mix"])
    macs = B * L * K * (1 + S)                                            # (the talker's taps beyond the clip's start are fewer)
    return {"case": f"S={S}", "sources": S, "samples_per_clip": L, "taps": K,
            "scene_ms_per_call": sc[0], "scene_ms_min": sc[1], "scene_ms_max": sc[2],
            "mix_ms_per_call": mx[0], "mix_ms_min": mx[1], "mix_ms_max": mx[2],
            "scene_over_mix": round(med["scene"] / med["mix"], 3), "gmac_per_s": round(macs / (med["scene"] * 1e-3) / 1e9, 1),
            "same_bits_as_mix": same_as_mix, "host_fftconvolve_s_per_clip": round(statistics.median(host_s), 5),
            "host_clips_timed": n_host, "host_ms_per_batch": round(statistics.median(host_s) * B * 1000.0, 2),
            "speedup_vs_host": round(statistics.median(host_s) * B * 1000.0 / med["scene"], 1),
            "max_ulps_of_row_peak_vs_host": round(ulps, 4), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rir-seconds", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-clips", type=int, default=2)
    ap.add_argument("--limit", type=float, default=180.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", type=int, default=None, metavar="S", help="(internal) run one case")
    a = ap.parse_args()
    if a.case is not None:
        return benchlib.print_case(run_case(a.batch, a.seconds, a.rir_seconds, a.case, a.iters, a.repeats, a.host_clips))
    common = benchlib.flags(a, "batch", "seconds", "rir_seconds", "iters", "repeats", "host_clips")
    rows, stopped = benchlib.run_cases(__file__, common, [(f"S={S}", (S,)) for S in SOURCES], a.limit)
    line = {"metric": "scene", "batch": a.batch, "fs": FS, "seconds": a.seconds, "rir_seconds": a.rir_seconds, "peak": PEAK,
            "early": EARLY, "launches_per_call": 6, "iters": a.iters, "repeats": a.repeats, "limit_s_per_case": a.limit,
            "cases": rows, "stopped": stopped, "host_threads": 1, "host_cpus_available": benchlib.host_cpus()}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
