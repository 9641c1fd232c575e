"""Tempo perturbation on the GPU vs the host, and beside the calls around it (cmgan_stretch / Engine.stretch vs the numpy
model of tests/stretch_model.py on one host thread; Engine.warp; Engine.mix without a RIR).

    python tools/stretch_bench.py [--batch 32] [--iters 100] [--repeats 7] [--host-clips 2] [--limit 240] [--out PATH]

Prints one JSON line (and writes it to --out when one is given: profiles/r16_stretch_bench.json was written by passing
--out).  Two cases at 16 kHz: --batch clips of ceil(32000 x 1.1) samples stretched to 32000 (2 s batches) and of
ceil(160000 x 1.1) stretched to 160000 (10 s), one rate per row, uniform in 0.9 .. 1.1, hop = 256, search = 160; the clips
are a harmonic tone with a gliding pitch under an envelope, plus noise.  Every case runs isolated under --limit seconds
and the calls are timed alternately (tools/benchlib.py).  Per case: device ms per Engine.stretch call (one launch, one
block per row), the same call with every rate at 1.0 (no frame is searched) and at 1.1, Engine.warp on the same batch at
the same rates, and Engine.mix without a RIR on the stretched batch (the median and the spread of `repeats` measurements
of `iters` calls), the frames and the searched frames per clip, the seconds the host takes per clip for the numpy model
(positions and cross-fade, timed on the first --host-clips clips), and a check of those clips against the model: every
position equal, the samples in float32 ulps."""
import argparse
import math
import os
import statistics
import sys
import time

import benchlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS = 16000
HI = 1.1
HOP, SEARCH = 256, 160


def clips(B, L, seed):
    """float32 [B, L]: eleven harmonics of a pitch that glides around 110 - 140 Hz, a 3 Hz envelope, noise at -34 dB."""
    import numpy as np
    rng = np.random.default_rng(seed)
    t = np.arange(L) / FS
    out = np.empty((B, L), dtype=np.float32)
    for b in range(B):
        f0 = 110.0 + 3.0 * b % 30 + 20.0 * np.sin(2 * np.pi * (1.0 + 0.1 * b) * t)
        ph = 2 * np.pi * np.cumsum(f0) / FS
        tone = sum(np.sin(h * ph) / h for h in range(1, 12))
        out[b] = 0.1 * tone * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 0.002 * rng.standard_normal(L)
    return out


def run_case(B, seconds, iters, repeats, host_clips):
    import numpy as np
    import torch
    import stretch_model as model
    from cmgan_amd.engine import Engine
    from cmgan_amd.mixing import warp_len

    if not torch.cuda.is_available():
        raise SystemExit("stretch_bench needs the GPU")
    eng = Engine()
    dev = eng.device
    L = math.ceil(seconds * FS * HI)
    N = warp_len(L, HI)
    rng = np.random.default_rng(seconds)
    x = clips(B, L, seconds)
    rate_np = rng.uniform(0.9, 1.1, B)
    wav = torch.from_numpy(x).to(dev)
    rate = torch.from_numpy(rate_np).to(dev)
    ones = torch.ones(B, dtype=torch.float64, device=dev)
    fast = torch.full((B,), HI, dtype=torch.float64, device=dev)
    out = torch.empty(B, N, dtype=torch.float32, device=dev)
    scratch = torch.empty_like(out)
    beside = benchlib.mix_beside(rng, B, dev)
    calls = {"stretch": lambda: eng.stretch(wav, rate, N, hop=HOP, search=SEARCH, out=out),
             "stretch_rate_1": lambda: eng.stretch(wav, ones, N, hop=HOP, search=SEARCH, out=scratch),
             "stretch_rate_1p1": lambda: eng.stretch(wav, fast, N, hop=HOP, search=SEARCH, out=scratch),
             "warp": lambda: eng.warp(wav, rate, N, out=scratch),
             "mix": lambda: eng.mix(out, *beside)}
    ms = benchlib.alternate(calls, iters, repeats, warmup=3)
    got, n_out, status, pos, searched = (t.cpu().numpy() for t in eng.stretch(wav, rate, N, hop=HOP, search=SEARCH, info=True))
    _, _, _, _, searched_fast = (t.cpu().numpy() for t in eng.stretch(wav, fast, N, hop=HOP, search=SEARCH, info=True))
    n_host = max(1, min(host_clips, B))
    model.positions(x[0, :3000], 3000, 1.05, HOP, SEARCH)             # (imports, first-use costs)
    host_s, pos_equal, ulps = 0.0, True, 0.0
    for b in range(n_host):
        t0 = time.perf_counter()
        p = model.positions(x[b], L, float(rate_np[b]), HOP, SEARCH, N)
        want = model.direct(x[b], L, float(rate_np[b]), HOP, SEARCH, N, p).astype(np.float32)
        host_s += (time.perf_counter() - t0) / n_host
        pos_equal = pos_equal and bool(np.array_equal(pos[b, :len(p[0])], p[0])) and int(searched[b]) == int(p[2].sum())
        err = np.abs(got[b, :len(want)].astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(want), 1e-30))
        ulps = max(ulps, float(np.max(err)))
    med = {k: statistics.median(v) for k, v in ms.items()}
    st, wp, mx = (benchlib.summary(ms[k]) for k in ("stretch", "warp", "mix"))
    K = -(-N // HOP)
    return {"case": f"{B}x{seconds}s", "samples_in_per_clip": L, "samples_out_per_clip": N, "frames_per_clip": K,
            "searched_frames_per_clip_mean": round(float(searched.mean()), 1), "searched_frames_per_clip_max": int(searched.max()),
            "searched_frames_per_clip_rate_1p1": round(float(searched_fast.mean()), 1),
            "stretch_ms_per_call": st[0], "stretch_ms_min": st[1], "stretch_ms_max": st[2],
            "stretch_rate_1_ms_per_call": benchlib.summary(ms["stretch_rate_1"])[0],
            "stretch_rate_1p1_ms_per_call": benchlib.summary(ms["stretch_rate_1p1"])[0],
            "warp_ms_per_call": wp[0], "warp_ms_min": wp[1], "warp_ms_max": wp[2],
            "mix_no_rir_ms_per_call": mx[0], "mix_ms_min": mx[1], "mix_ms_max": mx[2],
            "stretch_over_warp": round(med["stretch"] / med["warp"], 3),
            "stretch_over_mix": round(med["stretch"] / med["mix"], 3),
            "msamples_out_per_s": round(B * N / (med["stretch"] * 1e-3) / 1e6, 1),
            "us_per_searched_frame_of_the_slowest_row": round((med["stretch"] - med["stretch_rate_1"]) * 1e3 / max(int(searched.max()), 1), 3),
            "host_model_s_per_clip": round(host_s, 5), "host_clips_timed": n_host,
            "host_ms_per_batch": round(host_s * B * 1000.0, 2), "speedup_vs_host": round(host_s * B * 1000.0 / med["stretch"], 1),
            "rows_full": bool((n_out == N).all()), "rows_valid": bool((status == 0).all()),
            "positions_equal_to_the_model": pos_equal, "max_ulps_vs_f32_of_the_model": ulps,
            "device": torch.cuda.get_device_name(0), "blocks": B}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-clips", type=int, default=2)
    ap.add_argument("--limit", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", type=int, default=None, metavar="SECONDS", help="(internal) run one case")
    a = ap.parse_args()
    if a.case is not None:
        return benchlib.print_case(run_case(a.batch, a.case, a.iters, a.repeats, a.host_clips))
    rows, stopped = benchlib.run_cases(__file__, benchlib.flags(a, "batch", "iters", "repeats", "host_clips"),
                                       [(f"{sec}s", (sec,)) for sec in (2, 10)], a.limit)
    line = {"metric": "stretch", "batch": a.batch, "fs": FS, "rates": [0.9, 1.1], "hop": HOP, "search": SEARCH,
            "launches_per_call": 1, "iters": a.iters, "repeats": a.repeats, "limit_s_per_case": a.limit, "cases": rows,
            "stopped": stopped, "host_threads": 1, "host_cpus_available": benchlib.host_cpus()}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
