"""Paths on the GPU beside the call they extend, what their responses cost to simulate, and vs the host (cmgan_scene_path /
Engine.scene_path vs Engine.scene with the same column-0 responses; RirBank.simulate of the B P responses with and without
a diffuse tail; a float64 scipy.signal.fftconvolve chain of windowed segments on one host thread).

    python tools/path_bench.py [--batch 32] [--seconds 2] [--rir-seconds 0.5] [--iters 10] [--repeats 7]
                               [--host-clips 2] [--limit 240] [--out PATH]

Prints one JSON line (and writes it to --out when one is given: profiles/r23_path_bench.json was written by passing
--out).  At 16 kHz, --batch clips of --seconds, every response --rir-seconds long.  Every case runs isolated under --limit
seconds and the calls of a case are timed alternately (tools/benchlib.py).
  path S P   S = 0, 2 located sources and P = 1, 5, 9, 17 waypoints whose hop H = ceil((L - 1) / (P - 1)) spans the clip
             (P = 1: H = L), every row and source moving along all of them, a dry noise as well.  Device ms per
             Engine.scene_path call and per Engine.scene call with column 0 of the same tables (the median and the spread
             of `repeats` measurements of `iters` calls), their ratio beside the estimate 2 + tile / H of the header, whether
             P = 1 gave Engine.scene's bits, the seconds the host takes per clip for the talker's part in float64 (per
             waypoint the weighted clip through fftconvolve, summed), and the largest difference of those clips' speech
             from the host's, relative to the row's peak.
  sim tail   RirBank.simulate of batch x P rooms for P = 1, 5, 9, 17: the image-source method alone (tail = 0) or up to
             80 ms after the direct sound with a diffuse tail behind (tail = 80), ms per call, draws included."""
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
WAYPOINTS = (1, 5, 9, 17)
SOURCES = (0, 2)
TAILS = (0.0, 80.0)
PEAK = 0.99


def host_speech(clean, hs, H):
    """The talker's reverberant speech of one row by the definition in float64: (speech, seconds)."""
    import numpy as np
    from scipy.signal import fftconvolve
    t0 = time.perf_counter()
    L, P = len(clean), len(hs)
    m = np.arange(L)
    x = clean.astype(np.float64)
    out = np.zeros(L)
    for p, h in enumerate(hs):
        u = np.clip((H - np.abs(m - p * H)) / H, 0.0, None)
        if p == P - 1:
            u[m >= p * H] = 1.0
        d = int(np.argmax(np.abs(h)))
        out += fftconvolve(u * x, h.astype(np.float64))[d:d + L]
    return out, time.perf_counter() - t0


def run_path(B, seconds, rir_seconds, S, P, iters, repeats, host_clips):
    import numpy as np
    import torch
    from cmgan_amd.engine import Engine
    from cmgan_amd.mixing import tile

    if not torch.cuda.is_available():
        raise SystemExit("path_bench needs the GPU")
    eng = Engine()
    dev = eng.device
    L, K, Sc = int(seconds * FS), int(rir_seconds * FS), max(S, 1)
    H = L if P == 1 else math.ceil((L - 1) / (P - 1))
    rng = np.random.default_rng(23)
    x = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    rir_np = (rng.standard_normal((B * P * (1 + Sc), K)) * np.exp(-np.arange(K) / (0.15 * K))).astype(np.float32)
    rir_np[:, 40] = 2.0                                                   # a direct path behind a short onset
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    clean, rir = t(x, torch.float32), t(rir_np, torch.float32)
    bank, n_start, n_len, n_off, snr = benchlib.mix_beside(rng, B, dev)
    idx = torch.arange(B * P, dtype=torch.int32, device=dev).reshape(B, P)
    rlen = torch.full((B, P), K, dtype=torch.int32, device=dev)
    n_path = torch.full((B,), P, dtype=torch.int32, device=dev)
    src, src_path, src_static = [None] * 6, [None] * 3, [None] * 2
    if S:
        seg_len = 3 * FS
        src = [torch.full((B,), S, dtype=torch.int32, device=dev), bank, t(rng.integers(0, bank.numel() - seg_len, (B, S)), torch.int64),
               torch.full((B, S), seg_len, dtype=torch.int64, device=dev), t(rng.integers(0, seg_len, (B, S)), torch.int64),
               t(rng.uniform(0.0, 10.0, (B, S)), torch.float32)]
        s_idx = (B * P + torch.arange(B * S * P, dtype=torch.int32, device=dev)).reshape(B, S, P)
        s_rlen = torch.full((B, S, P), K, dtype=torch.int32, device=dev)
        src_path = [torch.full((B, S), P, dtype=torch.int32, device=dev), s_idx, s_rlen]
        src_static = [s_idx[:, :, 0].contiguous(), s_rlen[:, :, 0].contiguous()]
    idx0, rlen0 = idx[:, 0].contiguous(), rlen[:, 0].contiguous()
    calls = {"path": lambda: eng.scene_path(clean, H, n_path, rir, idx, rlen, bank, n_start, n_len, n_off, snr, *src, *src_path,
                                            peak=PEAK, early=-1),
             "scene": lambda: eng.scene(clean, bank, n_start, n_len, n_off, snr, *src, rir, idx0, rlen0, *src_static, peak=PEAK,
                                        early=-1)}
    ms = benchlib.alternate(calls, iters, repeats, warmup=2)
    same = bool(torch.equal(calls["path"]()[0], calls["scene"]()[0])) if P == 1 else None
    # the talker alone against the host: no noise, no sources, a peak nothing reaches
    far = torch.full((B,), 300.0, dtype=torch.float32, device=dev)
    got = eng.scene_path(clean, H, n_path, rir, idx, rlen, bank, n_start, n_len, n_off, far, peak=1e30, early=-1)[0].cpu().numpy()
    n_host = max(1, min(host_clips, B))
    host_s, rel = [], 0.0
    for b in range(n_host):
        want, s = host_speech(x[b], [rir_np[b * P + p] for p in range(P)], H)
        host_s.append(s)
        rel = max(rel, float(np.max(np.abs(got[b] - want)) / np.max(np.abs(want))))
    med = {k: statistics.median(v) for k, v in ms.items()}
    pa, sc = benchlib.summary(ms["path"]), benchlib.summary(ms["scene"])
    return {"case": f"path S={S} P={P}", "sources": S, "waypoints": P, "hop": H, "samples_per_clip": L, "taps": K,
            "path_ms_per_call": pa[0], "path_ms_min": pa[1], "path_ms_max": pa[2],
            "scene_ms_per_call": sc[0], "scene_ms_min": sc[1], "scene_ms_max": sc[2],
            "path_over_scene": round(med["path"] / med["scene"], 3), "estimate_2_plus_tile_over_hop": round(2.0 + tile() / H, 3),
            "same_bits_as_scene": same, "host_fftconvolve_s_per_clip": round(statistics.median(host_s), 5),
            "host_clips_timed": n_host, "host_talker_ms_per_batch": round(statistics.median(host_s) * B * 1000.0, 2),
            "max_error_of_row_peak_vs_host": float(f"{rel:.3e}"), "device": torch.cuda.get_device_name(0)}


def run_sim(B, rir_seconds, tail_ms, iters, repeats):
    import torch
    from cmgan_amd.engine import Engine
    from cmgan_amd.mixing import RirBank, RoomSampler

    if not torch.cuda.is_available():
        raise SystemExit("path_bench needs the GPU")
    eng = Engine()
    gen = torch.Generator(device=eng.device)
    gen.manual_seed(23)
    sampler = RoomSampler(rt60=(0.4, 1.2), generator=gen, tail_ms=tail_ms or None)
    calls = {f"P={P}": (lambda P=P: RirBank.simulate(eng, sampler, B * P, seconds=rir_seconds, sample_rate=FS)) for P in WAYPOINTS}
    ms = benchlib.alternate(calls, iters, repeats, warmup=1)
    row = {"case": f"sim tail={tail_ms:g}", "tail_ms": tail_ms, "rooms_per_waypoint": B, "taps": int(rir_seconds * FS),
           "device": torch.cuda.get_device_name(0)}
    for P in WAYPOINTS:
        row[f"ms_per_call_P{P}"], row[f"ms_min_P{P}"], row[f"ms_max_P{P}"] = benchlib.summary(ms[f"P={P}"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rir-seconds", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-clips", type=int, default=2)
    ap.add_argument("--limit", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", nargs="+", default=None, metavar="ARG", help="(internal) run one case: path S P | sim TAIL_MS")
    a = ap.parse_args()
    if a.case is not None:
        if a.case[0] == "path":
            return benchlib.print_case(run_path(a.batch, a.seconds, a.rir_seconds, int(a.case[1]), int(a.case[2]), a.iters,
                                                a.repeats, a.host_clips))
        return benchlib.print_case(run_sim(a.batch, a.rir_seconds, float(a.case[1]), max(1, a.iters // 5), a.repeats))
    common = benchlib.flags(a, "batch", "seconds", "rir_seconds", "iters", "repeats", "host_clips")
    cases = [(f"path S={S} P={P}", ("path", S, P)) for S in SOURCES for P in WAYPOINTS] + [(f"sim tail={t:g}", ("sim", t)) for t in TAILS]
    rows, stopped = benchlib.run_cases(__file__, common, cases, a.limit)
    device, = benchlib.lift(rows, "device")
    line = {"metric": "path", "batch": a.batch, "fs": FS, "seconds": a.seconds, "rir_seconds": a.rir_seconds, "peak": PEAK,
            "launches_per_call": 6, "iters": a.iters, "repeats": a.repeats, "limit_s_per_case": a.limit, "device": device,
            "cases": rows, "stopped": stopped, "host_threads": 1, "host_cpus_available": benchlib.host_cpus()}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
