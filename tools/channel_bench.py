"""The recording channel on the GPU vs the host, and beside the call it follows (cmgan_channel / Engine.channel vs
scipy.signal.sosfilt in float64 on one host thread; Engine.mix without a RIR).

    python tools/channel_bench.py [--batch 32] [--iters 100] [--repeats 7] [--host-clips 2] [--limit 120] [--out PATH]

Prints one JSON line (and writes it to --out when one is given: profiles/r13_channel_bench.json was written by passing
--out).  Six cases at 16 kHz: --batch clips of 2 s and of 10 s with S = 1, 4 and 8 sections per row (every row uses all
S; S = 8 is a high-pass, three equaliser sections and an 8th-order Butterworth band limit, the others its first
sections), half of the rows clipped.  Every case runs isolated under --limit seconds and the calls are timed alternately
(tools/benchlib.py).  Per case: device ms per Engine.channel call and per Engine.mix call without a RIR (the median and
the spread of `repeats` measurements of `iters` calls; a channel call is its four launches), the in-place call, the
seconds the host takes per clip
for sosfilt in float64 (timed on the first --host-clips clips), the worst |gpu - f32(host)| in float32 ulps, and the
arithmetic: a sample costs 5 S fused multiply-adds in each of the two passes over the row, and every thread of both
passes adds 8 (scan) + up to 8 (apply only) mat-vecs of N (N + 2) / 2 multiply-adds, N = 2 S."""
import argparse
import os
import statistics
import sys
import time

import benchlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS = 16000


def sections(B, S):
    """[B, S, 6] float64 (numpy): the first S of a high-pass, three equaliser sections and a Butterworth low-pass."""
    import numpy as np
    import torch
    from cmgan_amd.mixing import biquad_high_shelf, biquad_highpass, biquad_low_shelf, biquad_peaking, butter_lowpass_sos
    u = torch.rand(B, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(13))
    rows = [biquad_highpass(20.0 + 100.0 * u[:, 0], 0.5 ** 0.5, FS)[:, None],
            biquad_peaking(200.0 + 800.0 * u[:, 1], 12.0 * u[:, 2] - 6.0, 1.0, FS)[:, None],
            biquad_low_shelf(150.0 + 100.0 * u[:, 3], 4.0, 0.7, FS)[:, None],
            biquad_high_shelf(3000.0 + 1000.0 * u[:, 0], -4.0, 0.7, FS)[:, None],
            butter_lowpass_sos(8, 3400.0 + 400.0 * u[:, 1], FS)]
    return np.ascontiguousarray(torch.cat(rows, dim=1)[:, :S].numpy())


def run_case(B, seconds, S, iters, repeats, host_clips):
    import numpy as np
    import torch
    from scipy.signal import sosfilt
    from cmgan_amd import _lib
    from cmgan_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("channel_bench needs the GPU")
    eng = Engine()
    dev = eng.device
    tile = int(_lib.load().cmgan_channel_tile())
    L = seconds * FS
    rng = np.random.default_rng(seconds)
    x = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    sos_np = sections(B, S)
    clip_np = np.where(np.arange(B) % 2 == 0, np.inf, 0.15)
    wav = torch.from_numpy(x).to(dev)
    sos = torch.from_numpy(sos_np).to(dev)
    clip = torch.from_numpy(clip_np).to(dev)
    out = torch.empty_like(wav)
    scratch = wav.clone()
    beside = benchlib.mix_beside(rng, B, dev)
    calls = {"channel": lambda: eng.channel(wav, sos, None, clip, out=out),
             "in_place": lambda: eng.channel(scratch, sos, None, clip, out=scratch),
             "mix": lambda: eng.mix(wav, *beside)}
    ms = benchlib.alternate(calls, iters, repeats, warmup=3)
    got = eng.channel(wav, sos, None, clip).cpu().numpy()
    n_host = max(1, min(host_clips, B))
    sosfilt(sos_np[0], x[0, :2000].astype(np.float64))                # (imports, first-use costs)
    t0 = time.perf_counter()
    want = [np.clip(sosfilt(sos_np[b], x[b].astype(np.float64)), -clip_np[b], clip_np[b]) for b in range(n_host)]
    host_s = (time.perf_counter() - t0) / n_host
    ulps = max(float(np.max(np.abs(got[b].astype(np.float64) - want[b].astype(np.float32).astype(np.float64))
                            / np.spacing(np.abs(want[b]).astype(np.float32)))) for b in range(n_host))
    med = {k: statistics.median(v) for k, v in ms.items()}
    ch, ip, mx = (benchlib.summary(ms[k]) for k in ("channel", "in_place", "mix"))
    N = 2 * next(p for p in (1, 2, 4, 8) if S <= p)
    nt = -(-L // tile)
    fma = B * (2 * 5 * S * L + nt * 256 * (8 + 8 + 8) * (N * (N + 2) // 2))
    return {"case": f"{B}x{seconds}s S={S}", "samples_per_clip": L, "tiles_per_clip": nt, "sections": S,
            "channel_ms_per_call": ch[0], "channel_ms_min": ch[1], "channel_ms_max": ch[2], "in_place_ms_per_call": ip[0],
            "mix_no_rir_ms_per_call": mx[0], "mix_ms_min": mx[1], "mix_ms_max": mx[2],
            "channel_over_mix": round(med["channel"] / med["mix"], 3),
            "msamples_per_s": round(B * L / (med["channel"] * 1e-3) / 1e6, 1), "float64_fma_upper_bound": fma,
            "float64_gfma_per_s": round(fma / (med["channel"] * 1e-3) / 1e9, 1),
            "host_sosfilt_s_per_clip": round(host_s, 5), "host_clips_timed": n_host,
            "speedup_vs_host": round(host_s * B * 1000.0 / med["channel"], 1), "max_ulps_vs_f32_of_host": ulps,
            "device": torch.cuda.get_device_name(0), "tile": tile}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-clips", type=int, default=2)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", nargs=2, type=int, default=None, metavar=("SECONDS", "S"), help="(internal) run one case")
    a = ap.parse_args()
    if a.case is not None:
        return benchlib.print_case(run_case(a.batch, a.case[0], a.case[1], a.iters, a.repeats, a.host_clips))
    rows, stopped = benchlib.run_cases(__file__, benchlib.flags(a, "batch", "iters", "repeats", "host_clips"),
                                       [(f"{sec}s S={S}", (sec, S)) for sec in (2, 10) for S in (1, 4, 8)], a.limit)
    line = {"metric": "channel", "batch": a.batch, "fs": FS, "launches_per_call": 4, "iters": a.iters, "repeats": a.repeats,
            "limit_s_per_case": a.limit, "cases": rows, "stopped": stopped, "host_threads": 1,
            "host_cpus_available": benchlib.host_cpus()}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
