"""The synthetic noise on the GPU vs the host, and beside the call that consumes it (cmgan_noise / Engine.noise vs
scipy.signal.lfilter of numpy's Gaussian noise in float64 on one host thread; Engine.mix without a RIR, which mixes the
rows into a batch in DynamicMixer).

    python tools/noise_bench.py [--batch 32] [--iters 50] [--repeats 7] [--host-clips 1] [--limit 180] [--label TEXT] [--out PATH]

Prints one JSON line (and writes it to --out when one is given: profiles/r26_noise_bench.json was written by passing
--out).  Six cases at 16 kHz: --batch rows of 2 s and of 10 s with colouring filters of 63, 255 and 1023 taps, a spectrum,
envelope, hum and click table of its own per row (a NoiseSampler's draw with hum and clicks on every row).  Every case runs
isolated under --limit seconds and the calls are timed alternately (tools/benchlib.py).  Per case: device ms per
Engine.noise call (the median and the spread of `repeats` measurements of `iters` calls; a call is its two launches) for
the bare noise (filter alone), with the envelope, with envelope and tones, with envelope and clicks, and with all of it;
Engine.mix without a RIR on a batch of the same shape; the seconds the host takes per clip to draw Gaussian noise and
filter it with the row's taps (timed on the first --host-clips clips); and the rows' RMS.  --label names the build in the
line (CMGAN_HIP_LIB selects another one)."""
import argparse
import os
import statistics
import sys
import time

import benchlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS = 16000


def run_case(B, seconds, taps, iters, repeats, host_clips):
    import numpy as np
    import scipy.signal
    import torch
    from cmgan_amd import _lib
    from cmgan_amd.engine import Engine
    from cmgan_amd.mixing import NoiseSampler

    if not torch.cuda.is_available():
        raise SystemExit("noise_bench needs the GPU")
    eng = Engine()
    dev = eng.device
    lib = _lib.load()
    L = seconds * FS
    gen = torch.Generator(device=dev)
    gen.manual_seed(26)
    sampler = NoiseSampler(p_hum=1.0, p_clicks=1.0, hum_harmonics=(5, 5), n_taps=taps, generator=gen)
    d = sampler.draw(B, L, FS, device=dev)
    H = sampler.hop(FS)
    out = torch.empty(B, L, dtype=torch.float32, device=dev)
    wav = (0.1 * torch.randn(B, L, generator=gen, device=dev)).contiguous()
    beside = benchlib.mix_beside(np.random.default_rng(seconds), B, dev)
    env, tones, clicks = dict(env=d.env, env_hop=H), dict(tones=d.tones, n_tones=d.n_tones), dict(impulse=d.impulse)
    calls = {"noise": lambda: eng.noise(d.seed, d.fir, L, out=out),
             "env": lambda: eng.noise(d.seed, d.fir, L, out=out, **env),
             "env_tones": lambda: eng.noise(d.seed, d.fir, L, out=out, **env, **tones),
             "env_clicks": lambda: eng.noise(d.seed, d.fir, L, out=out, **env, **clicks),
             "full": lambda: eng.noise(d.seed, d.fir, L, out=out, **env, **tones, **clicks),
             "mix": lambda: eng.mix(wav, *beside)}
    ms = benchlib.alternate(calls, iters, repeats, warmup=3)
    rows, st = eng.noise(d.seed, d.fir, L, info=True, **env, **tones, **clicks)
    rms = rows.double().pow(2).mean(dim=1).sqrt()
    n_host = max(0, min(host_clips, B))
    host_s = None
    if n_host:
        fir = d.fir.cpu().numpy()
        rng = np.random.default_rng(1)
        scipy.signal.lfilter(fir[0], [1.0], rng.standard_normal(2000))       # (imports, first-use costs)
        t0 = time.perf_counter()
        for b in range(n_host):
            scipy.signal.lfilter(fir[b], [1.0], rng.standard_normal(L)).astype(np.float32)
        host_s = round((time.perf_counter() - t0) / n_host, 5)
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: round((max(v) - min(v)) / statistics.median(v), 4) for k, v in ms.items()}
    row = {"case": f"{B}x{seconds}s/{taps}", "samples_per_row": L, "taps": taps, "env_points": int(d.env.size(1)), "env_hop": H,
           "tones": int(d.tones.size(1))}
    for k in calls:
        s = benchlib.summary(ms[k])
        row.update({f"{k}_ms_per_call": s[0], f"{k}_ms_min": s[1], f"{k}_ms_max": s[2], f"{k}_spread": spread[k]})
    row.update({"full_over_mix": round(med["full"] / med["mix"], 3), "msamples_per_s": round(B * L / (med["full"] * 1e-3) / 1e6, 1),
                "gfma_per_s": round(B * L * taps / (med["noise"] * 1e-3) / 1e9, 1),
                "workspace_bytes": int(lib.cmgan_noise_workspace_bytes(B)), "invalid_rows": int(st.sum().item()),
                "rms_min": round(float(rms.min().item()), 3), "rms_max": round(float(rms.max().item()), 3),
                "host_lfilter_s_per_clip": host_s, "host_clips_timed": n_host,
                "speedup_vs_host": None if host_s is None else round(host_s * B * 1000.0 / med["full"], 1),
                "device": torch.cuda.get_device_name(0), "tile": int(lib.cmgan_noise_tile())})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-clips", type=int, default=1)
    ap.add_argument("--limit", type=float, default=180.0)
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", type=int, nargs=2, default=None, metavar=("SECONDS", "TAPS"), help="(internal) run one case")
    a = ap.parse_args()
    if a.case is not None:
        return benchlib.print_case(run_case(a.batch, a.case[0], a.case[1], a.iters, a.repeats, a.host_clips))
    rows, stopped = benchlib.run_cases(__file__, benchlib.flags(a, "batch", "iters", "repeats", "host_clips"),
                                       [(f"{sec}s/{taps}", (sec, taps)) for sec in (2, 10) for taps in (63, 255, 1023)], a.limit)
    device, tile = benchlib.lift(rows, "device", "tile")
    line = {"metric": "noise", "build": a.label, "batch": a.batch, "fs": FS, "launches_per_call": 2, "iters": a.iters,
            "repeats": a.repeats, "limit_s_per_case": a.limit, "device": device, "tile": tile, "cases": rows, "stopped": stopped,
            "host_threads": 1, "host_cpus_available": benchlib.host_cpus()}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
