"""The gain control on the GPU vs the host, and beside the calls around it (cmgan_dynamics / Engine.dynamics vs the serial
loop of tests/dynamics_model.py in float64 numpy on one host thread; Engine.mix without a RIR, which it follows in
DynamicMixer, and Engine.channel at 4 sections, which follows it).

    python tools/dynamics_bench.py [--batch 32] [--iters 100] [--repeats 7] [--host-clips 1] [--limit 180] [--label TEXT] [--out PATH]

Prints one JSON line (and writes it to --out when one is given: profiles/r25_dynamics_bench.json was written by passing
--out).  Two cases at 16 kHz: --batch clips of 2 s and of 10 s, a processor of its own per row (ratios 2 .. 20 and a
limiter, knees 0 .. 12 dB, attack 1 .. 30 ms, release 50 .. 500 ms, every fourth row with the attack slower than the
release), on noise whose level jumps between -50 and -6 dBFS.  Every case runs isolated under --limit seconds and the calls
are timed alternately (tools/benchlib.py).  Per case: device ms per Engine.dynamics call (the median and the spread of
`repeats` measurements of `iters` calls; a call is its three launches), the in-place call, the call with a separate key,
the call with info=True (a fourth launch), Engine.mix without a RIR and Engine.channel with 4 sections per row on the same
batch, the seconds the host takes per clip for the serial loop (timed on the first --host-clips clips), and the worst
|gpu - f32(host)| in float32 ulps.  --label names the build in the line (CMGAN_HIP_LIB selects another one)."""
import argparse
import os
import statistics
import sys
import time

import benchlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS = 16000


def table(B):
    """[B, 6] float64 (numpy): one processor per row."""
    import numpy as np
    import dynamics_model as M
    rng = np.random.default_rng(25)
    rows = []
    for b in range(B):
        ratio = np.inf if b % 5 == 4 else float(np.exp(rng.uniform(np.log(2.0), np.log(20.0))))
        att, rel = float(np.exp(rng.uniform(np.log(1.0), np.log(30.0)))), float(np.exp(rng.uniform(np.log(50.0), np.log(500.0))))
        if b % 4 == 3:
            att, rel = rel, att
        rows.append(M.params(float(rng.uniform(-36.0, -12.0)), ratio, float(rng.uniform(0.0, 12.0)), att, rel, float(rng.uniform(0.0, 6.0))))
    return np.stack(rows)


def sections(B):
    """[B, 4, 6] float64 (numpy): a high-pass and three equaliser sections, for the Engine.channel call beside."""
    import numpy as np
    import torch
    from cmgan_amd.mixing import biquad_high_shelf, biquad_highpass, biquad_low_shelf, biquad_peaking
    u = torch.rand(B, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(13))
    rows = [biquad_highpass(20.0 + 100.0 * u[:, 0], 0.5 ** 0.5, FS)[:, None],
            biquad_peaking(200.0 + 800.0 * u[:, 1], 12.0 * u[:, 2] - 6.0, 1.0, FS)[:, None],
            biquad_low_shelf(150.0 + 100.0 * u[:, 3], 4.0, 0.7, FS)[:, None],
            biquad_high_shelf(3000.0 + 1000.0 * u[:, 0], -4.0, 0.7, FS)[:, None]]
    return np.ascontiguousarray(torch.cat(rows, dim=1).numpy())


def run_case(B, seconds, iters, repeats, host_clips):
    import numpy as np
    import torch
    import dynamics_model as M
    from cmgan_amd import _lib
    from cmgan_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("dynamics_bench needs the GPU")
    eng = Engine()
    dev = eng.device
    tile = int(_lib.load().cmgan_dynamics_tile())
    L = seconds * FS
    rng = np.random.default_rng(seconds)
    x = np.stack([M.bursts(1000 * seconds + b, L) for b in range(B)])
    dyn_np = table(B)
    wav = torch.from_numpy(x).to(dev)
    key = torch.from_numpy(np.roll(x, 1, axis=0).copy()).to(dev)
    dyn = torch.from_numpy(dyn_np).to(dev)
    sos = torch.from_numpy(sections(B)).to(dev)
    out = torch.empty_like(wav)
    scratch = wav.clone()
    beside = benchlib.mix_beside(rng, B, dev)
    calls = {"dynamics": lambda: eng.dynamics(wav, dyn, out=out),
             "in_place": lambda: eng.dynamics(scratch, dyn, out=scratch),
             "keyed": lambda: eng.dynamics(wav, dyn, key, out=out),
             "info": lambda: eng.dynamics(wav, dyn, out=out, info=True),
             "mix": lambda: eng.mix(wav, *beside),
             "channel": lambda: eng.channel(wav, sos, out=out)}
    ms = benchlib.alternate(calls, iters, repeats, warmup=3)
    got, st, pk = eng.dynamics(wav, dyn, info=True)
    got = got.cpu().numpy()
    n_host = max(0, min(host_clips, B))
    host_s, ulps = None, None
    if n_host:
        M.serial(x[0, :2000], None, 2000, dyn_np[0])                    # (imports, first-use costs)
        t0 = time.perf_counter()
        want = [M.serial(x[b], None, L, dyn_np[b])[0] for b in range(n_host)]
        host_s = round((time.perf_counter() - t0) / n_host, 5)
        ulps = max(float(np.max(np.abs(got[b].astype(np.float64) - want[b].astype(np.float32).astype(np.float64))
                                / np.spacing(np.maximum(np.abs(want[b]).astype(np.float32), np.float32(1e-30))))) for b in range(n_host))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: round((max(v) - min(v)) / statistics.median(v), 4) for k, v in ms.items()}
    row = {"case": f"{B}x{seconds}s", "samples_per_clip": L, "tiles_per_clip": -(-L // tile)}
    for k in calls:
        s = benchlib.summary(ms[k])
        row.update({f"{k}_ms_per_call": s[0], f"{k}_ms_min": s[1], f"{k}_ms_max": s[2], f"{k}_spread": spread[k]})
    row.update({"dynamics_over_mix": round(med["dynamics"] / med["mix"], 3), "dynamics_over_channel": round(med["dynamics"] / med["channel"], 3),
                "msamples_per_s": round(B * L / (med["dynamics"] * 1e-3) / 1e6, 1),
                "workspace_bytes": int(_lib.load().cmgan_dynamics_workspace_bytes(B, L)),
                "invalid_rows": int(st.sum().item()), "peak_reduction_db_max": round(float(pk.max().item()), 3),
                "host_serial_s_per_clip": host_s, "host_clips_timed": n_host,
                "speedup_vs_host": None if host_s is None else round(host_s * B * 1000.0 / med["dynamics"], 1),
                "max_ulps_vs_f32_of_host": ulps, "device": torch.cuda.get_device_name(0), "tile": tile})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-clips", type=int, default=1)
    ap.add_argument("--limit", type=float, default=180.0)
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", type=int, default=None, metavar="SECONDS", help="(internal) run one case")
    a = ap.parse_args()
    if a.case is not None:
        return benchlib.print_case(run_case(a.batch, a.case, a.iters, a.repeats, a.host_clips))
    rows, stopped = benchlib.run_cases(__file__, benchlib.flags(a, "batch", "iters", "repeats", "host_clips"),
                                       [(f"{sec}s", (sec,)) for sec in (2, 10)], a.limit)
    device, tile = benchlib.lift(rows, "device", "tile")
    line = {"metric": "dynamics", "build": a.label, "batch": a.batch, "fs": FS, "launches_per_call": 3, "iters": a.iters,
            "repeats": a.repeats, "limit_s_per_case": a.limit, "device": device, "tile": tile, "cases": rows, "stopped": stopped,
            "host_threads": 1, "host_cpus_available": benchlib.host_cpus()}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
