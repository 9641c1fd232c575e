"""The transmission stage on the GPU vs the host, and beside the calls around it (cmgan_transmit / Engine.transmit vs the
numpy model of tests/transmit_model.py on one host thread; Engine.mix without a RIR; Engine.channel at 4 sections, which it
follows in DynamicMixer).

    python tools/transmit_bench.py [--batch 32] [--iters 100] [--repeats 7] [--host-clips 2] [--limit 240] [--out PATH]

Prints one JSON line (and writes it to --out when one is given: profiles/r27_transmit_bench.json was written by passing
--out).  Two cases at 16 kHz: --batch clips of 2 s and of 10 s (the clips of tools/stretch_bench.py: a harmonic tone with
a gliding pitch under an envelope, plus noise), G.711 mu-law, packets of 20 ms lost in bursts of mean length 2 (the
Gilbert-Elliott chain of cmgan_amd.mixing.TransmissionSampler) at a mean loss of 0 %, 5 % and 20 %, every run concealed,
lags 80 .. 240, window 320, fade 160.  Every case runs isolated under --limit seconds and the calls are timed alternately
(tools/benchlib.py).  Per case: device ms per Engine.transmit call at each loss (the median and the spread of `repeats`
measurements of `iters` calls; a call is its two launches), the call at 5 % in place and with gaps in place of the
concealment, Engine.mix without a RIR and Engine.channel with 4 sections per row on the same batch, the runs and the lost
frames per clip, the seconds the host takes per clip for the numpy model at 5 % and at 20 % (timed on the first
--host-clips clips), and a check of those clips against the model: every lag equal, the samples in float32 ulps."""
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
LOSS = (0.0, 0.05, 0.2)
BURST = 2.0
FRAME, PMIN, PMAX, WINDOW, FADE = 320, 80, 240, 320, 160


def tables(B, K, rate):
    """uint8 [B, K] (torch, host): the chain at mean loss `rate` and mean burst BURST, seeded by the rate."""
    import torch
    from cmgan_amd.mixing import TransmissionSampler
    gen = torch.Generator().manual_seed(int(1000 * rate) + 27)
    sampler = TransmissionSampler(p=1.0, loss=(rate, rate), burst=(BURST, BURST), generator=gen)
    return sampler.draw(B, K).lost


def run_case(B, seconds, iters, repeats, host_clips):
    import numpy as np
    import torch
    import transmit_model as M
    from dynamics_bench import sections
    from stretch_bench import clips
    from cmgan_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("transmit_bench needs the GPU")
    eng = Engine()
    dev = eng.device
    L = seconds * FS
    K = -(-L // FRAME)
    rng = np.random.default_rng(seconds)
    x = clips(B, L, seconds)
    wav = torch.from_numpy(x).to(dev)
    lost_np = {r: tables(B, K, r).numpy() for r in LOSS}
    lost = {r: torch.from_numpy(v).to(dev) for r, v in lost_np.items()}
    codec = torch.full((B,), M.ULAW, dtype=torch.int32, device=dev)
    conceal = torch.ones(B, dtype=torch.int32, device=dev)
    gaps = torch.zeros(B, dtype=torch.int32, device=dev)
    sos = torch.from_numpy(sections(B)).to(dev)
    out = torch.empty_like(wav)
    scratch = wav.clone()
    beside = benchlib.mix_beside(rng, B, dev)
    send = lambda r, plc=conceal, src=wav, dst=out: eng.transmit(src, lost[r], FRAME, codec, plc, out=dst)
    calls = {"loss_0": lambda: send(0.0), "loss_5": lambda: send(0.05), "loss_20": lambda: send(0.2),
             "loss_5_in_place": lambda: send(0.05, src=scratch, dst=scratch), "loss_5_gaps": lambda: send(0.05, plc=gaps),
             "mix": lambda: eng.mix(wav, *beside),
             "channel": lambda: eng.channel(wav, sos, out=out)}
    ms = benchlib.alternate(calls, iters, repeats, warmup=3)
    n_host = max(0, min(host_clips, B))
    host_s, lags_equal, ulps, invalid = {}, True, 0.0, 0
    M.transmit(x[0, :3000], 3000, M.table(10, 3), M.ULAW, 1)             # (imports, first-use costs)
    for r in (0.05, 0.2):
        got, st, lag = (t.cpu().numpy() for t in eng.transmit(wav, lost[r], FRAME, codec, conceal, info=True))
        invalid += int(st.sum())
        t0 = time.perf_counter()
        want = [M.transmit(x[b], L, lost_np[r][b], M.ULAW, 1) for b in range(n_host)]
        host_s[r] = round((time.perf_counter() - t0) / n_host, 5) if n_host else None
        for b, res in enumerate(want):
            lags_equal = lags_equal and bool(np.array_equal(lag[b], res.lag))
            err = np.abs(got[b].astype(np.float64) - res.y.astype(np.float64)) / np.spacing(np.maximum(np.abs(res.y), np.float32(1e-30)))
            ulps = max(ulps, float(np.max(err)))
    med = {k: statistics.median(v) for k, v in ms.items()}
    row = {"case": f"{B}x{seconds}s", "samples_per_clip": L, "frames_per_clip": K}
    for k in calls:
        s = benchlib.summary(ms[k])
        row.update({f"{k}_ms_per_call": s[0], f"{k}_ms_min": s[1], f"{k}_ms_max": s[2],
                    f"{k}_spread": round((max(ms[k]) - min(ms[k])) / statistics.median(ms[k]), 4)})
    for r in LOSS:
        t = lost_np[r].astype(np.int8)
        starts = (np.diff(np.concatenate([np.zeros((B, 1), dtype=np.int8), t], axis=1), axis=1) == 1).sum(axis=1)
        tag = f"loss_{int(round(100 * r))}"
        row.update({f"{tag}_lost_frames_per_clip_mean": round(float(t.sum(axis=1).mean()), 1),
                    f"{tag}_runs_per_clip_mean": round(float(starts.mean()), 1), f"{tag}_runs_per_clip_max": int(starts.max())})
    runs20 = max(int(row["loss_20_runs_per_clip_max"]), 1)
    row.update({"transmit_over_mix": round(med["loss_5"] / med["mix"], 3), "transmit_over_channel": round(med["loss_5"] / med["channel"], 3),
                "msamples_per_s_at_5": round(B * L / (med["loss_5"] * 1e-3) / 1e6, 1),
                "gb_per_s_at_0": round(8.0 * B * L / (med["loss_0"] * 1e-3) / 1e9, 1),
                "us_per_run_of_the_row_with_most_at_20": round((med["loss_20"] - med["loss_0"]) * 1e3 / runs20, 3),
                "host_model_s_per_clip_at_5": host_s[0.05], "host_model_s_per_clip_at_20": host_s[0.2], "host_clips_timed": n_host,
                "speedup_vs_host_at_5": None if not n_host else round(host_s[0.05] * B * 1000.0 / med["loss_5"], 1),
                "invalid_rows": invalid, "lags_equal_to_the_model": lags_equal, "max_ulps_vs_f32_of_the_model": ulps,
                "device": torch.cuda.get_device_name(0), "blocks": B})
    return row


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
    device, = benchlib.lift(rows, "device")
    line = {"metric": "transmit", "batch": a.batch, "fs": FS, "codec": "ulaw", "loss": list(LOSS), "mean_burst": BURST, "frame": FRAME,
            "pmin": PMIN, "pmax": PMAX, "window": WINDOW, "fade": FADE, "launches_per_call": 2, "iters": a.iters, "repeats": a.repeats,
            "limit_s_per_case": a.limit, "device": device, "cases": rows, "stopped": stopped, "host_threads": 1,
            "host_cpus_available": benchlib.host_cpus()}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
