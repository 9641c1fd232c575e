"""The hybrid room simulator - the image-source method to a junction, then the diffuse tail of cmgan_rir_tail /
Engine.rir_tail - beside the image-source method run to the end.

    python tools/rir_tail_bench.py [--rooms 32] [--seconds 1.0] [--tail-ms 80] [--iters 5] [--repeats 5] [--limit 400] [--out PATH]

Prints one JSON line (and writes it to --out).  Responses at 16 kHz of --seconds each in rooms of the default sizes with rt60
in (0.4, 1.2) s: `plain` (RoomSampler, Engine.rir) and `banded` (RoomSampler(bands=7, tilt=(0, 0.5)), Engine.rir_bands with
its 511-tap octave filterbank).  Both samplers of a case are seeded alike, so the full and the hybrid bank hold the same
rooms.  Cases, each isolated under --limit seconds (tools/benchlib.py).  Per case, timed in turn in ONE session so that all
see the same machine: `full`, the image-source call for the whole length with the image ranges that needs; `hybrid`, the
image-source call to the junctions (--tail-ms after the direct sound, with the smaller ranges RoomSampler(tail_ms=).n_images
gives) followed by Engine.rir_tail; `early`, that short image-source call alone; `tail`, Engine.rir_tail alone (with the copy
that puts the junctions back into the lengths it rewrites).  Then the split of one profiled rir_tail call over its two
launches.

What came out, by Engine.rir_stats on both banks: the median of T30 over the decay time that was given, per column, over the
rows whose T30 could be fitted (and how many could); and per row the energy of the hybrid in the 20 ms behind the junction
over the full response's there (median and the 5 % / 95 % quantiles).  These are findings, recorded in DESIGN.md 9m."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import benchlib  # noqa: E402

FS, NF = 16000, 511
CASES = ("plain", "banded")


def run_case(a, name):
    import torch
    from cmgan_amd.engine import Engine
    from cmgan_amd.mixing import RoomSampler

    if not torch.cuda.is_available():
        raise SystemExit("rir_tail_bench needs the GPU")
    torch.set_num_threads(1)
    eng = Engine()
    dev = eng.device
    R, K = a.rooms, int(round(FS * a.seconds))
    banded = name == "banded"
    kw = dict(rt60=(0.4, 1.2), **(dict(bands=7, tilt=(0.0, 0.5), filter_taps=NF) if banded else {}))

    def sampler(**more):
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        return RoomSampler(generator=gen, **kw, **more)

    full_s, hyb_s = sampler(), sampler(tail_ms=a.tail_ms)
    rooms, n_full = full_s.draw(R, K, FS, device=dev)
    rooms_h, junction = hyb_s.draw(R, K, FS, device=dev)
    assert torch.equal(rooms, rooms_h)
    bands = filt = None
    if banded:
        bands, filt = full_s.draw_bands(rooms), full_s.filters(FS, dev)
        assert torch.equal(bands, hyb_s.draw_bands(rooms))
    t = hyb_s.draw_tail(rooms, FS)
    assert torch.equal(t.n_full, n_full)
    N_full, N_short = full_s.n_images(K, FS), hyb_s.n_images(K, FS)
    new = lambda: (torch.empty(R, K, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.int32, device=dev))
    out_full, out_hyb = new(), new()

    def image_source(taps, N, out):
        if banded:
            return eng.rir_bands(rooms, bands, taps, K, filt, N, fs=FS, out=out)
        return eng.rir(rooms, taps, K, N, fs=FS, out=out)

    full = lambda: image_source(n_full, N_full, out_full)
    early = lambda: image_source(junction, N_short, out_hyb)
    extend = lambda: eng.rir_tail(*out_hyb, t.n_full, t.decay, t.seed, filt, fs=FS, window_ms=hyb_s.tail_window_ms)

    def hybrid():
        early()
        return extend()

    def tail():                                                   # on the early part left by the last `early` / `hybrid`
        out_hyb[1].copy_(junction)
        return extend()

    full()
    _, _, fit = hybrid()
    ms = benchlib.alternate({"full": full, "hybrid": hybrid, "early": early, "tail": tail}, a.iters, a.repeats, warmup=1)
    med = {k: benchlib.summary(v) for k, v in ms.items()}
    hybrid()
    eng.set_profiling(True)
    tail()
    torch.cuda.synchronize()
    split = {}
    for kernel, v in eng.profile():
        if kernel.startswith("rir_tail"):
            split[kernel] = round(split.get(kernel, 0.0) + v, 4)
    eng.set_profiling(False)
    full()
    _, _, fit = hybrid()
    q = lambda v, p: round(float(np.quantile(v, p)), 4) if v.size else None
    given = t.decay.cpu().numpy()                                 # [R, NB']
    measured = {}
    for label, (rir, length) in (("full", out_full), ("hybrid", out_hyb)):
        t30 = eng.rir_stats(rir, length, filt, fs=FS).t30.cpu().numpy()
        cols = t30[:, 1:] if banded else t30[:, :1]               # per band against its own time; plain: broad-band against rt60
        ok = np.isfinite(cols)
        ratio = np.where(ok, cols / given, np.nan)
        measured[label] = {"t30_over_given_median": q(ratio[ok], 0.5), "t30_over_given_q05": q(ratio[ok], 0.05),
                           "t30_over_given_q95": q(ratio[ok], 0.95), "fitted": int(ok.sum()), "of": int(ok.size),
                           "t30_over_given_median_per_column": [q(ratio[ok[:, c], c], 0.5) for c in range(cols.shape[1])]}
    hf, hh, kx = out_full[0].cpu().numpy().astype(np.float64), out_hyb[0].cpu().numpy().astype(np.float64), junction.cpu().numpy()
    span = int(round(0.02 * FS))
    energy = np.array([np.sum(hh[r, kx[r]:kx[r] + span] ** 2) / np.sum(hf[r, kx[r]:kx[r] + span] ** 2) for r in range(R)
                       if kx[r] + span <= int(n_full[r]) and np.any(hf[r, kx[r]:kx[r] + span])])
    full_ms, hyb_ms, early_ms, tail_ms = (statistics.median(ms[k]) for k in ("full", "hybrid", "early", "tail"))
    return {"case": name, "bands": 7 if banded else 0, "filter_taps": NF if banded else 1, "taps": K,
            "mean_junction": float(junction.float().mean()), "mean_n_full": float(n_full.float().mean()),
            "n_images_full": list(N_full), "n_images_hybrid": list(N_short),
            **{f"{k}_ms": med[k][0] for k in med}, **{f"{k}_ms_min": med[k][1] for k in med}, **{f"{k}_ms_max": med[k][2] for k in med},
            "hybrid_over_full": round(hyb_ms / full_ms, 4), "full_over_hybrid": round(full_ms / hyb_ms, 2),
            "tail_share_of_hybrid": round(tail_ms / hyb_ms, 4), "tail_over_early": round(tail_ms / early_ms, 4),
            "launch_ms": split, "rows_extended": int((fit.status == 0).sum()), "rows": R,
            "measured": measured, "tail_energy_20ms_over_full": {"median": q(energy, 0.5), "q05": q(energy, 0.05), "q95": q(energy, 0.95),
                                                                  "rows": int(energy.size)},
            "tile": int(eng.lib.cmgan_rir_tail_tile()), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--tail-ms", type=float, default=80.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=float, default=400.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", nargs=1, default=None, metavar="BANK", help="(internal) run one case")
    a = ap.parse_args()
    if a.case is not None:
        return benchlib.print_case(run_case(a, a.case[0]))
    rows, stopped = benchlib.run_cases(__file__, benchlib.flags(a, "rooms", "seconds", "tail_ms", "iters", "repeats"),
                                       [(name, (name,)) for name in CASES], a.limit)
    device, tile = benchlib.lift(rows, "device", "tile")
    line = {"metric": "rir_tail", "rooms": a.rooms, "rir_s": a.seconds, "tail_ms": a.tail_ms, "fs": FS, "rt60": [0.4, 1.2],
            "window_ms": 30.0, "iters": a.iters, "repeats": a.repeats, "limit_s_per_case": a.limit, "cases": rows,
            "stopped": stopped, "tile": tile, "device": device, "host_cpus": benchlib.host_cpus()}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
