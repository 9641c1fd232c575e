"""Banded room impulse responses on the GPU (cmgan_rir_bands / Engine.rir_bands) beside the textbook multi-band method,
NB calls of Engine.rir.

    python tools/rir_bands_bench.py [--rooms 32] [--seconds 0.5] [--iters 10] [--repeats 5] [--host-rooms 1] [--limit 180]
                                    [--out PATH]

Prints one JSON line (and writes it to --out).  Rooms at 16 kHz, c = 343 m/s, tw = 40, as tools/rir_bench.py draws them:
`fixed`, --rooms copies of a 6 x 5 x 3 m room at rt60 0.5 s with their own source / receiver positions, and `sampled`,
--rooms rooms of the default RoomSampler; each with NB = 1, 3 and 7 bands of 511-tap filters (octave_filterbank), a tilt
drawn in (0, 0.5) and an air attenuation drawn per band in ranges chosen for this tool only (they stand for no
atmosphere; a non-zero m makes the kernel pay its exp per image and band).  Every (rooms, NB) pair is an isolated case
under --limit seconds (tools/benchlib.py).  Per case, timed in turn in ONE session so that all see the same machine:
Engine.rir_bands, ONE Engine.rir call and NB Engine.rir calls (the band-pass filters and the sum that the textbook method
still needs after them are NOT included: the comparison favours it).  Then the split of one profiled rir_bands call over
its launches, and the worst difference from the float64 model of tests/rir_bands_model.py on the first --host-rooms rooms,
over its bound and over the response's peak."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import benchlib  # noqa: E402

FS, C, TW, NF = 16000, 343.0, 40, 511
ROOMS = ("fixed_6x5x3_rt60_0.5", "default_room_sampler")
BANDS = (1, 3, 7)
TRAIN_STEP_MS = 157.0


def run_case(a, name, NB):
    import torch
    from cmgan_amd.engine import Engine
    from cmgan_amd.mixing import RoomSampler

    import rir_bands_model as BM

    if not torch.cuda.is_available():
        raise SystemExit("rir_bands_bench needs the GPU")
    eng = Engine()
    dev = eng.device
    R, K = a.rooms, int(round(FS * a.seconds))
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    size = (6.0, 5.0, 3.0)
    band_kw = dict(bands=NB, tilt=(0.0, 0.5), air=[(0.0005 * (b + 1), 0.001 * (b + 1)) for b in range(NB)], filter_taps=NF)
    samplers = (RoomSampler(dims=(size, size), rt60=(0.5, 0.5), generator=gen, **band_kw), RoomSampler(generator=gen, **band_kw))
    for sampler in samplers[:ROOMS.index(name) + 1]:             # (the draws before this case's move the generator)
        rooms, n_taps = sampler.draw(R, K, FS, device=dev)
    bands = sampler.draw_bands(rooms)
    filt = sampler.filters(FS, dev)
    N = sampler.n_images(K, FS, C, TW)                           # covers K + D taps
    N1 = RoomSampler(dims=(sampler.lo, sampler.hi)).n_images(K, FS, C, TW)      # what one Engine.rir call needs
    out = (torch.empty(R, K, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.int32, device=dev))
    fused = lambda: eng.rir_bands(rooms, bands, n_taps, K, filt, N, fs=FS, c=C, tw=TW, out=out)
    tables = [torch.cat([rooms[:, 0:9], bands[:, b, 0:6]], dim=1).contiguous() for b in range(NB)]
    outs = [(torch.empty_like(out[0]), torch.empty_like(out[1])) for _ in range(NB)]
    one = lambda: eng.rir(tables[0], n_taps, K, N1, fs=FS, c=C, tw=TW, out=outs[0])

    def textbook():
        for b in range(NB):
            eng.rir(tables[b], n_taps, K, N1, fs=FS, c=C, tw=TW, out=outs[b])

    ms = benchlib.alternate({"rir_bands": fused, "rir_once": one, "rir_nb_times": textbook}, a.iters, a.repeats, warmup=2)
    med = {k: benchlib.summary(v) for k, v in ms.items()}
    eng.set_profiling(True)
    fused()
    torch.cuda.synchronize()
    split = {}
    for kernel, t in eng.profile():
        if kernel.startswith("rir_bands"):
            split[kernel] = round(split.get(kernel, 0.0) + t, 4)
    eng.set_profiling(False)
    got = fused()[0].cpu().numpy()
    rooms_h, bands_h, taps_h, filt_h = rooms.cpu().numpy(), bands.cpu().numpy(), n_taps.cpu().numpy(), filt.cpu().numpy()
    over_bound = over_peak = 0.0
    n_host = max(0, min(a.host_rooms, R))
    for r in range(n_host):
        h, bound, _, _, _ = BM.rir_bands_row(rooms_h[r], bands_h[r], int(taps_h[r]), K, N, filt_h, FS, C, TW)
        err = np.abs(got[r] - h)
        over_bound = max(over_bound, float(np.max(err[bound > 0] / bound[bound > 0])))
        over_peak = max(over_peak, float(np.max(err)) / float(np.max(np.abs(h))))
    fused_ms, once_ms, nb_ms = (statistics.median(ms[k]) for k in ("rir_bands", "rir_once", "rir_nb_times"))
    return {"case": f"{name}/NB={NB}", "bands": NB, "filter_taps": NF, "taps": K, "n_images": list(N), "n_images_rir": list(N1),
            "rir_bands_ms": med["rir_bands"][0], "rir_bands_ms_min": med["rir_bands"][1], "rir_bands_ms_max": med["rir_bands"][2],
            "rir_once_ms": med["rir_once"][0], "rir_once_ms_min": med["rir_once"][1], "rir_once_ms_max": med["rir_once"][2],
            "rir_nb_times_ms": med["rir_nb_times"][0], "rir_nb_times_ms_min": med["rir_nb_times"][1],
            "rir_nb_times_ms_max": med["rir_nb_times"][2],
            "launch_ms": split, "rir_bands_over_rir_once": round(fused_ms / once_ms, 3),
            "rir_bands_over_rir_nb_times": round(fused_ms / nb_ms, 3), "rir_bands_over_train_step": round(fused_ms / TRAIN_STEP_MS, 4),
            "host_rooms_checked": n_host, "max_err_over_bound": over_bound, "max_err_over_peak": over_peak,
            "mean_n_taps": float(np.mean(taps_h)), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-rooms", type=int, default=1)
    ap.add_argument("--limit", type=float, default=180.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", nargs=2, default=None, metavar=("ROOMS", "NB"), help="(internal) run one case")
    a = ap.parse_args()
    if a.case is not None:
        return benchlib.print_case(run_case(a, a.case[0], int(a.case[1])))
    rows, stopped = benchlib.run_cases(__file__, benchlib.flags(a, "rooms", "seconds", "iters", "repeats", "host_rooms"),
                                       [(f"{name}/NB={nb}", (name, nb)) for name in ROOMS for nb in BANDS], a.limit)
    (device,) = benchlib.lift(rows, "device")
    line = {"metric": "rir_bands", "rooms": a.rooms, "rir_s": a.seconds, "fs": FS, "c": C, "tw": TW, "filter_taps": NF,
            "iters": a.iters, "repeats": a.repeats, "limit_s_per_case": a.limit, "cases": rows, "stopped": stopped,
            "train_step_ms_batch32": TRAIN_STEP_MS, "device": device}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
