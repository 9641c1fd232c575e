"""The room-response meter on the GPU (cmgan_rir_stats / Engine.rir_stats) beside the calls that make the responses it
measures, and beside a host meter.

    python tools/rir_stats_bench.py [--rooms 32] [--seconds 0.5] [--iters 10] [--repeats 5] [--host-rooms 32] [--limit 240]
                                    [--out PATH]

Prints one JSON line (and writes it to --out).  Responses at 16 kHz of --seconds each, from the default RoomSampler
(`plain`, simulated by Engine.rir) and from RoomSampler(bands=7, tilt=(0, 0.5)) (`banded`, simulated by Engine.rir_bands
with its 511-tap octave filterbank).  Cases, each isolated under --limit seconds (tools/benchlib.py): the plain bank
measured broad-band, in 3 and in 7 octave bands of 511 taps, and the banded bank in its own 7 bands.  Per case, timed in
turn in ONE session so that all see the same machine: Engine.rir_stats and the Engine.rir / Engine.rir_bands call that made
the bank; then the split of one profiled rir_stats call over its two launches; then the same measurement of the first
--host-rooms responses by a float64 numpy / scipy.signal.fftconvolve meter on one host thread (the definition of
include/cmgan_hip.h, written for speed: FFT convolution, cumulative sums, closed-form regressions), with the worst
difference of T30 between the two.  The bank's download that a host meter would need first is not in its time.

What the rooms came out as: the measured broad-band T30 over the rt60 the sampler asked Sabine's formula for (median and
the 5 % / 95 % quantiles of the ratio, over the rows whose T30 could be fitted, and how many could), and the median T30
per band.  These are findings, recorded in DESIGN.md 9l; nothing is corrected by them."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from scipy.signal import fftconvolve  # noqa: E402

import benchlib  # noqa: E402

FS, NF = 16000, 511
CASES = (("plain", 0), ("plain", 3), ("plain", 7), ("banded", 7))
DOWN = (10.0 ** -0.5, 10.0 ** -1.0, 10.0 ** -2.5, 10.0 ** -3.5)


def host_meter(h, lens, filt, fs, direct_ms=2.5):
    """T30 (and the other columns, computed and dropped) of every row and slice on the host: float64 [R, NB + 1]."""
    R = h.shape[0]
    S = 1 + (0 if filt is None else filt.shape[0])
    D = 0 if filt is None else (filt.shape[1] - 1) // 2
    w, o50 = int(np.floor(direct_ms * fs / 1000.0 + 0.5)), (fs + 10) // 20
    t30 = np.full((R, S), np.nan)
    for r in range(R):
        n = int(lens[r])
        x = h[r, :n].astype(np.float64)
        k0 = int(np.argmax(np.abs(x)))
        for s in range(S):
            y = x if s == 0 else fftconvolve(x, filt[s - 1])[D:D + n]
            e = y * y
            edc = np.cumsum(e[::-1])[::-1]
            E = edc[0]
            if not E > 0:
                continue
            lo, hi, k50 = max(k0 - w, 0), min(k0 + w, n - 1), min(k0 + o50, n)
            direct = e[lo:hi + 1].sum()
            _ = (direct / (e[:lo].sum() + e[hi + 1:].sum() + 1e-300), e[:k50].sum() / E,
                 (np.maximum(np.arange(n) - k0, 0) * e).sum() / (fs * E))
            ka = [int(np.argmax(edc <= c * E)) if np.any(edc <= c * E) else n for c in DOWN]
            for beg, end, keep in ((0, ka[1], False), (ka[0], ka[2], False), (ka[0], ka[3], True)):
                m = end - beg
                if end >= n or m < 2:
                    continue
                L = 10.0 * np.log10(edc[beg:end] / E)
                slope = fs * np.dot(np.arange(beg, end) - 0.5 * (beg + end - 1), L) / (m * (m * m - 1.0) / 12.0)
                if keep and slope < 0:
                    t30[r, s] = -60.0 / slope
    return t30


def sabine_rt60(rooms):
    """The rt60 a drawn room table asked Sabine's formula for: 0.161 V / (S alpha), alpha = 1 - beta^2 of column 9."""
    lx, ly, lz = rooms[:, 0], rooms[:, 1], rooms[:, 2]
    alpha = 1.0 - rooms[:, 9] ** 2
    return 0.161 * lx * ly * lz / (2.0 * (lx * ly + ly * lz + lx * lz) * alpha)


def run_case(a, name, NB):
    import torch
    from cmgan_amd.engine import Engine
    from cmgan_amd.mixing import RoomSampler, octave_filterbank

    if not torch.cuda.is_available():
        raise SystemExit("rir_stats_bench needs the GPU")
    torch.set_num_threads(1)
    eng = Engine()
    dev = eng.device
    R, K = a.rooms, int(round(FS * a.seconds))
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    banded = name == "banded"
    sampler = RoomSampler(generator=gen, bands=7, tilt=(0.0, 0.5), filter_taps=NF) if banded else RoomSampler(generator=gen)
    rooms, n_taps = sampler.draw(R, K, FS, device=dev)
    N = sampler.n_images(K, FS)
    out = (torch.empty(R, K, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.int32, device=dev))
    if banded:
        bands, filt = sampler.draw_bands(rooms), sampler.filters(FS, dev)
        make = lambda: eng.rir_bands(rooms, bands, n_taps, K, filt, N, fs=FS, out=out)
    else:
        filt = None if NB == 0 else octave_filterbank(FS, NB, NF).to(dev)
        make = lambda: eng.rir(rooms, n_taps, K, N, fs=FS, out=out)
    rir, length = make()
    meter = lambda: eng.rir_stats(rir, length, filt, fs=FS)
    maker = "rir_bands" if banded else "rir"
    ms = benchlib.alternate({"rir_stats": meter, maker: make}, a.iters, a.repeats, warmup=2)
    med = {k: benchlib.summary(v) for k, v in ms.items()}
    eng.set_profiling(True)
    meter()
    torch.cuda.synchronize()
    split = {}
    for kernel, t in eng.profile():
        if kernel.startswith("rir_stats"):
            split[kernel] = round(split.get(kernel, 0.0) + t, 4)
    eng.set_profiling(False)
    st = meter()
    t30 = st.t30.cpu().numpy()
    status = st.status.cpu().numpy()
    h, lens, rooms_h = rir.cpu().numpy(), length.cpu().numpy(), rooms.cpu().numpy()
    n_host = max(0, min(a.host_rooms, R))
    filt_h = None if filt is None else filt.cpu().numpy()
    host_meter(h[:1], lens[:1], filt_h, FS)                       # (warm: the FFT plans)
    t0 = time.perf_counter()
    host = host_meter(h[:n_host], lens[:n_host], filt_h, FS)
    host_ms = (time.perf_counter() - t0) * 1e3
    both = np.isfinite(host) & np.isfinite(t30[:n_host])
    worst = float(np.max(np.abs(host[both] - t30[:n_host][both]) / t30[:n_host][both])) if both.any() else None
    fitted = np.isfinite(t30[:, 0])
    ratio = t30[fitted, 0] / sabine_rt60(rooms_h)[fitted]
    q = lambda v, p: round(float(np.quantile(v, p)), 4) if v.size else None
    stats_ms, make_ms = statistics.median(ms["rir_stats"]), statistics.median(ms[maker])
    return {"case": f"{name}/NB={NB}", "bank": name, "bands": NB, "filter_taps": NF if NB else 1, "taps": K,
            "mean_n_taps": float(np.mean(lens)), "made_by": maker,
            "rir_stats_ms": med["rir_stats"][0], "rir_stats_ms_min": med["rir_stats"][1], "rir_stats_ms_max": med["rir_stats"][2],
            "made_by_ms": med[maker][0], "made_by_ms_min": med[maker][1], "made_by_ms_max": med[maker][2],
            "rir_stats_over_made_by": round(stats_ms / make_ms, 4), "launch_ms": split,
            "host_rooms": n_host, "host_threads": 1, "host_meter_ms": round(host_ms, 2),
            "host_meter_ms_scaled_to_bank": round(host_ms * R / max(n_host, 1), 2),
            "host_over_rir_stats": round(host_ms * R / max(n_host, 1) / stats_ms, 1) if n_host else None,
            "t30_host_vs_gpu_worst_rel": worst,
            "rows_with_t30": int(fitted.sum()), "rows": R, "rows_status_nonzero_broadband": int(np.count_nonzero(status[:, 0])),
            "t30_over_sabine_rt60": {"median": q(ratio, 0.5), "q05": q(ratio, 0.05), "q95": q(ratio, 0.95)},
            "sabine_rt60_median_s": q(sabine_rt60(rooms_h), 0.5),
            "t30_median_s_per_slice": [q(t30[np.isfinite(t30[:, s]), s], 0.5) for s in range(t30.shape[1])],
            "tile": int(eng.lib.cmgan_rir_stats_tile()), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-rooms", type=int, default=32)
    ap.add_argument("--limit", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", nargs=2, default=None, metavar=("BANK", "NB"), help="(internal) run one case")
    a = ap.parse_args()
    if a.case is not None:
        return benchlib.print_case(run_case(a, a.case[0], int(a.case[1])))
    rows, stopped = benchlib.run_cases(__file__, benchlib.flags(a, "rooms", "seconds", "iters", "repeats", "host_rooms"),
                                       [(f"{name}/NB={nb}", (name, nb)) for name, nb in CASES], a.limit)
    device, tile = benchlib.lift(rows, "device", "tile")
    line = {"metric": "rir_stats", "rooms": a.rooms, "rir_s": a.seconds, "fs": FS, "filter_taps": NF, "iters": a.iters,
            "repeats": a.repeats, "limit_s_per_case": a.limit, "cases": rows, "stopped": stopped, "tile": tile, "device": device,
            "host_cpus": benchlib.host_cpus()}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
