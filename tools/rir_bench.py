"""Room impulse responses on the GPU vs the host (cmgan_rir / Engine.rir vs the image-source method in float64 numpy).

    python tools/rir_bench.py [--rooms 32] [--seconds 0.5] [--iters 10] [--repeats 5] [--host-rooms 2] [--limit 120]
                              [--out PATH]

Prints one JSON line (and writes it to --out).  Two cases at 16 kHz, c = 343 m/s, tw = 40: `fixed`, --rooms copies of a
6 x 5 x 3 m room at rt60 0.5 s with their own source / receiver positions, and `sampled`, --rooms rooms drawn by the
default RoomSampler, both with the image ranges RoomSampler.n_images gives and both drawn from one generator in that
order, each an isolated case under --limit seconds (tools/benchlib.py; the second case replays the first one's draw).
Per case: device ms per Engine.rir call (the median and the spread of `repeats` measurements of `iters` calls; a call is
both of its launches), the seconds the host takes per room for the same sum, vectorised over images in float64 numpy on
one thread (measured on the first --host-rooms rooms), the worst difference between the two over the response's peak,
and the work: the images that reach the responses, the (image, tap) pairs inside a window - 9 float64 operations each
as the kernel writes them - and the list entries the threads visit, one add + compare each."""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import benchlib  # noqa: E402

FS, C, TW, DMIN = 16000, 343.0, 40, 0.01
FP64_VECTOR_PEAK_TFLOPS = 78.6                                   # MI355X data sheet
CASES = ("fixed_6x5x3_rt60_0.5", "default_room_sampler")


def host_images(room, N):
    """(tau in samples, amplitude) of every image of one room, float64."""
    L, s, m, b = room[0:3], room[3:6], room[6:9], room[9:15].reshape(3, 2)
    off, coef = [], []
    for ax in range(3):
        n = np.arange(-N[ax], N[ax] + 1, dtype=np.float64)[:, None]
        p = np.array([0.0, 1.0])[None, :]
        off.append(((1 - 2 * p) * s[ax] + 2 * n * L[ax] - m[ax]).ravel())
        coef.append((b[ax, 0] ** np.abs(n - p) * b[ax, 1] ** np.abs(n)).ravel())
    d = np.sqrt(off[0][:, None, None] ** 2 + off[1][None, :, None] ** 2 + off[2][None, None, :] ** 2).ravel()
    a = (coef[0][:, None, None] * coef[1][None, :, None] * coef[2][None, None, :]).ravel() / (4 * np.pi * np.maximum(d, DMIN))
    return d * FS / C, a


def host_rir(room, n_taps, K, N, chunk=40000):
    """The definition of cmgan_rir for one room on the host.  Returns float64 [K]."""
    tau, a = host_images(room, N)
    keep = tau - TW < n_taps
    tau, a = tau[keep], a[keep]
    h = np.zeros(K)
    span = np.arange(0, 2 * TW + 2)[None, :]
    for i in range(0, tau.size, chunk):
        ta, aa = tau[i:i + chunk, None], a[i:i + chunk, None]
        k = np.floor(ta).astype(np.int64) - TW + span
        t = k - ta
        inside = (np.abs(t) < TW) & (k >= 0) & (k < n_taps)
        with np.errstate(invalid="ignore", divide="ignore"):
            v = aa * 0.5 * (1 + np.cos(np.pi * t / TW)) * np.where(t == 0, 1.0, np.sin(np.pi * t) / (np.pi * t))
        h += np.bincount(k[inside], weights=v[inside], minlength=K)
    return h


def work(rooms, n_taps, K, N, tile):
    """(images that reach a response, (image, tap) pairs inside a window, list entries visited by the threads)."""
    images = pairs = visits = 0
    for room, kr in zip(rooms, n_taps):
        tau = np.sort(host_images(room, N)[0])
        tau = tau[tau - TW < kr]
        images += tau.size
        lo = np.maximum(np.floor(tau - TW).astype(np.int64) + 1, 0)
        hi = np.minimum(np.ceil(tau + TW).astype(np.int64) - 1, kr - 1)
        pairs += int(np.sum(np.maximum(hi - lo + 1, 0)))
        for k0 in range(0, int(kr), tile):
            k_last = min(k0 + tile, int(kr)) - 1
            n = np.searchsorted(tau, k_last + TW, "left") - np.searchsorted(tau, k0 - TW, "right")
            visits += int(n) * (k_last - k0 + 1)
    return images, pairs, visits


def run_case(a, name):
    import torch
    from cmgan_amd import _lib
    from cmgan_amd.engine import Engine
    from cmgan_amd.mixing import RoomSampler

    if not torch.cuda.is_available():
        raise SystemExit("rir_bench needs the GPU")
    eng = Engine()
    dev = eng.device
    tile = int(_lib.load().cmgan_rir_tile())
    R, K = a.rooms, int(round(FS * a.seconds))
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    size = (6.0, 5.0, 3.0)
    samplers = (RoomSampler(dims=(size, size), rt60=(0.5, 0.5), generator=gen), RoomSampler(generator=gen))
    for sampler in samplers[:CASES.index(name) + 1]:             # (the draws before this case's move the generator)
        rooms, n_taps = sampler.draw(R, K, FS, device=dev)
    N = sampler.n_images(K, FS, C, TW)
    call = lambda: eng.rir(rooms, n_taps, K, N, fs=FS, c=C, tw=TW)
    ms = benchlib.alternate({name: call}, a.iters, a.repeats, warmup=2)[name]
    rir, length = call()
    rooms_h, taps_h, got = rooms.cpu().numpy(), n_taps.cpu().numpy(), rir.cpu().numpy()
    n_host = max(1, min(a.host_rooms, R))
    host_rir(rooms_h[0], 64, K, (1, 1, 1))                       # (imports, first-use costs)
    t0 = time.perf_counter()
    want = [host_rir(rooms_h[r], int(taps_h[r]), K, N) for r in range(n_host)]
    host_s = (time.perf_counter() - t0) / n_host
    err = max(float(np.max(np.abs(got[r] - want[r]))) / float(np.max(np.abs(want[r]))) for r in range(n_host))
    images, pairs, visits = work(rooms_h, taps_h, K, N, tile)
    dev_ms, (med, lo, hi) = statistics.median(ms), benchlib.summary(ms)
    flop = 9 * pairs + 2 * visits
    return {"case": name, "taps": K, "n_images": list(N), "images_enumerated_per_room": 8 * math.prod(2 * n + 1 for n in N),
            "images_reaching": images, "pairs_in_window": pairs, "list_entries_visited": visits,
            "device_ms_per_call": med, "device_ms_min": lo, "device_ms_max": hi,
            "device_ms_per_room": round(dev_ms / R, 5), "float64_flop": flop,
            "float64_tflops": round(flop / (dev_ms * 1e-3) / 1e12, 3),
            "frac_of_fp64_vector_peak": round(flop / (dev_ms * 1e-3) / 1e12 / FP64_VECTOR_PEAK_TFLOPS, 4),
            "host_float64_s_per_room": round(host_s, 4), "host_rooms_timed": n_host,
            "speedup_vs_host": round(host_s * R * 1000.0 / dev_ms, 1), "max_err_over_peak_vs_host": err,
            "mean_n_taps": float(np.mean(taps_h)), "device": torch.cuda.get_device_name(0), "tile": tile}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-rooms", type=int, default=2)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", choices=CASES, default=None, help="(internal) run one case")
    a = ap.parse_args()
    if a.case is not None:
        return benchlib.print_case(run_case(a, a.case))
    rows, stopped = benchlib.run_cases(__file__, benchlib.flags(a, "rooms", "seconds", "iters", "repeats", "host_rooms"),
                                       [(name, (name,)) for name in CASES], a.limit)
    device, tile = benchlib.lift(rows, "device", "tile")
    line = {"metric": "rir", "rooms": a.rooms, "rir_s": a.seconds, "fs": FS, "c": C, "tw": TW, "tile": tile, "iters": a.iters,
            "repeats": a.repeats, "limit_s_per_case": a.limit, "cases": rows, "stopped": stopped, "host_threads": 1,
            "host_cpus_available": benchlib.host_cpus(), "fp64_vector_peak_tflops": FP64_VECTOR_PEAK_TFLOPS,
            "train_step_ms_batch32": 157.0, "device": device}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
