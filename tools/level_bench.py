"""The active speech level on the GPU vs the host, and beside the call it now precedes (cmgan_speech_level /
Engine.speech_level vs the same definition in float64 numpy + scipy.signal.lfilter; Engine.mix without a RIR).

    python tools/level_bench.py [--batch 32] [--iters 200] [--repeats 7] [--host-clips 4] [--limit 120] [--out PATH]

Prints one JSON line (and writes it to --out).  Two cases at 16 kHz: --batch clips of 2 s and of 10 s, seeded bursts of
noise with pauses.  Every case runs isolated under --limit seconds and the two calls are timed alternately
(tools/benchlib.py).  Per case: device ms per Engine.speech_level call and per Engine.mix call without a RIR (the median
and the spread of `repeats` measurements of `iters` calls; a level call is its four launches), the fraction of the mix call that the measurement adds, the
seconds the host takes per clip for the same definition (two lfilter passes and fifteen threshold scans in float64 on one
thread, timed on the first --host-clips clips), whether the integer counts are equal and the worst relative difference
of the three levels, and the bytes the kernels move: the clips are read twice (4 bytes a sample each time); the per-tile
states are 56 + 64 bytes per 1024 samples written and read once."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import benchlib  # noqa: E402

FS = 16000
MARGIN_DB = 15.9


def host_level(x, fs):
    """The definition of cmgan_speech_level for one clip on the host.  Returns (ms, active_ms, activity, counts [15])."""
    from scipy.signal import lfilter
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    g = np.exp(-1.0 / (0.03 * fs))
    hang = -(-fs // 5)
    q = lfilter([1.0 - g], [1.0, -g], lfilter([1.0 - g], [1.0, -g], np.abs(x)))
    idx = np.arange(n)
    a = np.zeros(15, dtype=np.int64)
    for j in range(15):
        last = np.maximum.accumulate(np.where(q >= 2.0 ** (j - 15), idx, -2 * (hang + 1)))
        a[j] = np.count_nonzero(idx - last <= hang)
    sq = float(np.dot(x, x))
    J = int(np.count_nonzero(a > 0))
    if n == 0 or sq == 0.0 or J == 0:
        return 0.0, 0.0, 0.0, a
    A = 10.0 * np.log10(sq / a[:J])
    D = A - 20.0 * np.log10(2.0 ** (np.arange(J) - 15.0))
    star = A[J - 1]
    if D[0] <= MARGIN_DB:
        star = A[0]
    else:
        for j in range(1, J):
            if D[j] <= MARGIN_DB:
                star = A[j - 1] + (D[j - 1] - MARGIN_DB) / (D[j - 1] - D[j]) * (A[j] - A[j - 1])
                break
    ms, active = sq / n, 10.0 ** (star / 10.0)
    return ms, active, ms / active, a


def clips(B, L, seed):
    """Seeded bursts of noise at levels spread over 70 dB, with pauses, peak 0.4."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, L), dtype=np.float32)
    for b in range(B):
        i = 0
        while i < L:
            m = int(rng.integers(FS // 100, FS // 2))
            amp = 10.0 ** (-float(rng.uniform(0.0, 3.5))) if rng.random() < 0.7 else 0.0
            x[b, i:i + m] = (0.1 * amp * rng.standard_normal(min(m, L - i))).astype(np.float32)
            i += m
        x[b] *= 0.4 / max(float(np.max(np.abs(x[b]))), 1e-30)
    return x


def run_case(B, seconds, iters, repeats, host_clips):
    import torch
    from cmgan_amd import _lib
    from cmgan_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("level_bench needs the GPU")
    eng = Engine()
    dev = eng.device
    tile = int(_lib.load().cmgan_speech_level_tile())
    beside = benchlib.mix_beside(np.random.default_rng(1), B, dev)
    L = seconds * FS
    x = clips(B, L, seed=seconds)
    wav = torch.from_numpy(x).to(dev)
    calls = {"level": lambda: eng.speech_level(wav, fs=FS, counts=True), "mix": lambda: eng.mix(wav, *beside)}
    ms = benchlib.alternate(calls, iters, repeats, warmup=3)
    lv, cnt = calls["level"]()
    got = torch.stack(list(lv), dim=1).cpu().numpy()
    got_cnt = cnt.cpu().numpy()
    n_host = max(1, min(host_clips, B))
    host_level(x[0, :2000], FS)                                       # (imports, first-use costs)
    t0 = time.perf_counter()
    want = [host_level(x[b], FS) for b in range(n_host)]
    host_s = (time.perf_counter() - t0) / n_host
    counts_equal = all(np.array_equal(got_cnt[b, :15], want[b][3]) for b in range(n_host))
    rel = max(abs(got[b, k] - want[b][k]) / abs(want[b][k]) for b in range(n_host) for k in range(3) if want[b][k] != 0.0)
    lm, mm = statistics.median(ms["level"]), statistics.median(ms["mix"])
    lvl, mix = benchlib.summary(ms["level"]), benchlib.summary(ms["mix"])
    nt = -(-L // tile)
    moved = B * (2 * 4 * L + nt * (56 + 64) * 2)
    return {"case": f"{B}x{seconds}s", "samples_per_clip": L, "tiles_per_clip": nt,
            "level_ms_per_call": lvl[0], "level_ms_min": lvl[1], "level_ms_max": lvl[2],
            "mix_no_rir_ms_per_call": mix[0], "mix_ms_min": mix[1], "mix_ms_max": mix[2],
            "level_over_mix": round(lm / mm, 3), "bytes_moved": moved,
            "level_gb_per_s": round(moved / (lm * 1e-3) / 1e9, 1),
            "host_float64_s_per_clip": round(host_s, 5), "host_clips_timed": n_host,
            "speedup_vs_host": round(host_s * B * 1000.0 / lm, 1),
            "counts_equal_host": bool(counts_equal), "max_rel_diff_levels_vs_host": float(rel),
            "mean_activity": float(np.mean(got[:, 2])), "device": torch.cuda.get_device_name(0), "tile": tile}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-clips", type=int, default=4)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", type=int, default=None, metavar="SECONDS", help="(internal) run one case")
    a = ap.parse_args()
    if a.case is not None:
        return benchlib.print_case(run_case(a.batch, a.case, a.iters, a.repeats, a.host_clips))
    rows, stopped = benchlib.run_cases(__file__, benchlib.flags(a, "batch", "iters", "repeats", "host_clips"),
                                       [(f"{sec}s", (sec,)) for sec in (2, 10)], a.limit)
    device, tile = benchlib.lift(rows, "device", "tile")
    line = {"metric": "speech_level", "batch": a.batch, "fs": FS, "tile": tile, "launches_per_call": 4, "iters": a.iters,
            "repeats": a.repeats, "limit_s_per_case": a.limit, "cases": rows, "stopped": stopped, "host_threads": 1,
            "host_cpus_available": benchlib.host_cpus(), "mix_no_rir_ms_r09": 0.046, "device": device}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
