"""Dynamic mixing on the GPU vs the host (cmgan_mix / Engine.mix vs a float64 numpy / scipy mixer).

    python tools/mix_bench.py [--batch 32] [--seconds 2] [--rir-seconds 0.5] [--iters 50] [--repeats 5] [--limit 120]
                              [--out PATH]

Prints one JSON line (and writes it to --out).  For B clips of the given length at 16 kHz, without a RIR and with RIRs of
--rir-seconds, each of the two an isolated case under --limit seconds (tools/benchlib.py): device ms per Engine.mix call
(the median and the spread of `repeats` measurements of `iters` calls; a call is all of its launches), and the seconds the host takes to mix the same batch with
the same draws in float64 - scipy.signal.fftconvolve for the reverberation, numpy for the rest - at numpy's and scipy's
default threading (one thread: scipy.fft workers = 1, the other operations are element-wise), plus the worst difference
between the two results over the batch's peak."""
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


def host_mix(clean, bank, start, length, off, snr, rir, idx, rlen, peak, early):
    """The semantics of cmgan_mix in float64 on the host, a row at a time.  Returns (noisy, target) float32."""
    from scipy.signal import fftconvolve
    B, L = clean.shape
    noisy, target = np.empty((B, L), np.float32), np.empty((B, L), np.float32)
    bank64 = bank.astype(np.float64)
    for b in range(B):
        x = clean[b].astype(np.float64)
        if rir is None:
            speech, tgt = x, x
        else:
            h = rir[idx[b], :rlen[b]].astype(np.float64)
            d = int(np.argmax(np.abs(h)))
            speech = np.zeros(L)
            full = fftconvolve(x, h)
            n = min(L, full.size - d)
            speech[:n] = full[d:d + n]
            if early < 0:
                tgt = x
            else:
                tgt = np.zeros(L)
                full = fftconvolve(x, h[:min(d + early, h.size - 1) + 1])
                n = min(L, full.size - d)
                tgt[:n] = full[d:d + n]
        nz = bank64[start[b] + (off[b] + np.arange(L)) % length[b]]
        ps, pn = np.mean(speech * speech), np.mean(nz * nz)
        g = 0.0 if ps == 0.0 or pn == 0.0 else np.sqrt(ps / (pn * 10.0 ** (float(snr[b]) / 10.0)))
        v = speech + g * nz
        m = np.max(np.abs(v))
        s = peak / m if m > peak else 1.0
        noisy[b], target[b] = v * s, tgt * s
    return noisy, target


def run_case(a, name):
    import torch
    from cmgan_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("mix_bench needs the GPU")
    eng = Engine()
    dev = eng.device
    B, L, K = a.batch, int(FS * a.seconds), int(FS * a.rir_seconds)
    rng = np.random.default_rng(0)
    clean = (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    items = [rng.standard_normal(n).astype(np.float32) for n in (5 * FS, 3 * FS, FS // 2, 7 * FS)]
    bank = np.concatenate(items)
    lens = np.array([it.size for it in items], dtype=np.int64)
    item = rng.integers(0, len(items), B)
    start, length = (np.cumsum(lens) - lens)[item], lens[item]
    off = (rng.random(B) * length).astype(np.int64)
    snr = rng.uniform(0.0, 20.0, B).astype(np.float32)
    R = 8
    rir = (rng.standard_normal((R, K)) * np.exp(-np.arange(K) / (0.15 * K))).astype(np.float32)
    rir[:, 40] = 3.0                                             # a direct path after a short onset
    idx = rng.integers(0, R, B).astype(np.int32)
    rlen = np.full(B, K, dtype=np.int32)
    peak, early = float(np.float32(0.99)), int(0.05 * FS)
    t = lambda v: torch.from_numpy(v).to(dev)
    d_clean, d_bank, d_start, d_len, d_off, d_snr = t(clean), t(bank), t(start), t(length), t(off), t(snr)
    d_rir, d_idx, d_rlen = t(rir), t(idx), t(rlen)
    with_rir = name == "rir"
    call = (lambda: eng.mix(d_clean, d_bank, d_start, d_len, d_off, d_snr, d_rir, d_idx, d_rlen, peak=peak, early=early)) \
        if with_rir else (lambda: eng.mix(d_clean, d_bank, d_start, d_len, d_off, d_snr, peak=peak))
    ms = benchlib.alternate({name: call}, a.iters, a.repeats, warmup=5)[name]
    noisy, target, info = call()
    host_args = (clean, bank, start, length, off, snr) + ((rir, idx, rlen, peak, early) if with_rir
                                                          else (None, None, None, peak, -1))
    host_mix(*[v[:1] if i in (0,) else v for i, v in enumerate(host_args)])           # (imports, FFT plans)
    t0 = time.perf_counter()
    want_n, want_t = host_mix(*host_args)
    host_s = time.perf_counter() - t0
    pk = float(np.max(np.abs(want_n)))
    err = max(float(np.max(np.abs(noisy.cpu().numpy() - want_n))), float(np.max(np.abs(target.cpu().numpy() - want_t)))) / pk
    dev_ms, (med, lo, hi) = statistics.median(ms), benchlib.summary(ms)
    return {"case": name, "rir_taps": K if with_rir else 0, "early_samples": early if with_rir else -1,
            "device_ms_per_call": med, "device_ms_min": lo, "device_ms_max": hi,
            "fma_per_call": int(B) * L * (K if with_rir else 1),
            "host_float64_s": round(host_s, 4), "speedup_vs_host": round(host_s * 1000.0 / dev_ms, 1),
            "max_err_over_peak_vs_host": err, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rir-seconds", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", choices=("no_rir", "rir"), default=None, help="(internal) run one case")
    a = ap.parse_args()
    if a.case is not None:
        return benchlib.print_case(run_case(a, a.case))
    rows, stopped = benchlib.run_cases(__file__, benchlib.flags(a, "batch", "seconds", "rir_seconds", "iters", "repeats"),
                                       [(name, (name,)) for name in ("no_rir", "rir")], a.limit)
    device, = benchlib.lift(rows, "device")
    line = {"metric": "mix", "batch": a.batch, "clip_s": a.seconds, "rir_s": a.rir_seconds, "fs": FS, "iters": a.iters,
            "repeats": a.repeats, "limit_s_per_case": a.limit, "cases": rows, "stopped": stopped, "host_threads": 1,
            "host_cpus_available": benchlib.host_cpus(), "train_step_ms_batch32": 157.0, "device": device}
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
