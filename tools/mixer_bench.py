"""Host cost of a DynamicMixer call: wall clock per `mixer(clean)` at the training shape.

    python tools/mixer_bench.py [--root DIR] [--label NAME] [--batch 32] [--seconds 2] [--rir-seconds 0.5] [--calls 200]
                                [--repeats 5] [--out PATH]

The mixer is host-bound Python around small launches, so what a change to cmgan_amd/mixing.py can move is the time per
call, not the kernels.  For configuration 1 (defaults) and configuration 12 (every stage at once: rooms, levels, channel,
speed, tempo, pitch, sources) of tests/mixer_cases.py at the given shape, prints one JSON line (and writes it to --out):
the wall clock around `calls` calls after a warm-up with one torch.cuda.synchronize() at the end, per call, as the median
and the spread of `repeats` such measurements (the loop is tools/benchlib.py's; the tool stays in one process: it times
the host).  --root names the tree whose cmgan_amd package is timed (default: this
one); set CMGAN_HIP_LIB to time two trees' Python against one built library in the same session."""
import argparse
import os
import sys
import time

import benchlib

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--label", default="")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rir-seconds", type=float, default=0.5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import torch
    import cmgan_amd
    from cmgan_amd.engine import Engine
    from cmgan_amd.mixing import ChannelSampler, DynamicMixer, NoiseBank, RoomSampler

    if not torch.cuda.is_available():
        raise SystemExit("mixer_bench needs the GPU")
    eng = Engine()
    dev = eng.device
    B, L = a.batch, int(FS * a.seconds)
    rng = np.random.default_rng(0)
    clean = torch.from_numpy((0.1 * rng.standard_normal((B, L))).astype(np.float32)).to(dev)
    noise = NoiseBank.from_arrays([rng.standard_normal(n).astype(np.float32) for n in (5 * FS, 3 * FS, FS // 2, 7 * FS)], device=dev)
    talkers = NoiseBank.from_arrays([rng.standard_normal(n).astype(np.float32) for n in (4 * FS, 6 * FS)], device=dev)
    gen = lambda s: torch.Generator(device=dev).manual_seed(s)
    configs = {
        "defaults": lambda: DynamicMixer(eng, noise, generator=gen(1)),
        "everything": lambda: DynamicMixer(
            eng, noise, generator=gen(1), rooms=RoomSampler(generator=gen(2)), rir_seconds=a.rir_seconds, p_reverb=0.5,
            early_ms=20, snr_on="active", level_db=(-30, -20), channel=ChannelSampler(generator=gen(3)), channel_on="both",
            speed=(0.9, 1.1), p_speed=0.5, tempo=(0.9, 1.1), p_tempo=0.5, pitch=(-2, 2), sources=(0, 2), source_bank=talkers,
            source_snr_db=(0, 10)),
    }

    def wall_ms(call, calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000.0 / calls

    rows = []
    for name, make in configs.items():
        mixer = make()
        ms = benchlib.alternate({name: lambda: mixer(clean)}, a.calls, a.repeats, warmup=10, timer=wall_ms)[name]
        med, lo, hi = benchlib.summary(ms)
        rows.append({"case": name, "ms_per_call": med, "ms_min": lo, "ms_max": hi, "repeats_ms": [round(v, 4) for v in ms]})
    line = {"metric": "mixer_call", "label": a.label, "package": os.path.relpath(os.path.dirname(os.path.abspath(cmgan_amd.__file__)), HERE),
            "batch": B, "clip_s": a.seconds, "rir_s": a.rir_seconds, "fs": FS, "calls": a.calls, "repeats": a.repeats,
            "cases": rows, "device": torch.cuda.get_device_name(0)}
    benchlib.emit(line, a.out)


if __name__ == "__main__":
    main()
