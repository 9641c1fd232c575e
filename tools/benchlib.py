"""What the feature benchmarks under tools/ share: timing, case isolation and output.  Plain functions, no state.

Timing.  `event_ms` is milliseconds per call from one pair of HIP events around `iters` calls; `alternate` warms every
call up, synchronizes, then times the calls in turn, `repeats` rounds, so that all of them see the same machine;
`summary` is the (median, min, max) a tool reports.

Isolation.  `run_cases` is the parent side: every case runs in a fresh `python <tool> ... --case ...` process under a time
limit, one child at a time, and after a case that fails, prints no row or runs out of time no further case is started.
The parent never opens the GPU, so a fault in a case cannot leave a second process on the card.  `print_case` is the
child side.

Output.  `emit` prints the tool's one JSON line, writes it to --out when one is given (there is no default: an evidence
file under profiles/ is written only by asking for it) and exits with status 1 when the run was stopped."""
import json
import os
import statistics
import subprocess
import sys

FS = 16000


def event_ms(call, iters):
    """Device ms per call: HIP events around `iters` calls, then one synchronize."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def cuda_sync():
    import torch
    torch.cuda.synchronize()


def alternate(calls, iters, repeats, warmup, timer=event_ms, sync=cuda_sync):
    """{name: [timer(call, iters)] * repeats} for the ordered mapping name -> call."""
    for _ in range(warmup):
        for c in calls.values():
            c()
    sync()
    ms = {k: [] for k in calls}
    for _ in range(repeats):
        for k, c in calls.items():
            ms[k].append(timer(c, iters))
    return ms


def summary(ms, places=4):
    """(median, min, max) of the measurements, rounded."""
    return round(statistics.median(ms), places), round(min(ms), places), round(max(ms), places)


def flags(a, *names):
    """The parsed options `names` of `a` as command-line arguments, for a child."""
    return [v for n in names for v in ("--" + n.replace("_", "-"), str(getattr(a, n)))]


def run_cases(tool, common, cases, limit):
    """Runs `python tool *common --case *args` for every (label, args) of `cases`.  Returns (rows, stopped)."""
    rows = []
    for label, args in cases:
        cmd = [sys.executable, os.path.abspath(tool), *map(str, common), "--case", *map(str, args)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)      # (kills and reaps the child)
        except subprocess.TimeoutExpired:
            return rows, f"{label}: no result within {limit} s"
        line = next((l for l in r.stdout.splitlines() if l.startswith("CASE ")), None)
        if r.returncode != 0 or line is None:
            return rows, f"{label}: exit status {r.returncode}: {r.stderr.strip()[-400:]}"
        rows.append(json.loads(line[5:]))
    return rows, None


def print_case(row):
    print("CASE " + json.dumps(row), flush=True)


def lift(rows, *keys):
    """Takes `keys` (what only a child can report: the device, a tile size) out of every row, for the tool's line: the
    first row's values, None without rows."""
    vals = [[r.pop(k) for k in keys] for r in rows]
    return vals[0] if vals else [None] * len(keys)


def host_cpus():
    return len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()


def emit(line, out=None, stopped=None):
    s = json.dumps(line)
    print(s)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(s + "\n")
    if stopped:
        raise SystemExit(1)


def mix_beside(rng, B, dev):
    """(bank, start, length, off, snr) of the Engine.mix call without a RIR that a tool times beside its own: a 10 s
    noise bank drawn from `rng`, every row looping all of it from its own offset, SNRs from 0 to 20 dB."""
    import numpy as np
    import torch
    bank = torch.from_numpy((0.1 * rng.standard_normal(10 * FS)).astype(np.float32)).to(dev)
    start = torch.zeros(B, dtype=torch.int64, device=dev)
    length = torch.full((B,), bank.numel(), dtype=torch.int64, device=dev)
    off = torch.arange(B, dtype=torch.int64, device=dev) * 977
    snr = torch.linspace(0.0, 20.0, B, dtype=torch.float32, device=dev)
    return bank, start, length, off, snr
