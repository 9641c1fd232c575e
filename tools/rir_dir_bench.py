"""Directional room impulse responses on the GPU (cmgan_rir_dir / cmgan_rir_bands_dir: Engine.rir and Engine.rir_bands with
orient= and pattern=) beside the plain calls, and the plain calls of this build beside another checkout's.

    python tools/rir_dir_bench.py [--rooms 32] [--seconds 0.5] [--iters 10] [--repeats 5] [--limit 180] [--out PATH]
                                  [--parent-root DIR] [--ab-rounds 4]

Prints one JSON line (and writes it to --out).  Rooms at 16 kHz, c = 343 m/s, tw = 40, as tools/rir_bench.py draws them:
`fixed`, --rooms copies of a 6 x 5 x 3 m room at rt60 0.5 s with their own source / receiver positions, and `sampled`,
--rooms rooms of the default RoomSampler; the banded calls at 7 bands of 511-tap filters with the tilt and air ranges of
tools/rir_bands_bench.py.  The directions are a directional RoomSampler's draw_dirs: talkers between hyper- and
sub-cardioid, more directional upwards by 0 .. 0.1 per octave, microphones between cardioid and omni.  Every room set is an
isolated case under --limit seconds (tools/benchlib.py); in it Engine.rir without and with the tables and Engine.rir_bands
without and with them are timed in turn in ONE session, so that all four see the same machine.  Per pair the ratio
directional / plain of the medians is given beside the spread of the --repeats measurements, (max - min) / median of each
call: a ratio inside the spread says the directional call costs what the plain one does.

--parent-root DIR: a checkout of another commit (the parent) with its library built.  The plain calls are then timed in
child processes that import the package from DIR and from this tree in turn, --ab-rounds rounds, the order reversed every
other round (tools/ab_bench.sh's scheme), and both medians over the rounds, their ratio and the spread go into the line."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FS, C, TW, NB, NF = 16000, 343.0, 40, 7, 511
ROOMS = ("fixed_6x5x3_rt60_0.5", "default_room_sampler")


def _tables(a, name, pkg_root, directional):
    """The engine and the tables of a room set, from the package under `pkg_root`."""
    sys.path.insert(0, pkg_root)
    import torch
    from cmgan_amd.engine import Engine
    from cmgan_amd.mixing import RoomSampler

    if not torch.cuda.is_available():
        raise SystemExit("rir_dir_bench needs the GPU")
    eng = Engine()
    dev = eng.device
    R, K = a.rooms, int(round(FS * a.seconds))
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    size = (6.0, 5.0, 3.0)
    kw = dict(bands=NB, tilt=(0.0, 0.5), air=[(0.0005 * (b + 1), 0.001 * (b + 1)) for b in range(NB)], filter_taps=NF)
    if directional:
        kw.update(source_pattern=(0.25, 0.75), mic_pattern=(0.5, 1.0), pattern_tilt=(0.0, 0.1))
    samplers = (RoomSampler(dims=(size, size), rt60=(0.5, 0.5), generator=gen, **kw), RoomSampler(generator=gen, **kw))
    for sampler in samplers[:ROOMS.index(name) + 1]:             # (the draws before this case's move the generator)
        rooms, n_taps = sampler.draw(R, K, FS, device=dev)
    bands = sampler.draw_bands(rooms)
    t = dict(eng=eng, rooms=rooms, n_taps=n_taps, bands=bands, filt=sampler.filters(FS, dev), K=K,
             N_bands=sampler.n_images(K, FS, C, TW), N=RoomSampler(dims=(sampler.lo, sampler.hi)).n_images(K, FS, C, TW),
             out=(torch.empty(R, K, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.int32, device=dev)),
             device=torch.cuda.get_device_name(0))
    if directional:
        t["orient"], t["pattern"] = sampler.draw_dirs(rooms)
    return t


def _plain_calls(t):
    eng = t["eng"]
    return {"rir": lambda: eng.rir(t["rooms"], t["n_taps"], t["K"], t["N"], fs=FS, c=C, tw=TW, out=t["out"]),
            "rir_bands": lambda: eng.rir_bands(t["rooms"], t["bands"], t["n_taps"], t["K"], t["filt"], t["N_bands"], fs=FS, c=C,
                                               tw=TW, out=t["out"])}


def _spread(ms):
    return round((max(ms) - min(ms)) / statistics.median(ms), 4)


def run_case(a, name):
    """Engine.rir and Engine.rir_bands, each without and with the tables, in one session."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import benchlib
    t = _tables(a, name, ROOT, True)
    eng, o, p = t["eng"], t["orient"], t["pattern"]
    calls = _plain_calls(t)
    p1 = p[:, 3:4].contiguous()                                   # the single-band call: the 1 kHz band's pair
    calls["rir_dir"] = lambda: eng.rir(t["rooms"], t["n_taps"], t["K"], t["N"], fs=FS, c=C, tw=TW, out=t["out"], orient=o, pattern=p1)
    calls["rir_bands_dir"] = lambda: eng.rir_bands(t["rooms"], t["bands"], t["n_taps"], t["K"], t["filt"], t["N_bands"], fs=FS,
                                                   c=C, tw=TW, out=t["out"], orient=o, pattern=p)
    order = {k: calls[k] for k in ("rir", "rir_dir", "rir_bands", "rir_bands_dir")}
    ms = benchlib.alternate(order, a.iters, a.repeats, warmup=2)
    row = {"case": name, "taps": t["K"], "bands": NB, "filter_taps": NF, "n_images": list(t["N"]), "n_images_bands": list(t["N_bands"]),
           "device": t["device"]}
    for k, v in ms.items():
        med, lo, hi = benchlib.summary(v)
        row.update({k + "_ms": med, k + "_ms_min": lo, k + "_ms_max": hi, k + "_spread": _spread(v)})
    row["rir_dir_over_rir"] = round(statistics.median(ms["rir_dir"]) / statistics.median(ms["rir"]), 4)
    row["rir_bands_dir_over_rir_bands"] = round(statistics.median(ms["rir_bands_dir"]) / statistics.median(ms["rir_bands"]), 4)
    return row


def run_plain(a, name, which):
    """The plain calls alone, from the package of this tree ("this") or of --parent-root ("parent")."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import benchlib
    t = _tables(a, name, ROOT if which == "this" else os.path.abspath(a.parent_root), False)
    ms = benchlib.alternate(_plain_calls(t), a.iters, a.repeats, warmup=2)
    return {"case": name, "build": which, "rir_ms": ms["rir"], "rir_bands_ms": ms["rir_bands"], "device": t["device"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=float, default=180.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--ab-rounds", type=int, default=4)
    ap.add_argument("--case", nargs="+", default=None, metavar="ARG", help="(internal) run one case")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import benchlib
    if a.case is not None:
        return benchlib.print_case(run_case(a, a.case[0]) if len(a.case) == 1 else run_plain(a, a.case[0], a.case[1]))
    common = benchlib.flags(a, "rooms", "seconds", "iters", "repeats")
    rows, stopped = benchlib.run_cases(__file__, common, [(name, (name,)) for name in ROOMS], a.limit)
    (device,) = benchlib.lift(rows, "device")
    line = {"metric": "rir_dir", "rooms": a.rooms, "rir_s": a.seconds, "fs": FS, "c": C, "tw": TW, "bands": NB, "filter_taps": NF,
            "iters": a.iters, "repeats": a.repeats, "limit_s_per_case": a.limit, "cases": rows, "device": device}
    if a.parent_root is not None and not stopped:
        cases = []
        for rnd in range(a.ab_rounds):
            for which in (("this", "parent") if rnd % 2 == 0 else ("parent", "this")):
                cases += [(f"{name}/{which}/round{rnd + 1}", (name, which)) for name in ROOMS]
        ab, stopped = benchlib.run_cases(__file__, common + ["--parent-root", a.parent_root], cases, a.limit)
        out = []
        for name in ROOMS:
            row = {"case": name, "rounds": a.ab_rounds}
            for call in ("rir", "rir_bands"):
                per = {w: [statistics.median(r[call + "_ms"]) for r in ab if r["case"] == name and r["build"] == w]
                       for w in ("this", "parent")}
                if not (per["this"] and per["parent"]):
                    continue
                for w, v in per.items():
                    row.update({f"{call}_{w}_ms": round(statistics.median(v), 4), f"{call}_{w}_spread": _spread(v)})
                row[f"{call}_this_over_parent"] = round(statistics.median(per["this"]) / statistics.median(per["parent"]), 4)
            out.append(row)
        line["plain_calls_this_build_beside_parent"] = out
    line["stopped"] = stopped
    benchlib.emit(line, a.out, stopped)


if __name__ == "__main__":
    main()
