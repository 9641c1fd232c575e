"""tools/benchlib.py, the harness under every feature benchmark, on the CPU: a case runs in a process of its own under a
time limit and nothing more is started after one that fails, prints no row or runs out of time (the rule the shared GPU
machines depend on); the calls are measured alternately after the warm-up; the summary rounds as the tools always did;
the line goes to --out only when one is given, and no tool names an output file by default."""
import argparse
import importlib
import json
import os
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import benchlib  # noqa: E402

STUB = os.path.join(ROOT, "tests", "bench_stub_tool.py")
TOOLS = ("channel_bench", "warp_bench", "scene_bench", "stretch_bench", "level_bench", "mix_bench", "rir_bench",
         "resample_bench", "metrics_bench", "mixer_bench")
WROTE_TO_PROFILES = ("channel_bench", "warp_bench", "scene_bench", "stretch_bench")       # their --out once had a default


def run_stub(tmp_path, kinds, limit=60.0):
    """(rows, stopped, labels the stub saw start, pid of the last child) for cases a, b, c ... of the given kinds."""
    marker = str(tmp_path / "started")
    cases = [(f"case {chr(97 + i)}", (kind, chr(97 + i))) for i, kind in enumerate(kinds)]
    rows, stopped = benchlib.run_cases(STUB, ["--marker", marker], cases, limit)
    with open(marker) as f:
        started = f.read().split()
    with open(marker + ".pid") as f:
        return rows, stopped, started, int(f.read())


def test_every_case_runs_in_order(tmp_path):
    rows, stopped, started, _ = run_stub(tmp_path, ["row", "row", "row"])
    assert rows == [{"case": c, "value": 1} for c in "abc"]
    assert stopped is None and started == ["a", "b", "c"]


def test_a_failing_case_stops_the_run(tmp_path):
    rows, stopped, started, _ = run_stub(tmp_path, ["row", "fail", "row"])
    assert rows == [{"case": "a", "value": 1}]
    assert stopped == "case b: exit status 3: boom in b"
    assert started == ["a", "b"]                                  # c was never started


def test_a_case_without_a_row_stops_the_run(tmp_path):
    rows, stopped, started, _ = run_stub(tmp_path, ["row", "silent", "row"])
    assert rows == [{"case": "a", "value": 1}]
    assert stopped == "case b: exit status 0: "
    assert started == ["a", "b"]


def test_a_case_out_of_time_stops_the_run_and_is_gone(tmp_path):
    t0 = time.monotonic()
    rows, stopped, started, pid = run_stub(tmp_path, ["row", "sleep", "row"], limit=1.0)
    assert time.monotonic() - t0 < 15.0                           # (process start-up, not a measurement)
    assert rows == [{"case": "a", "value": 1}]
    assert stopped == "case b: no result within 1.0 s"
    assert started == ["a", "b"]
    with pytest.raises(ProcessLookupError):                       # killed and waited for: the pid names nothing
        os.kill(pid, 0)


def test_calls_alternate_after_the_warm_up():
    log = []
    calls = {name: (lambda n=name: log.append(("call", n))) for name in ("x", "y", "z")}

    def timer(call, iters):
        call()
        log.append(("timed", log.pop()[1], iters))
        return float(len(log))

    ms = benchlib.alternate(calls, 7, repeats=3, warmup=2, timer=timer, sync=lambda: log.append("sync"))
    assert log == [("call", n) for n in "xyzxyz"] + ["sync"] + [("timed", n, 7) for n in "xyzxyzxyz"]
    assert list(ms) == ["x", "y", "z"] and all(len(v) == 3 for v in ms.values())
    assert ms["x"] == [8.0, 11.0, 14.0] and ms["z"] == [10.0, 13.0, 16.0]


def test_summary_is_median_min_max_rounded():
    assert benchlib.summary([3.00004, 1.0, 2.0]) == (2.0, 1.0, 3.0)
    assert benchlib.summary([0.12345, 0.12355], places=3) == (0.123, 0.123, 0.124)
    assert benchlib.summary([0.83756], places=3) == (0.838, 0.838, 0.838)


def test_lift_takes_the_device_keys_out_of_the_rows():
    rows = [{"case": "a", "device": "d", "tile": 1024}, {"case": "b", "device": "d", "tile": 1024}]
    assert benchlib.lift(rows, "device", "tile") == ["d", 1024] and rows == [{"case": "a"}, {"case": "b"}]
    assert benchlib.lift([], "device", "tile") == [None, None]


def test_flags_spell_the_options_as_the_parser_does():
    a = argparse.Namespace(batch=4, host_clips=1, seconds=0.5)
    assert benchlib.flags(a, "batch", "host_clips", "seconds") == ["--batch", "4", "--host-clips", "1", "--seconds", "0.5"]


def test_emit_prints_and_writes_only_where_asked(tmp_path, capsys, monkeypatch):
    line = {"metric": "m", "cases": [{"case": "a"}], "stopped": None}
    monkeypatch.chdir(tmp_path)
    benchlib.emit(line)                                           # returns: status 0
    assert capsys.readouterr().out == json.dumps(line) + "\n"
    assert os.listdir(tmp_path) == []
    out = tmp_path / "new" / "folder" / "line.json"
    benchlib.emit(line, str(out))
    assert capsys.readouterr().out == json.dumps(line) + "\n"
    assert out.read_text() == json.dumps(line) + "\n"


def test_emit_exits_1_after_a_stopped_run(tmp_path, capsys):
    line = {"metric": "m", "cases": [], "stopped": "case a: no result within 1.0 s"}
    out = tmp_path / "line.json"
    with pytest.raises(SystemExit) as e:
        benchlib.emit(line, str(out), line["stopped"])
    assert e.value.code == 1
    assert capsys.readouterr().out == json.dumps(line) + "\n" and out.read_text() == json.dumps(line) + "\n"


@pytest.mark.parametrize("tool", TOOLS)
def test_tool_parses_on_the_cpu_and_names_no_output_file(tool, monkeypatch, capsys):
    assert set(WROTE_TO_PROFILES) <= set(TOOLS)
    mod = importlib.import_module(tool)
    monkeypatch.setattr(sys, "argv", [tool + ".py", "--help"])
    with pytest.raises(SystemExit) as e:
        mod.main()
    assert e.value.code == 0 and "--out" in capsys.readouterr().out

    class Parsed(Exception):
        pass

    parse = argparse.ArgumentParser.parse_args

    def defaults_only(self, args=None, namespace=None):
        raise Parsed(parse(self, []))

    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", defaults_only)
    with pytest.raises(Parsed) as e:
        mod.main()
    a = e.value.args[0]
    assert a.out is None
    if tool != "mixer_bench":                                     # (that one stays in one process: it times the host)
        assert a.case is None and a.limit >= 120.0
