"""A stand-in for a tools/*_bench.py child, for tests/test_bench_harness.py: needs neither torch nor a GPU.

    python tests/bench_stub_tool.py --marker PATH --case KIND LABEL

Appends LABEL to the file PATH and writes its pid to PATH.pid when it starts, then: `row` prints a row through the
harness's child helper, `fail` writes to stderr and exits with status 3, `silent` prints no row and exits with status 0,
`sleep` sleeps for 60 s before its row."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import benchlib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--marker", required=True)
    ap.add_argument("--case", nargs=2, required=True, metavar=("KIND", "LABEL"))
    a = ap.parse_args()
    kind, label = a.case
    with open(a.marker, "a") as f:
        f.write(label + "\n")
    with open(a.marker + ".pid", "w") as f:
        f.write(str(os.getpid()))
    if kind == "fail":
        sys.stderr.write(f"  boom in {label}\n")
        raise SystemExit(3)
    if kind == "silent":
        print("nothing to report")
        return
    if kind == "sleep":
        time.sleep(60)
    print("a line before the row")
    benchlib.print_case({"case": label, "value": len(label)})


if __name__ == "__main__":
    main()
