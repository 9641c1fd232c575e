"""The bits of Engine.rir and Engine.rir_bands at one commit, as an anchor from outside for changes that must not move them:
writes tests/golden/rir_parent_bits.npz (read by test_the_bits_are_the_recorded_ones of tests/test_gpu_rir.py and
tests/test_gpu_rir_bands.py).

For every case of tests/rir_cases.py (T = cmgan_rir_tile()) it stores the responses as uint32 views and the lengths as
uint32 views of the int32 vector under "rir/<case>/rir", "rir/<case>/len", "rir_bands/<case>/rir" and
"rir_bands/<case>/len", and a text field "provenance" with the commit the library was built from and the compiler's
version string.  The inputs are not stored: they are the literal tables and seeds of rir_cases.py.  Every case is asserted
to be non-trivial (rir_cases.nontrivial) before it is written.

These bits are a property of the kernels' fixed enumeration order and of the toolchain's pow, exp, sqrt, sinpi and
cospi, not of the definition of the response.  After a toolchain change that moves them, regenerate the file at a commit
where the model-based tests (tests/test_gpu_rir.py, tests/test_gpu_rir_bands.py) pass.  Needs the GPU.

    python tests/golden/make_rir_bits.py [--out FILE] [--commit HASH]"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rir_cases as RC
from cmgan_amd.build import HIPCC
from cmgan_amd.engine import Engine

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rir_parent_bits.npz"))
    ap.add_argument("--commit", default=None, help="the commit of the build (default: git rev-parse HEAD)")
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    hipcc = subprocess.run([HIPCC, "--version"], capture_output=True, text=True, check=True).stdout.strip()
    eng = Engine(device=DEV)
    T, cap = int(eng.lib.cmgan_rir_tile()), int(eng.lib.cmgan_rir_list_capacity())
    out = {"provenance": np.array(f"commit {commit}\n{hipcc}")}
    for call, cases in (("rir", RC.rir_cases(T)), ("rir_bands", RC.rir_bands_cases(T))):
        for name, case in cases.items():
            got = {k: v.cpu().numpy() for k, v in RC.run(eng, case, DEV).items()}
            RC.nontrivial(name, case, got["rir"], got["len"], T, cap)
            for k, v in got.items():
                out[f"{call}/{name}/{k}"] = v.view(np.uint32)
            print(f"{call}/{name}", got["rir"].shape, f"peak {np.max(np.abs(got['rir'])):.4f}", got["len"].tolist(), flush=True)
    np.savez_compressed(a.out, **out)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, {len(out) - 1} arrays", flush=True)


if __name__ == "__main__":
    main()
