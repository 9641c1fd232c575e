"""DynamicMixer's outputs at one commit, as an anchor from outside for changes that must not move them: writes
tests/golden/mixer_parent_bits.npz (read by tests/test_gpu_mix.py::test_mixer_gives_the_recorded_bits).

For the 12 configurations of tests/mixer_cases.py::bits_configs, at B = 3 and L = 1536 with inputs from fixed seeds (none
stored), it stores under "<configuration>/<field>" the unsigned integer views of target, noisy, every MixInfo / SceneInfo
vector and every tensor of last_draw, last_stretch and last_level, the text "None" for a field that is None, and a text
field "provenance" with the commit the library was built from, the compiler's version string and torch.__version__.

These bits are a property of the kernels' fixed summation order, of the toolchain's pow and sqrt and of torch's device
generators, not of the definition of the mix.  After a toolchain change that moves them, regenerate the file at a commit
where the model-based tests (tests/test_gpu_mix.py, tests/test_gpu_scene.py, ...) pass.  Needs the GPU.

    python tests/golden/make_mixer_bits.py [--out FILE] [--commit HASH]"""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mixer_cases as C
from cmgan_amd.build import HIPCC
from cmgan_amd.engine import Engine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mixer_parent_bits.npz"))
    ap.add_argument("--commit", default=None, help="the commit of the build (default: git rev-parse HEAD)")
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    hipcc = subprocess.run([HIPCC, "--version"], capture_output=True, text=True, check=True).stdout.strip()
    out = {"provenance": np.array(f"commit {commit}\n{hipcc}\ntorch {torch.__version__}")}
    for name, mixer, clean in C.bits_configs(Engine(device="cuda:0")):
        for field, t in C.mixed_fields(mixer, clean):
            out[f"{name}/{field}"] = np.array("None") if t is None else C.unsigned(t)
        print(name, tuple(out[f"{name}/noisy"].shape), flush=True)
    np.savez_compressed(a.out, **out)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, {len(out) - 1} arrays", flush=True)


if __name__ == "__main__":
    main()
