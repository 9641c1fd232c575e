"""The bits of Engine.mix at one commit, as an anchor from outside for changes that must not move them: writes
tests/golden/mix_parent_bits.npz (read by tests/test_gpu_scene.py::test_without_sources_the_bits_are_engine_mix).

For the registered batches tile-{T - 1}, tile-{2 T + T // 2 + 7}, chunk and peak of tests/scene_model.py (T =
cmgan_mix_tile()), early in (-1, 20), with and without the RIR bank - 16 cases - it stores noisy and target as uint32
views and the four MixInfo vectors (g, scale, Ps, Pn) as uint64 views under "<batch>/early<e>/<rir|dry>/<name>", and a
text field "provenance" with the commit the library was built from and the compiler's version string.  The inputs are not
stored: they come from the seeds of scene_model.py.

These bits are a property of the kernels' fixed summation order and of the toolchain's pow and sqrt, not of the
definition of the mix.  After a toolchain change that moves them, regenerate the file at a commit where the model-based
tests (tests/test_gpu_mix.py, tests/test_gpu_scene.py) pass.  Needs the GPU.

    python tests/golden/make_mix_bits.py [--out FILE] [--commit HASH]"""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scene_model as M
from cmgan_amd.build import HIPCC
from cmgan_amd.engine import Engine
from cmgan_amd.mixing import tile

DEV = "cuda:0"
INFO = ("g", "scale", "Ps", "Pn")


def batch_names(T):
    return [f"tile-{T - 1}", f"tile-{2 * T + T // 2 + 7}", "chunk", "peak"]


def key(name, early, rir):
    return f"{name}/early{early}/{'rir' if rir else 'dry'}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mix_parent_bits.npz"))
    ap.add_argument("--commit", default=None, help="the commit of the build (default: git rev-parse HEAD)")
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    hipcc = subprocess.run([HIPCC, "--version"], capture_output=True, text=True, check=True).stdout.strip()
    eng = Engine(device=DEV)
    T = tile()
    batches = M.build_batches(T)
    t = lambda x: torch.from_numpy(np.array(x)).to(DEV)
    out = {"provenance": np.array(f"commit {commit}\n{hipcc}")}
    for name in batch_names(T):
        bt = batches[name]
        dry = [t(getattr(bt, k)) for k in ("clean", "noise_bank", "noise_start", "noise_len", "noise_off", "snr_db")]
        bank = [t(getattr(bt, k)) for k in ("rir", "rir_index", "rir_len")]
        for early in (-1, 20):
            for rir in (True, False):
                noisy, target, info = eng.mix(*dry, *(bank if rir else (None, None, None)), peak=bt.peak, early=early)
                k = key(name, early, rir)
                out[f"{k}/noisy"] = noisy.cpu().numpy().view(np.uint32)
                out[f"{k}/target"] = target.cpu().numpy().view(np.uint32)
                for f in INFO:
                    out[f"{k}/{f}"] = getattr(info, f).cpu().numpy().view(np.uint64)
                print(k, tuple(noisy.shape), flush=True)
    np.savez_compressed(a.out, **out)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, {len(out) - 1} arrays", flush=True)


if __name__ == "__main__":
    main()
