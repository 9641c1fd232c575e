"""DynamicMixer's draws and option messages at one commit, as an anchor from outside for changes that must not move them:
writes tests/golden/mixer_parent_draws.npz and tests/golden/mixer_parent_messages.json (read by
tests/test_mix_host.py::test_draws_and_messages_are_the_recorded_ones).

For each of the 384 option combinations of tests/mixer_cases.py::draw_cases it stores every field of draw(6), every field
of draw_stretch(6, d.speed) and the final get_state() of the mixer's, the room sampler's and the channel sampler's
generators (fixed seeds; CPU).  "blob" holds the fields' unsigned integer views end to end, "manifest" (JSON) one row per
field in the same order - [name, dtype, shape, strides, bytes], [name, null] for None - under each case's name, and
"provenance" the commit and torch.__version__.  The JSON file maps each entry of BAD_OPTIONS to [exception type, full text].

The draws are a property of torch's CPU generators as much as of the mixer: after a torch change that moves them, record
again AT THE COMMIT THE FILES WERE MADE AT (their provenance says which), not at the one under test.  Needs no GPU.

    python tests/golden/make_mixer_draws.py [--commit HASH]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mixer_cases as C

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit of the tree (default: git rev-parse HEAD)")
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    manifest, parts = {}, []
    for name, opt in C.draw_cases():
        mixer, gens = C.draw_mixer(opt, C.NoEngine())
        manifest[name], raw = C.pack(C.drawn_fields(mixer, gens))
        parts.append(raw)
    out = os.path.join(GOLDEN, "mixer_parent_draws.npz")
    np.savez_compressed(out, blob=np.concatenate(parts), manifest=np.array(json.dumps(manifest)),
                        provenance=np.array(f"commit {commit}\ntorch {torch.__version__}"))
    print(f"{out}: {os.path.getsize(out)} bytes, {len(manifest)} cases", flush=True)
    messages = {name: C.message_of(make, kw) for name, make, kw in C.BAD_OPTIONS}
    out = os.path.join(GOLDEN, "mixer_parent_messages.json")
    with open(out, "w") as f:
        json.dump(dict(provenance=f"commit {commit}", messages=messages), f, indent=1)
        f.write("\n")
    print(f"{out}: {len(messages)} messages", flush=True)


if __name__ == "__main__":
    main()
