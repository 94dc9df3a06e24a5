#!/usr/bin/env python3
"""What the commands of tests/sums_cases.py compute on a given build of the library: one JSON line per command with the SHA-256 of every output array.
Every one of them ends in a column or channel sum of ccv_amd/csrc/chan_sums.cpp, whose order of additions decides the bits; two builds that are meant
to compute the same -- before and after a change to those sums or to the workspace layout of their callers -- give two identical files.

usage: tools/sums_snapshot.py [--lib PATH] > FILE
       --lib PATH   the library to load: libnnc_mi355x.so (default: the tree's own, on a GPU) or an emulator build, tests/emu/_build/libnnc_mi355x_emu.so
                    (the cases marked GPU-only are left out there)"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    args = ap.parse_args()
    from ccv_amd import nnc
    import sums_cases
    lib = nnc.load(args.lib)
    emulator = "emu" in os.path.basename(lib.path)
    for name, run, gpu_only in sums_cases.CASES:
        if gpu_only and emulator:
            continue
        print(json.dumps({"case": name, "sha256": [hashlib.sha256(x.tobytes()).hexdigest() for x in run(lib)]}), flush=True)


if __name__ == "__main__":
    main()
