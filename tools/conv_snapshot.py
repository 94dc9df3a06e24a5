#!/usr/bin/env python3
"""What the convolution commands of tests/conv_route_cases.py do on a given build of the library: one JSON line per command with the route it took
(last kernel name, launches of the two shared backward kernels, half tensors staged / handed on) and the SHA-256 of every output array.  Two builds
that are meant to compute the same -- before and after a change to the host side of ccv_amd/csrc/cmd_conv.cpp -- give two identical files.

usage: tools/conv_snapshot.py [--lib PATH] [--routes] > FILE
       --lib PATH   the library to load: libnnc_mi355x.so (default: the tree's own, on a GPU) or an emulator build, tests/emu/_build/libnnc_mi355x_emu.so
       --routes     print the routes alone, as the EXPECTED table of tests/test_conv_routes.py"""
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
    ap.add_argument("--routes", action="store_true")
    args = ap.parse_args()
    from ccv_amd import nnc
    import conv_route_cases as crc
    lib = nnc.load(args.lib)
    table = {}
    for case in crc.CASES:
        for key, kind, algo in crc.commands(case):
            for fuse_relu in (False, True):
                route, outs = crc.run(lib, case, kind, algo, fuse_relu)
                key2 = key + ("+relu" if fuse_relu else "")
                table.setdefault(case.name, {})[key2] = route
                if not args.routes:
                    print(json.dumps({"case": case.name, "command": key2, "kernel": route[0], "shared": route[1], "half": route[2],
                                      "sha256": [hashlib.sha256(x.tobytes()).hexdigest() for x in outs]}))
    if args.routes:
        print("EXPECTED = {")
        for name, rows in table.items():
            print("    %r: {" % name)
            for key, route in rows.items():
                print("        %r: %r," % (key, route))
            print("    },")
        print("}")


if __name__ == "__main__":
    main()
