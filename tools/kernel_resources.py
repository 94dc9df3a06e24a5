#!/usr/bin/env python3
"""Register / scratch / LDS budget of the register-resident Winograd kernels, from the compiler's own resource-usage remarks.

Compiles ccv_amd/csrc/cmd_conv.cpp for gfx950 with the library's flags plus -Rpass-analysis=kernel-resource-usage (device side only, the object is
thrown away; ~3 minutes, no GPU needed) and prints one row per kernel whose demangled name contains a pattern: VGPRs, AGPRs, SGPRs, the
VGPR / SGPR spill counts, scratch bytes per lane, LDS bytes per workgroup and occupancy.  Not a test; it reads nothing but the remarks.

usage: tools/kernel_resources.py [pattern ...]        (default patterns: wino_fused_kernel wino_wgrad_fused_kernel)
       tools/kernel_resources.py --remarks FILE [pattern ...]   parse a saved remark listing instead of compiling"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ccv_amd", "csrc")
FIELDS = [("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("VGPRs Spill", "vgpr spill"), ("SGPRs Spill", "sgpr spill"),
          ("ScratchSize [bytes/lane]", "scratch B/lane"), ("LDS Size [bytes/block]", "LDS B"), ("Occupancy [waves/SIMD]", "occupancy")]


def remarks_of_build():
    hipcc = os.environ.get("HIPCC", os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc"))
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
               "-c", "cmd_conv.cpp", "-o", os.path.join(tmp, "cmd_conv.o")]
        r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            sys.exit(r.returncode)
        return r.stderr


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
        return out[:len(names)] if len(out) >= len(names) else names
    except OSError:
        return names


def main(argv):
    text = None
    if argv[:1] == ["--remarks"]:
        text = open(argv[1]).read()
        argv = argv[2:]
    patterns = argv or ["wino_fused_kernel", "wino_wgrad_fused_kernel"]
    if text is None:
        text = remarks_of_build()
    kernels = []
    for block in re.split(r"remark: [^\n]*?Function Name: ", text)[1:]:
        name = block.split(None, 1)[0]
        vals = {}
        for key, _ in FIELDS:
            m = re.search(re.escape(key) + r": (\S+)", block)
            vals[key] = m.group(1) if m else "?"
        kernels.append((name, vals))
    names = demangle([k[0] for k in kernels])
    rows = []
    for (_, vals), dem in zip(kernels, names):
        short = re.sub(r"\(.*$", "", dem).replace("void ", "").replace("nnc::", "").replace("(anonymous namespace)::", "")
        if any(p in short for p in patterns):
            rows.append([short] + [vals[k] for k, _ in FIELDS])
    head = ["kernel"] + [h for _, h in FIELDS]
    width = [max(len(str(r[i])) for r in [head] + rows) for i in range(len(head))]
    for r in [head] + sorted(rows):
        print("  ".join(str(c).ljust(w) if i == 0 else str(c).rjust(w) for i, (c, w) in enumerate(zip(r, width))))


if __name__ == "__main__":
    main(sys.argv[1:])
