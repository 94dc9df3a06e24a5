#!/usr/bin/env python
"""Time GEMM_FORWARD of M CCV_16F rows against a dense CCV_16F weight [N, K] (transpose_b: the dense layer's form) at a transformer's layer shapes and an LM head
-- each as ONE command through the command interface, HIP-event timed on a stream after a warm-up of every row.  Per row: the median of `--repeats` windows of at
least `--window-ms`, their spread (max - min), and the weight's 2 N K bytes per second of that median as a share of the 6.29 TB/s copy rate.  The commands of a
window walk over as many copies of the weight as together exceed 320 MB, so that no copy is still in a cache when its turn comes again.
Uses nothing but the command interface and tolerates a library without the GEMM_F16_ROWS keys (--lib): both sides of a comparison come from this script, and
--report lays them side by side.
usage: python tools/gemm_rows_bench.py [--lib PATH] [--label NAME] [--repeats 11] [--window-ms 20] [--rows-key n] [--slices n] [--rows SUBSTRING] [--json OUT]
       python tools/gemm_rows_bench.py --report NEW.json PARENT.json"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

NK = [(4096, 4096), (11008, 4096), (4096, 11008), (32000, 4096)]
MS = [1, 4, 16, 32]
COLD_BYTES = 320 << 20  # more than the 256 MB the last-level cache holds
COPY_RATE = 6.29e12     # bytes per second of a device copy


def measure(args):
    from ccv_amd import nnc
    L = nnc.load(args.lib)
    print("library", L.dll.nnc_mi355x_version().decode(), "(%s)" % args.label)
    has_keys = L.tune_get("GEMM_F16_ROWS") >= 0
    if has_keys:
        L.tune_set("GEMM_F16_ROWS", args.rows_key)
        L.tune_set("GEMM_F16_ROWS_SLICES", args.slices)
        print("GEMM_F16_ROWS =", L.tune_get("GEMM_F16_ROWS"), " GEMM_F16_ROWS_SLICES =", L.tune_get("GEMM_F16_ROWS_SLICES"))
    else:
        print("this build has no GEMM_F16_ROWS key: the 64 x 64 tile, split-K and its fold")
    s = L.stream_new(0)
    e0, e1 = L.dll.nnc_mi355x_event_new(), L.dll.nnc_mi355x_event_new()
    L.dll.nnc_mi355x_event_elapsed_ms.restype = nnc.C.c_float
    rng = np.random.default_rng(0)
    cmd = nnc.CMD_GEMM_FORWARD(nnc.NO_TRANSPOSE, nnc.TRANSPOSE(0, 1))
    block = (rng.random(1 << 20, dtype=np.float32) - 0.5).astype(np.float16)

    def dev(*shape):  # (random halves of ordinary magnitude: a block of 2^20 of them repeated)
        n = int(np.prod(shape))
        return L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_16F, shape, 0), np.resize(block, n).reshape(shape))

    def window(a, ws, bias, out, reps):
        L.dll.nnc_mi355x_event_record(e0, s)
        for r in range(reps):
            assert L.cmd_exec(cmd, nnc.NO_HINT, 0, [a, ws[r % len(ws)]] + ([bias] if bias is not None else []), [out], s) == 0
        L.dll.nnc_mi355x_event_record(e1, s)
        L.stream_wait(s)
        return L.dll.nnc_mi355x_event_elapsed_ms(e0, e1) / reps

    out = []
    print("row: median ms per command (spread) | share of the copy rate | kernel")
    for (N, K) in NK:
        if args.rows and not any(args.rows in "N=%d K=%d M=%d " % (N, K, M) for M in MS):
            continue
        copies = COLD_BYTES // (2 * N * K) + 1
        ws = [dev(N, K) for _ in range(copies)]
        for M in MS:
            for with_bias in ((True, False) if (N, K) == NK[0] and M == 1 else (True,)):
                name = "N=%d K=%d M=%d %s" % (N, K, M, "bias" if with_bias else "no bias")
                if args.rows and args.rows not in name:
                    continue
                a, bias, b = dev(M, K), (dev(N) if with_bias else None), dev(M, N)
                window(a, ws, bias, b, copies)  # the warm-up: code objects, arena and workspace growth
                kernel = L.dll.nnc_mi355x_last_kernel_name().decode()
                one = window(a, ws, bias, b, copies)
                reps = max(copies, min(4000, int(args.window_ms / max(one, 1e-3)) + 1))
                ms = sorted(window(a, ws, bias, b, reps) for _ in range(max(1, args.repeats)))
                med, spread = ms[len(ms) // 2], ms[-1] - ms[0]
                out.append(dict(row=name, ms=med, spread=spread, bytes=2 * N * K, kernel=kernel))
                print("%-36s %8.4f ms (%.4f) | %.2f | %s" % (name, med, spread, 2 * N * K / (med * 1e-3) / COPY_RATE, kernel), flush=True)
        del ws
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(label=args.label, rows_key=L.tune_get("GEMM_F16_ROWS") if has_keys else None, slices=args.slices, rows=out), f)


def report(paths):
    new, old = (json.load(open(p)) for p in paths)
    print("Median ms per command (spread = max - min of the windows), commands issued back to back on one stream, the weight cold.  `of copy`: the weight's 2 N K")
    print("bytes per second of the median as a share of the 6.29 TB/s copy rate (bound: HBM).  `margin`: (%s - %s) / (the two spreads together); a row counts as" % (old["label"], new["label"]))
    print("faster where it is above 1.\n")
    head = ["row", new["label"], "of copy", "kernel", old["label"], "of copy", "kernel", "margin", "%s / %s" % (old["label"], new["label"])]
    print("| " + " | ".join(head) + " |")
    print("|" + "---|" * len(head))
    olds = {r["row"]: r for r in old["rows"]}
    lost = []
    for r in new["rows"]:
        p = olds[r["row"]]
        margin = (p["ms"] - r["ms"]) / max(p["spread"] + r["spread"], 1e-9)
        if margin <= 1:
            lost.append(r["row"])
        share = lambda x: x["bytes"] / (x["ms"] * 1e-3) / COPY_RATE
        print("| %s | %.4f (%.4f) | %.2f | %s | %.4f (%.4f) | %.2f | %s | %.1f | %.2fx |" % (r["row"], r["ms"], r["spread"], share(r), r["kernel"], p["ms"], p["spread"], share(p), p["kernel"], margin, p["ms"] / r["ms"]))
    print("\nRows not faster than %s by more than the combined spread: %s." % (old["label"], "; ".join(lost) or "none"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libnnc_mi355x.so")
    ap.add_argument("--label", default="this tree", help="'parent' for the parent commit's build")
    ap.add_argument("--repeats", type=int, default=11, help="timed windows per row: the median and the spread are reported")
    ap.add_argument("--window-ms", type=float, default=20.0, help="least work timed per window")
    ap.add_argument("--rows-key", type=int, default=1, help="set the GEMM_F16_ROWS tuning key (a build that has it)")
    ap.add_argument("--slices", type=int, default=0, help="set the GEMM_F16_ROWS_SLICES tuning key (a build that has it)")
    ap.add_argument("--rows", default=None, help="only the rows whose name contains this")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--report", nargs=2, default=None, metavar=("NEW", "PARENT"), help="JSON files of two runs: print the comparison as markdown")
    args = ap.parse_args()
    if args.report:
        report(args.report)
    else:
        measure(args)


if __name__ == "__main__":
    main()
