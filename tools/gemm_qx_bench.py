#!/usr/bin/env python
"""Time GEMM_FORWARD of M CCV_16F rows against a palettized weight [N, K] (transpose_b: the dense layer's form) at a transformer's layer shapes -- each as ONE
command through the command interface, HIP-event timed on a stream after a warm-up of every row.  Per row: the median of `--repeats` windows of at least
`--window-ms`, their spread (max - min), and the bytes of the weight's stream per second of that median.  The commands of a window walk over as many copies of
the weight as together exceed 320 MB, so that no copy is still in a cache when its turn comes again: the stream comes from HBM every time.  A second, separate
pass with the in-library profile on reads the device time of gemm_qx_f16_kernel alone (its launch record), where the build has that kernel.
Uses nothing but the command interface and tolerates a library without the GEMM_QX_* tuning keys (--lib): both sides of a comparison come from this script,
and --report lays them side by side.
usage: python tools/gemm_qx_bench.py [--lib PATH] [--label NAME] [--repeats 11] [--window-ms 20] [--fused M] [--slices n] [--rows SUBSTRING] [--json OUT]
       python tools/gemm_qx_bench.py --report NEW.json PARENT.json"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

NK = [(4096, 4096), (11008, 4096), (4096, 11008)]
MS = [1, 4, 16, 32]
QNIB = [(4, 128), (6, 512), (8, 4096)]
COLD_BYTES = 320 << 20  # more than the 256 MB the last-level cache holds


def random_stream(rng, count, qbits, nib):
    """A stream of full blocks: random half palettes of ordinary magnitude, random index bytes (any bytes are valid indices)."""
    assert count % nib == 0
    pal = rng.standard_normal((count // nib, 1 << qbits)).astype(np.float16).view(np.uint8)
    idx = rng.integers(0, 256, size=(count // nib, nib // 8 * qbits), dtype=np.uint8)
    return np.concatenate([pal, idx], axis=1).reshape(-1)


def measure(args):
    from ccv_amd import nnc
    L = nnc.load(args.lib)
    print("library", L.dll.nnc_mi355x_version().decode(), args.lib or "")
    has_keys = L.tune_get("GEMM_QX_FUSED") >= 0
    if has_keys:
        if args.fused is not None:
            L.tune_set("GEMM_QX_FUSED", args.fused)
        L.tune_set("GEMM_QX_SLICES", args.slices)
        print("GEMM_QX_FUSED =", L.tune_get("GEMM_QX_FUSED"), " GEMM_QX_SLICES =", L.tune_get("GEMM_QX_SLICES"))
    else:
        print("this build has no GEMM_QX_FUSED key: the weight is expanded first")
    s = L.stream_new(0)
    e0, e1 = L.dll.nnc_mi355x_event_new(), L.dll.nnc_mi355x_event_new()
    L.dll.nnc_mi355x_event_elapsed_ms.restype = nnc.C.c_float
    rng = np.random.default_rng(0)
    cmd = nnc.CMD_GEMM_FORWARD(nnc.NO_TRANSPOSE, nnc.TRANSPOSE(0, 1))

    def dev(*shape):
        return L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_16F, shape, 0), (rng.random(shape, dtype=np.float32) - 0.5).astype(np.float16))

    def window(ins, out, reps):
        L.dll.nnc_mi355x_event_record(e0, s)
        for r in range(reps):
            a, ws, bias = ins
            assert L.cmd_exec(cmd, nnc.NO_HINT, 0, [a, ws[r % len(ws)], bias], [out], s) == 0
        L.dll.nnc_mi355x_event_record(e1, s)
        L.stream_wait(s)
        return L.dll.nnc_mi355x_event_elapsed_ms(e0, e1) / reps

    out = []
    print("row: median ms per command (spread) | stream GB/s | gemm_qx_f16_kernel alone, ms | launches")
    for (N, K) in NK:
        for (q, nib) in QNIB:
            if args.rows and not any(args.rows in "N=%d K=%d Q=%d/%d M=%d" % (N, K, q, nib, M) for M in MS):
                continue
            stream = random_stream(rng, N * K, q, nib)
            copies = COLD_BYTES // stream.nbytes + 1
            params = nnc.tensor_palettize(nnc.GPU_TENSOR_NHWC(0, nnc.CCV_16F, N, K), q, nib)
            ws = [nnc.PalettizedTensor(L, params, stream) for _ in range(copies)]
            for M in MS:
                name = "N=%d K=%d Q=%d/%d M=%d" % (N, K, q, nib, M)
                if args.rows and args.rows not in name:
                    continue
                ins, b = (dev(M, K), ws, dev(N)), dev(M, N)
                window(ins, b, copies)  # the warm-up: code objects, arena and workspace growth
                L.profile_enable(0); L.profile_enable(1)
                window(ins, b, max(copies, 16))
                recs = L.profile_records()
                L.profile_enable(0)
                launches = sorted(set(r[0].split("|")[-1].split("::")[-1] for r in recs))
                kern = sorted(r[3] for r in recs if "gemm_qx_f16_kernel" in r[0])
                one = window(ins, b, copies)
                reps = max(copies, min(4000, int(args.window_ms / max(one, 1e-3)) + 1))
                ms = sorted(window(ins, b, reps) for _ in range(max(1, args.repeats)))
                med, spread = ms[len(ms) // 2], ms[-1] - ms[0]
                out.append(dict(row=name, ms=med, spread=spread, bytes=int(stream.nbytes), kernel_ms=kern[len(kern) // 2] if kern else None, launches=launches))
                print("%-34s %8.4f ms (%.4f) | %7.1f | %s | %s" % (name, med, spread, stream.nbytes / med / 1e6, "%.4f" % kern[len(kern) // 2] if kern else "-", ",".join(launches)), flush=True)
            del ws
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(label=args.label, fused=L.tune_get("GEMM_QX_FUSED") if has_keys else None, rows=out), f)


def report(paths):
    new, old = (json.load(open(p)) for p in paths)
    print("Median ms per command (spread = max - min of the windows), commands issued back to back on one stream, the weight cold.  `GB/s`: bytes of the weight's")
    print("stream per second.  `kernel`: gemm_qx_f16_kernel alone from its launch record (profile pass), its GB/s and that as a share of the 8 TB/s HBM peak.")
    print("`margin`: (parent - this tree) / (the two spreads together); a row counts as faster where it is above 1.\n")
    head = ["row", "this tree", "GB/s", "kernel ms", "kernel GB/s", "of peak", "parent", "margin", "parent / this tree"]
    print("| " + " | ".join(head) + " |")
    print("|" + "---|" * len(head))
    olds = {r["row"]: r for r in old["rows"]}
    lost = []
    for r in new["rows"]:
        p = olds[r["row"]]
        margin = (p["ms"] - r["ms"]) / max(p["spread"] + r["spread"], 1e-9)
        if margin <= 1:
            lost.append(r["row"])
        k = r.get("kernel_ms")
        kcells = ["%.4f" % k, "%.0f" % (r["bytes"] / k / 1e6), "%.2f" % (r["bytes"] / k / 1e6 / 8000)] if k else ["-", "-", "-"]
        print("| %s | %.4f (%.4f) | %.0f | %s | %.4f (%.4f) | %.1f | %.2fx |" % (r["row"], r["ms"], r["spread"], r["bytes"] / r["ms"] / 1e6, " | ".join(kcells), p["ms"], p["spread"], margin, p["ms"] / r["ms"]))
    print("\nRows not faster than the parent by more than the combined spread: %s." % ("; ".join(lost) or "none"))
    print("\nLaunch records of one command, this tree / parent (depalettize_kernel files none):\n")
    for r in new["rows"]:
        print("- %s: %s / %s" % (r["row"], ", ".join(r["launches"]) or "-", ", ".join(olds[r["row"]]["launches"]) or "-"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libnnc_mi355x.so")
    ap.add_argument("--label", default="this tree", help="'parent' for the parent commit's build")
    ap.add_argument("--repeats", type=int, default=11, help="timed windows per row: the median and the spread are reported")
    ap.add_argument("--window-ms", type=float, default=20.0, help="least work timed per window")
    ap.add_argument("--fused", type=int, default=None, help="set the GEMM_QX_FUSED tuning key (a build that has it)")
    ap.add_argument("--slices", type=int, default=0, help="set the GEMM_QX_SLICES tuning key (a build that has it)")
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
