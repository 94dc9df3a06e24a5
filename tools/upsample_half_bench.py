#!/usr/bin/env python
"""Time UPSAMPLE_FORWARD / UPSAMPLE_BACKWARD in half precision (both tensors CCV_16F, as an all-half graph issues them) at sizes a user runs: the nearest 2x steps
of a diffusion decoder at batch 2, the bilinear 2x steps of a feature-pyramid / segmentation decoder with align_corners 0 and 1, and a bilinear 1.5x step -- each
forward and backward, NCHW and NHWC, as ONE command through the command interface, HIP-event timed on a stream.  Per row: the median of `--repeats` windows,
their spread (max - min), the bytes the native route must move (both tensors once) and that traffic as a fraction of 6.29 TB/s, the measured copy rate of the
MI355X (profiles/row_half_bench.md).  Uses nothing but the command interface, so it runs unchanged on a build without the UPSAMPLE_HALF_NATIVE key (--lib): both
sides of a comparison come from this script, run alternately, and --report lays the runs side by side.
usage: python tools/upsample_half_bench.py [--lib PATH] [--label NAME] [--repeats 7] [--window-ms 20] [--upsample-half-native 0|1] [--json OUT]
       python tools/upsample_half_bench.py --report NEW1.json PARENT1.json NEW2.json PARENT2.json > profiles/upsample_half_bench.md"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HBM_COPY_TBS = 6.29
# (type: 0 nearest / 1 bilinear, align_corners, N, C, source (h, w), output (h, w))
ROWS = [(0, 0, 2, 1280, (8, 8), (16, 16)), (0, 0, 2, 1280, (16, 16), (32, 32)), (0, 0, 2, 640, (32, 32), (64, 64)), (0, 0, 2, 320, (64, 64), (128, 128)),
        (1, 0, 8, 256, (32, 32), (64, 64)), (1, 1, 8, 256, (32, 32), (64, 64)), (1, 0, 8, 256, (64, 64), (128, 128)), (1, 1, 8, 256, (64, 64), (128, 128)),
        (1, 0, 4, 128, (40, 40), (60, 60))]


def measure(args):
    from ccv_amd import nnc
    L = nnc.load(args.lib)
    print("library", L.dll.nnc_mi355x_version().decode(), args.lib or "")
    if args.upsample_half_native is not None:
        try:
            L.tune_set("UPSAMPLE_HALF_NATIVE", args.upsample_half_native)
            print("UPSAMPLE_HALF_NATIVE =", args.upsample_half_native)
        except KeyError:
            print("this build has no UPSAMPLE_HALF_NATIVE key: skipped")
    s = L.stream_new(0)
    e0, e1 = L.dll.nnc_mi355x_event_new(), L.dll.nnc_mi355x_event_new()
    L.dll.nnc_mi355x_event_elapsed_ms.restype = nnc.C.c_float
    H = np.float16

    def window(cmd, ins, outs, reps):
        L.dll.nnc_mi355x_event_record(e0, s)
        for _ in range(reps):
            assert L.cmd_exec(cmd, nnc.NO_HINT, 0, ins, outs, s) == 0
        L.dll.nnc_mi355x_event_record(e1, s)
        L.stream_wait(s)
        return L.dll.nnc_mi355x_event_elapsed_ms(e0, e1) / reps

    def timed(cmd, ins, outs):
        """(median ms per call, spread, launch names of one call): a first call (code objects, arena growth) under the launch records, one timed call to size the windows, the windows"""
        L.profile_enable(0); L.profile_enable(1)
        assert L.cmd_exec(cmd, nnc.NO_HINT, 0, ins, outs, s) == 0
        L.stream_wait(s)
        names = sorted(set(r[0].split("|")[-1].split("::")[-1] for r in L.profile_records()))
        L.profile_enable(0)
        one = window(cmd, ins, outs, 1)
        reps = max(3, min(200, int(args.window_ms / max(one, 1e-3)) + 1))
        ms = sorted(window(cmd, ins, outs, reps) for _ in range(max(1, args.repeats)))
        return ms[len(ms) // 2], ms[-1] - ms[0], names

    rng = np.random.default_rng(0)
    pool = ((rng.random(max(n * c * d[0] * d[1] for _, _, n, c, _, d in ROWS), dtype=np.float32) - 0.5) * 4).astype(H)  # U(-2, 2), cut to every shape below

    def dev(shape, fmt, zero=False):
        x = np.zeros(shape, H) if zero else pool[:int(np.prod(shape))].reshape(shape)
        return L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, fmt, nnc.CCV_16F, shape, 0), x)

    out = []
    print("per row median ms (spread) | MB the native route moves | fraction of %.2f TB/s | launches" % HBM_COPY_TBS)
    for up_type, align, n, c, src, dst in ROWS:
        for lay, fmt in (("NCHW", nnc.NCHW), ("NHWC", nnc.NHWC)):
            ashape, bshape = ((n, c) + src, (n, c) + dst) if lay == "NCHW" else ((n,) + src + (c,), (n,) + dst + (c,))
            moved = 2 * (int(np.prod(ashape)) + int(np.prod(bshape)))
            for forward in (True, False):
                cmd = nnc.CMD_UPSAMPLE("UPSAMPLE_FORWARD" if forward else "UPSAMPLE_BACKWARD", up_type, dst[1] / src[1], dst[0] / src[0], align)
                x, y = dev(ashape if forward else bshape, fmt), dev(bshape if forward else ashape, fmt, True)
                ms, spread, names = timed(cmd, [x], [y])
                name = "%s %s %s%s %s -> %dx%d" % ("nearest" if up_type == 0 else "bilinear", "forward" if forward else "backward", lay, ", align_corners" if align else "", list(ashape), dst[0], dst[1])
                frac = moved / (ms * 1e-3) / (HBM_COPY_TBS * 1e12)
                out.append(dict(row=name, ms=ms, spread=spread, mb=moved / 1e6, hbm=frac, launches=names))
                print("%-72s %9.4f ms (%.4f) | %8.2f MB | %5.3f | %s" % (name, ms, spread, moved / 1e6, frac, ",".join(names)), flush=True)
                x.free(); y.free()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(label=args.label, rows=out), f)


def report(paths):
    runs = [json.load(open(p)) for p in paths]
    new = [r for r in runs if r["label"] != "parent"]
    old = [r for r in runs if r["label"] == "parent"]
    print("# Upsample in half precision: one command, both tensors CCV_16F\n")
    print("Written by `tools/upsample_half_bench.py --report`; the runs below were measured alternately (this tree, parent, ...) in one session on one MI355X.")
    print("Per run: the median of the timed windows in milliseconds and, in brackets, their spread (max - min).  `MB`: what the native route must move (both")
    print("tensors once).  `of copy rate`: those bytes per second of this tree's slower run, as a fraction of %.2f TB/s.  `parent spread`: the largest of the" % HBM_COPY_TBS)
    print("parent's window spreads and the distance between its runs.  `margin`: (the parent's faster run - this tree's slower run) / parent spread; a row is done")
    print("where it is above 2.  A window repeats one command on the same tensors, and every row's tensors stay under the 256 MiB last-level cache: the fractions")
    print("say how far a row is from what the memory system can deliver at best, not what a cold call costs.\n")
    head = ["row", "MB"] + ["%s, run %d" % (lab, i + 1) for i in range(max(len(new), len(old))) for lab in ("this tree", "parent")][:len(runs)] + ["of copy rate", "parent spread", "margin", "parent / this tree"]
    print("| " + " | ".join(head) + " |")
    print("|" + "---|" * len(head))
    worst, lost, ratios = None, [], []
    for k, r0 in enumerate(new[0]["rows"]):
        ns, os_ = [r["rows"][k] for r in new], [r["rows"][k] for r in old]
        cells = []
        for i in range(max(len(ns), len(os_))):
            for xs in (ns, os_):
                if i < len(xs):
                    cells.append("%.4f (%.4f)" % (xs[i]["ms"], xs[i]["spread"]))
        slow_new, fast_old = max(x["ms"] for x in ns), min(x["ms"] for x in os_)
        spread = max([x["spread"] for x in os_] + [max(x["ms"] for x in os_) - fast_old])
        frac = r0["mb"] * 1e6 / (slow_new * 1e-3) / (HBM_COPY_TBS * 1e12)
        margin = (fast_old - slow_new) / max(spread, 1e-9)
        ratios.append(fast_old / slow_new)
        if worst is None or frac < worst[0]:
            worst = (frac, r0["row"])
        if margin <= 2:
            lost.append(r0["row"])
        print("| %s | %.1f | %s | %.3f | %.4f | %.1f | %.1fx |" % (r0["row"], r0["mb"], " | ".join(cells), frac, spread, margin, fast_old / slow_new))
    print("\nThe parent's faster run over this tree's slower run: %.1fx - %.1fx." % (min(ratios), max(ratios)))
    print("\nLowest fraction of the copy rate: %s, %.3f." % (worst[1], worst[0]))
    print("\nRows not faster than the parent by more than twice its spread: %s." % (", ".join(lost) or "none"))
    print("\nKernels of one command, this tree / parent (the parent's conversions to and from fp32 images and its fp32 kernels file no launch records):\n")
    for r0, p0 in zip(new[0]["rows"], old[0]["rows"]):
        print("- %s: %s / %s" % (r0["row"], ", ".join(r0["launches"]) or "-", ", ".join(p0["launches"]) or "-"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libnnc_mi355x.so")
    ap.add_argument("--label", default="this tree", help="'parent' for the parent commit's build")
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per row: the median and the spread are reported")
    ap.add_argument("--window-ms", type=float, default=20.0, help="least work timed per window")
    ap.add_argument("--upsample-half-native", type=int, default=None, help="set the UPSAMPLE_HALF_NATIVE tuning key")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--report", nargs="+", default=None, help="JSON files of earlier runs: print the comparison as markdown")
    args = ap.parse_args()
    if args.report:
        report(args.report)
    else:
        measure(args)


if __name__ == "__main__":
    main()
