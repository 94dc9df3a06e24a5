#!/usr/bin/env python
"""Time GROUP_NORM in half precision (every tensor CCV_16F, as an all-half graph issues it) on the maps of a diffusion UNet: batch 2, 32 groups, both layouts;
forward with scale and bias, backward with every gradient, backward with h alone -- each as ONE command through the command interface, HIP-event timed on a
stream.  Per row: the median of `--repeats` windows, their spread (max - min), the bytes the native route must move (forward: a read twice and b written;
backward: g and a read twice and h written; a planar run that fits the registers is read once; parameters and statistics are noise) and that traffic as a fraction of
6.29 TB/s, the measured copy rate of the MI355X (profiles/row_half_bench.md).  Uses nothing but the command interface, so it runs unchanged on a build
without the GNORM_HALF_NATIVE key (--lib): both sides of a comparison come from this script, run alternately, and --report lays the runs side by side.
usage: python tools/gnorm_half_bench.py [--lib PATH] [--label NAME] [--repeats 7] [--window-ms 20] [--gnorm-half-native 0|1] [--json OUT]
       python tools/gnorm_half_bench.py --report NEW1.json PARENT1.json NEW2.json PARENT2.json > profiles/gnorm_half_bench.md"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

N, GROUPS = 2, 32
SHAPES = [(320, 64, 64), (640, 32, 32), (1280, 16, 16), (1280, 8, 8), (960, 32, 32), (1920, 16, 16), (2560, 8, 8)]  # C, H, W; the last three: the decoder's concatenated maps
HBM_COPY_TBS = 6.29
REG_MAX = 16384  # group_ops.h GN_REG_MAX: a planar run this long is read once


def measure(args):
    from ccv_amd import nnc
    L = nnc.load(args.lib)
    print("library", L.dll.nnc_mi355x_version().decode(), args.lib or "")
    if args.gnorm_half_native is not None:
        try:
            L.tune_set("GNORM_HALF_NATIVE", args.gnorm_half_native)
            print("GNORM_HALF_NATIVE =", args.gnorm_half_native)
        except KeyError:
            print("this build has no GNORM_HALF_NATIVE key: skipped")
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
        """(median ms per call, spread, launch names of one call): a first call (code objects, workspace growth) under the launch records, one timed call to size the windows, the windows"""
        L.profile_enable(0); L.profile_enable(1)
        assert L.cmd_exec(cmd, nnc.NO_HINT, 0, ins, outs, s) == 0
        L.stream_wait(s)
        names = sorted(set(r[0].split("|")[-1].split("::")[-1] for r in L.profile_records()))
        L.profile_enable(0)
        one = window(cmd, ins, outs, 1)
        reps = max(3, min(200, int(args.window_ms / max(one, 1e-3)) + 1))
        ms = sorted(window(cmd, ins, outs, reps) for _ in range(max(1, args.repeats)))
        return ms[len(ms) // 2], ms[-1] - ms[0], names

    def dev(x):
        return L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_16F, x.shape, 0), x)

    rng = np.random.default_rng(0)
    out = []

    def row(leg, lay, shape, cmd, ins, outs, nbytes):
        ms, spread, names = timed(cmd, ins, outs)
        frac = nbytes / (ms * 1e-3) / (HBM_COPY_TBS * 1e12)
        what = "%s %d x %d x %d" % ((lay,) + shape)
        out.append(dict(leg=leg, shape=what, ms=ms, spread=spread, mb=nbytes / 1e6, hbm=frac, launches=names))
        print("%-12s %-24s %9.4f ms (%.4f) | %8.2f MB | %5.3f | %s" % (leg, what, ms, spread, nbytes / 1e6, frac, ",".join(names)), flush=True)

    print("per leg median ms (spread) | MB the native route moves | fraction of %.2f TB/s | launches" % HBM_COPY_TBS)
    for C, Hh, W in SHAPES:
        for lay in ("NCHW", "NHWC"):
            nchw = lay == "NCHW"
            shape = (N, C, Hh, W) if nchw else (N, Hh, W, C)
            sshape = (N, GROUPS, 1, 1) if nchw else (N, 1, 1, GROUPS)
            pshape = (1, C, 1, 1) if nchw else (1, 1, 1, C)
            axis, red = (1, (2, 3)) if nchw else (3, (1, 2))
            a = dev(((rng.random(shape, dtype=np.float32) - 0.5) * 8).astype(H))
            g = dev(((rng.random(shape, dtype=np.float32) - 0.5) * 4).astype(H))
            b, h = dev(np.zeros(shape, H)), dev(np.zeros(shape, H))
            scale, bias, dscale, dbias = dev(np.ones(pshape, H)), dev(np.zeros(pshape, H)), dev(np.zeros(pshape, H)), dev(np.zeros(pshape, H))
            mean, istd = dev(np.zeros(sshape, H)), dev(np.zeros(sshape, H))
            big = N * C * Hh * W * 2
            once = nchw and C // GROUPS * Hh * W <= REG_MAX
            fwd = nnc.CMD_GROUP_NORM("GROUP_NORM_FORWARD", axis, GROUPS, 1e-5, 1, *red)
            bwd = nnc.CMD_GROUP_NORM("GROUP_NORM_BACKWARD", axis, GROUPS, 1e-5, 1, *red)
            row("fwd", lay, (C, Hh, W), fwd, [a, scale, bias], [b, mean, istd], (2 if once else 3) * big)  # (leaves the statistics the backward legs read)
            row("bwd all", lay, (C, Hh, W), bwd, [g, None, None, a, scale, None, None, mean, istd], [h, dscale, dbias], 5 * big)
            row("bwd h", lay, (C, Hh, W), bwd, [g, None, None, a, scale, None, None, mean, istd], [h], (3 if once else 5) * big)
            for t in (a, g, b, h, scale, bias, dscale, dbias, mean, istd):
                t.free()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(label=args.label, rows=out), f)


def report(paths):
    runs = [json.load(open(p)) for p in paths]
    new = [r for r in runs if r["label"] != "parent"]
    old = [r for r in runs if r["label"] == "parent"]
    print("# Group norm in half precision: one command, every tensor CCV_16F, batch %d, %d groups\n" % (N, GROUPS))
    print("Written by `tools/gnorm_half_bench.py --report`; the runs below were measured alternately (this tree, parent, ...) in one session on one MI355X.")
    print("Per run: the median of the timed windows in milliseconds and, in brackets, their spread (max - min).  `MB`: what the native route moves (the maps;")
    print("a planar run of at most %d elements is read once, everything else twice).  `of copy rate`: those bytes per second of this tree's slower run, as a" % REG_MAX)
    print("fraction of %.2f TB/s.  `parent spread`: the largest of the parent's window spreads and the distance between its runs.  `margin`: (the parent's" % HBM_COPY_TBS)
    print("faster run - this tree's slower run) / parent spread; a row is done where it is above 2.\n")
    head = ["leg", "layout C x H x W", "MB"] + ["%s, run %d" % (lab, i + 1) for i in range(max(len(new), len(old))) for lab in ("this tree", "parent")][:len(runs)] + ["of copy rate", "parent spread", "margin"]
    print("| " + " | ".join(head) + " |")
    print("|" + "---|" * len(head))
    worst, lost = None, []
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
        if worst is None or frac < worst[0]:
            worst = (frac, r0["leg"], r0["shape"])
        if margin <= 2:
            lost.append("%s at %s" % (r0["leg"], r0["shape"]))
        print("| %s | %s | %.1f | %s | %.3f | %.4f | %.1f |" % (r0["leg"], r0["shape"], r0["mb"], " | ".join(cells), frac, spread, margin))
    print("\nLowest fraction of the copy rate: %s at %s, %.3f." % (worst[1], worst[2], worst[0]))
    print("\nRows not faster than the parent by more than twice its spread: %s." % (", ".join(lost) or "none"))
    print("\nKernels of one command, this tree / parent (the parent's conversions to and from fp32 images and its fp32 kernels file no launch records):\n")
    for r0, p0 in zip(new[0]["rows"], old[0]["rows"]):
        print("- %s, %s: %s / %s" % (r0["leg"], r0["shape"], ", ".join(r0["launches"]) or "-", ", ".join(p0["launches"]) or "-"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libnnc_mi355x.so")
    ap.add_argument("--label", default="this tree", help="'parent' for the parent commit's build")
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per leg: the median and the spread are reported")
    ap.add_argument("--window-ms", type=float, default=20.0, help="least work timed per window")
    ap.add_argument("--gnorm-half-native", type=int, default=None, help="set the GNORM_HALF_NATIVE tuning key")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--report", nargs="+", default=None, help="JSON files of earlier runs: print the comparison as markdown")
    args = ap.parse_args()
    if args.report:
        report(args.report)
    else:
        measure(args)


if __name__ == "__main__":
    main()
