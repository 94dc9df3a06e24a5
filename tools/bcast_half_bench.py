#!/usr/bin/env python
"""Time the broadcast arithmetic commands in half precision (every tensor CCV_16F, as an all-half graph issues them) at sizes a user runs: ADD with a bias
vector, with a same-shape operand and with one value per NCHW channel, and the backward of each; same-shape MUL forward and backward; SCALAR_MUL in place;
REDUCE_MEAN as the global average pool of an NCHW and an NHWC map, forward and backward; REDUCE_SUM of a whole tensor to one value -- each as ONE command
through the command interface, HIP-event timed on a stream.  Per row: the median of `--repeats` windows, their spread (max - min), the bytes the native
route must move (every large tensor read or written once; the small operands are noise) and that traffic as a fraction of 6.29 TB/s, the measured copy rate
of the MI355X (profiles/row_half_bench.md).  Uses nothing but the command interface, so it runs unchanged on a build without the BCAST_HALF_NATIVE key
(--lib): both sides of a comparison come from this script, run alternately, and --report lays the runs side by side.
usage: python tools/bcast_half_bench.py [--lib PATH] [--label NAME] [--repeats 7] [--window-ms 20] [--bcast-half-native 0|1] [--json OUT]
       python tools/bcast_half_bench.py --report NEW1.json PARENT1.json NEW2.json PARENT2.json > profiles/bcast_half_bench.md"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HBM_COPY_TBS = 6.29
P, Q, S = 0.7, -1.3, 0.3
SEQ, NCHW, GATE, POOL_NCHW, POOL_NHWC = (8, 1024, 4096), (256, 64, 56, 56), (8, 1024, 11008), (256, 2048, 7, 7), (256, 7, 7, 2048)
SCALAR_N = 64 << 20


def measure(args):
    from ccv_amd import nnc
    L = nnc.load(args.lib)
    print("library", L.dll.nnc_mi355x_version().decode(), args.lib or "")
    if args.bcast_half_native is not None:
        try:
            L.tune_set("BCAST_HALF_NATIVE", args.bcast_half_native)
            print("BCAST_HALF_NATIVE =", args.bcast_half_native)
        except KeyError:
            print("this build has no BCAST_HALF_NATIVE key: skipped")
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

    rng = np.random.default_rng(0)
    pool = ((rng.random(int(np.prod(GATE)), dtype=np.float32) - 0.5) * 4).astype(H)  # U(-2, 2), cut to every shape below

    def dev(shape, zero=False):
        n = int(np.prod(shape))
        x = np.zeros(shape, H) if zero else pool[:n].reshape(shape)
        return L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_16F, shape, 0), x)

    out = []

    def row(name, cmd, ins, outs, large):
        """large: the number of large-tensor passes the native route must make (reads + writes), times the large tensor's bytes"""
        ms, spread, names = timed(cmd, ins, outs)
        frac = large / (ms * 1e-3) / (HBM_COPY_TBS * 1e12)
        out.append(dict(row=name, ms=ms, spread=spread, mb=large / 1e6, hbm=frac, launches=names))
        print("%-58s %9.4f ms (%.4f) | %8.2f MB | %5.3f | %s" % (name, ms, spread, large / 1e6, frac, ",".join(names)), flush=True)

    def free(*ts):
        for t in ts:
            t.free()

    print("per row median ms (spread) | MB the native route moves | fraction of %.2f TB/s | launches" % HBM_COPY_TBS)
    add, addb = nnc.CMD_ADD_FORWARD(P, Q), nnc.CMD_ADD_BACKWARD(P, Q)
    # ADD [8, 1024, 4096] + [4096], + same shape, and the backward of each
    big = int(np.prod(SEQ)) * 2
    a, b, c, v, dv = dev(SEQ), dev(SEQ), dev(SEQ, True), dev(SEQ[-1:]), dev(SEQ[-1:], True)
    row("ADD [8,1024,4096] + [4096]", add, [a, v], [c], 2 * big)
    row("ADD [8,1024,4096] + [4096] backward", addb, [a], [c, dv], 2 * big)
    row("ADD [8,1024,4096] + same shape", add, [a, b], [c], 3 * big)
    row("ADD [8,1024,4096] + same shape backward", addb, [a], [b, c], 3 * big)
    one = dev((1,), True)
    row("REDUCE_SUM [8,1024,4096] over all axes", nnc.CMD_REDUCE_SUM_FORWARD(0, 1, 2), [a], [one], big)
    free(a, b, c, v, dv, one)
    # ADD [256, 64, 56, 56] + [1, 64, 1, 1]
    big = int(np.prod(NCHW)) * 2
    a, c, v, dv = dev(NCHW), dev(NCHW, True), dev((1, NCHW[1], 1, 1)), dev((1, NCHW[1], 1, 1), True)
    row("ADD [256,64,56,56] + [1,64,1,1]", add, [a, v], [c], 2 * big)
    row("ADD [256,64,56,56] + [1,64,1,1] backward", addb, [a], [c, dv], 2 * big)
    free(a, c, v, dv)
    # MUL, same shape
    big = int(np.prod(GATE)) * 2
    g, a, b, da, db = dev(GATE), dev(GATE), dev(GATE), dev(GATE, True), dev(GATE, True)
    row("MUL [8,1024,11008] same shape", nnc.CMD_MUL_FORWARD(P), [a, b], [da], 3 * big)
    row("MUL [8,1024,11008] same shape backward", nnc.CMD_MUL_BACKWARD(P), [g, a, b], [da, db], 5 * big)
    free(g, a, b, da, db)
    # SCALAR_MUL in place (s = 1 here: the tensor keeps its values over the timed calls; the kernel multiplies all the same)
    a = dev((SCALAR_N,))
    row("SCALAR_MUL 64 M elements, in place", nnc.CMD_SCALAR_MUL_FORWARD(1.0), [a], [a], 2 * SCALAR_N * 2)
    free(a)
    # REDUCE_MEAN: the global average pool
    for shape, axes, name in ((POOL_NCHW, (2, 3), "[256,2048,7,7] -> [256,2048,1,1]"), (POOL_NHWC, (1, 2), "[256,7,7,2048] -> [256,1,1,2048]")):
        small = tuple(1 if k in axes else d for k, d in enumerate(shape))
        big = int(np.prod(shape)) * 2
        a, h, m = dev(shape), dev(shape, True), dev(small, True)
        row("REDUCE_MEAN %s" % name, nnc.CMD_REDUCE_MEAN_FORWARD(*axes), [a], [m], big)
        row("REDUCE_MEAN %s backward" % name, nnc.CMD_REDUCE_MEAN_BACKWARD(*axes), [m], [h], big)
        free(a, h, m)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(label=args.label, rows=out), f)


def report(paths):
    runs = [json.load(open(p)) for p in paths]
    new = [r for r in runs if r["label"] != "parent"]
    old = [r for r in runs if r["label"] == "parent"]
    print("# Broadcast arithmetic in half precision: one command, every tensor CCV_16F\n")
    print("Written by `tools/bcast_half_bench.py --report`; the runs below were measured alternately (this tree, parent, ...) in one session on one MI355X.")
    print("Per run: the median of the timed windows in milliseconds and, in brackets, their spread (max - min).  `MB`: what the native route must move (every")
    print("large tensor read or written once).  `of copy rate`: those bytes per second of this tree's slower run, as a fraction of %.2f TB/s.  `parent spread`:" % HBM_COPY_TBS)
    print("the largest of the parent's window spreads and the distance between its runs.  `margin`: (the parent's faster run - this tree's slower run) / parent")
    print("spread; a row is done where it is above 2.  A fraction above 1 is no error of the clock: a window repeats one command on the same tensors, and the rows")
    print("whose tensors together stay under the 256 MiB last-level cache are served from it in part.\n")
    head = ["row", "MB"] + ["%s, run %d" % (lab, i + 1) for i in range(max(len(new), len(old))) for lab in ("this tree", "parent")][:len(runs)] + ["of copy rate", "parent spread", "margin"]
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
            worst = (frac, r0["row"])
        if margin <= 2:
            lost.append(r0["row"])
        print("| %s | %.1f | %s | %.3f | %.4f | %.1f |" % (r0["row"], r0["mb"], " | ".join(cells), frac, spread, margin))
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
    ap.add_argument("--bcast-half-native", type=int, default=None, help="set the BCAST_HALF_NATIVE tuning key")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--report", nargs="+", default=None, help="JSON files of earlier runs: print the comparison as markdown")
    args = ap.parse_args()
    if args.report:
        report(args.report)
    else:
        measure(args)


if __name__ == "__main__":
    main()
