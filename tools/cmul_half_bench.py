#!/usr/bin/env python
"""Time CMUL_FORWARD / CMUL_BACKWARD in half precision (every tensor CCV_16F, as an all-half graph issues them) at sizes a user runs: rotary position embeddings
applied to q of [batch, tokens, heads, 128] from a table of [1, tokens, 1, 128] -- the forward command, the gradient of q (dq = g conj(table): a map) and the
gradient of the table (g conj(q) summed over batch and heads: one lane per output vector walks the sum) -- the same on a CLIP-text-sized [2,77,12,64], a
same-shape [4096,3072] product forward and backward, and the first shape pair in fp32 as the unchanged control -- each as ONE command through the command
interface, HIP-event timed on a stream.  Per row: the median of `--repeats` windows, their spread (max - min), the bytes the native route must move (every tensor
of the command once) and that traffic as a fraction of 6.29 TB/s, the measured copy rate of the MI355X (profiles/row_half_bench.md).  Uses nothing but the command
interface, so it runs unchanged on a build without the key (--lib): both sides of a comparison come from this script, run alternately, and --report lays the
runs side by side.
usage: python tools/cmul_half_bench.py [--lib PATH] [--label NAME] [--repeats 21] [--window-ms 5] [--cmul-half-native 0|1] [--json OUT]
       python tools/cmul_half_bench.py --report NEW1.json PARENT1.json [NEW2.json PARENT2.json]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HBM_COPY_TBS = 6.29
ROTARY = [((2, 4096, 24, 128), (1, 4096, 1, 128)), ((1, 2048, 32, 128), (1, 2048, 1, 128)), ((2, 77, 12, 64), (1, 77, 1, 64))]
SAME = (4096, 3072)


def measure(args):
    from ccv_amd import nnc
    L = nnc.load(args.lib)
    print("library", L.dll.nnc_mi355x_version().decode(), args.lib or "")
    if args.cmul_half_native is not None:
        try:
            L.tune_set("CMUL_HALF_NATIVE", args.cmul_half_native)
            print("CMUL_HALF_NATIVE =", args.cmul_half_native)
        except KeyError:
            print("this build has no CMUL_HALF_NATIVE key: skipped")
    s = L.stream_new(0)
    e0, e1 = L.dll.nnc_mi355x_event_new(), L.dll.nnc_mi355x_event_new()
    L.dll.nnc_mi355x_event_elapsed_ms.restype = nnc.C.c_float
    H, F = np.float16, np.float32

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
        reps = max(1, min(200, int(args.window_ms / max(one, 1e-3)) + 1))
        ms = sorted(window(cmd, ins, outs, reps) for _ in range(max(1, args.repeats)))
        return ms[len(ms) // 2], ms[-1] - ms[0], names

    rng = np.random.default_rng(0)
    pool = ((rng.random(1 << 22, dtype=F) - 0.5) * 4).astype(H)  # U(-2, 2), repeated to every shape below

    def dev(shape, dtype=H, zero=False):
        x = np.zeros(shape, dtype) if zero else np.resize(pool, shape).astype(dtype)
        return L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_16F if dtype == H else nnc.CCV_32F, shape, 0), x)

    out = []

    def row(name, moved, cmd, ins, outs):
        ms, spread, names = timed(cmd, ins, outs)
        frac = moved / (ms * 1e-3) / (HBM_COPY_TBS * 1e12)
        out.append(dict(row=name, ms=ms, spread=spread, mb=moved / 1e6, hbm=frac, launches=names))
        print("%-64s %9.4f ms (%.4f) | %8.2f MB | %5.3f | %s" % (name, ms, spread, moved / 1e6, frac, ",".join(names)), flush=True)

    print("per row median ms (spread) | MB the native route moves | fraction of %.2f TB/s | launches" % HBM_COPY_TBS)
    fwd, bwd = nnc.CMD_CMUL_FORWARD(), nnc.CMD_CMUL_BACKWARD()

    def rotary(big, small, dtype, tname, backward):
        nb, ns, e = int(np.prod(big)), int(np.prod(small)), np.dtype(dtype).itemsize
        q, rot, g = dev(big, dtype), dev(small, dtype), dev(big, dtype)
        c, drot = dev(big, dtype, True), dev(small, dtype, True)
        what = "%s %s x %s" % (tname, list(big), list(small))
        row("forward " + what, e * (2 * nb + ns), fwd, [q, rot], [c])
        if backward > 0:
            row("dq " + what, e * (2 * nb + ns), bwd, [g, q, rot], [c, None])
        if backward > 1:
            row("gradient of the table " + what, e * (2 * nb + ns), bwd, [g, q, rot], [None, drot])
        for t in (q, rot, g, c, drot):
            t.free()

    rotary(ROTARY[0][0], ROTARY[0][1], H, "half", 2)
    rotary(ROTARY[1][0], ROTARY[1][1], H, "half", 1)
    rotary(ROTARY[2][0], ROTARY[2][1], H, "half", 0)
    n = int(np.prod(SAME))
    a, b, g, da, db = dev(SAME), dev(SAME), dev(SAME), dev(SAME, zero=True), dev(SAME, zero=True)
    row("forward half %s same-shape" % list(SAME), 2 * 3 * n, fwd, [a, b], [da])
    row("backward, both outputs half %s same-shape" % list(SAME), 2 * 6 * n, bwd, [g, a, b], [da, db])  # two launches: g and the other operand read, the gradient written, twice
    for t in (a, b, g, da, db):
        t.free()
    rotary(ROTARY[0][0], ROTARY[0][1], F, "fp32", 0)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(label=args.label, rows=out), f)


def report(paths):
    runs = [json.load(open(p)) for p in paths]
    new = [r for r in runs if r["label"] != "parent"]
    old = [r for r in runs if r["label"] == "parent"]
    print("Median ms (spread = max - min of the windows).  `MB`: what the native route must move.  `of copy rate`: those bytes per second of this tree's slower run, as a")
    print("fraction of %.2f TB/s.  `parent spread`: the largest of the parent's window spreads and the distance between its runs.  `margin`: (the parent's faster run -" % HBM_COPY_TBS)
    print("this tree's slower run) / parent spread; a row counts as faster where it is above 2.\n")
    head = ["row", "MB"] + ["%s, run %d" % (lab, i + 1) for i in range(max(len(new), len(old))) for lab in ("this tree", "parent")][:len(runs)] + ["of copy rate", "parent spread", "margin", "parent / this tree"]
    print("| " + " | ".join(head) + " |")
    print("|" + "---|" * len(head))
    lost = []
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
        if margin <= 2 and " fp32 " not in r0["row"]:  # (the fp32 row is the control: the same kernel on both sides)
            lost.append(r0["row"])
        print("| %s | %.2f | %s | %.3f | %.4f | %.1f | %.2fx |" % (r0["row"], r0["mb"], " | ".join(cells), frac, spread, margin, fast_old / slow_new))
    print("\nHalf rows not faster than the parent by more than twice its spread: %s." % ("; ".join(lost) or "none"))
    print("\nKernels of one command, this tree / parent (conversions to and from fp32 images and the fp32 kernel file no launch records):\n")
    for r0, p0 in zip(new[0]["rows"], old[0]["rows"]):
        print("- %s: %s / %s" % (r0["row"], ", ".join(r0["launches"]) or "-", ", ".join(p0["launches"]) or "-"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libnnc_mi355x.so")
    ap.add_argument("--label", default="this tree", help="'parent' for the parent commit's build")
    ap.add_argument("--repeats", type=int, default=21, help="timed windows per row: the median and the spread are reported")
    ap.add_argument("--window-ms", type=float, default=5.0, help="least work timed per window")
    ap.add_argument("--cmul-half-native", type=int, default=None, help="set the CMUL_HALF_NATIVE tuning key")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--report", nargs="+", default=None, help="JSON files of earlier runs: print the comparison as markdown")
    args = ap.parse_args()
    if args.report:
        report(args.report)
    else:
        measure(args)


if __name__ == "__main__":
    main()
