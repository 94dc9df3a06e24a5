#!/usr/bin/env python
"""Time INDEX_SELECT_FORWARD / INDEX_SELECT_BACKWARD and PAD in half precision (every data tensor CCV_16F, as an all-half graph issues them) at sizes a user runs:
gathers from and scatter-adds into a CLIP-sized [49408, 768] and a language-model-sized [32000, 4096] embedding table with 77, 77 * 16 and 8192 indices, drawn
uniformly and drawn with one index repeated in half the positions; the fp32 scatter-add of the same shapes (INDEX_BACK_TILES moves it too); and the pad of
[8, 320, 64, 64] by one pixel on each side of both image axes, zero and replicate, and its crop -- each as ONE command through the command interface, HIP-event
timed on a stream.  Per row: the median of `--repeats` windows, their spread (max - min), the bytes the native route must move and that traffic as a fraction of
6.29 TB/s, the measured copy rate of the MI355X (profiles/row_half_bench.md).  Bytes: a gather reads and writes the selected rows; a scatter-add reads g and
writes all of h; a pad reads a and writes b.  Uses nothing but the command interface, so it runs unchanged on a build without the keys (--lib): both sides of a
comparison come from this script, run alternately, and --report lays the runs side by side.
usage: python tools/index_pad_half_bench.py [--lib PATH] [--label NAME] [--repeats 21] [--window-ms 5] [--index-pad-half-native 0|1] [--index-back-tiles 0|1] [--json OUT]
       python tools/index_pad_half_bench.py --report NEW1.json PARENT1.json [NEW2.json PARENT2.json]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HBM_COPY_TBS = 6.29
TABLES = [(49408, 768), (32000, 4096)]
COUNTS = [77, 77 * 16, 8192]
PAD = ((8, 320, 64, 64), (0, 0, 1, 1), (0, 0, 1, 1))


def measure(args):
    from ccv_amd import nnc
    L = nnc.load(args.lib)
    print("library", L.dll.nnc_mi355x_version().decode(), args.lib or "")
    for key, value in (("INDEX_PAD_HALF_NATIVE", args.index_pad_half_native), ("INDEX_BACK_TILES", args.index_back_tiles)):
        if value is not None:
            try:
                L.tune_set(key, value)
                print(key, "=", value)
            except KeyError:
                print("this build has no %s key: skipped" % key)
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

    def dev(shape, dtype=H, zero=False, fmt=None):
        x = np.zeros(shape, dtype) if zero else np.resize(pool, shape).astype(dtype)
        return L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, fmt or nnc.NHWC, nnc.CCV_16F if dtype == H else nnc.CCV_32F, shape, 0), x)

    out = []

    def row(name, moved, cmd, ins, outs):
        ms, spread, names = timed(cmd, ins, outs)
        frac = moved / (ms * 1e-3) / (HBM_COPY_TBS * 1e12)
        out.append(dict(row=name, ms=ms, spread=spread, mb=moved / 1e6, hbm=frac, launches=names))
        print("%-64s %9.4f ms (%.4f) | %8.2f MB | %5.3f | %s" % (name, ms, spread, moved / 1e6, frac, ",".join(names)), flush=True)

    print("per row median ms (spread) | MB the native route moves | fraction of %.2f TB/s | launches" % HBM_COPY_TBS)
    fwd, bwd = nnc.generic_cmd("INDEX_SELECT_FORWARD"), nnc.generic_cmd("INDEX_SELECT_BACKWARD")
    for rows, cols in TABLES:
        table, grad = dev((rows, cols)), dev((rows, cols), zero=True)
        grad32 = dev((rows, cols), F, True)
        for n in COUNTS:
            sel, sel32, into = dev((n, cols)), dev((n, cols), F), dev((n, cols), zero=True)
            for draw in ("uniform", "half on one row"):
                idx = np.random.default_rng(n).integers(0, rows, n).astype(np.int32)
                if draw != "uniform":
                    idx[::2] = rows // 3
                it = L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_32S, (n,), 0), idx)
                what = "[%d,%d] %d indices, %s" % (rows, cols, n, draw)
                row("gather half " + what, 2 * 2 * n * cols, fwd, [table, it], [into])
                row("scatter-add half " + what, 2 * (n + rows) * cols, bwd, [sel, None, it], [grad])
                row("scatter-add fp32 " + what, 4 * (n + rows) * cols, bwd, [sel32, None, it], [grad32])
                it.free()
            sel.free(); sel32.free(); into.free()
        table.free(); grad.free(); grad32.free()
    shape, begin, end = PAD
    big = tuple(d + b + e for d, b, e in zip(shape, begin, end))
    na, nb = int(np.prod(shape)), int(np.prod(big))
    for dtype, tname in ((H, "half"), (F, "fp32")):
        a, b = dev(shape, dtype, fmt=nnc.NCHW), dev(big, dtype, True, fmt=nnc.NCHW)
        e = np.dtype(dtype).itemsize
        row("pad zero %s %s" % (tname, list(shape)), e * (na + nb), nnc.CMD_PAD("PAD_FORWARD", 0, begin, end), [a], [b])
        row("pad replicate %s %s" % (tname, list(shape)), e * (na + nb), nnc.CMD_PAD("PAD_FORWARD", 1, begin, end), [a], [b])
        row("pad backward %s %s" % (tname, list(shape)), e * 2 * na, nnc.CMD_PAD("PAD_BACKWARD", 0, begin, end), [b], [a])
        a.free(); b.free()
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
        if margin <= 2:
            lost.append(r0["row"])
        print("| %s | %.2f | %s | %.3f | %.4f | %.1f | %.2fx |" % (r0["row"], r0["mb"], " | ".join(cells), frac, spread, margin, fast_old / slow_new))
    print("\nRows not faster than the parent by more than twice its spread: %s." % ("; ".join(lost) or "none"))
    print("\nKernels of one command, this tree / parent (conversions to and from fp32 images and the parent's fp32 kernels file no launch records):\n")
    for r0, p0 in zip(new[0]["rows"], old[0]["rows"]):
        print("- %s: %s / %s" % (r0["row"], ", ".join(r0["launches"]) or "-", ", ".join(p0["launches"]) or "-"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libnnc_mi355x.so")
    ap.add_argument("--label", default="this tree", help="'parent' for the parent commit's build")
    ap.add_argument("--repeats", type=int, default=21, help="timed windows per row: the median and the spread are reported")
    ap.add_argument("--window-ms", type=float, default=5.0, help="least work timed per window")
    ap.add_argument("--index-pad-half-native", type=int, default=None, help="set the INDEX_PAD_HALF_NATIVE tuning key")
    ap.add_argument("--index-back-tiles", type=int, default=None, help="set the INDEX_BACK_TILES tuning key")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--report", nargs="+", default=None, help="JSON files of earlier runs: print the comparison as markdown")
    args = ap.parse_args()
    if args.report:
        report(args.report)
    else:
        measure(args)


if __name__ == "__main__":
    main()
