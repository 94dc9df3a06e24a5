#!/usr/bin/env python
"""Time the commands a half-precision trainer issues on its gradients between backward and the optimizer -- REDUCE_NORM2_FORWARD into an fp32 element,
REDUCE_ISNAN_FORWARD into an int32 element and MUL_FORWARD(1) by an fp32 element IN PLACE -- on dense CCV_16F tensors of a transformer's gradient shapes:
[32000, 4096], [4096, 11008], [4096, 4096], the small [4096] and [11008], the whole clip sequence of ccv_cnnp_model_parameters_clip_grad_norm over a list of 200
gradients of mixed sizes (where the launch count shows), and the first shape in fp32 as the unchanged control -- each through the command interface, HIP-event
timed on a stream.  Per row: the median of `--repeats` windows, their spread (max - min), the fastest and the slowest window, the bytes the native route must move
(norm and NaN check: the tensor read once; scale: read and written once) and that traffic as a fraction of 6.29 TB/s, the measured copy rate of the MI355X
(profiles/row_half_bench.md).  Uses nothing but the command interface, so it runs unchanged on a build without the key (--lib): both sides of a comparison come
from this script, run alternately, and --report lays them side by side.
A large tensor (8 MB and more) is one of a ring of copies of at least 512 MiB that consecutive commands walk, so no command finds its tensor in the 256 MiB
Infinity Cache: those rows are HBM rates on both sides.  --sweep measures the one-workgroup threshold (see sweep()).
usage: python tools/grad_half_bench.py [--lib PATH] [--label NAME] [--repeats 21] [--window-ms 5] [--grad-half-native 0|1] [--json OUT]
       python tools/grad_half_bench.py --sweep [--repeats 15]
       python tools/grad_half_bench.py --report NEW1.json PARENT1.json [NEW2.json PARENT2.json]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HBM_COPY_TBS = 6.29
ROTATE_BYTES = 2 << 28  # twice the 256 MiB Infinity Cache
SWEEP = [4096, 16384, 32768, 65536, 98304, 131072, 196608, 262144, 524288]
LARGE = [(32000, 4096), (4096, 11008), (4096, 4096)]
SMALL = [(4096,), (11008,)]
# the list of 200: 8 MLP matrices, 24 attention matrices, 168 norm scales and biases
LIST = [(4096, 11008)] * 8 + [(4096, 4096)] * 24 + [(4096,), (11008,), (4096,)] * 56


def measure(args):
    from ccv_amd import nnc
    L = nnc.load(args.lib)
    print("library", L.dll.nnc_mi355x_version().decode(), args.lib or "")
    if args.grad_half_native is not None:
        try:
            L.tune_set("GRAD_HALF_NATIVE", args.grad_half_native)
            print("GRAD_HALF_NATIVE =", args.grad_half_native)
        except KeyError:
            print("this build has no GRAD_HALF_NATIVE key: skipped")
    s = L.stream_new(0)
    e0, e1 = L.dll.nnc_mi355x_event_new(), L.dll.nnc_mi355x_event_new()
    L.dll.nnc_mi355x_event_elapsed_ms.restype = nnc.C.c_float
    H, F, I = np.float16, np.float32, np.int32
    DT = {H: nnc.CCV_16F, F: nnc.CCV_32F, I: nnc.CCV_32S}

    def window(fn, reps):
        L.dll.nnc_mi355x_event_record(e0, s)
        for _ in range(reps):
            fn()
        L.dll.nnc_mi355x_event_record(e1, s)
        L.stream_wait(s)
        return L.dll.nnc_mi355x_event_elapsed_ms(e0, e1) / reps

    def timed(fn):
        """(sorted window times in ms per call, launch names of one call): a first call (code objects, arena growth) under the launch records, one timed call to size the windows, the windows"""
        L.profile_enable(0); L.profile_enable(1)
        fn()
        L.stream_wait(s)
        names = sorted(set(r[0].split("|")[-1].split("::")[-1] for r in L.profile_records()))
        L.profile_enable(0)
        one = window(fn, 1)
        reps = max(1, min(200, int(args.window_ms / max(one, 1e-3)) + 1))
        return sorted(window(fn, reps) for _ in range(max(1, args.repeats))), names

    rng = np.random.default_rng(0)
    pool = ((rng.random(1 << 22, dtype=F) - 0.5) * 4).astype(H)  # U(-2, 2), repeated to every shape below

    def dev(shape, dtype=H, value=None):
        x = np.full(shape, value, dtype) if value is not None else np.resize(pool, shape).astype(dtype)
        return L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, DT[dtype], shape, 0), x)

    def run(cmd, ins, outs):
        assert L.cmd_exec(cmd, nnc.NO_HINT, 0, ins, outs, s) == 0

    out = []

    def row(name, moved, fn):
        ms, names = timed(fn)
        med = ms[len(ms) // 2]
        frac = moved / (med * 1e-3) / (HBM_COPY_TBS * 1e12)
        out.append(dict(row=name, ms=med, spread=ms[-1] - ms[0], fastest=ms[0], slowest=ms[-1], mb=moved / 1e6, hbm=frac, launches=names))
        print("%-56s %9.4f ms (%.4f) [%.4f .. %.4f] | %8.2f MB | %5.3f | %s" % (name, med, ms[-1] - ms[0], ms[0], ms[-1], moved / 1e6, frac, ",".join(names)), flush=True)

    print("per row median ms (spread) [fastest .. slowest window] | MB the native route moves | fraction of %.2f TB/s | launches" % HBM_COPY_TBS)
    norm2_cmd, mul_cmd = nnc.CMD_REDUCE_NORM2_FORWARD(), nnc.CMD_MUL_FORWARD(1)
    one_f, flag = dev((1,), F, 1.0), dev((1,), I, 0)

    def three(shape, dtype, tname):
        """a large tensor is one of a ring of copies of at least 2 x 256 MiB that consecutive commands walk: no command finds its tensor in the Infinity Cache"""
        n, e = int(np.prod(shape)), np.dtype(dtype).itemsize
        copies = -(-ROTATE_BYTES // (n * e)) if n * e >= (1 << 23) else 1
        ring, norm = [dev(shape, dtype) for _ in range(copies)], dev((1,), F, 0.0)
        turn = [0]

        def nxt():
            turn[0] = (turn[0] + 1) % copies
            return ring[turn[0]]
        isnan_cmd = nnc.CMD_REDUCE_ISNAN_FORWARD(*range(len(shape)))
        what = "%s %s" % (tname, list(shape))
        row("norm2 " + what, e * n, lambda: run(norm2_cmd, [nxt()], [norm]))
        row("isnan " + what, e * n, lambda: run(isnan_cmd, [nxt()], [flag]))

        def scale():
            g = nxt()
            run(mul_cmd, [g, one_f], [g])
        row("scale in place " + what, 2 * e * n, scale)
        for g in ring:
            g.free()
        norm.free()

    for shape in LARGE + SMALL:
        three(shape, H, "half")

    grads = [dev(shape) for shape in LIST]
    total, norm2, maxn = dev((1,), F, 0.0), dev((1,), F, 0.0), dev((1,), F, 0.0)

    def clip():  # ccv_cnnp_model_addons.c: per gradient the norm, its square, the running sum; the scale; per gradient the scale in place
        run(nnc.CMD_SET_FORWARD(0), [], [total])
        for g in grads:
            run(norm2_cmd, [g], [norm2])
            run(mul_cmd, [norm2, norm2], [norm2])
            run(nnc.CMD_ADD_FORWARD(1, 1), [total, norm2], [total])
        run(nnc.CMD_EWSQRT_FORWARD(), [total], [total])
        run(nnc.CMD_SET_FORWARD(1.0), [], [maxn])
        run(nnc.CMD_EWDIV_FORWARD(), [maxn, total], [total])
        run(nnc.CMD_CLAMP_FORWARD(float("nan"), 1), [total], [total])
        for g in grads:
            run(mul_cmd, [g, total], [g])
    row("clip sequence, %d half gradients" % len(grads), 6 * sum(int(np.prod(sh)) for sh in LIST), clip)
    for g in grads:
        g.free()
    three(LARGE[0], F, "fp32")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(label=args.label, rows=out), f)


def sweep(args):
    """The one-workgroup threshold: the norm of one half tensor of n elements into an fp32 element with ONE workgroup at every size (GRAD_HALF_NATIVE = 2^30: the key
    above 1 is the threshold in elements) and with a first stage and a fold at every size above 2 (GRAD_HALF_NATIVE = 2), alternately, twice.  Per row: ms per command
    issued back to back on one stream (median of the windows [fastest .. slowest]: what a host that feeds the stream command by command sees; the kernel hides
    under the issue cost until it is longer), and the sum of the launch records of one command (HIP events around each single launch: the device's side, with the
    events' own cost in it, the kernel boundary between two launches not)."""
    from ccv_amd import nnc
    L = nnc.load(args.lib)
    s = L.stream_new(0)
    e0, e1 = L.dll.nnc_mi355x_event_new(), L.dll.nnc_mi355x_event_new()
    L.dll.nnc_mi355x_event_elapsed_ms.restype = nnc.C.c_float
    H, F = np.float16, np.float32
    rng = np.random.default_rng(0)
    cmd = nnc.CMD_REDUCE_NORM2_FORWARD()
    print("| n | launches | run | ms per command, back to back | ms in the launch records |")
    print("|---|---|---|---|---|")
    try:
        for rnd in (1, 2):
            for key, form in ((1 << 30, "one workgroup"), (2, "first stage + fold")):
                L.tune_set("GRAD_HALF_NATIVE", key)
                for n in SWEEP:
                    x = ((rng.random(n, dtype=F) - 0.5) * 4).astype(H)
                    g = L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_16F, (n,), 0), x)
                    o = L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_32F, (1,), 0), np.zeros(1, F))

                    def window(reps):
                        L.dll.nnc_mi355x_event_record(e0, s)
                        for _ in range(reps):
                            assert L.cmd_exec(cmd, nnc.NO_HINT, 0, [g], [o], s) == 0
                        L.dll.nnc_mi355x_event_record(e1, s)
                        L.stream_wait(s)
                        return L.dll.nnc_mi355x_event_elapsed_ms(e0, e1) / reps
                    window(3)
                    ms = sorted(window(args.sweep_reps) for _ in range(max(1, args.repeats)))
                    recs = []
                    for _ in range(9):
                        L.profile_enable(0); L.profile_enable(1)
                        assert L.cmd_exec(cmd, nnc.NO_HINT, 0, [g], [o], s) == 0
                        L.stream_wait(s)
                        recs.append(sum(r[3] for r in L.profile_records()))
                        L.profile_enable(0)
                    want = float(np.sqrt((x.astype(np.float64) ** 2).sum()))
                    assert abs(float(o.numpy()[0]) - want) <= (n + 2) * 2.0 ** -24 * want
                    print("| %d | %s | %d | %.4f [%.4f .. %.4f] | %.4f |" % (n, form, rnd, ms[len(ms) // 2], ms[0], ms[-1], sorted(recs)[4]), flush=True)
                    g.free(); o.free()
    finally:
        L.tune_set("GRAD_HALF_NATIVE", 1)


def report(paths):
    runs = [json.load(open(p)) for p in paths]
    new = [r for r in runs if r["label"] != "parent"]
    old = [r for r in runs if r["label"] == "parent"]
    print("Median ms [fastest .. slowest window] per run.  `MB`: what the native route must move.  `of copy rate`: those bytes per second at this tree's slowest window,")
    print("as a fraction of %.2f TB/s.  `faster`: a half row counts where this tree's SLOWEST window of every run is below the parent's FASTEST window of every run; the fp32" % HBM_COPY_TBS)
    print("rows are the control (the same kernels on both sides) and must overlap.\n")
    head = ["row", "MB"] + ["%s, run %d" % (lab, i + 1) for i in range(max(len(new), len(old))) for lab in ("this tree", "parent")][:len(runs)] + ["of copy rate", "faster / overlap", "parent / this tree"]
    print("| " + " | ".join(head) + " |")
    print("|" + "---|" * len(head))
    lost, apart = [], []
    for k, r0 in enumerate(new[0]["rows"]):
        ns, os_ = [r["rows"][k] for r in new], [r["rows"][k] for r in old]
        cells = []
        for i in range(max(len(ns), len(os_))):
            for xs in (ns, os_):
                if i < len(xs):
                    cells.append("%.4f [%.4f .. %.4f]" % (xs[i]["ms"], xs[i]["fastest"], xs[i]["slowest"]))
        slow_new, fast_new = max(x["slowest"] for x in ns), min(x["fastest"] for x in ns)
        slow_old, fast_old = max(x["slowest"] for x in os_), min(x["fastest"] for x in os_)
        frac = r0["mb"] * 1e6 / (slow_new * 1e-3) / (HBM_COPY_TBS * 1e12)
        if " fp32 " in r0["row"]:
            ok = fast_new <= slow_old and fast_old <= slow_new
            verdict = "overlap" if ok else "APART"
            if not ok:
                apart.append(r0["row"])
        else:
            ok = slow_new < fast_old
            verdict = "faster" if ok else "NOT faster"
            if not ok:
                lost.append(r0["row"])
        med = lambda xs: sorted(x["ms"] for x in xs)[len(xs) // 2]
        print("| %s | %.2f | %s | %.3f | %s | %.2fx |" % (r0["row"], r0["mb"], " | ".join(cells), frac, verdict, med(os_) / med(ns)))
    print("\nHalf rows whose slowest window is not below the parent's fastest: %s." % ("; ".join(lost) or "none"))
    print("fp32 control rows whose windows do not overlap: %s." % ("; ".join(apart) or "none"))
    print("\nKernels of one command, this tree / parent (conversions to and from fp32 images and the generic fp32 kernels file no launch records):\n")
    for r0, p0 in zip(new[0]["rows"], old[0]["rows"]):
        print("- %s: %s / %s" % (r0["row"], ", ".join(r0["launches"]) or "-", ", ".join(p0["launches"]) or "-"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libnnc_mi355x.so")
    ap.add_argument("--label", default="this tree", help="'parent' for the parent commit's build")
    ap.add_argument("--repeats", type=int, default=21, help="timed windows per row: the median, the spread, the fastest and the slowest are reported")
    ap.add_argument("--window-ms", type=float, default=5.0, help="least work timed per window")
    ap.add_argument("--grad-half-native", type=int, default=None, help="set the GRAD_HALF_NATIVE tuning key")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--sweep", action="store_true", help="the one-workgroup threshold: the norm at sizes around it, one workgroup against two launches (markdown rows)")
    ap.add_argument("--sweep-reps", type=int, default=500, help="--sweep: commands per window")
    ap.add_argument("--report", nargs="+", default=None, help="JSON files of earlier runs: print the comparison as markdown")
    args = ap.parse_args()
    if args.report:
        report(args.report)
    elif args.sweep:
        sweep(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
