#!/usr/bin/env python
"""Time the optimizer commands a half-precision trainer ends its step with: ONE command per parameter tensor, issued in place (b = a, n = m, u = v) back to
back on a stream, for the parameter tensors of EfficientNet-B0 (the reference's ImageNet trainer) and of ResNet-50 v1d -- both lists are derived below from
the networks' block tables.  Legs: RMSPROP and ADAM, every tensor half ("hh") and half gradients into fp32 parameters and state ("hf").  A walk over the
whole list is one HIP-event window; reported are the median of `--repeats` walks, their spread (max - min) and the microseconds per command.  Then one tensor
of 16 Mi elements per leg (ADAM with amsgrad as well) and the native-half SGD command at the same count: median time and achieved bytes per second, every tensor counted once, beside
6.29 TB/s, the measured copy rate of the MI355X.
Uses nothing but the command interface, so it runs unchanged on another build (--lib) or with the tuning key at 0: both sides of a comparison come from
this script.  `--json OUT` keeps a run's rows; `--report A.json B.json ... --md OUT.md` writes the table of several runs side by side.
usage: python tools/optim_half_bench.py [--lib PATH] [--label NAME] [--repeats 7] [--opt-half-native 0|1] [--json OUT]
       python tools/optim_half_bench.py --report RUN.json [RUN.json ...] --md profiles/optim_half_bench.md"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_COPY_TBS = 6.29
BIG = 16 << 20

# EfficientNet-B0: (repeats, kernel, stride, expansion, in, out) per stage; squeeze-excite at a quarter of the block's input channels
B0_BLOCKS = [(1, 3, 1, 1, 32, 16), (2, 3, 2, 6, 16, 24), (2, 5, 2, 6, 24, 40), (3, 3, 2, 6, 40, 80), (3, 5, 1, 6, 80, 112), (4, 5, 2, 6, 112, 192), (1, 3, 1, 6, 192, 320)]
# ResNet-50 v1d: (blocks, bottleneck width) per stage; the stem is three 3 x 3 convolutions, the shortcut of a stage's first block a 1 x 1 convolution behind an average pool
R50_STAGES = [(3, 64), (4, 128), (6, 256), (3, 512)]


def bn(c):
    return [c, c]  # scale, bias


def efficientnet_b0_params():
    p = [3 * 3 * 3 * 32] + bn(32)
    for repeats, k, _stride, e, cin, cout in B0_BLOCKS:
        for r in range(repeats):
            c = cin if r == 0 else cout
            mid, se = c * e, max(1, c // 4)
            if e != 1:
                p += [c * mid] + bn(mid)
            p += [k * k * mid] + bn(mid)
            p += [mid * se, se, se * mid, mid]  # squeeze-excite: two 1 x 1 convolutions with biases
            p += [mid * cout] + bn(cout)
    return p + [320 * 1280] + bn(1280) + [1280 * 1000, 1000]


def resnet50_v1d_params():
    p = [3 * 3 * 3 * 32] + bn(32) + [3 * 3 * 32 * 32] + bn(32) + [3 * 3 * 32 * 64] + bn(64)
    cin = 64
    for blocks, mid in R50_STAGES:
        for r in range(blocks):
            if r == 0:
                p += [cin * mid * 4] + bn(mid * 4)
            p += [cin * mid] + bn(mid) + [3 * 3 * mid * mid] + bn(mid) + [mid * mid * 4] + bn(mid * 4)
            cin = mid * 4
    return p + [2048 * 1000, 1000]


LISTS = [("EfficientNet-B0", efficientnet_b0_params), ("ResNet-50 v1d", resnet50_v1d_params)]


def measure(args):
    from ccv_amd import nnc
    L = nnc.load(args.lib)
    version = L.dll.nnc_mi355x_version().decode()
    print("library", version, args.lib or "")
    if args.opt_half_native is not None:
        try:
            L.tune_set("OPT_HALF_NATIVE", args.opt_half_native)
            print("OPT_HALF_NATIVE =", args.opt_half_native)
        except KeyError:
            print("this build has no OPT_HALF_NATIVE key: skipped")
    s = L.stream_new(0)
    e0, e1 = L.dll.nnc_mi355x_event_new(), L.dll.nnc_mi355x_event_new()
    L.dll.nnc_mi355x_event_elapsed_ms.restype = nnc.C.c_float
    H, F = nnc.CCV_16F, nnc.CCV_32F
    rms = nnc.CMD_RMSPROP_FORWARD(0.001, 1e-5, 0.9, 0.9, 1e-3)
    adam = nnc.CMD_ADAM_FORWARD(3, 0.001, 0.9, 0.999, 0.0, 1e-8)
    adam_ams = nnc.CMD_ADAM_FORWARD(3, 0.001, 0.9, 0.999, 0.0, 1e-8, amsgrad=1)
    sgd = nnc.CMD_SGD_FORWARD(0, 0.001, 1.0, 1e-5, 0.9, 0.0)

    def tensors(n, tg, tp, states):
        """g and `states` parameter / state tensors of n elements, set to small values"""
        ts = [L.tensor(nnc.GPU_TENSOR_NHWC(0, tg, n))] + [L.tensor(nnc.GPU_TENSOR_NHWC(0, tp, n)) for _ in range(states)]
        L.cmd_exec(nnc.CMD_SET_FORWARD(0.01), nnc.NO_HINT, 0, [], ts, s)
        return ts

    def walk(cmd, sets, reps=1):
        L.dll.nnc_mi355x_event_record(e0, s)
        for _ in range(reps):
            for ts in sets:
                assert L.cmd_exec(cmd, nnc.NO_HINT, 0, ts, ts[1:], s) == 0
        L.dll.nnc_mi355x_event_record(e1, s)
        L.stream_wait(s)
        return L.dll.nnc_mi355x_event_elapsed_ms(e0, e1) / reps

    def timed(cmd, sets, reps=1):
        """(median ms, spread) of --repeats windows after three warm walks (code objects, workspace and staging growth, the first touches of fresh allocations)"""
        for _ in range(3):
            walk(cmd, sets)
        ms = sorted(walk(cmd, sets, reps) for _ in range(max(1, args.repeats)))
        return ms[len(ms) // 2], ms[-1] - ms[0]

    rows = []
    legs = [("RMSPROP", rms, 3), ("ADAM", adam, 3)]
    for net, params in LISTS:
        sizes = params()
        small = sum(1 for n in sizes if n < 2000)
        print("\n%s: %d parameter tensors, %d of them under 2 000 elements, %.2f M elements" % (net, len(sizes), small, sum(sizes) / 1e6))
        for combo, tg, tp in (("hh", H, H), ("hf", H, F)):
            sets = [tensors(n, tg, tp, 3) for n in sizes]
            for name, cmd, _ in legs:
                ms, spread = timed(cmd, sets)
                rows.append(dict(kind="list", net=net, leg="%s %s" % (name, combo), tensors=len(sizes), ms=ms, spread=spread, us_per_cmd=ms * 1e3 / len(sizes)))
                print("%-16s %-10s walk %8.3f ms (spread %.3f) | %6.2f us per command" % (net, name + " " + combo, ms, spread, ms * 1e3 / len(sizes)), flush=True)
            for ts in sets:
                for t in ts:
                    t.free()
    print("\n%d elements: median ms (spread) | bytes per element | TB/s | fraction of %.2f TB/s" % (BIG, HBM_COPY_TBS))
    big = [("SGD hh", sgd, H, H, 2, 10), ("RMSPROP hh", rms, H, H, 3, 14), ("ADAM hh", adam, H, H, 3, 14), ("ADAM amsgrad hh", adam_ams, H, H, 4, 18),
           ("RMSPROP hf", rms, H, F, 3, 30), ("ADAM hf", adam, H, F, 3, 30)]
    for name, cmd, tg, tp, states, bpe in big:
        ts = tensors(BIG, tg, tp, states)
        ms, spread = timed(cmd, [ts], reps=10)
        tbs = BIG * bpe / (ms * 1e-3) / 1e12
        rows.append(dict(kind="big", leg=name, ms=ms, spread=spread, bytes_per_element=bpe, tbs=tbs))
        print("%-16s %8.4f ms (%.4f) | %2d | %5.2f TB/s | %5.3f" % (name, ms, spread, bpe, tbs, tbs / HBM_COPY_TBS), flush=True)
        for t in ts:
            t.free()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(label=args.label or version, rows=rows), f)


def report(args):
    runs = [json.load(open(p)) for p in args.report]
    out = ["# Optimizer commands in half precision: one command per parameter tensor", "",
           "Written by `tools/optim_half_bench.py --report`; the runs below were measured one after the other in one session on one MI355X.", "",
           "## Parameter lists: a walk over the whole list, milliseconds (spread of the repeats) and microseconds per command", "",
           "| list | leg | tensors | " + " | ".join(r["label"] for r in runs) + " |", "|---|---|---|" + "---|" * len(runs)]
    keys = [(r["net"], r["leg"], r["tensors"]) for r in runs[0]["rows"] if r["kind"] == "list"]
    for net, leg, count in keys:
        cells = []
        for run in runs:
            m = [r for r in run["rows"] if r["kind"] == "list" and r["net"] == net and r["leg"] == leg]
            cells.append("%.3f (%.3f), %.2f us" % (m[0]["ms"], m[0]["spread"], m[0]["us_per_cmd"]) if m else "-")
        out.append("| %s | %s | %d | %s |" % (net, leg, count, " | ".join(cells)))
    out += ["", "## One tensor of %d elements: milliseconds (spread), achieved TB/s with every tensor counted once (copy rate: %.2f TB/s)" % (BIG, HBM_COPY_TBS), "",
            "| leg | bytes per element | " + " | ".join(r["label"] for r in runs) + " |", "|---|---|" + "---|" * len(runs)]
    for leg, bpe in [(r["leg"], r["bytes_per_element"]) for r in runs[0]["rows"] if r["kind"] == "big"]:
        cells = []
        for run in runs:
            m = [r for r in run["rows"] if r["kind"] == "big" and r["leg"] == leg]
            cells.append("%.4f (%.4f), %.2f TB/s" % (m[0]["ms"], m[0]["spread"], m[0]["tbs"]) if m else "-")
        out.append("| %s | %d | %s |" % (leg, bpe, " | ".join(cells)))
    with open(args.md, "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libnnc_mi355x.so")
    ap.add_argument("--label", default=None, help="the run's column title in the report")
    ap.add_argument("--repeats", type=int, default=7, help="timed walks per leg: the median and the spread are reported")
    ap.add_argument("--opt-half-native", type=int, default=None, help="set the OPT_HALF_NATIVE tuning key")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--report", nargs="+", default=None, help="runs written with --json: print them side by side instead of measuring")
    ap.add_argument("--md", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "optim_half_bench.md"))
    args = ap.parse_args()
    if args.report:
        report(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
