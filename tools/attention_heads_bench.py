#!/usr/bin/env python
"""Time SCALED_DOT_PRODUCT_ATTENTION_FORWARD on CCV_16F tensors at the head sizes of the diffusion U-Nets (40, 80, 160) and of current transformers (256, grouped
heads, causal), with D = 64 as the control (sdpa_forw_f16_kernel on both sides) -- each as ONE command through the command interface, HIP-event timed on a stream
after a warm-up of every shape.  Per row: the median of `--repeats` windows of at least `--window-ms`, their spread (max - min) and the TFLOP/s of
2 B Hq R C (D + Dv) products (halved for causal rows).  Uses nothing but the command interface, so it runs unchanged on a build without sdpa_fwd_anyd_f16_kernel
(--lib): both sides of a comparison come from this script, run alternately, and --report lays the runs side by side.  --key2 adds, for information, rows with the
tuning key SDPA_F16_ANYD at 2 (the new kernel on sdpa_forw_f16_kernel's shapes) at D = 64 and D = 128.  --backward times ONE
SCALED_DOT_PRODUCT_ATTENTION_BACKWARD (g, q, k, v -> dq, dk, dv) per row on the same shapes instead: the TFLOP/s are then those of the five backward products
S, dP, dQ, dK, dV, 2 B Hq R C (3 D + 2 Dv) (the forward re-run inside the command is not counted as work).
usage: python tools/attention_heads_bench.py [--backward] [--lib PATH] [--label NAME] [--repeats 11] [--window-ms 20] [--key2] [--json OUT]
       python tools/attention_heads_bench.py --report NEW1.json PARENT1.json [NEW2.json PARENT2.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

# B, R, C, Hq, Hk, D, causal
SHAPES = [(2, 4096, 4096, 8, 8, 40, False), (2, 4096, 77, 8, 8, 40, False), (2, 1024, 1024, 8, 8, 80, False), (2, 256, 256, 8, 8, 160, False),
          (1, 2048, 2048, 8, 1, 256, True), (1, 4096, 4096, 16, 16, 64, False)]
KEY2 = [(1, 4096, 4096, 16, 16, 64, False), (1, 4096, 4096, 16, 16, 128, False)]


def name_of(shape):
    return "(%d,%d,%d,%d,%d,%d)%s" % (shape[:6] + (" causal" if shape[6] else "",))


def measure(args):
    from ccv_amd import nnc
    L = nnc.load(args.lib)
    print("library", L.dll.nnc_mi355x_version().decode(), args.lib or "")
    s = L.stream_new(0)
    e0, e1 = L.dll.nnc_mi355x_event_new(), L.dll.nnc_mi355x_event_new()
    L.dll.nnc_mi355x_event_elapsed_ms.restype = nnc.C.c_float
    rng = np.random.default_rng(0)
    pool = (rng.random(1 << 22, dtype=np.float32) - 0.5).astype(np.float16)

    def dev(*shape):
        return L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_16F, shape, 0), np.resize(pool, shape))

    def command(shape):
        B, R, C, Hq, Hk, D, causal = shape
        cmd = nnc.generic_cmd("SCALED_DOT_PRODUCT_ATTENTION_BACKWARD" if args.backward else "SCALED_DOT_PRODUCT_ATTENTION_FORWARD")
        cmd.info.f1.v = float(1.0 / np.sqrt(D))       # scaled_dot_product_attention.scale
        cmd.info.blas.transpose_a[1] = int(causal)    # .is_causal
        if args.backward:
            return cmd, [dev(B, R, Hq, D), None, None, dev(B, R, Hq, D), dev(B, C, Hk, D), dev(B, C, Hk, D)], [dev(B, R, Hq, D), dev(B, C, Hk, D), dev(B, C, Hk, D)]
        return cmd, [dev(B, R, Hq, D), dev(B, C, Hk, D), dev(B, C, Hk, D)], [dev(B, R, Hq, D)]

    def window(cmd, ins, outs, reps):
        L.dll.nnc_mi355x_event_record(e0, s)
        for _ in range(reps):
            assert L.cmd_exec(cmd, nnc.NO_HINT, 0, ins, outs, s) == 0
        L.dll.nnc_mi355x_event_record(e1, s)
        L.stream_wait(s)
        return L.dll.nnc_mi355x_event_elapsed_ms(e0, e1) / reps

    rows = [(name_of(sh), sh, 1) for sh in SHAPES] + ([("SDPA_F16_ANYD = %d: " % k + name_of(sh), sh, k) for sh in KEY2 for k in (1, 2)] if args.key2 else [])
    work, launches = {}, {}
    for name, shape, key in rows:  # the warm-up of every shape: code objects, arena growth, the launch records of one command
        if args.key2:
            L.tune_set("SDPA_F16_ANYD", key)
        work[name] = command(shape)
        L.profile_enable(0); L.profile_enable(1)
        for _ in range(3):
            assert L.cmd_exec(*((work[name][0], nnc.NO_HINT, 0) + work[name][1:] + (s,))) == 0
        L.stream_wait(s)
        launches[name] = sorted(set(r[0].split("|")[-1].split("::")[-1] for r in L.profile_records()))
        L.profile_enable(0)
    out = []
    print("per row median ms (spread) | TFLOP/s | launches")
    for name, shape, key in rows:
        if args.key2:
            L.tune_set("SDPA_F16_ANYD", key)
        B, R, C, Hq, Hk, D, causal = shape
        cmd, ins, outs = work[name]
        one = window(cmd, ins, outs, 1)
        reps = max(1, min(2000, int(args.window_ms / max(one, 1e-3)) + 1))
        ms = sorted(window(cmd, ins, outs, reps) for _ in range(max(1, args.repeats)))
        med, spread = ms[len(ms) // 2], ms[-1] - ms[0]
        flop = 2.0 * B * Hq * R * C * (5 if args.backward else 2) * D * (0.5 if causal else 1.0)
        out.append(dict(row=name, ms=med, spread=spread, flop=flop, launches=launches[name]))
        print("%-44s %9.4f ms (%.4f) | %7.1f | %s" % (out[-1]["row"], med, spread, flop / med / 1e9, ",".join(launches[name])), flush=True)
    if args.key2:
        L.tune_set("SDPA_F16_ANYD", 1)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(label=args.label, backward=args.backward, rows=out), f)


def report(paths):
    runs = [json.load(open(p)) for p in paths]
    new, old = [r for r in runs if r["label"] != "parent"], [r for r in runs if r["label"] == "parent"]
    print("Median ms (spread = max - min of the windows).  `TFLOP/s`: 2 B Hq R C %s, halved for causal rows, per second of this tree's slower run.  `parent spread`:" % ("(3 D + 2 Dv)" if runs[0].get("backward") else "(D + Dv)"))
    print("the largest of the parent's window spreads and the distance between its runs.  `margin`: (the parent's faster run - this tree's slower run) / parent spread;")
    print("a row counts as faster where it is above 2.\n")
    head = ["(B,R,C,Hq,Hk,D)"] + ["%s, run %d" % (lab, i + 1) for i in range(max(len(new), len(old))) for lab in ("this tree", "parent")][:len(runs)] + ["TFLOP/s", "parent TFLOP/s", "parent spread", "margin", "parent / this tree"]
    print("| " + " | ".join(head) + " |")
    print("|" + "---|" * len(head))
    lost = []
    for k, r0 in enumerate(old[0]["rows"]):  # (the parent's rows: the rows both sides have)
        ns, os_ = [r["rows"][k] for r in new], [r["rows"][k] for r in old]
        assert all(x["row"] == r0["row"] for x in ns + os_)
        cells = ["%.4f (%.4f)" % (xs[i]["ms"], xs[i]["spread"]) for i in range(max(len(ns), len(os_))) for xs in (ns, os_) if i < len(xs)]
        slow_new, fast_old = max(x["ms"] for x in ns), min(x["ms"] for x in os_)
        spread = max([x["spread"] for x in os_] + [max(x["ms"] for x in os_) - fast_old])
        margin = (fast_old - slow_new) / max(spread, 1e-9)
        if margin <= 2:
            lost.append(r0["row"])
        print("| %s | %s | %.1f | %.1f | %.4f | %.1f | %.2fx |" % (r0["row"], " | ".join(cells), r0["flop"] / slow_new / 1e9, r0["flop"] / fast_old / 1e9, spread, margin, fast_old / slow_new))
    print("\nRows not faster than the parent by more than twice its spread: %s." % ("; ".join(lost) or "none"))
    print("\nKernels of one command, this tree / parent (conversions to and from fp32 images file no launch records):\n")
    for r0, p0 in zip(new[0]["rows"], old[0]["rows"]):
        print("- %s: %s / %s" % (r0["row"], ", ".join(r0["launches"]) or "-", ", ".join(p0["launches"]) or "-"))
    extra = [r for r in new[0]["rows"][len(old[0]["rows"]):]]
    if extra:
        print("\nFor information, this tree only: the tuning key SDPA_F16_ANYD at 1 (sdpa_forw_f16_kernel) and at 2 (sdpa_fwd_anyd_f16_kernel) on the same tensors, median ms (spread), TFLOP/s per run:\n")
        for k in range(len(old[0]["rows"]), len(new[0]["rows"])):
            print("- %s: %s" % (new[0]["rows"][k]["row"], "; ".join("%.4f (%.4f), %.1f" % (r["rows"][k]["ms"], r["rows"][k]["spread"], r["rows"][k]["flop"] / r["rows"][k]["ms"] / 1e9) for r in new)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backward", action="store_true", help="time SCALED_DOT_PRODUCT_ATTENTION_BACKWARD instead of the forward command")
    ap.add_argument("--lib", default=None, help="another build of libnnc_mi355x.so")
    ap.add_argument("--label", default="this tree", help="'parent' for the parent commit's build")
    ap.add_argument("--repeats", type=int, default=11, help="timed windows per row: the median and the spread are reported")
    ap.add_argument("--window-ms", type=float, default=20.0, help="least work timed per window")
    ap.add_argument("--key2", action="store_true", help="also time SDPA_F16_ANYD = 1 against 2 at D = 64 and D = 128 (a build that has the key)")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--report", nargs="+", default=None, help="JSON files of earlier runs: print the comparison as markdown")
    args = ap.parse_args()
    if args.report:
        report(args.report)
    else:
        measure(args)


if __name__ == "__main__":
    main()
