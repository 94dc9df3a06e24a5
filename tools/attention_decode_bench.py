#!/usr/bin/env python
"""Time SCALED_DOT_PRODUCT_ATTENTION_FORWARD on CCV_16F tensors at the shapes of a language model's decode step -- one query row (four for speculative decoding)
against a key / value cache of C keys -- each as ONE command through the command interface, HIP-event timed on a stream after a warm-up of every shape.  Per row:
the median of `--repeats` windows of at least `--window-ms`, their spread (max - min), and the compulsory bytes (K and V once per key head, q and o) per second.
Uses nothing but the command interface and tune_set, so it runs on a build without sdpa_decode_f16_kernel (--lib, where the keys do not exist and are left alone):
both sides of a comparison come from this script, run alternately, and --report lays the runs side by side.
--tiles N sets SDPA_DECODE_TILES (sdpa_decode_tiles_f16_kernel for up to 32 N packed rows per key head) and times the rows with 40 .. 256 packed rows in place of
the decode rows: the comparison is then the SAME library with --tiles 1 --label parent (the former routes) against --tiles 8.  --min-blocks N forces on each of those
rows the split count the launch's rule gives with N blocks as the shortest split (the rule restated here), to measure the rule's constant.
usage: python tools/attention_decode_bench.py [--lib PATH] [--label NAME] [--decode 1] [--splits 0] [--tiles N [--min-blocks N]] [--repeats 11] [--window-ms 200] [--json OUT]
       python tools/attention_decode_bench.py --report NEW1.json PARENT1.json [NEW2.json PARENT2.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

COPY_RATE = 6.29e12  # bytes per second of a device copy, DESIGN.md section 5
# B, R, C, Hq, Hk, D
SHAPES = [(b, 1, c, 32, 8, 128) for b in (1, 8) for c in (128, 256, 512, 2048, 8192, 32768)]
SHAPES += [(1, 1, 2048, 16, 16, 64), (1, 1, 8192, 8, 1, 256), (1, 4, 8192, 32, 8, 128), (1, 128, 8192, 32, 8, 128)]  # multi-head, multi-query, speculative, the control
# --tiles: 40, 64, 128 and 256 packed rows per key head (verification of a speculated run, a chunked prefill's tail), multi-query with two rows, a batch of eight
TILE_SHAPES = [(1, r, c, 32, 8, 128) for r in (10, 16, 32, 64) for c in (512, 2048, 8192, 32768)] + [(1, 2, 8192, 32, 1, 128), (8, 8, 2048, 32, 8, 128)]


def rule_splits(shape, min_blocks, cus=256):
    """The split count sdpa_decode_tiles_f16_run chooses, with `min_blocks` in place of its shortest split."""
    B, R, C, Hq, Hk, D = shape
    M = R * (Hq // Hk)
    wgs = B * Hk * -(-M // (64 if M <= 64 else 128))
    return max(1, min(1 if wgs >= cus else -(-cus // wgs), ((C + 31) // 32) // min_blocks))


def measure(args):
    from ccv_amd import nnc
    L = nnc.load(args.lib)
    print("library", L.dll.nnc_mi355x_version().decode(), args.lib or "")
    if args.label != "parent" or args.tiles:
        L.tune_set("SDPA_F16_DECODE", args.decode)
        L.tune_set("SDPA_DECODE_SPLITS", args.splits)
    if args.tiles:
        L.tune_set("SDPA_DECODE_TILES", args.tiles)
    s = L.stream_new(0)
    e0, e1 = L.dll.nnc_mi355x_event_new(), L.dll.nnc_mi355x_event_new()
    L.dll.nnc_mi355x_event_elapsed_ms.restype = nnc.C.c_float
    pool = (np.random.default_rng(0).random(1 << 22, dtype=np.float32) - 0.5).astype(np.float16)

    def dev(*shape):
        return L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_16F, shape, 0), np.resize(pool, shape))

    def window(cmd, ins, outs, reps):
        L.dll.nnc_mi355x_event_record(e0, s)
        for _ in range(reps):
            assert L.cmd_exec(cmd, nnc.NO_HINT, 0, ins, outs, s) == 0
        L.dll.nnc_mi355x_event_record(e1, s)
        L.stream_wait(s)
        return L.dll.nnc_mi355x_event_elapsed_ms(e0, e1) / reps

    out = []
    print("(B,R,C,Hq,Hk,D) median ms (spread) | compulsory TB/s | launches")
    for shape in (TILE_SHAPES if args.tiles else SHAPES):
        B, R, C, Hq, Hk, D = shape
        if args.tiles and args.min_blocks:
            L.tune_set("SDPA_DECODE_SPLITS", rule_splits(shape, args.min_blocks))
        cmd = nnc.generic_cmd("SCALED_DOT_PRODUCT_ATTENTION_FORWARD")
        cmd.info.f1.v = float(1.0 / np.sqrt(D))  # scaled_dot_product_attention.scale
        ins, outs = [dev(B, R, Hq, D), dev(B, C, Hk, D), dev(B, C, Hk, D)], [dev(B, R, Hq, D)]
        L.profile_enable(0); L.profile_enable(1)
        for _ in range(3):  # the warm-up: code objects, arena growth, the launch records of one command
            assert L.cmd_exec(cmd, nnc.NO_HINT, 0, ins, outs, s) == 0
        L.stream_wait(s)
        launches = sorted(set(r[0].split("|")[-1].split("::")[-1] for r in L.profile_records()))
        L.profile_enable(0)
        one = window(cmd, ins, outs, 1)
        reps = max(1, min(20000, int(args.window_ms / max(one, 1e-3)) + 1))
        ms = sorted(window(cmd, ins, outs, reps) for _ in range(max(1, args.repeats)))
        med, spread = ms[len(ms) // 2], ms[-1] - ms[0]
        nbytes = 2.0 * B * (2 * C * Hk * D + 2 * R * Hq * D)
        out.append(dict(row="(%d,%d,%d,%d,%d,%d)" % shape, ms=med, spread=spread, bytes=nbytes, launches=launches))
        print("%-28s %9.4f ms (%.4f) | %6.3f | %s" % (out[-1]["row"], med, spread, nbytes / med / 1e9, ",".join(launches)), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(label=args.label, decode=args.decode, splits=args.splits, tiles=args.tiles, min_blocks=args.min_blocks, rows=out), f)


def report(paths):
    runs = [json.load(open(p)) for p in paths]
    new, old = [r for r in runs if r["label"] != "parent"], [r for r in runs if r["label"] == "parent"]
    print("Median ms (spread = max - min of the windows).  `parent spread`: the largest of the parent's window spreads and the distance between its runs.  `margin`:")
    print("(the parent's faster run - this tree's slower run) / parent spread; a row counts as faster where it is above 2.  `of copy rate`: compulsory bytes per second")
    print("of this tree's slower run over %.1f TB/s.\n" % (COPY_RATE / 1e12))
    n = max(len(new), len(old))
    head = ["(B,R,C,Hq,Hk,D)"] + ["%s, run %d" % (lab, i + 1) for i in range(n) for lab in ("this tree", "parent")] + ["parent spread", "margin", "parent / this tree", "of copy rate", "launches"]
    print("| " + " | ".join(head) + " |")
    print("|" + "---|" * len(head))
    for k, r0 in enumerate(old[0]["rows"]):
        ns, os_ = [r["rows"][k] for r in new], [r["rows"][k] for r in old]
        assert all(x["row"] == r0["row"] for x in ns + os_)
        cells = ["%.4f (%.4f)" % (xs[i]["ms"], xs[i]["spread"]) for i in range(n) for xs in (ns, os_)]
        slow_new, fast_old = max(x["ms"] for x in ns), min(x["ms"] for x in os_)
        spread = max([x["spread"] for x in os_] + [max(x["ms"] for x in os_) - fast_old])
        print("| %s | %s | %.4f | %.1f | %.2fx | %.1f %% | %s |" % (r0["row"], " | ".join(cells), spread, (fast_old - slow_new) / max(spread, 1e-9), fast_old / slow_new, 100 * r0["bytes"] / (slow_new * 1e-3) / COPY_RATE, ", ".join(ns[0]["launches"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libnnc_mi355x.so")
    ap.add_argument("--label", default="this tree", help="'parent' for the parent commit's build (the tuning keys are then left alone)")
    ap.add_argument("--decode", type=int, default=1, help="the SDPA_F16_DECODE tuning key")
    ap.add_argument("--splits", type=int, default=0, help="the SDPA_DECODE_SPLITS tuning key")
    ap.add_argument("--tiles", type=int, default=0, help="the SDPA_DECODE_TILES tuning key; the rows are then those with 40 .. 256 packed rows per key head")
    ap.add_argument("--min-blocks", type=int, default=0, help="with --tiles: force the splits of the launch's rule with this shortest split, in 32-key blocks")
    ap.add_argument("--repeats", type=int, default=11, help="timed windows per row: the median and the spread are reported")
    ap.add_argument("--window-ms", type=float, default=200.0, help="least work timed per window")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--report", nargs="+", default=None, help="JSON files of earlier runs: print the comparison as markdown")
    args = ap.parse_args()
    if args.report:
        report(args.report)
    else:
        measure(args)


if __name__ == "__main__":
    main()
