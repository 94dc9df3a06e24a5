#!/usr/bin/env python
"""Time the element-wise legs of EfficientNet-B0's MBConv blocks (the reference's ImageNet trainer) at batch 128 on the block's maps: swish forward and
backward, MUL of the map by the squeeze-excite vector forward and backward (both gradients), dropout (`entirety`) forward and backward -- each as ONE
command through the command interface, HIP-event timed on a stream -- in NCHW and NHWC, in half, the MUL legs in fp32 as well.  Per row and leg: the
median of `--repeats` windows, their spread (max - min), the bytes the command must move (every tensor once) and that traffic as a fraction of 6.29 TB/s,
the measured copy rate of the MI355X.  Uses nothing but the command interface, so it runs unchanged on another build (--lib): both sides of a comparison
come from this script.  The dropout legs run with p = 0 by default: every call then takes the branch that moves data, and the windows do not mix the two.
usage: python tools/mbconv_half_bench.py [--batch 128] [--layouts NCHW,NHWC] [--lib PATH] [--repeats 5] [--window-ms 20] [--json OUT] [--act-half-native 0|1] [--mul-planes 0|1]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccv_amd import nnc

# (channels, H = W): the maps the blocks' activations, squeeze-excite scales and drop-connect run on
MAPS = [(32, 112), (96, 112), (96, 56), (144, 56), (144, 28), (240, 28), (240, 14), (480, 14), (672, 14), (672, 7), (1152, 7), (1280, 7)]
HBM_COPY_TBS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--layouts", default="NCHW,NHWC")
    ap.add_argument("--lib", default=None, help="another build of libnnc_mi355x.so")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per leg: the median and the spread are reported")
    ap.add_argument("--window-ms", type=float, default=20.0, help="least work timed per window")
    ap.add_argument("--dropout-p", type=float, default=0.0)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    ap.add_argument("--act-half-native", type=int, default=None, help="set the ACT_HALF_NATIVE tuning key")
    ap.add_argument("--mul-planes", type=int, default=None, help="set the MUL_PLANES tuning key")
    args = ap.parse_args()
    L = nnc.load(args.lib)
    print("library", L.dll.nnc_mi355x_version().decode(), args.lib or "")
    for key, value in (("ACT_HALF_NATIVE", args.act_half_native), ("MUL_PLANES", args.mul_planes)):
        if value is not None:
            try:
                L.tune_set(key, value)
                print(key, "=", value)
            except KeyError:
                print("this build has no %s key: skipped" % key)
    s = L.stream_new(0)
    e0, e1 = L.dll.nnc_mi355x_event_new(), L.dll.nnc_mi355x_event_new()
    L.dll.nnc_mi355x_event_elapsed_ms.restype = nnc.C.c_float

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
        names = sorted(set(r[0].split("|")[0] for r in L.profile_records()))
        L.profile_enable(0)
        one = window(cmd, ins, outs, 1)
        reps = max(3, min(200, int(args.window_ms / max(one, 1e-3)) + 1))
        ms = sorted(window(cmd, ins, outs, reps) for _ in range(max(1, args.repeats)))
        return ms[len(ms) // 2], ms[-1] - ms[0], names

    drop_f = nnc.CMD_DROPOUT_FORWARD(args.dropout_p, 1)
    drop_b = nnc.CMD_DROPOUT_FORWARD(args.dropout_p, 1)
    drop_b.cmd = nnc.CMD["DROPOUT_BACKWARD"]
    n, rows = args.batch, []
    for layout in args.layouts.split(","):
        nchw = layout == "NCHW"
        for ty in ("f16", "f32"):
            F, es = (nnc.CCV_16F, 2) if ty == "f16" else (nnc.CCV_32F, 4)
            act = (lambda c, hw: L.tensor(nnc.GPU_TENSOR_NCHW(0, F, n, c, hw, hw))) if nchw else (lambda c, hw: L.tensor(nnc.GPU_TENSOR_NHWC(0, F, n, hw, hw, c)))
            vec = (lambda c: L.tensor(nnc.GPU_TENSOR_NCHW(0, F, n, c, 1, 1))) if nchw else (lambda c: L.tensor(nnc.GPU_TENSOR_NHWC(0, F, n, 1, 1, c)))
            print("\n%s %s batch %d: per leg median ms (spread) | MB moved (every tensor once) | fraction of %.2f TB/s | launches" % (layout, ty, n, HBM_COPY_TBS))
            for c, hw in MAPS:
                a, g, b, h, sv, ds = act(c, hw), act(c, hw), act(c, hw), act(c, hw), vec(c), vec(c)
                mask = L.tensor(nnc.GPU_TENSOR_NHWC(0, F, 64))
                L.cmd_exec(nnc.CMD_SET_FORWARD(0.5), nnc.NO_HINT, 0, [], [a, g, sv], s)
                big, small = n * c * hw * hw * es, n * c * es
                legs = [("mul_fwd", nnc.CMD_MUL_FORWARD(1.0), [a, sv], [b], 2 * big + small),
                        ("mul_bwd", nnc.CMD_MUL_BACKWARD(1.0), [g, a, sv], [h, ds], 3 * big + 2 * small)]
                if ty == "f16":
                    legs = [("swish_fwd", nnc.generic_cmd("SWISH_FORWARD"), [a], [b], 2 * big),
                            ("swish_bwd", nnc.generic_cmd("SWISH_BACKWARD"), [g, a], [h], 3 * big)] + legs + [
                            ("drop_fwd", drop_f, [a], [b, mask], 2 * big),
                            ("drop_bwd", drop_b, [g, None, None, None, mask], [h], 2 * big)]
                for what, cmd, ins, outs, nbytes in legs:
                    ms, spread, names = timed(cmd, ins, outs)
                    frac = nbytes / (ms * 1e-3) / (HBM_COPY_TBS * 1e12)
                    rows.append(dict(layout=layout, type=ty, map="%d@%d^2" % (c, hw), leg=what, ms=ms, spread=spread, mb=nbytes / 1e6, hbm=frac, launches=names))
                    print("%-12s %-9s %9.4f ms (%.4f) | %8.2f MB | %5.3f | %s" % ("%d@%d^2" % (c, hw), what, ms, spread, nbytes / 1e6, frac, ",".join(names)), flush=True)
                for t in (a, g, b, h, sv, ds, mask):
                    t.free()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f)


if __name__ == "__main__":
    main()
