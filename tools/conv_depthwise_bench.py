#!/usr/bin/env python
"""Time the depthwise convolutions of EfficientNet-B0 (the reference's ImageNet trainer: groups = filters, 3 x 3 or 5 x 5, stride 1 or 2, padding (k - 1) / 2)
at batch 128 -- forward, data gradient, filter + bias gradient, each as ONE command through the command interface, HIP-event timed on a stream -- in the trainer's
layout (NCHW) and in NHWC, fp32 and half.  Per row and leg: the time, the bytes the command must move (every tensor once) and that traffic as a fraction of
6.29 TB/s, the measured copy rate of the MI355X.  Uses nothing but the command interface, so it runs unchanged on a build without the depthwise kernels
(the tuning key is then unknown and skipped): both sides of a comparison come from this script.
usage: python tools/conv_depthwise_bench.py [--batch 128] [--layouts NCHW,NHWC] [--types f32,f16] [--depthwise 0|1] [--lib PATH] [--window-ms 40]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccv_amd import nnc

# (channels, H = W, kernel, stride)
LAYERS = [(32, 112, 3, 1), (96, 112, 3, 2), (144, 56, 3, 1), (144, 56, 5, 2), (240, 28, 5, 1), (240, 28, 3, 2),
          (480, 14, 3, 1), (480, 14, 5, 1), (672, 14, 5, 1), (672, 14, 5, 2), (1152, 7, 5, 1), (1152, 7, 3, 1)]
HBM_COPY_TBS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--layouts", default="NCHW,NHWC")
    ap.add_argument("--types", default="f32,f16")
    ap.add_argument("--depthwise", type=int, default=None, help="set the CONV_DEPTHWISE tuning key (0: the grouped-GEMM route)")
    ap.add_argument("--lib", default=None, help="another build of libnnc_mi355x.so")
    ap.add_argument("--window-ms", type=float, default=40.0, help="least work timed per leg")
    args = ap.parse_args()
    L = nnc.load(args.lib)
    print("library", L.dll.nnc_mi355x_version().decode())
    if args.depthwise is not None:
        try:
            L.tune_set("CONV_DEPTHWISE", args.depthwise)
            print("CONV_DEPTHWISE =", args.depthwise)
        except KeyError:
            print("this build has no CONV_DEPTHWISE key: skipped")
    s = L.stream_new(0)
    e0, e1 = L.dll.nnc_mi355x_event_new(), L.dll.nnc_mi355x_event_new()
    L.dll.nnc_mi355x_event_elapsed_ms.restype = nnc.C.c_float

    def window(cmd, hint, ins, outs, reps):
        L.dll.nnc_mi355x_event_record(e0, s)
        for _ in range(reps):
            assert L.cmd_exec(cmd, hint, 0, ins, outs, s) == 0
        L.dll.nnc_mi355x_event_record(e1, s)
        L.stream_wait(s)
        return L.dll.nnc_mi355x_event_elapsed_ms(e0, e1) / reps

    def timed(cmd, hint, ins, outs):
        """(ms per call, launch names of one call): a first call (code objects, workspace growth) under the launch records, one timed call to size the window, the window"""
        L.profile_enable(0); L.profile_enable(1)
        assert L.cmd_exec(cmd, hint, 0, ins, outs, s) == 0
        L.stream_wait(s)
        names = sorted(set(r[0].split("|")[0] for r in L.profile_records()))
        L.profile_enable(0)
        one = window(cmd, hint, ins, outs, 1)
        reps = max(3, min(200, int(args.window_ms / max(one, 1e-3)) + 1))
        return window(cmd, hint, ins, outs, reps), names

    n = args.batch
    for layout in args.layouts.split(","):
        for ty in args.types.split(","):
            F, es = (nnc.CCV_16F, 2) if ty == "f16" else (nnc.CCV_32F, 4)
            nchw = layout == "NCHW"
            act = (lambda c, hw: L.tensor(nnc.GPU_TENSOR_NCHW(0, F, n, c, hw, hw))) if nchw else (lambda c, hw: L.tensor(nnc.GPU_TENSOR_NHWC(0, F, n, hw, hw, c)))
            flt = (lambda c, k: L.tensor(nnc.GPU_TENSOR_NCHW(0, F, c, 1, k, k))) if nchw else (lambda c, k: L.tensor(nnc.GPU_TENSOR_NHWC(0, F, c, k, k, 1)))
            vec = lambda c: L.tensor(nnc.GPU_TENSOR_NHWC(0, F, c))
            print("\n%s %s batch %d: per leg ms | MB moved (every tensor once) | fraction of %.2f TB/s | launches" % (layout, ty, n, HBM_COPY_TBS))
            for c, hw, k, stride in LAYERS:
                pad = (k - 1) // 2
                ohw = (hw + 2 * pad - k) // stride + 1
                a, w, bias, b = act(c, hw), flt(c, k), vec(c), act(c, ohw)
                g, h, dw, db = act(c, ohw), act(c, hw), flt(c, k), vec(c)
                L.cmd_exec(nnc.CMD_SET_FORWARD(0.01), nnc.HINT(), 0, [], [a, w, bias, g], s)
                hint = nnc.HINT((stride, stride), (pad, pad))
                fwd, bwd = nnc.CMD_CONVOLUTION_FORWARD(c, c, k, k, 1), nnc.CMD_CONVOLUTION_BACKWARD(c, c, k, k, 1)
                big, small, filt = n * c * hw * hw * es, n * c * ohw * ohw * es, c * k * k * es
                legs = [("fwd", fwd, [a, w, bias], [b], big + small + filt + c * es),
                        ("dgrad", bwd, [g, None, w], [h], small + big + filt),
                        ("wgrad", bwd, [g, a, None], [None, dw, db], small + big + filt + c * es)]
                for what, cmd, ins, outs, nbytes in legs:
                    ms, names = timed(cmd, hint, ins, outs)
                    print("%-22s %-5s %9.4f ms | %8.2f MB | %5.3f | %s" % ("C%d %d^2 k%d s%d" % (c, hw, k, stride), what, ms, nbytes / 1e6, nbytes / (ms * 1e-3) / (HBM_COPY_TBS * 1e12), ",".join(names)), flush=True)
                for t in (a, w, bias, b, g, h, dw, db):
                    t.free()


if __name__ == "__main__":
    main()
