"""The convolution commands of tests/test_conv_routes.py and tools/conv_snapshot.py: one tiny case per route of ccv_amd/csrc/cmd_conv.cpp, each the
smallest size at which that route is still taken, and the function that runs one command of a case and reports the route it took."""
import contextlib
import ctypes as C
import numpy as np
from ccv_amd import nnc
from harness import exec_on, out_hw

F, H = np.float32, np.float16


class Case:
    """3 x 3, stride 1, padding 1, NHWC fp32 unless stated.  act / par: the element types of the activations (a, b, g, h) and of the parameters
    (w, bias, dw, dbias); tune: (tuning key, value) set around every command of the case and restored behind it."""

    def __init__(self, name, n, h, w, c, k, ksize=3, pad=1, stride=1, groups=1, fmt="NHWC", act=F, par=F, tune=None, back_algo=-1):
        self.name, self.fmt, self.act, self.par, self.tune, self.back_algo = name, fmt, act, par, tune, back_algo
        self.groups, self.k, self.ksize, self.cg = groups, k, ksize, c // groups
        self.hint = nnc.HINT((stride, stride), (pad, pad))
        oh, ow = out_hw(h, w, ksize, ksize, self.hint)
        rng = np.random.default_rng(sum(map(ord, name)))
        rnd = lambda dt, *shape, scale=1.0: ((rng.random(shape, dtype=F) - 0.5) * 2 * scale).astype(dt)
        # a: a rectified map -- exact zeros, and negative zeros where a tenth of its elements are overwritten: the backward commands' mask
        a = np.maximum(rnd(act, n, h, w, c), 0)
        a[rng.random(a.shape) < 0.1] = -0.0
        assert (a > 0).any() and (a == 0).any() and np.signbit(a[a == 0]).any() and not np.signbit(a[a == 0]).all()
        wt = rnd(par, k, ksize, ksize, self.cg, scale=1.0 / (ksize * ksize * self.cg) ** 0.5)
        bias = rnd(par, k, scale=0.5)
        wt[0], bias[0] = 0, 0  # a filter of zeros without bias: output channel 0 is exact zeros on every route
        self.a, self.w, self.bias, self.g = self.lay(a), self.lay(wt), bias, self.lay(rnd(act, n, oh, ow, k))

    def lay(self, x):
        return x if self.fmt == "NHWC" else np.ascontiguousarray(x.transpose(0, 3, 1, 2))

    def __repr__(self):
        return self.name


FORWARD_CASES = [
    Case("c8_k8_5x5", 2, 5, 5, 8, 8),                       # under the fused kernel's 16-channel floor: algorithm 2 lands on via-HBM Winograd
    Case("c16_k40_6x40", 2, 6, 40, 16, 40),                 # fused kernel, ragged last 32-channel block, clipped 2 x 8 group
    Case("c3_k16_9x9", 2, 9, 9, 3, 16),                     # 3-channel kernel; implicit GEMM under algorithm 0
    Case("c16_k32_7x7_1x1", 2, 7, 7, 16, 32, ksize=1, pad=0),  # pointwise GEMM
    Case("c6_k10_8x8", 2, 8, 8, 6, 10),                     # scalar implicit GEMM (C not a multiple of 4)
    Case("dw16_8x8", 2, 8, 8, 16, 16, groups=16),           # depthwise
    Case("dw16_8x8_nchw", 2, 8, 8, 16, 16, groups=16, fmt="NCHW"),
    Case("dw16_8x8_half_a", 2, 8, 8, 16, 16, groups=16, act=H),  # a half input and an fp32 filter: staged, so NOT depthwise
    Case("nchw_c8_k8_4x4_1x1", 2, 4, 4, 8, 8, ksize=1, pad=0, fmt="NCHW"),  # conv1x1_nchw_forw
    Case("nchw_c8_k8_6x6", 2, 6, 6, 8, 8, fmt="NCHW"),      # the layout-staging route
    Case("half_c8_k8_6x6", 2, 6, 6, 8, 8, act=H, par=H),    # native half core
    Case("half_nchw_c8_k8_6x6_f16", 2, 6, 6, 8, 8, fmt="NCHW", act=H, par=H, tune=("CONV_NCHW_HALF_F16", 4)),    # least channels below C = 8: f16 branch
    Case("half_nchw_c8_k8_6x6_f32", 2, 6, 6, 8, 8, fmt="NCHW", act=H, par=H, tune=("CONV_NCHW_HALF_F16", 64)),   # ... above: fp32 branch
]
BACKWARD_ONLY_CASES = [
    Case("c8_k8_5x5_n3_algo1", 3, 5, 5, 8, 8, back_algo=1),      # via-HBM Winograd both ways: one pass over the output gradient for both of its transforms
    Case("c40_k40_6x40_algo2", 2, 6, 40, 40, 40, back_algo=2),  # FUSE_RELU | 2: the filter gradient's input pass writes the fused data gradient's mask bits
    Case("c8_k8_8x8_s2", 2, 8, 8, 8, 8, stride=2),          # parity-class data gradient
]
CASES = FORWARD_CASES + BACKWARD_ONLY_CASES
FORWARD_ALGOS = (-1, 0, 1, 2)
BACKWARD_KINDS = ("dx", "dw", "all")  # the data gradient alone, the filter gradient alone, both with the bias gradient


def _shared(lib):
    f = lib.dll.nnc_mi355x_debug_conv_back_shared
    f.restype, f.argtypes = C.c_long, [C.c_int]
    return int(f(0)), int(f(1))


def _half_counts(lib):
    a, b = C.c_long(0), C.c_long(0)
    lib.dll.nnc_mi355x_debug_half_counts(C.byref(a), C.byref(b))
    return a.value, b.value


@contextlib.contextmanager
def _tuned(lib, tune):
    if tune is None:
        yield
        return
    old = lib.tune_get(tune[0])
    lib.tune_set(*tune)
    try:
        yield
    finally:
        lib.tune_set(tune[0], old)


def run(lib, case, kind, algo, fuse_relu):
    """One command: kind "fwd", or a backward command asking for "dx", "dw" or "all" three gradients.  Returns the route -- (last kernel name, launches
    of the two shared backward kernels, tensors staged as fp32 images / handed on as halves during the command) -- and the list of output arrays."""
    algorithm = (nnc.CONV_ALGO_FUSE_RELU | (0xff if algo < 0 else algo)) if fuse_relu else algo
    if kind == "fwd":
        cmd = nnc.CMD_CONVOLUTION_FORWARD(case.groups, case.k, case.ksize, case.ksize, case.cg)
        ins, outs = [case.a, case.w, case.bias], [np.full(case.g.shape, 7, case.act)]
    else:
        cmd = nnc.CMD_CONVOLUTION_BACKWARD(case.groups, case.k, case.ksize, case.ksize, case.cg)
        ins = [case.g, case.a, case.w]
        outs = {"dx": [np.full_like(case.a, 3)], "dw": [None, np.zeros_like(case.w)], "all": [np.full_like(case.a, 3), np.zeros_like(case.w), np.zeros_like(case.bias)]}[kind]
    cmd.algorithm = algorithm
    with _tuned(lib, case.tune):
        shared0, half0 = _shared(lib), _half_counts(lib)
        r, got = exec_on(lib, nnc.GPU_MEMORY, cmd, case.hint, 0, ins, outs, case.fmt)
        shared1, half1 = _shared(lib), _half_counts(lib)
    assert r == 0, (case, kind, algo, fuse_relu, r)
    route = (lib.dll.nnc_mi355x_last_kernel_name().decode(), (shared1[0] - shared0[0], shared1[1] - shared0[1]), (half1[0] - half0[0], half1[1] - half0[1]))
    return route, [x for x in got if x is not None]


def commands(case):
    """(key, kind, algorithm) of every command pair -- plain and FUSE_RELU -- the case is run with"""
    out = [("fwd/%d" % algo, "fwd", algo) for algo in FORWARD_ALGOS] if case in FORWARD_CASES else []
    return out + [(kind, kind, case.back_algo) for kind in BACKWARD_KINDS]
