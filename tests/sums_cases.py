"""The commands of tools/sums_snapshot.py: every command that ends in a column or channel sum of ccv_amd/csrc/chan_sums.cpp -- bias gradients of GEMM,
convolution and LSTM, layer-norm / RMS-norm parameter gradients, batch-norm statistics -- each at the smallest shape that reaches one branch of those sums
(16-byte or scalar rows kernel, one slice or several with a short last one, 16-byte or scalar plane lanes, one- or two-level fold of given partials).
CASES is a list of (name, function(lib) -> list of output arrays, gpu_only)."""
import contextlib
import os
import sys
import numpy as np
from ccv_amd import nnc
from harness import exec_on
import conv_route_cases as crc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import lstm_numpy  # noqa: E402

F, H = np.float32, np.float16


def _rnd(name, dt, *shape, scale=1.0):
    rng = np.random.default_rng(sum(map(ord, name)) + len(shape) * 1000 + int(np.prod(shape)))
    return ((rng.random(shape, dtype=F) - F(0.5)) * F(2 * scale)).astype(dt)


@contextlib.contextmanager
def _tuned(lib, key, value):
    old = lib.tune_get(key)
    if value is not None:
        lib.tune_set(key, value)
    try:
        yield
    finally:
        lib.tune_set(key, old)


def _run(lib, cmd, flags, ins, outs, fmt="NHWC", hint=None):
    r, got = exec_on(lib, nnc.GPU_MEMORY, cmd, hint or nnc.NO_HINT, flags, ins, outs, fmt)
    assert r == 0, r
    return [x for x in got if x is not None]


def gemm_back(name, dt, m, n, k=12, batch=0, flags=0):
    def run(lib):
        pre = (batch,) if batch else ()
        g, a, w = _rnd(name + "g", dt, *(pre + (m, n))), _rnd(name + "a", dt, *(pre + (m, k))), _rnd(name + "w", dt, k, n, scale=1.0 / k)
        outs = [np.zeros_like(a), _rnd(name + "dw", dt, k, n), _rnd(name + "db", dt, n)]  # (read only under ACCUMULATE_OUTPUT)
        return _run(lib, nnc.CMD_GEMM_BACKWARD(), flags, [g, a, w], outs)
    return name, run, False


def rownorm_back(name, rows, n):
    def run(lib):
        a, g = _rnd(name + "a", F, rows, n, scale=2.0), _rnd(name + "g", F, rows, n)
        scale = _rnd(name + "s", F, 1, n) + F(1.5)
        mean = a.mean(axis=1, keepdims=True).astype(F)
        istd = (1.0 / np.sqrt(a.var(axis=1, keepdims=True) + 1e-5)).astype(F)
        irms = (1.0 / np.sqrt((a * a).mean(axis=1, keepdims=True) + 1e-5)).astype(F)
        z = lambda: np.zeros((1, n), F)
        out = _run(lib, nnc.CMD_NORM("LAYER_NORM_BACKWARD", 1e-5, 1, 1), 0, [g, None, None, a, scale, None, None, mean, istd], [np.zeros_like(a), z(), z()])
        return out + _run(lib, nnc.CMD_NORM("RMSNORM_BACKWARD", 1e-5, 0, 1), 0, [g, None, a, scale, None, irms], [np.zeros_like(a), z()])
    return name, run, False


def bnorm(name, dt, shape, fmt, cluster=0):
    """forward in training mode, then backward from the statistics it saved; cluster: TUNE_BN_CLUSTER around both (None: the default)"""
    def run(lib):
        caxis = 3 if fmt == "NHWC" else 1
        sshape = tuple(shape[caxis] if i == caxis else 1 for i in range(4))
        axes = tuple(i for i in range(4) if i != caxis)
        x, g = _rnd(name + "x", dt, *shape, scale=2.0), _rnd(name + "g", dt, *shape)
        scale, bias = _rnd(name + "s", F, *sshape) + F(1.5), _rnd(name + "b", F, *sshape)
        mean, var = _rnd(name + "m", F, *sshape), _rnd(name + "v", F, *sshape) + F(1.5)
        with _tuned(lib, "BN_CLUSTER", cluster):
            ts = [lib.tensor(nnc.tensor_param(nnc.GPU_MEMORY, crc_fmt(fmt), nnc._NP_DT[np.dtype(a.dtype)], a.shape), a) for a in
                  (x, scale, bias, mean, var, np.zeros_like(x), np.zeros(sshape, F), np.zeros(sshape, F), g, np.zeros_like(x), np.zeros(sshape, F), np.zeros(sshape, F))]
            tx, tsc, tb, tm, tv, ty, tsm, tsi, tg, th, tds, tdb = ts
            assert lib.cmd_exec(nnc.CMD_BATCH_NORM_FORWARD(1e-4, 0, 0.9, *axes), nnc.NO_HINT, 0, [tx, tsc, tb, tm, tv], [ty, tm, tv, tsm, tsi]) == 0
            assert lib.cmd_exec(nnc.CMD_BATCH_NORM_BACKWARD(1e-4, 0, 0.9, *axes), nnc.NO_HINT, 0, [tg] + [None] * 4 + [tx, tsc] + [None] * 6 + [tsm, tsi], [th, tds, tdb]) == 0
        return [t.numpy() for t in (ty, tm, tv, tsm, tsi, th, tds, tdb)]
    return name, run, False


def crc_fmt(fmt):
    return {"NHWC": nnc.NHWC, "NCHW": nnc.NCHW}[fmt]


def conv_back(name, n, h, w, c, k, gpu_only=False, **kw):
    """the backward command with all three gradients (tests/conv_route_cases.py builds the tensors and runs it)"""
    def run(lib):
        case = crc.Case(name, n, h, w, c, k, **kw)
        return crc.run(lib, case, "all", case.back_algo, False)[1]
    return name, run, gpu_only


def lstm_back(name, T, B, I, Hd):
    def run(lib):
        nw = lstm_numpy.weight_count(I, Hd, Hd, 1, 1, 1)
        x, w = _rnd(name + "x", F, T, B, I), _rnd(name + "w", F, nw // Hd, Hd, scale=0.3)
        fcmd, bcmd = nnc.CMD_LSTM_FORWARD(Hd, 0, 1, 1, 0, 0, 0.0, 0), nnc.CMD_LSTM_BACKWARD(Hd, 0, 1, 1, 0, 0, 0.0, 0)
        rrows = (lib.dll.nnc_mi355x_lstm_reserve_space_size(fcmd, nnc.CCV_32F, I, B, T) // 4 + Hd - 1) // Hd
        gpu = lambda a: lib.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_32F, a.shape), np.ascontiguousarray(a))
        x_t, w_t, y_t, r_t = gpu(x), gpu(w), gpu(np.zeros((T, B, Hd), F)), gpu(np.zeros((rrows, Hd), F))
        assert lib.cmd_exec(fcmd, nnc.NO_HINT, 0, [x_t, None, None, None, w_t], [y_t, None, None, r_t]) == 0
        dx_t, dw_t = gpu(np.zeros_like(x)), gpu(np.zeros_like(w))
        ins = [gpu(_rnd(name + "gy", F, T, B, Hd)), None, None, None, x_t, None, None, None, w_t, y_t, None, None, r_t]
        assert lib.cmd_exec(bcmd, nnc.NO_HINT, 0, ins, [dx_t, None, None, None, dw_t]) == 0
        return [y_t.numpy(), dx_t.numpy(), dw_t.numpy()]
    return name, run, False


CASES = [
    # GEMM backward with a bias gradient: colsum_f32 / colsum_f16 over g
    gemm_back("gemm_f32_130x68", F, 130, 68),    # three slices, the last one short; two column tiles, the second part-filled; 16-byte kernel
    gemm_back("gemm_f32_130x67", F, 130, 67),    # scalar kernel
    gemm_back("gemm_f32_40x8", F, 40, 8),        # one slice
    gemm_back("gemm_f16_130x68", H, 130, 68),
    gemm_back("gemm_f16_130x67", H, 130, 67),
    gemm_back("gemm_f16_40x8", H, 40, 8),
    gemm_back("gemm_f32_batch3_70x20", F, 70, 20, batch=3),  # the batch entries behind the first accumulate
    gemm_back("gemm_f32_130x68_acc", F, 130, 68, flags=nnc.ACCUMULATE_OUTPUT),
    gemm_back("gemm_f16_batch3_70x20_acc", H, 70, 20, batch=3, flags=nnc.ACCUMULATE_OUTPUT),
    # layer norm / RMS norm backward: dbias = colsum_f32 over g, dscale = colsum_f32 over the chunk partials behind its head
    rownorm_back("rownorm_200x96", 200, 96),     # four chunks
    rownorm_back("rownorm_5x10", 5, 10),
    # batch norm forward (training) + backward on the plane / rows routes (BN_CLUSTER = 0)
    bnorm("bn_f32_nhwc_3x5x5x70", F, (3, 5, 5, 70), "NHWC"),  # rows kernel with RSum, RCenteredSq, RXhatG
    bnorm("bn_f16_nhwc_3x5x5x70", H, (3, 5, 5, 70), "NHWC"),
    bnorm("bn_f32_nchw_3x6x8x8", F, (3, 6, 8, 8), "NCHW"),    # planes of 64 elements: 16-byte lanes in both types
    bnorm("bn_f16_nchw_3x6x8x8", H, (3, 6, 8, 8), "NCHW"),
    bnorm("bn_f32_nchw_3x6x7x7", F, (3, 6, 7, 7), "NCHW"),    # planes of 49: scalar lanes
    bnorm("bn_f16_nchw_3x6x7x7", H, (3, 6, 7, 7), "NCHW"),
    bnorm("bn_f32_nchw_3x6x8x8_default", F, (3, 6, 8, 8), "NCHW", cluster=None),
    # convolution backward with dbias
    conv_back("conv_c32_k32_12x12_algo1", 2, 12, 12, 32, 32, back_algo=1),  # Winograd block partials folded by colsum_f32
    conv_back("conv_c32_k32_12x12_algo0", 2, 12, 12, 32, 32, back_algo=0),  # colsum_f32 over g
    conv_back("conv_nchw_1x1_c16_k24_8x8", 2, 8, 8, 16, 24, ksize=1, pad=0, fmt="NCHW"),  # chan_sum_planes, 16-byte lanes
    conv_back("conv_nchw_1x1_c16_k24_7x7", 2, 7, 7, 16, 24, ksize=1, pad=0, fmt="NCHW"),  # planes of 49: not the planar route (it wants whole 4-element chunks), colsum_f32 over the re-laid g
    conv_back("conv_half_nchw_1x1_c16_k24_8x8", 2, 8, 8, 16, 24, ksize=1, pad=0, fmt="NCHW", act=H, par=H),  # chan_sum_planes_f16, 16-byte lanes
    conv_back("conv_half_nchw_1x1_c16_k24_7x7", 2, 7, 7, 16, 24, ksize=1, pad=0, fmt="NCHW", act=H, par=H),
    conv_back("conv_nchw_1x1_c16_k24_6x6", 2, 6, 6, 16, 24, ksize=1, pad=0, fmt="NCHW"),  # planes of 36: chan_sum_planes, 16-byte lanes of floats ...
    conv_back("conv_half_nchw_1x1_c16_k24_6x6", 2, 6, 6, 16, 24, ksize=1, pad=0, fmt="NCHW", act=H, par=H),  # ... chan_sum_planes_f16 on scalar lanes (36 halves are no whole 16-byte chunks)
    conv_back("conv_half_c16_k24_6x6", 2, 6, 6, 16, 24, act=H, par=H),  # colsum_f16
    conv_back("conv_half_nchw_c64_k72_8x16", 3, 8, 16, 64, 72, fmt="NCHW", act=H, par=H),  # colsum_partials_f16, one level
    conv_back("conv_half_nchw_c64_k64_8x16_n264", 264, 8, 16, 64, 64, gpu_only=True, fmt="NCHW", act=H, par=H),  # ... 528 partial rows: two levels (minutes on the emulator)
    # LSTM backward with bias: colsum_f32 over the gate gradients
    lstm_back("lstm_t3_b2_h8", 3, 2, 5, 8),
]
