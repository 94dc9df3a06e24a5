"""A backward convolution that computes both gradients reads a tensor ONCE where two of its kernels used to read the same one (tunable
CONV_BACK_SHARE, cmd_conv.cpp `tl_share`): the output gradient's two Winograd transforms in one kernel (wino_outgrad_both_kernel), and the fused
data gradient's ReLU mask bits written by the filter gradient's input transform (wino_input_kernel<true>).  Same expressions in the same order:
every result is EQUAL, bit for bit, to the command with the tunable off (the separate kernels).  Runs on the CPU HIP emulator in the `not gpu`
tier and on the MI355X in the `gpu` tier."""
import ctypes as C
import numpy as np
import pytest
from ccv_amd import nnc
from harness import exec_on, out_hw

F = np.float32


def srnd(rng, *shape, scale=1.0):
    return ((rng.random(shape, dtype=F) - 0.5) * 2 * scale).astype(F)


def _shared(lib, what):
    f = lib.dll.nnc_mi355x_debug_conv_back_shared
    f.restype, f.argtypes = C.c_long, [C.c_int]
    return int(f(what))


def _backward(lib, share, algo, flags, g, a, wt, hint, outs, bits=None):
    """One CONVOLUTION_BACKWARD with CONV_BACK_SHARE = share; bits: a uint8 array that receives the fused data gradient's mask bits.
    Returns (outputs, bytes of the mask-bit buffer, launches of the two shared kernels during the call)."""
    cmd = nnc.CMD_CONVOLUTION_BACKWARD(1, wt.shape[0], 3, 3, wt.shape[3])
    cmd.algorithm = algo
    grab = lib.dll.nnc_mi355x_debug_conv_mask_bits
    grab.restype, grab.argtypes = C.c_size_t, [C.c_void_p, C.c_size_t]
    before = (_shared(lib, 0), _shared(lib, 1))
    lib.tune_set("CONV_BACK_SHARE", share)
    try:
        if bits is not None:
            grab(bits.ctypes.data_as(C.c_void_p), bits.nbytes)
        r, got = exec_on(lib, nnc.GPU_MEMORY, cmd, hint, flags, [g, a, wt], [o.copy() for o in outs])
        size = int(grab(None, 0))
    finally:
        lib.tune_set("CONV_BACK_SHARE", 3)
    assert r == 0
    return got, size, (_shared(lib, 0) - before[0], _shared(lib, 1) - before[1])


ONCE_CASES = [
    # n, h, w, c, k
    (3, 5, 5, 8, 8),      # 2 x 2 tiles, one clipped each way (1 valid row / column)
    (3, 13, 13, 8, 8),    # conv5's size: 4 tiles with 1 valid column / row in the last
    (3, 9, 6, 8, 16),     # unequal sides, C != K
]


@pytest.mark.parametrize("flags", [0, nnc.ACCUMULATE_OUTPUT], ids=["store", "accumulate"])
@pytest.mark.parametrize("case", ONCE_CASES, ids=[str(c) for c in ONCE_CASES])
def test_output_gradient_read_once_is_bit_identical(backend, case, flags):
    """Both gradients and the bias gradient via HBM (algorithm 1), padding 1: one kernel makes the data gradient's V, the filter gradient's W and the
    bias partial sums.  dx, dw and dbias equal the separate kernels' bit for bit, with and without CCV_NNC_ACCUMULATE_OUTPUT."""
    n, h, w, c, k = case
    rng = np.random.default_rng(3)
    a, wt, g = srnd(rng, n, h, w, c), srnd(rng, k, 3, 3, c, scale=1.0 / (9 * c)), srnd(rng, n, h, w, k)
    outs = [np.full_like(a, 3), srnd(rng, k, 3, 3, c), srnd(rng, k)]
    hint = nnc.HINT((1, 1), (1, 1))
    want, _, ran0 = _backward(backend, 0, 1, flags, g, a, wt, hint, outs)
    got, _, ran = _backward(backend, 3, 1, flags, g, a, wt, hint, outs)
    assert ran0 == (0, 0) and ran == (1, 0), (ran0, ran)
    assert np.abs(want[1] - outs[1]).max() > 0 and np.abs(want[2] - outs[2]).max() > 0
    for i, name in enumerate(("dx", "dw", "dbias")):
        assert np.array_equal(got[i], want[i]), name
    # ... and they are the gradients: the direct loops in float64 on the same inputs (dbias only; dx / dw are pinned by test_parity_ops.py for the separate kernels)
    want_db = g.sum(axis=(0, 1, 2), dtype=np.float64) + (outs[2] if flags else 0)
    np.testing.assert_allclose(got[2], want_db, rtol=1e-4, atol=1e-5 * max(1.0, float(np.abs(want_db).max())))


@pytest.mark.parametrize("pad,k", [(0, 8), (1, 24)], ids=["no padding", "no bias sums in the transform"])
def test_output_gradient_read_once_falls_back(backend, pad, k):
    """padding 0: the two tile grids have different origins (and extents).  K / 4 = 6 does not divide 256: the bias gradient does not ride on the
    transform, and the one-pass kernel exists with the bias sums only (winograd.h).  The separate kernels run, the results are the same."""
    n, h, w, c = 3, 9, 10, 8
    rng = np.random.default_rng(4)
    hint = nnc.HINT((1, 1), (pad, pad))
    oh, ow = out_hw(h, w, 3, 3, hint)
    a, wt, g = srnd(rng, n, h, w, c), srnd(rng, k, 3, 3, c, scale=1.0 / (9 * c)), srnd(rng, n, oh, ow, k)
    outs = [np.full_like(a, 3), np.zeros_like(wt), np.zeros(k, F)]
    want, _, ran0 = _backward(backend, 0, 1, 0, g, a, wt, hint, outs)
    got, _, ran = _backward(backend, 3, 1, 0, g, a, wt, hint, outs)
    assert ran0 == (0, 0) and ran == (0, 0), (ran0, ran)
    for i in range(3):
        assert np.array_equal(got[i], want[i]), i


MASK_CASES = [
    # n, h, w, c, k, takes the 2 x 8 tile groups
    (2, 9, 20, 160, 160, False),  # 3 x 5 tiles: 4 x 4 and 2 x 8 groups cover them equally (2 groups), the plan keeps 4 x 4 -- the packing kernel runs, as for conv1_2 / conv2_2
    # (algorithm 2 takes the same kernels at any channel count the fused data gradient accepts: the 2 x 8 cases stay small)
    (2, 6, 40, 40, 40, True),     # 2 x 10 tiles: 2 x 8 groups -- one full and one clipped group in x (2 of 8 tile columns), a clipped row pair (2 of 4 rows); 40 channels: the second block holds 8 of 32 (kq >= K zeros)
    (2, 5, 20, 24, 24, True),     # 2 x 5 tiles: one clipped group (5 of 8 columns), 1 valid row in the second tile row; one ragged block
]


@pytest.mark.parametrize("case", MASK_CASES, ids=[str(c) for c in MASK_CASES])
def test_mask_bits_from_the_filter_gradients_input_pass(backend, case):
    """NNC_MI355X_CONV_ALGO_FUSE_RELU with the via-HBM filter gradient and the fused masked data gradient on the same map (VGG-D: 128 < C <= 256).  With 2 x 8 tile
    groups the mask bits come from wino_input_kernel<true> and no packing kernel runs: the buffer equals wino_mask_pack_kernel<2, 8>'s byte for byte
    (zeros for clipped tiles and channels beyond K included), dx / dw / dbias equal the separate kernels' bit for bit."""
    n, h, w, c, k, two_by_eight = case
    rng = np.random.default_rng(5)
    a = np.maximum(srnd(rng, n, h, w, c), 0)
    a[rng.random(a.shape) < 0.1] = -0.0
    assert (a == 0).any() and np.signbit(a[a == 0]).any() and not np.signbit(a[a == 0]).all()  # exact zeros and negative zeros: both masked out
    wt, g = srnd(rng, k, 3, 3, c, scale=1.0 / (9 * c)), srnd(rng, n, h, w, k)
    outs = [np.full_like(a, 3), np.zeros_like(wt), np.zeros(k, F)]
    hint = nnc.HINT((1, 1), (1, 1))
    algo = nnc.CONV_ALGO_FUSE_RELU | 2
    cap = 1 << 20
    bits0, bits1 = np.full(cap, 0xa5, np.uint8), np.full(cap, 0x5a, np.uint8)
    want, size0, ran0 = _backward(backend, 0, algo, 0, g, a, wt, hint, outs, bits0)
    assert backend.dll.nnc_mi355x_last_kernel_name().decode() == "conv_dgrad_wino_fused"
    got, size1, ran = _backward(backend, 3, algo, 0, g, a, wt, hint, outs, bits1)
    assert backend.dll.nnc_mi355x_last_kernel_name().decode() == "conv_dgrad_wino_fused"
    assert ran0 == (0, 0) and ran == (0, 1 if two_by_eight else 0), (ran0, ran)
    assert 0 < size0 == size1 <= cap and size0 % 1024 == 0
    assert np.array_equal(bits1[:size1], bits0[:size0])
    assert bits0[:size0].any() and not bits0[:size0].all()
    for i, name in enumerate(("dx", "dw", "dbias")):
        assert np.array_equal(got[i], want[i]), name
    assert (got[0][a <= 0] == 0).all() and (got[0][a > 0] != 0).any()
