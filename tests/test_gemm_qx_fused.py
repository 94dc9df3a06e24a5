"""GEMM_FORWARD of a few CCV_16F rows against a palettized weight [N, K] (transpose_b, the dense layer's form) on gemm_qx_f16_kernel
(ccv_amd/csrc/gemm_qx_f16.h; tunables GEMM_QX_FUSED, GEMM_QX_SLICES): the weight's index stream is decoded inside the contraction.

The bound of every comparison against float64 is derived, not measured.  With S = sum_k |a_k| |w_k| + |bias| per output element:
    |got - ref| <= 2^-11 |ref| + (K + 2) 2^-23 S + 2^-24
products of two halves are exact in fp32, an fp32 sum of K + 2 terms in any order is off by at most the middle term, and the result is rounded to half once."""
import ctypes
import itertools
import mmap
import os
import sys
import numpy as np
import pytest
from ccv_amd import nnc
from harness import make_tensors

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
from palettize_numpy import pack_stream, expand  # noqa: E402

T01 = nnc.TRANSPOSE(0, 1)


def operands(rng, qbits, a_shape, w_shape, nib, bias, exact=False):
    """a, (palettes, indices), bias, and the float64 weight matrix the stream expands to.  exact: small integers over 8, every partial sum exact in fp32."""
    count = w_shape[0] * w_shape[1]
    blocks = (count + nib - 1) // nib
    draw = (lambda shape: rng.integers(-8, 9, size=shape) / 8) if exact else rng.standard_normal
    palettes = draw((blocks, 1 << qbits)).astype(np.float16).view(np.uint16)
    indices = rng.integers(0, 1 << qbits, size=count)
    w = expand(palettes, indices, nib, nnc.CCV_16F).view(np.float16).reshape(w_shape).astype(np.float64)
    return draw(a_shape).astype(np.float16), (palettes, indices), (draw(bias).astype(np.float16) if bias else None), w


def qx_tensor(lib, stream, qbits, nib, w_shape):
    return nnc.PalettizedTensor(lib, nnc.tensor_palettize(nnc.GPU_TENSOR_NHWC(0, nnc.CCV_16F, *w_shape), qbits, nib), stream)


def run(lib, a, tw, bias, n, tb=T01, flags=0, b0=None, fused=32, slices=0):
    """The command with the two tuning keys at `fused` and `slices` (restored afterwards); returns (b, the kernel it ran on last)."""
    keys = lib.tune_get("GEMM_QX_FUSED"), lib.tune_get("GEMM_QX_SLICES")
    lib.tune_set("GEMM_QX_FUSED", fused)
    lib.tune_set("GEMM_QX_SLICES", slices)
    try:
        return command(lib, a, tw, bias, n, tb, flags, b0)
    finally:
        lib.tune_set("GEMM_QX_FUSED", keys[0])
        lib.tune_set("GEMM_QX_SLICES", keys[1])


def command(lib, a, tw, bias, n, tb, flags, b0):
    ta, tbias = make_tensors(lib, nnc.GPU_MEMORY, [a, bias])
    (tout,) = make_tensors(lib, nnc.GPU_MEMORY, [np.zeros(a.shape[:-1] + (n,), a.dtype) if b0 is None else b0])
    assert lib.cmd_exec(nnc.CMD_GEMM_FORWARD(nnc.NO_TRANSPOSE, tb), nnc.NO_HINT, flags, [ta, tw] + ([tbias] if bias is not None else []), [tout]) == 0
    lib.stream_wait(None)
    return tout.numpy(), lib.dll.nnc_mi355x_last_kernel_name().decode()


def check(got, a, w, bias):
    a64 = a.astype(np.float64)
    extra = 0 if bias is None else bias.astype(np.float64)
    ref, s = a64 @ w.T + extra, np.abs(a64) @ np.abs(w).T + np.abs(extra)
    err, bound = np.abs(got.astype(np.float64) - ref), 2.0 ** -11 * np.abs(ref) + (a.shape[-1] + 2) * 2.0 ** -23 * s + 2.0 ** -24
    assert (err <= bound).all(), (float((err / bound).max()), np.argwhere(err > bound)[:4])


# every Q x M x N x K x number_in_blocks: a partial tile and more than one, less than one matrix step / an odd number of groups / several steps, blocks smaller and
# larger than a row, straddling rows, a short last block -- every tenth of the 405, with and without bias in turn; then the 3-d a and the forced slices of unequal length
CROSS = list(itertools.product((4, 5, 6, 7, 8), (1, 5, 32), (8, 40, 64), (8, 24, 200), (8, 64, 128)))
CASES = [(q, (m,), n, k, nib, i % 20 == 0, 0) for i, (q, m, n, k, nib) in enumerate(CROSS) if i % 10 == 0]
CASES += [(5, (2, 3), 40, 24, 64, True, 0), (6, (5,), 40, 200, 64, True, 3)]


@pytest.mark.parametrize("qbits,rows,n,k,nib,bias,slices", CASES)
def test_fused_gemm_matches_float64(backend, qbits, rows, n, k, nib, bias, slices):
    lib = backend
    rng = np.random.default_rng([qbits, n, k, nib])
    a, (palettes, indices), tbias, w = operands(rng, qbits, rows + (k,), (n, k), nib, (n,) if bias else None)
    tw = qx_tensor(lib, pack_stream(palettes, indices, qbits, nib, nnc.CCV_16F), qbits, nib, (n, k))
    got, kernel = run(lib, a, tw, tbias, n, slices=slices)
    assert kernel == "gemm_qx_f16"
    check(got, a, w, tbias)


@pytest.mark.parametrize("qbits", [4, 5, 6, 7, 8])
def test_fused_and_expanded_routes_agree_on_exact_inputs(backend, qbits):
    """Small integers over 8: every partial sum is exact in fp32, so the order of the sums cannot show and both routes give the same bits.  On general inputs
    they need not: the fused kernel and the dense contraction sum in different orders."""
    lib = backend
    a, (palettes, indices), bias, _ = operands(np.random.default_rng(qbits), qbits, (5, 72), (40, 72), 64, (40,), exact=True)
    tw = qx_tensor(lib, pack_stream(palettes, indices, qbits, 64, nnc.CCV_16F), qbits, 64, (40, 72))
    fused, kernel = run(lib, a, tw, bias, 40, fused=32)
    dense, other = run(lib, a, tw, bias, 40, fused=0)
    assert kernel == "gemm_qx_f16" and other != "gemm_qx_f16"
    assert (fused.view(np.uint16) == dense.view(np.uint16)).all()


# what differs from the taken case (M = 5, N = 40, K = 24, 64 per block, transpose_b, half a, no accumulation)
REFUSED = {"M=33": dict(m=33), "no transpose_b": dict(tb=nnc.NO_TRANSPOSE), "K=12": dict(k=12), "number_in_blocks=4": dict(nib=4),
           "fp32 a": dict(dtype=np.float32), "ACCUMULATE_OUTPUT": dict(flags=nnc.ACCUMULATE_OUTPUT)}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refused_shapes_keep_the_expanding_route(backend, what):
    lib = backend
    m, k, nib, tb, dtype, flags = (REFUSED[what].get(key, default) for key, default in (("m", 5), ("k", 24), ("nib", 64), ("tb", T01), ("dtype", np.float16), ("flags", 0)))
    w_shape = (40, k) if tb == T01 else (k, 40)
    rng = np.random.default_rng(len(what))
    a, (palettes, indices), _, w = operands(rng, 6, (m, k), w_shape, nib, None)
    tw = qx_tensor(lib, pack_stream(palettes, indices, 6, nib, nnc.CCV_16F), 6, nib, w_shape)
    b0 = rng.standard_normal((m, 40)).astype(dtype) if flags else None  # (GEMM_FORWARD writes b whatever the flag says, as the reference's rows do)
    got, kernel = run(lib, a.astype(dtype), tw, None, 40, tb=tb, flags=flags, b0=b0)
    assert kernel != "gemm_qx_f16"
    check(got, a, w if tb == T01 else w.T, None)


@pytest.mark.parametrize("qbits", [4, 5, 6, 7, 8])
def test_fused_gemm_reads_nothing_past_the_stream(emu_lib, qbits):
    """As test_depalettize_reads_nothing_past_the_stream: on the emulator device memory is host memory, the stream ends exactly at a page boundary with an
    inaccessible page behind it -- an 8-byte index load of the stream's last groups that reached past its end would fault."""
    lib = emu_lib
    n, k, nib = 40, 24, 64
    a, (palettes, indices), _, w = operands(np.random.default_rng(qbits), qbits, (1, k), (n, k), nib, None)
    stream = pack_stream(palettes, indices, qbits, nib, nnc.CCV_16F)
    size = int(lib.palettized_bytes(nnc.CCV_16F, n * k, qbits, nib))
    assert size <= stream.nbytes
    page = mmap.PAGESIZE
    pages = (size + 1 + page - 1) // page
    mm = mmap.mmap(-1, (pages + 1) * page)
    base = ctypes.addressof(ctypes.c_char.from_buffer(mm))
    libc = ctypes.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    start = base + pages * page - size - (size & 1)  # (the palettes are read as 2-byte words: an odd-sized stream leaves one accessible byte behind it)
    ctypes.memmove(start, stream.ctypes.data, size)
    tw = qx_tensor(lib, stream, qbits, nib, (n, k))
    tw.struct.data = start
    assert libc.mprotect(base + pages * page, page, 0) == 0  # PROT_NONE
    try:
        got, kernel = run(lib, a, tw, None, n)
    finally:
        libc.mprotect(base + pages * page, page, mmap.PROT_READ | mmap.PROT_WRITE)
    assert kernel == "gemm_qx_f16"
    check(got, a, w, None)
