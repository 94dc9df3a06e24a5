"""GEMM_FORWARD of at most 32 CCV_16F rows against a dense CCV_16F weight [N, K] (transpose_b, the dense layer's form) on gemm_rows_f16_kernel
(ccv_amd/csrc/gemm_rows_f16.h; tunables GEMM_F16_ROWS, GEMM_F16_ROWS_SLICES): the weight goes from memory straight into the matrix instruction.

The bound of every comparison against float64 is derived, not measured (tests/test_gemm_qx_fused.py).  With S = sum_k |a_k| |w_k| + |bias| per output element:
    |got - ref| <= 2^-11 |ref| + (K + 2) 2^-23 S + 2^-24
products of two halves are exact in fp32, an fp32 sum of K + 2 terms in any order is off by at most the middle term, and the result is rounded to half once."""
import ctypes
import itertools
import mmap
import numpy as np
import pytest
from ccv_amd import nnc
from harness import make_tensors

T01 = nnc.TRANSPOSE(0, 1)
NAME = "gemm_rows_f16"


def operands(rng, a_shape, w_shape, bias, exact=False):
    """exact: small integers over 8, every partial sum exact in fp32."""
    draw = (lambda shape: rng.integers(-8, 9, size=shape) / 8) if exact else rng.standard_normal
    return draw(a_shape).astype(np.float16), draw(w_shape).astype(np.float16), (draw(bias).astype(np.float16) if bias else None)


def run(lib, a, w, bias, n, tb=T01, flags=0, rows=1, slices=0, pad=0, tw=None):
    """The command with the two tuning keys at `rows` and `slices` (restored afterwards); returns (b, the kernel it ran on last).
    pad: a, w and b are views of matrices whose rows are 8 pad (b: pad) elements longer."""
    keys = lib.tune_get("GEMM_F16_ROWS"), lib.tune_get("GEMM_F16_ROWS_SLICES")
    padded = lambda x, by: np.concatenate([x, np.full(x.shape[:-1] + (by,), 7, x.dtype)], axis=-1)
    view = lambda t, x, by: t.view(x.shape, (x.shape[-1] + by, 1)) if by else t
    b0 = np.zeros(a.shape[:-1] + (n,), a.dtype)
    ta, tw0, tbias, tb_full = make_tensors(lib, nnc.GPU_MEMORY, [padded(a, 8 * pad), padded(w, 8 * pad), bias, padded(b0, pad)])
    ins = [view(ta, a, 8 * pad), tw if tw is not None else view(tw0, w, 8 * pad)] + ([tbias] if bias is not None else [])
    lib.tune_set("GEMM_F16_ROWS", rows)
    lib.tune_set("GEMM_F16_ROWS_SLICES", slices)
    try:
        assert lib.cmd_exec(nnc.CMD_GEMM_FORWARD(nnc.NO_TRANSPOSE, tb), nnc.NO_HINT, flags, ins, [view(tb_full, b0, pad)]) == 0
        lib.stream_wait(None)
    finally:
        lib.tune_set("GEMM_F16_ROWS", keys[0])
        lib.tune_set("GEMM_F16_ROWS_SLICES", keys[1])
    got = tb_full.numpy()
    assert (got[..., n:] == 7).all()  # nothing written between b's rows
    return got[..., :n], lib.dll.nnc_mi355x_last_kernel_name().decode()


def check(got, a, w, bias):
    a64, w64 = a.astype(np.float64), w.astype(np.float64)
    extra = 0 if bias is None else bias.astype(np.float64)
    ref, s = a64 @ w64.T + extra, np.abs(a64) @ np.abs(w64).T + np.abs(extra)
    err, bound = np.abs(got.astype(np.float64) - ref), 2.0 ** -11 * np.abs(ref) + (a.shape[-1] + 2) * 2.0 ** -23 * s + 2.0 ** -24
    assert (err <= bound).all(), (float((err / bound).max()), np.argwhere(err > bound)[:4])


# every third of M x N x K (one K for each M and N, each K three times for each M): less than a tile / a partial second tile / whole tiles, less than one matrix step / an odd number of groups / several steps, with and
# without bias in turn.  Then K = 1288 (161 groups: two chunks of 64 and a ragged third, so the ring is refilled) in one forced slice and under the launch's own rule,
# the 3-d a, padded row strides of a, w and b, and three forced slices of 10, 10 and 5 groups.  (rows, n, k, bias, slices, pad)
CROSS = list(itertools.product((1, 5, 32), (8, 40, 64), (8, 24, 200)))
CASES = [((m,), n, k, i % 2 == 0, 0, 0) for i, (m, n, k) in enumerate(CROSS) if (i + i // 3 + i // 9) % 3 == 0]
CASES += [((5,), 40, 1288, True, 1, 0), ((32,), 64, 1288, False, 0, 0), ((2, 3), 40, 24, True, 0, 0), ((5,), 40, 200, True, 0, 1), ((5,), 40, 200, False, 3, 0)]


@pytest.mark.parametrize("rows,n,k,bias,slices,pad", CASES)
def test_rows_gemm_matches_float64(backend, rows, n, k, bias, slices, pad):
    a, w, tbias = operands(np.random.default_rng([n, k, slices]), rows + (k,), (n, k), (n,) if bias else None)
    got, kernel = run(backend, a, w, tbias, n, slices=slices, pad=pad)
    assert kernel == NAME
    check(got, a, w, tbias)


def test_two_runs_give_the_same_bits(backend):
    a, w, bias = operands(np.random.default_rng(1), (5, 1288), (40, 1288), (40,))
    first, second = (run(backend, a, w, bias, 40, slices=4)[0] for _ in range(2))
    assert (first.view(np.uint16) == second.view(np.uint16)).all()


def test_rows_and_tile_routes_agree_on_exact_inputs(backend):
    """Small integers over 8: every partial sum is exact in fp32, so the order of the sums cannot show and both routes give the same bits."""
    a, w, bias = operands(np.random.default_rng(2), (5, 200), (40, 200), (40,), exact=True)
    rows, kernel = run(backend, a, w, bias, 40, rows=1)
    tile, other = run(backend, a, w, bias, 40, rows=0)
    assert kernel == NAME and other != NAME
    assert (rows.view(np.uint16) == tile.view(np.uint16)).all()


# what differs from the taken case (M = 5, N = 40, K = 24, transpose_b, half a, a row-vector bias or none, no accumulation, GEMM_F16_ROWS = 1)
REFUSED = {"M=33": dict(m=33), "no transpose_b": dict(tb=nnc.NO_TRANSPOSE), "K=12": dict(k=12), "fp32 a": dict(dtype=np.float32),
           "ACCUMULATE_OUTPUT": dict(flags=nnc.ACCUMULATE_OUTPUT), "bias [M, N]": dict(bias=(5, 40)), "default keys": dict(rows=None)}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refused_commands_keep_their_kernel(backend, what):
    lib = backend
    m, k, tb, dtype, flags, bias, rows = (REFUSED[what].get(key, default) for key, default in (("m", 5), ("k", 24), ("tb", T01), ("dtype", np.float16), ("flags", 0), ("bias", None), ("rows", 1)))
    a, w, tbias = operands(np.random.default_rng(len(what)), (m, k), (40, k) if tb == T01 else (k, 40), bias)
    got, kernel = run(lib, a.astype(dtype), w, tbias, 40, tb=tb, flags=flags, rows=lib.tune_get("GEMM_F16_ROWS") if rows is None else rows)
    assert kernel != NAME
    check(got, a, w if tb == T01 else w.T, tbias)


def test_rows_gemm_reads_nothing_past_the_weight(emu_lib):
    """On the emulator device memory is host memory: w's last byte is the last byte of a page with an inaccessible page behind it."""
    lib = emu_lib
    n, k = 40, 24
    a, w, _ = operands(np.random.default_rng(3), (1, k), (n, k), None)
    page = mmap.PAGESIZE
    mm = mmap.mmap(-1, 2 * page)
    base = ctypes.addressof(ctypes.c_char.from_buffer(mm))
    libc = ctypes.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    ctypes.memmove(base + page - w.nbytes, w.ctypes.data, w.nbytes)
    (tw,) = make_tensors(lib, nnc.GPU_MEMORY, [w])
    tw.struct.data = base + page - w.nbytes
    assert libc.mprotect(base + page, page, 0) == 0  # PROT_NONE
    try:
        got, kernel = run(lib, a, w, None, n, tw=tw)
    finally:
        libc.mprotect(base + page, page, mmap.PROT_READ | mmap.PROT_WRITE)
    assert kernel == NAME
    check(got, a, w, None)
