"""Depthwise convolutions (groups == channels == filters) on the direct kernels of ccv_amd/csrc/conv_depthwise.h: forward, data gradient,
filter + bias gradient, fp32 and half, NHWC and NCHW, against the reference's CPU backend.  The oracle's convolution backward exists for
NHWC only, so the NCHW cases run it in NHWC and compare after transposition (as tests/test_resnet_block.py does); half-precision cases hand
the oracle the same half values widened to fp32 (as tests/test_half.py does).  Tolerances are the project's existing ones:
fp32 rtol 1e-4, atol 2e-5 * max(1, max|ref|) (test_conv_random.py); half test_half.py's _close."""
import numpy as np
import pytest
from ccv_amd import nnc
from harness import exec_on, out_hw
from test_half import _close

F, H = np.float32, np.float16
DW_BIT = "CONV_DEPTHWISE"


def _rnd(rng, dtype, *shape, scale=1.0):
    return ((rng.random(shape, dtype=F) - 0.5) * 2 * scale).astype(dtype)


def _check(got, want, dtype, what=""):
    assert got.dtype == dtype, what
    if dtype == H:
        _close(got, want)
    else:
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-5 * max(1.0, float(np.abs(want).max())), err_msg=what)


_ORACLE = {}


class Case:
    """One geometry with its tensors (NHWC, the filter [C][k][k][mult]) and the oracle's results, computed once and never written to."""

    def __init__(self, ref_lib, geom, dtype, groups=None, mult=1, seed=7):
        n, h, w, c, k, stride, pad, dil = geom
        self.geom, self.dtype, self.c, self.k, self.kout = geom, dtype, c, k, c * mult
        self.groups = c if groups is None else groups
        cg = c // self.groups
        rng = np.random.default_rng(seed)
        self.hint = nnc.HINT((stride, stride), (pad, pad))
        ek = (k - 1) * dil + 1
        self.oh, self.ow = out_hw(h, w, ek, ek, self.hint)
        assert self.oh >= 1 and self.ow >= 1
        self.dil = (dil, dil) if dil > 1 else None
        self.a = _rnd(rng, dtype, n, h, w, c)
        self.w = _rnd(rng, dtype, self.kout, k, k, cg, scale=1.0 / k)
        self.bias = _rnd(rng, dtype, self.kout, scale=0.5)
        self.g = _rnd(rng, dtype, n, self.oh, self.ow, self.kout)
        self.dw0 = _rnd(rng, dtype, self.kout, k, k, cg)      # non-zero initial contents of the outputs
        self.dbias0 = _rnd(rng, dtype, self.kout)
        self.ref = ref_lib

    def cmds(self):
        cg = self.c // self.groups
        return (nnc.CMD_CONVOLUTION_FORWARD(self.groups, self.kout, self.k, self.k, cg, dilation=self.dil),
                nnc.CMD_CONVOLUTION_BACKWARD(self.groups, self.kout, self.k, self.k, cg, dilation=self.dil))

    def oracle(self, flags=0, bias=True):
        key = (self.geom, self.dtype, self.groups, self.kout, flags, bias)
        if key not in _ORACLE:
            fwd, bwd = self.cmds()
            up = lambda x: x.astype(F)
            r, (b,) = exec_on(self.ref, nnc.CPU_MEMORY, fwd, self.hint, 0, [up(self.a), up(self.w)] + ([up(self.bias)] if bias else []), [np.zeros(self.g.shape, F)], backend=nnc.BACKEND_CPU_REF)
            assert r == 0
            r, (h, dw, dbias) = exec_on(self.ref, nnc.CPU_MEMORY, bwd, self.hint, flags, [up(self.g), up(self.a), up(self.w)], [np.zeros(self.a.shape, F), up(self.dw0), up(self.dbias0)], backend=nnc.BACKEND_CPU_REF)
            assert r == 0
            for x in (b, h, dw, dbias):
                x.setflags(write=False)
            _ORACLE[key] = (b, h, dw, dbias)
        return _ORACLE[key]


def _to(fmt, x):
    """NHWC array -> the layout under test (activations transposed; a depthwise filter [C][k][k][1] and [C][1][k][k] are the same bytes)"""
    if x is None or fmt == "NHWC" or x.ndim != 4:
        return x
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def _from(fmt, x):
    if x is None or fmt == "NHWC" or x.ndim != 4:
        return x
    return np.ascontiguousarray(x.transpose(0, 2, 3, 1))


def run_forward(L, case, fmt, bias=True, algorithm=-1):
    fwd, _ = case.cmds()
    fwd.algorithm = algorithm
    ins = [_to(fmt, case.a), _to(fmt, case.w)] + ([case.bias] if bias else [])
    r, (b,) = exec_on(L, nnc.GPU_MEMORY, fwd, case.hint, 0, ins, [_to(fmt, np.full(case.g.shape, 3, case.dtype))], fmt)
    assert r == 0
    return _from(fmt, b)


def run_backward(L, case, fmt, flags=0, want=(True, True, True)):
    """want: which of (h, dw, dbias) the command is given"""
    _, bwd = case.cmds()
    outs = [_to(fmt, np.full(case.a.shape, 3, case.dtype)) if want[0] else None, _to(fmt, case.dw0) if want[1] else None, case.dbias0 if want[2] else None]
    while outs and outs[-1] is None:
        outs.pop()
    r, got = exec_on(L, nnc.GPU_MEMORY, bwd, case.hint, flags, [_to(fmt, case.g), _to(fmt, case.a), _to(fmt, case.w)], outs, fmt)
    assert r == 0
    got = [_from(fmt, x) for x in got] + [None] * (3 - len(got))
    return got


def _records(L, fn):
    L.profile_enable(1)
    try:
        out = fn()
        L.stream_wait(None)
        names = [r[0] for r in L.profile_records()]
    finally:
        L.profile_enable(0)
    return out, names


def _check_all(L, case, fmt, flags=0):
    want_b, want_h, want_dw, want_dbias = case.oracle(flags)
    _check(run_forward(L, case, fmt), want_b, case.dtype, "forward")
    h, dw, dbias = run_backward(L, case, fmt, flags)
    _check(h, want_h, case.dtype, "data gradient")
    _check(dw, want_dw, case.dtype, "filter gradient")
    if not flags:  # (the CPU oracle overwrites dbias under ACCUMULATE_OUTPUT: tests/test_half.py test_conv_backward_half)
        _check(dbias, want_dbias, case.dtype, "bias gradient")
    return h, dw, dbias


@pytest.mark.parametrize("fmt", ["NHWC", "NCHW"])
@pytest.mark.parametrize("dtype", [F, H], ids=["f32", "f16"])
def test_route_taken(backend, ref_lib, dtype, fmt):
    """A depthwise command runs the conv_dw kernels and no contraction; with the tuning key at 0 it runs none of them and agrees."""
    case = Case(ref_lib, (2, 9, 10, 16, 3, 1, 1, 1), dtype)
    both = lambda: (run_forward(backend, case, fmt), run_backward(backend, case, fmt))
    (b1, back1), names = _records(backend, both)
    assert any("conv_dw_fwd" in x for x in names) and any("conv_dw_dgrad" in x for x in names), names
    assert any("conv_dw_wgrad" in x for x in names) and any("conv_dw_fold" in x for x in names), names
    assert not any("mfma_gemm" in x for x in names), names
    backend.tune_set(DW_BIT, 0)
    try:
        (b0, back0), names0 = _records(backend, both)
    finally:
        backend.tune_set(DW_BIT, 1)
    assert names0 and not any("conv_dw" in x for x in names0), names0
    _check(b1, b0.astype(F), dtype, "forward, both routes")
    for x, y, what in zip(back1, back0, ("data gradient", "filter gradient", "bias gradient")):
        _check(x, y.astype(F), dtype, what + ", both routes")
    want = case.oracle()
    for x, y in zip((b1,) + tuple(back1), want):
        _check(x, y, dtype)


NHWC_GEOMETRY = [
    # n, h, w, C, k, stride, pad, dilation
    (2, 7, 9, 12, 3, 1, 1, 1),     # fp32 only: three 4-wide vectors, not a multiple of 8
    (2, 9, 11, 8, 5, 2, 2, 1),
    (1, 8, 8, 16, 3, 1, 2, 2),     # dilated
    (2, 6, 7, 8, 3, 1, 0, 1),      # no padding
    (2, 2, 3, 8, 5, 1, 2, 1),      # map smaller than the kernel
    (1, 5, 23, 40, 3, 1, 1, 1),    # ragged run along W; five 8-wide vectors in half
    (1, 4, 4, 264, 3, 2, 1, 1),    # more channels than one workgroup's block (256)
]


# (the half cases use only C % 8 == 0: C = 12 in half is a fall-back, test_fallbacks_stay_correct)
NHWC_CASES = [(g, dt) for g in NHWC_GEOMETRY for dt in (F, H) if dt == F or g[3] % 8 == 0]


@pytest.mark.parametrize("geom,dtype", NHWC_CASES, ids=["n%d_%dx%d_c%d_k%d_s%d_p%d_d%d" % g + ("-f16" if dt == H else "-f32") for g, dt in NHWC_CASES])
def test_geometry_nhwc(backend, ref_lib, geom, dtype):
    case = Case(ref_lib, geom, dtype)
    _, names = _records(backend, lambda: _check_all(backend, case, "NHWC"))
    assert any("conv_dw" in x for x in names), names


NCHW_GEOMETRY = [
    (3, 7, 7, 16, 5, 1, 2, 1),     # 48 small planes: several per workgroup and per wave
    (2, 14, 14, 8, 3, 2, 1, 1),    # stride 2: the register-segment form forward, the hole pattern back
    (2, 17, 13, 8, 3, 1, 1, 1),    # rows of 13: row starts (and every second plane) off 16-byte alignment
    (2, 1, 1, 8, 3, 1, 1, 1),      # 1 x 1 planes
    (1, 9, 12, 8, 3, 1, 2, 2),     # dilated: the one-output-per-lane form
    (1, 100, 90, 8, 5, 2, 2, 1),   # a plane larger than a workgroup's LDS share (9000 > 8192 elements): bands of rows, both stencils and the filter gradient
]


@pytest.mark.parametrize("dtype", [F, H], ids=["f32", "f16"])
@pytest.mark.parametrize("geom", NCHW_GEOMETRY, ids=["n%d_%dx%d_c%d_k%d_s%d_p%d_d%d" % g for g in NCHW_GEOMETRY])
def test_geometry_nchw(backend, ref_lib, geom, dtype):
    case = Case(ref_lib, geom, dtype)
    _, names = _records(backend, lambda: _check_all(backend, case, "NCHW"))
    assert any("conv_dw" in x for x in names), names


@pytest.mark.parametrize("fmt", ["NHWC", "NCHW"])
@pytest.mark.parametrize("dtype", [F, H], ids=["f32", "f16"])
def test_filter_gradient_across_slices(backend, ref_lib, dtype, fmt):
    """n = 3, 20 x 20, C = 8, 3 x 3, the filter gradient's partial sums come from several slices (cmd_conv.cpp conv_dw_wgrad):
    NHWC -- row slices of max(4, ceil(N * OH / 1024)) = 4 of the 60 output rows, times the 256 / (channel vectors * 10) pixel phases of a
    workgroup: 15 x 12 = 180 slices in fp32 (two 4-channel vectors), 15 x 25 = 375 in half (one 8-channel vector);
    NCHW -- planes of 400 elements, 4096 / 400 = 10 fit: 8 channels of ONE image per workgroup, so a slice per image: 3.
    The fold adds them in a fixed order: the same bits on every run; ACCUMULATE_OUTPUT adds into dw."""
    case = Case(ref_lib, (3, 20, 20, 8, 3, 1, 1, 1), dtype)
    for flags in (0, nnc.ACCUMULATE_OUTPUT):
        first = _check_all(backend, case, fmt, flags)
        again = run_backward(backend, case, fmt, flags)
        for x, y in zip(first, again):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("fmt", ["NHWC", "NCHW"])
@pytest.mark.parametrize("dtype", [F, H], ids=["f32", "f16"])
def test_optional_tensors(backend, ref_lib, dtype, fmt):
    case = Case(ref_lib, (2, 6, 9, 8, 3, 1, 1, 1), dtype)
    want_b, want_h, want_dw, want_dbias = case.oracle()

    def run():
        h, dw, dbias = run_backward(backend, case, fmt, want=(False, True, True))   # no data gradient
        assert h is None
        _check(dw, want_dw, dtype)
        _check(dbias, want_dbias, dtype)
        h, dw, dbias = run_backward(backend, case, fmt, want=(True, False, False))  # the data gradient alone
        assert dw is None and dbias is None
        _check(h, want_h, dtype)
        _check(run_forward(backend, case, fmt, bias=False), case.oracle(bias=False)[0], dtype)
    _, names = _records(backend, run)
    assert any("conv_dw" in x for x in names) and not any("mfma_gemm" in x for x in names), names


def test_fallbacks_stay_correct(backend, ref_lib):
    """Commands the depthwise route does not take keep the route they had, and its results."""
    for geom, dtype, groups, mult in (((2, 6, 7, 12, 3, 1, 1, 1), H, None, 1),   # C = 12 in half NHWC: no whole 8-channel vectors
                                      ((2, 6, 7, 4, 3, 1, 1, 1), F, None, 1),    # groups = C = 4: fewer than 8 channels
                                      ((2, 6, 7, 8, 3, 1, 1, 1), F, None, 2)):   # K = 2 C with groups = C: a channel multiplier
        case = Case(ref_lib, geom, dtype, groups, mult)
        _, names = _records(backend, lambda: _check_all(backend, case, "NHWC"))
        assert names and not any("conv_dw" in x for x in names), names
    # a channel-slice view of a wider NHWC parent: 8 of 16 channels, pixel stride 16
    case = Case(ref_lib, (2, 6, 7, 8, 3, 1, 1, 1), F)
    n, h, w, c = case.a.shape
    wide = np.zeros((n, h, w, 2 * c), F)
    wide[..., c:] = case.a
    parent = backend.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_32F, wide.shape), wide)
    view = parent.view((n, h, w, c), (h * w * 2 * c, w * 2 * c, 2 * c, 1), offset=c)
    wt = backend.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_32F, case.w.shape), case.w)
    bias = backend.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_32F, case.bias.shape), case.bias)
    out = backend.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_32F, case.g.shape), np.zeros(case.g.shape, F))
    fwd, _ = case.cmds()
    r, names = _records(backend, lambda: backend.cmd_exec(fwd, case.hint, 0, [view, wt, bias], [out]))
    assert r == 0 and names and not any("conv_dw" in x for x in names), names
    _check(out.numpy(), case.oracle()[0], F)


@pytest.mark.parametrize("fmt", ["NHWC", "NCHW"])
@pytest.mark.parametrize("dtype", [F, H], ids=["f32", "f16"])
def test_fuse_relu(backend, ref_lib, dtype, fmt):
    """algorithm = FUSE_RELU | 0xff on a depthwise forward: bit for bit the plain command followed by RELU_FORWARD in place."""
    case = Case(ref_lib, (2, 9, 10, 16, 3, 1, 1, 1), dtype)
    fused, names = _records(backend, lambda: run_forward(backend, case, fmt, algorithm=nnc.CONV_ALGO_FUSE_RELU | 0xff))
    assert any("conv_dw_fwd" in x for x in names), names
    plain = run_forward(backend, case, fmt)
    dt = nnc.CCV_16F if dtype == H else nnc.CCV_32F
    t = backend.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, dt, plain.shape), plain)
    assert backend.cmd_exec(nnc.CMD_RELU_FORWARD(), nnc.NO_HINT, 0, [t], [t]) == 0
    want = t.numpy()
    assert (fused >= 0).all() and (fused == 0).any() and (plain < 0).any()
    assert np.array_equal(fused.view(np.uint16 if dtype == H else np.uint32), want.view(np.uint16 if dtype == H else np.uint32))
