"""UPSAMPLE_FORWARD / UPSAMPLE_BACKWARD on dense CCV_16F tensors without fp32 images (ccv_amd/csrc/upsample_ops.h; tunable UPSAMPLE_HALF_NATIVE): nearest and
bilinear, align_corners 0 and 1, NCHW and NHWC, 3-d and 4-d.

There is no tolerance in this file.  The fp32 kernels are bit-exact against the reference's CPU backend (tests/test_parity_act_opt.py::test_upsample), so the half
route through fp32 images is half(reference(float(x))) with one round-to-nearest-even; the native kernels compute the same fp32 value before the one rounding.
Every native result is therefore compared bit for bit with the command under the key at 0 and with the reference on the widened inputs rounded by
.astype(float16).  Inputs are U(-2, 2) exact halves, N = 2 unless said.
"""
import os
import re
import numpy as np
import pytest
from ccv_amd import nnc
from harness import exec_on, make_tensors
from test_mbconv_half import counts, records, key_off, bits, ref_run, aliased

F, H = np.float32, np.float16
KEY = "UPSAMPLE_HALF_NATIVE"

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccv_amd", "csrc", "upsample_ops.h")
with open(_HDR) as _f:
    _TEXT = _f.read()
ROWS, THREADS = (int(re.search(r"constexpr int %s = (\d+);" % k, _TEXT).group(1)) for k in ("UP_ROWS", "UP_THREADS"))
CUS = 256  # compute units of an MI355X (and of the emulator's device)

FMTS = ["NCHW", "NHWC"]
MODES = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (type: 0 nearest, 1 bilinear; align_corners)
TYPE = {0: "nearest", 1: "bilinear"}

_DATA = {}


def data(shape, seed=0):
    """U(-2, 2) exact halves, made once per (shape, seed), read-only"""
    key = (tuple(shape), seed)
    if key not in _DATA:
        rng = np.random.default_rng(2000 + seed + 7 * int(np.prod(shape)) + len(shape))
        x = ((rng.random(shape) - 0.5) * 4).astype(H)
        x.setflags(write=False)
        _DATA[key] = x
    return _DATA[key]


def shapes(fmt, n, c, src, dst):
    """(source shape, resampled shape); n = None: a 3-d tensor, one image"""
    lead = () if n is None else (n,)
    if fmt == "NCHW":
        return lead + (c,) + tuple(src), lead + (c,) + tuple(dst)
    return lead + tuple(src) + (c,), lead + tuple(dst) + (c,)


def command(forward, up_type, align, src, dst):
    return nnc.CMD_UPSAMPLE("UPSAMPLE_FORWARD" if forward else "UPSAMPLE_BACKWARD", up_type, dst[1] / src[1], dst[0] / src[0], align)


def fill(shape, dtype=H):
    return np.full(shape, 3, dtype)


def run(L, cmd, x, out, fmt, flags=0):
    r, res = exec_on(L, nnc.GPU_MEMORY, cmd, nnc.NO_HINT, flags, [x], [out], fmt)
    assert r == 0, "backend returned %d" % r
    return res[0]


_REF = {}


def reference(ref, forward, fmt, up_type, align, src, dst, x, oshape):
    """half(reference(float(x))): computed once per case, read-only"""
    key = (forward, fmt, up_type, align, tuple(src), tuple(dst), x.shape)
    if key not in _REF:
        r = ref_run(ref, command(forward, up_type, align, src, dst), [x], [np.zeros(oshape, H)], fmt)[0].astype(H)
        r.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def same(a, b, what):
    assert a.dtype == H and b.dtype == H and a.shape == b.shape, what
    assert np.array_equal(bits(a), bits(b)), "%s: %d of %d elements differ" % (what, int((bits(a) != bits(b)).sum()), a.size)


def check_bits(L, ref, fmt, up_type, align, n, c, src, dst):
    """criteria (a) - (d) of both commands on one case"""
    ashape, bshape = shapes(fmt, n, c, src, dst)
    for forward in (True, False):
        x, oshape = (data(ashape), bshape) if forward else (data(bshape, 1), ashape)
        cmd = command(forward, up_type, align, src, dst)
        what = "%s %s %s align %d %s -> %s" % ("forward" if forward else "backward", fmt, TYPE[up_type], align, list(ashape), list(bshape))
        s0, n0 = counts(L)
        got = run(L, cmd, x, fill(oshape), fmt)
        assert counts(L) == (s0, n0 + 2), (what, counts(L), (s0, n0))  # (a)
        with key_off(L, KEY):
            s0, n0 = counts(L)
            off = run(L, cmd, x, fill(oshape), fmt)
            assert counts(L) == (s0 + 2, n0), (what, counts(L), (s0, n0))
        same(got, off, what + ", against the key at 0")  # (b)
        same(got, reference(ref, forward, fmt, up_type, align, src, dst, x, oshape), what + ", against the reference")  # (c)
        same(got, run(L, cmd, x, fill(oshape), fmt), what + ", two runs")  # (d)


# ---- 1. bits ------------------------------------------------------------------------------------------------------------------------------------------
CASES = [  # source, output, C
    ((3, 4), (6, 8), 8),       # one vector per row / per pixel
    ((5, 8), (10, 16), 3),     # planar vector, interleaved scalar
    ((4, 6), (7, 9), 16),      # non-integer ratio, planar scalar, two channel vectors per pixel
    ((3, 3), (3, 3), 8),       # identity, ratio 1
    ((2, 5), (2, 10), 8),      # one axis only
    ((8, 8), (32, 32), 8),     # 4x, the widest hit intervals
    ((3, 4), (5, 12), 3),      # width a multiple of 8 plus a tail of 4; planes of 60 halves: plane bases alternate in alignment
    ((1, 1), (4, 8), 8),       # only with align_corners = 0 (a zero ratio otherwise)
]


BITS = [(t, al, s, d, c) for s, d, c in CASES for t, al in MODES if not (al and 1 in s)]  # (a 1-wide source axis with align_corners: test_zero_ratio_keeps_its_route)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("up_type,align,src,dst,c", BITS, ids=["%s-align%d-%dx%d-%dx%d-c%d" % ((TYPE[t], al) + s + d + (c,)) for t, al, s, d, c in BITS])
def test_bits(backend, ref_lib, fmt, up_type, align, src, dst, c):
    check_bits(backend, ref_lib, fmt, up_type, align, 2, c, src, dst)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("up_type,align", MODES)
def test_bits_of_one_image(backend, ref_lib, fmt, up_type, align):
    """a 3-d tensor"""
    check_bits(backend, ref_lib, fmt, up_type, align, None, 8, (5, 8), (10, 16))


@pytest.mark.parametrize("bh", [ROWS - 1, ROWS, ROWS + 1])
@pytest.mark.parametrize("up_type,align", MODES)
def test_bits_at_the_rows_a_planar_lane_walks(backend, ref_lib, bh, up_type, align):
    """UP_ROWS output rows per lane of the planar forward kernels: one row fewer, exactly that many, one more (a second chunk of one row)"""
    check_bits(backend, ref_lib, "NCHW", up_type, align, 2, 3, (2, 4), (bh, 8))


# ---- 2. instances -------------------------------------------------------------------------------------------------------------------------------------
def kernel_names(fmt, up_type, wf, wb):
    lay = fmt.lower()
    return ("upsample_forw|nnc::up_forw_%s_kernel<%s,%d>" % (lay, TYPE[up_type], wf), "upsample_back|nnc::up_back_%s_kernel<%s,%d>" % (lay, TYPE[up_type], wb))


def instance(L, fmt, up_type, align, c, src, dst, misaligned=False, key=1):
    """the launch records of the forward and the backward command of one case"""
    ashape, bshape = shapes(fmt, 2, c, src, dst)
    out = []
    for forward in (True, False):
        x, oshape = (data(ashape), bshape) if forward else (data(bshape, 1), ashape)
        cmd = command(forward, up_type, align, src, dst)
        if misaligned and fmt == "NHWC":
            xt, ot = aliased(L, [x, fill(oshape)], 1)
            assert xt.ptr % 16 == 2 and ot.ptr % 16 == 2
        elif misaligned:  # (aliased() makes NHWC tensors)
            (xt,) = make_tensors(L, nnc.GPU_MEMORY, [np.concatenate([np.zeros(1, H), x.ravel(), np.zeros(7, H)])], fmt)
            (ot,) = make_tensors(L, nnc.GPU_MEMORY, [np.full(int(np.prod(oshape)) + 8, 3, H)], fmt)
            xt, ot = xt.alias(x.shape, 1), ot.alias(oshape, 1)
            assert xt.ptr % 16 == 2 and ot.ptr % 16 == 2
        else:
            (xt,) = make_tensors(L, nnc.GPU_MEMORY, [x], fmt)
            (ot,) = make_tensors(L, nnc.GPU_MEMORY, [fill(oshape)], fmt)
            assert xt.ptr % 16 == 0 and ot.ptr % 16 == 0
        L.tune_set(KEY, key)
        try:
            s0, n0 = counts(L)
            r, names = records(L, lambda: L.cmd_exec(cmd, nnc.NO_HINT, 0, [xt], [ot]))
        finally:
            L.tune_set(KEY, 1)
        assert r == 0 and counts(L) == (s0, n0 + 2) and len(names) == 1, names
        assert L.dll.nnc_mi355x_last_kernel_name().decode() == "up_%s_%s" % ("forw" if forward else "back", fmt.lower())  # a literal of the library
        with key_off(L, KEY):
            (o2,) = make_tensors(L, nnc.GPU_MEMORY, [fill(oshape)], fmt)
            assert L.cmd_exec(cmd, nnc.NO_HINT, 0, [xt], [o2]) == 0
        same(ot.numpy(), o2.numpy(), "%s %s, misaligned %d" % (names[0], fmt, misaligned))
        out.append(names[0])
    return tuple(out)


@pytest.mark.parametrize("up_type,align", MODES)
def test_instances(backend, up_type, align):
    """Interleaved: eight channels per lane where C % 8 == 0 on aligned bases.  Planar: only the nearest forward kernel has a vector instance (BW % 8 == 0, aligned);
    bilinear forward and both backward kernels run a lane per element (upsample_ops.h, up_vector_width)."""
    L = backend
    L.dll.nnc_mi355x_last_kernel_name.restype = nnc.C.c_char_p
    pv = 8 if up_type == 0 else 1  # the planar forward instance on aligned rows of whole vectors
    assert instance(L, "NCHW", up_type, align, 8, (3, 4), (6, 8)) == kernel_names("NCHW", up_type, pv, 1)
    assert instance(L, "NCHW", up_type, align, 3, (5, 8), (10, 16)) == kernel_names("NCHW", up_type, pv, 1)
    assert instance(L, "NCHW", up_type, align, 16, (4, 6), (7, 9)) == kernel_names("NCHW", up_type, 1, 1)  # BW = 9
    assert instance(L, "NCHW", up_type, align, 3, (3, 4), (5, 12)) == kernel_names("NCHW", up_type, 1, 1)  # BW = 12: every other row starts 8 bytes off
    assert instance(L, "NHWC", up_type, align, 8, (3, 4), (6, 8)) == kernel_names("NHWC", up_type, 8, 8)
    assert instance(L, "NHWC", up_type, align, 16, (4, 6), (7, 9)) == kernel_names("NHWC", up_type, 8, 8)
    assert instance(L, "NHWC", up_type, align, 3, (5, 8), (10, 16)) == kernel_names("NHWC", up_type, 1, 1)  # C = 3
    # bases moved by one half: the scalar instances, the same bits
    assert instance(L, "NCHW", up_type, align, 3, (5, 8), (10, 16), True) == kernel_names("NCHW", up_type, 1, 1)
    assert instance(L, "NHWC", up_type, align, 8, (3, 4), (6, 8), True) == kernel_names("NHWC", up_type, 1, 1)
    # the measurement value of the key: the scalar instances everywhere, the same bits
    assert instance(L, "NCHW", up_type, align, 3, (5, 8), (10, 16), key=2) == kernel_names("NCHW", up_type, 1, 1)
    assert instance(L, "NHWC", up_type, align, 8, (3, 4), (6, 8), key=2) == kernel_names("NHWC", up_type, 1, 1)


def plan(L, nchw, n, c, src, dst, up_type, align):
    f = L.dll.nnc_mi355x_debug_upsample_plan
    f.restype, f.argtypes = nnc.C.c_int, [nnc.C.c_int, nnc.C.POINTER(nnc.C.c_int), nnc.C.c_int, nnc.C.c_int]
    return f(int(nchw), (nnc.C.c_int * 6)(n, c, src[0], src[1], dst[0], dst[1]), up_type, align)


def test_plan_arithmetic(backend):
    """The plan on extents alone (nothing is allocated): widths, the refusals that are arithmetic, and the 2^31-element boundary of the 32-bit indices."""
    L = backend
    for up_type, align in MODES:
        pv = 8 if up_type == 0 else 1  # planar: only the nearest forward kernel has a vector instance
        assert plan(L, 1, 2, 8, (3, 4), (6, 8), up_type, align) == pv + 16 * 1
        assert plan(L, 1, 2, 3, (5, 8), (10, 16), up_type, align) == pv + 16 * 1
        assert plan(L, 1, 2, 16, (4, 6), (7, 9), up_type, align) == 1 + 16 * 1
        assert plan(L, 0, 2, 16, (4, 6), (7, 9), up_type, align) == 8 + 16 * 8
        assert plan(L, 0, 2, 3, (5, 8), (10, 16), up_type, align) == 1 + 16 * 1
        assert plan(L, 1, 2, 8, (6, 8), (3, 4), up_type, align) == 0      # a ratio above 1
        assert plan(L, 1, 2, 8, (3, 4), (6, 3), up_type, align) == 0      # ... on one axis
        assert (plan(L, 1, 2, 8, (1, 4), (4, 8), up_type, align) == 0) == bool(align)  # a zero ratio
        # 32768 planes of 256 x 256 outputs are 2^31 elements
        assert plan(L, 1, 1, 32768, (128, 128), (256, 256), up_type, align) == 0 and plan(L, 0, 1, 32768, (128, 128), (256, 256), up_type, align) == 0
        assert plan(L, 1, 1, 32767, (128, 128), (256, 256), up_type, align) == pv + 16 * 1 and plan(L, 0, 32767, 8, (64, 64), (64, 128), up_type, align) == 8 + 16 * 8
        assert plan(L, 0, 32768, 8, (64, 64), (64, 128), up_type, align) == 0
    assert plan(L, 1, 2, 8, (3, 4), (6, 8), 2, 0) == 0 and plan(L, 1, 2, 8, (3, 4), (6, 8), -1, 0) == 0  # a type that is neither


# ---- 3. several trips per lane ------------------------------------------------------------------------------------------------------------------------
TRIPS = [("NCHW", True, 1), ("NCHW", False, 1), ("NHWC", True, 1), ("NHWC", False, 1), ("NCHW", True, 0)]  # (the last: the planar vector instance, nearest forward)


@pytest.mark.parametrize("fmt,forward,up_type", TRIPS, ids=["%s-%s-%s" % (f, "forward" if d else "backward", TYPE[t]) for f, d, t in TRIPS])
def test_several_trips_per_lane(backend, ref_lib, fmt, forward, up_type):
    """GRID_WG_PER_CU = 1: 256 workgroups of UP_THREADS lanes, and more work items than that in every instance, so lanes come round again -- with another
    column group, row and plane.  2x."""
    L = backend
    n, c, src, dst = 2, 72, (64, 64), (128, 128)
    lanes = CUS * THREADS
    wf, wb = (8 if up_type == 0 else 1, 1) if fmt == "NCHW" else (8, 8)  # (planar bilinear and backward: a lane per element)
    items = {("NCHW", True): n * c * (dst[0] // ROWS) * (dst[1] // wf), ("NCHW", False): n * c * src[0] * src[1],
             ("NHWC", True): n * dst[0] * dst[1] * (c // 8), ("NHWC", False): n * src[0] * src[1] * (c // 8)}[(fmt, forward)]
    assert items > lanes, (items, lanes)
    ashape, bshape = shapes(fmt, n, c, src, dst)
    x, oshape = (data(ashape), bshape) if forward else (data(bshape, 1), ashape)
    cmd = command(forward, up_type, 0, src, dst)
    what = "%s %s" % (fmt, "forward" if forward else "backward")
    with key_off(L, KEY):
        off = run(L, cmd, x, fill(oshape), fmt)
    old = L.tune_get("GRID_WG_PER_CU")
    L.tune_set("GRID_WG_PER_CU", 1)
    try:
        s0, n0 = counts(L)
        got, names = records(L, lambda: run(L, cmd, x, fill(oshape), fmt))
        assert counts(L) == (s0, n0 + 2) and names == [kernel_names(fmt, up_type, wf, wb)[0 if forward else 1]], names
        again = run(L, cmd, x, fill(oshape), fmt)
    finally:
        L.tune_set("GRID_WG_PER_CU", old)
    same(got, off, what + ", against the key at 0")
    same(got, reference(ref_lib, forward, fmt, up_type, 0, src, dst, x, oshape), what + ", against the reference")
    same(got, again, what + ", two runs")


# ---- 4. routes and refusals ---------------------------------------------------------------------------------------------------------------------------
def test_key_is_on(backend):
    assert backend.tune_get(KEY) == 1


def staged_like_key_off(L, fn, halves, what):
    """fn() -> (return value, output or None): staged as before, the return value and the bits of the key at 0, no native record"""
    with key_off(L, KEY):
        s0, n0 = counts(L)
        r_off, off = fn()
        assert counts(L) == (s0 + halves, n0), (what, counts(L), (s0, n0))
    s0, n0 = counts(L)
    (r, got), names = records(L, fn)
    assert counts(L) == (s0 + halves, n0), (what, counts(L), (s0, n0))
    assert r == r_off, (what, r, r_off)
    assert not any("nnc::up_" in x for x in names), names
    if r == 0:
        assert got.dtype == off.dtype and np.array_equal(bits(got), bits(off)), what
    return r, got, names


@pytest.mark.parametrize("fmt", FMTS)
def test_refusals_keep_their_route_and_their_results(backend, fmt):
    L = backend
    src, dst, c = (5, 8), (10, 16), 8
    ashape, bshape = shapes(fmt, 2, c, src, dst)
    a, g = data(ashape), data(bshape, 1)
    for up_type, align in MODES:
        fwd, bwd = command(True, up_type, align, src, dst), command(False, up_type, align, src, dst)

        def view_in():  # the input is a view (dense strides) into a larger allocation
            (t,) = make_tensors(L, nnc.GPU_MEMORY, [np.concatenate([np.zeros(8, H), a.ravel(), np.zeros(8, H)])], fmt)
            strides = tuple(int(np.prod(ashape[k + 1:])) for k in range(4))
            (o,) = make_tensors(L, nnc.GPU_MEMORY, [fill(bshape)], fmt)
            return L.cmd_exec(fwd, nnc.NO_HINT, 0, [t.view(ashape, strides, 8)], [o]), o.numpy()

        r, got, _ = staged_like_key_off(L, view_in, 2, "a view operand")
        assert r == 0
        with key_off(L, KEY):
            same(got, run(L, fwd, a, fill(bshape), fmt), "a view operand")

        def accumulate(cmd, x, oshape):
            return lambda: exec_on(L, nnc.GPU_MEMORY, cmd, nnc.NO_HINT, nnc.ACCUMULATE_OUTPUT, [x], [fill(oshape)], fmt)

        for cmd, x, oshape in ((fwd, a, bshape), (bwd, g, ashape)):
            r, got, _ = staged_like_key_off(L, lambda: (lambda t: (t[0], t[1][0]))(accumulate(cmd, x, oshape)()), 2, "ACCUMULATE_OUTPUT")
            assert r == 0
            # half in, fp32 out
            mixed = lambda: (lambda t: (t[0], t[1][0]))(exec_on(L, nnc.GPU_MEMORY, cmd, nnc.NO_HINT, 0, [x], [fill(oshape, F)], fmt))
            r, got, _ = staged_like_key_off(L, mixed, 1, "a half input with an fp32 output")
            assert r == 0 and got.dtype == F
        # a shrinking ratio: refused with the key at either value
        shrink = lambda: (exec_on(L, nnc.GPU_MEMORY, command(True, up_type, align, dst, src), nnc.NO_HINT, 0, [g], [fill(ashape)], fmt)[0], None)
        r, _, _ = staged_like_key_off(L, shrink, 2, "a shrinking ratio")
        assert r == -1


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("up_type", [0, 1])
def test_zero_ratio_keeps_its_route(backend, fmt, up_type):
    """align_corners = 1 with a 1-wide source axis (forward only): the route and the bits of the key at 0"""
    L = backend
    for src, dst in (((1, 4), (4, 8)), ((3, 1), (6, 8)), ((1, 1), (4, 8))):
        ashape, bshape = shapes(fmt, 2, 8, src, dst)
        fn = lambda: (lambda t: (t[0], t[1][0]))(exec_on(L, nnc.GPU_MEMORY, command(True, up_type, 1, src, dst), nnc.NO_HINT, 0, [data(ashape)], [fill(bshape)], fmt))
        r, _, _ = staged_like_key_off(L, fn, 2, "a zero ratio %s" % (src,))
        assert r == 0


@pytest.mark.parametrize("fmt", FMTS)
def test_fp32_commands_keep_their_kernels(backend, ref_lib, fmt):
    L = backend
    src, dst = (5, 8), (10, 16)
    ashape, bshape = shapes(fmt, 2, 8, src, dst)
    for up_type, align in MODES:
        for forward in (True, False):
            x, oshape = (data(ashape).astype(F), bshape) if forward else (data(bshape, 1).astype(F), ashape)
            cmd = command(forward, up_type, align, src, dst)
            s0, n0 = counts(L)
            got, names = records(L, lambda: run(L, cmd, x, fill(oshape, F), fmt))
            assert counts(L) == (s0, n0)
            assert names == ["upsample_forw|nnc::upsample_forw_kernel" if forward else "upsample_back|nnc::upsample_back_kernel"], names
            want = ref_run(ref_lib, cmd, [x], [np.zeros(oshape, F)], fmt)[0]
            assert got.dtype == F and np.array_equal(bits(got), bits(want))
