"""INDEX_SELECT_FORWARD / BACKWARD and PAD_FORWARD / BACKWARD on dense CCV_16F tensors without fp32 images (ccv_amd/csrc/index_ops.h; tunable
INDEX_PAD_HALF_NATIVE), and the ordered scatter-add of both types on the tile kernel (tunable INDEX_BACK_TILES).

Every native result is compared bit for bit with the command under the key at 0 (fp32 images) and with the reference's CPU backend on the widened inputs rounded once
by .astype(float16).  The reference's own half scatter-add rounds after every add, so it is not the oracle; the contract is: per (destination row, column) the
sum starts at +0.f, adds the sources in ascending source-row order in fp32, and is rounded once.  The one tolerance in this file is on fp32-index gathers, whose
fp32 kernel is not bit-pinned to the reference (tests/test_parity_act_opt.py::test_index_select allows 1e-6): there the result must be within
half_bound(want, |a0 w0| + |a1 w1|) of the float64 value -- one rounding to half plus sixteen fp32 ulps of the terms (test_mbconv_half.half_bound).
Inputs are U(-2, 2) exact halves; outputs are pre-filled with 3.
"""
import os
import re
import numpy as np
import pytest
from ccv_amd import nnc
from harness import make_tensors
from test_mbconv_half import counts, records, key_off, bits, ref_run, aliased, half_bound, within

F, H, D, I = np.float32, np.float16, np.float64, np.int32
KEY, TILES = "INDEX_PAD_HALF_NATIVE", "INDEX_BACK_TILES"

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccv_amd", "csrc", "index_ops.h")
with open(_HDR) as _f:
    _TEXT = _f.read()
TR, CHUNK = (int(re.search(r"constexpr int %s = (\d+);" % k, _TEXT).group(1)) for k in ("IDX_TILE_ROWS", "IDX_CHUNK"))

FWD, BWD = nnc.generic_cmd("INDEX_SELECT_FORWARD"), nnc.generic_cmd("INDEX_SELECT_BACKWARD")
COLS = [1, 3, 8, 16, 130, 136]  # 1: a 1-d tensor; 8, 16, 136: whole vectors of eight halves; 130, 136: more than one trip of a wave over a row
ROWS = 20

_DATA = {}


def data(shape, seed=0, dtype=H):
    """U(-2, 2) exact halves, made once per (shape, seed), read-only"""
    key = (tuple(shape), seed, dtype)
    if key not in _DATA:
        rng = np.random.default_rng(3000 + seed + 7 * int(np.prod(shape)) + len(shape))
        x = ((rng.random(shape) - 0.5) * 4).astype(H).astype(dtype)
        x.setflags(write=False)
        _DATA[key] = x
    return _DATA[key]


def shape2(rows, cols):
    return (rows,) if cols == 1 else (rows, cols)


def fill(shape, dtype=H):
    return np.full(shape, 3, dtype)


def same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert np.array_equal(bits(a), bits(b)), "%s: %d of %d elements differ" % (what, int((bits(a) != bits(b)).sum()), a.size)


def execute(L, cmd, ins, out, misaligned=False, flags=0):
    """half arrays one element off a 16-byte boundary where asked; -> (return value, output)"""
    def tensor(x):
        if x is None:
            return None
        if x.size == 0:  # a tensor of no elements: all extents zero, over memory of its own
            (t,) = make_tensors(L, nnc.GPU_MEMORY, [np.zeros(8, x.dtype)])
            return t.alias((0,), 0)
        if misaligned and x.dtype == H:
            (t,) = aliased(L, [x], 1)
            assert t.ptr % 16 == 2
            return t
        (t,) = make_tensors(L, nnc.GPU_MEMORY, [x])
        assert t.ptr % 16 == 0
        return t
    it, ot = [tensor(x) for x in ins], tensor(out)
    r = L.cmd_exec(cmd, nnc.NO_HINT, flags, it, [ot])
    return r, ot.numpy() if out.size else out


def check(L, cmd, ins, oshape, name, want, misaligned=False, bound=None):
    """criteria (a) - (e) on one case.  want: half(reference(float(x))), or the float64 value with `bound`"""
    what = "%s %s -> %s%s" % (name, [None if x is None else list(x.shape) for x in ins], list(oshape), ", misaligned" if misaligned else "")
    s0, n0 = counts(L)
    (r, got), names = records(L, lambda: execute(L, cmd, ins, fill(oshape), misaligned))
    assert r == 0, (what, r)
    assert counts(L) == (s0, n0 + 2), (what, counts(L), (s0, n0))  # (a)
    assert names == ([name] if got.size else []), (what, names)  # (e)
    with key_off(L, KEY):
        s0, n0 = counts(L)
        r, off = execute(L, cmd, ins, fill(oshape), misaligned)
        assert r == 0 and counts(L) == (s0 + 2, n0), (what, r, counts(L), (s0, n0))
    same(got, off, what + ", against the key at 0")  # (b)
    if bound is None:
        same(got, want, what + ", against the reference")  # (c)
    else:
        print(what, "worst error / bound", float((np.abs(got.astype(D) - want) / bound).max()))
        within(got, want, bound, what)
    r, again = execute(L, cmd, ins, fill(oshape), misaligned)
    same(got, again, what + ", two runs")  # (d)
    return got


# ---- 1. gather ------------------------------------------------------------------------------------------------------------------------------------------
IDX = np.array([0, 19, 5, 7, 5, 3, 12, 19, 1, 8, 0], I)  # a repeat, the first and the last row
FIDX = np.array([0.0, 19.0, 5.25, 7.5, 5.25, 18.75, 12.125, 0.5, 1.0, 8.875, 18.0], F)  # the last row itself (its upper neighbour is clamped) and the row below it


def gather_name(w, f32):
    return "index_select_forw|nnc::index_gather_kernel<half,%d,%s>" % (w, "f32" if f32 else "i32")


def lerp64(a, fidx):
    """(want, S): the float64 value of the interpolation with the fp32 kernel's fp32 weights, and the sum of the magnitudes of its terms"""
    j0 = fidx.astype(I)
    j1 = np.minimum(j0 + 1, a.shape[0] - 1)
    w1 = (fidx - j0.astype(F)).astype(F)
    w0 = (F(1) - w1).astype(F)
    sh = (-1,) + (1,) * (a.ndim - 1)
    t0, t1 = a[j0].astype(D) * w0.astype(D).reshape(sh), a[j1].astype(D) * w1.astype(D).reshape(sh)
    return t0 + t1, np.abs(t0) + np.abs(t1)


_REF = {}


def reference(ref, key, cmd, ins, oshape):
    """half(reference(float(x))): computed once per case, read-only"""
    if key not in _REF:
        r = ref_run(ref, cmd, ins, [np.zeros(oshape, H)])[0].astype(H)
        r.setflags(write=False)
        _REF[key] = r
    return _REF[key]


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("cols", COLS)
def test_gather(backend, ref_lib, cols, misaligned):
    a, oshape = data(shape2(ROWS, cols)), shape2(len(IDX), cols)
    w = 8 if cols % 8 == 0 and not misaligned else 1
    got = check(backend, FWD, [a, IDX], oshape, gather_name(w, False), reference(ref_lib, ("gather", cols), FWD, [a, IDX], oshape), misaligned)
    same(got, a[IDX], "a copy of rows")
    want, s = lerp64(a, FIDX)
    check(backend, FWD, [a, FIDX], oshape, gather_name(w, True), want, misaligned, bound=half_bound(want, s))


def test_gather_of_no_rows(backend):
    """zero indices: nothing is launched, nothing is written"""
    check(backend, FWD, [data((ROWS,)), np.zeros(0, I)], (0,), gather_name(1, False), np.zeros(0, H))


# ---- 2. ordered scatter-add -----------------------------------------------------------------------------------------------------------------------------
def scatter_name(t, w):
    return "index_select_back|nnc::index_scatter_tile_kernel<%s,%d>" % (t, w)


def scatter(L, ref, key, g, idx, h_rows, cols, misaligned=False):
    hshape = shape2(h_rows, cols)
    w = 8 if cols % 8 == 0 and not misaligned else 1
    want = reference(ref, ("scatter",) + key, BWD, [g, None, idx], hshape) if len(idx) else np.zeros(hshape, H)  # (the reference asserts on a tensor of no indices)
    got = check(L, BWD, [g, None, idx], hshape, scatter_name("half", w), want, misaligned)
    unnamed = np.setdiff1d(np.arange(h_rows), idx)
    assert not bits(got[unnamed]).any(), "rows no index names are +0"
    return got


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("cols", COLS)
def test_scatter_add(backend, ref_lib, cols, misaligned):
    scatter(backend, ref_lib, (cols, "idx"), data(shape2(len(IDX), cols), 1), IDX, ROWS, cols, misaligned)


def boundary_indices(h_rows, skip_middle):
    """rows on both sides of every tile boundary inside h, each named more than once; skip_middle: the second tile is not named at all"""
    rows = [r for r in (0, TR - 1, TR, 2 * TR - 1, 2 * TR) if r < h_rows and not (skip_middle and TR <= r < 2 * TR)]
    return np.array((rows + rows[::-1] + rows)[:13], I)


BOUNDARY = [(TR - 1, False), (TR, False), (TR + 1, False), (2 * TR + 1, False), (2 * TR + 1, True)]


@pytest.mark.parametrize("h_rows,skip_middle", BOUNDARY, ids=["%d%s" % (h, "-skip" if s else "") for h, s in BOUNDARY])
def test_scatter_add_at_tile_boundaries(backend, ref_lib, h_rows, skip_middle):
    idx = boundary_indices(h_rows, skip_middle)
    for cols in (8, 3):
        got = scatter(backend, ref_lib, ("boundary", h_rows, skip_middle, cols), data(shape2(len(idx), cols), 2), idx, h_rows, cols)
        if skip_middle:
            assert not bits(got[TR:2 * TR]).any(), "a tile no index names is all zeros over the 3s"


@pytest.mark.parametrize("sources", [CHUNK - 1, CHUNK, CHUNK + 1])
def test_scatter_add_at_chunk_boundaries(backend, ref_lib, sources):
    """the indices a wave examines per step: one fewer, exactly that many, one more (a second step of one index)"""
    idx = np.random.default_rng(sources).integers(0, ROWS, sources).astype(I)
    idx[-1] = ROWS - 1  # the last source is seen
    idx[0] = 0
    scatter(backend, ref_lib, ("chunk", sources), data((sources, 8), 3), idx, ROWS, 8)


HOT = 300


_HOT = []


def hot_case():
    """300 rows of eight U(-2, 2) halves whose fp32 sum in source order and in reversed order round to different halves in some element.  fp32 sums of 300 such
    values differ by an ulp or two with the order, and a half has 13 bits fewer, so most draws do not show it: the first seed that does is taken (a few
    thousand draws of 2400 values), and the property is then checked with plain fp32 adds, one source at a time."""
    if not _HOT:
        for seed in range(100000):
            g = ((np.random.default_rng(4000 + seed).random((HOT, 8)) - 0.5) * 4).astype(H)
            up = g.astype(F)
            if (bits(np.cumsum(up, axis=0, dtype=F)[-1].astype(H)) != bits(np.cumsum(up[::-1], axis=0, dtype=F)[-1].astype(H))).any():
                break
        fwd, rev = np.zeros(8, F), np.zeros(8, F)
        for i in range(HOT):
            fwd, rev = fwd + g[i].astype(F), rev + g[HOT - 1 - i].astype(F)
        assert (bits(fwd.astype(H)) != bits(rev.astype(H))).any(), "the case does not test order"
        g.setflags(write=False)
        _HOT.append((g, np.full(HOT, 5, I), fwd.astype(H)))
    return _HOT[0]


def test_scatter_add_hot_row_keeps_the_order(backend, ref_lib):
    """300 sources into one row: the sum in source order, which a reversed sum of the same data does not equal after rounding to half (checked first)"""
    g, idx, want = hot_case()
    got = scatter(backend, ref_lib, ("hot",), g, idx, ROWS, 8)
    scatter(backend, ref_lib, ("hot",), g, idx, ROWS, 8, True)  # the scalar instance
    same(got[5], want, "the sum in ascending source order")


def test_scatter_add_equal_rows_in_one_wave_and_across_two(backend, ref_lib):
    """65 sources cycling over 3 rows: equal destinations among the 64 indices of one load and in the next"""
    idx = (np.arange(65) % 3 + TR - 1).astype(I)  # rows on both sides of a tile boundary
    scatter(backend, ref_lib, ("cycle",), data((65, 8), 5), idx, ROWS, 8)


def test_scatter_add_of_no_sources(backend):
    """g_rows = 0: h is all zeros"""
    got = check(backend, BWD, [np.zeros(0, H), None, np.zeros(0, I)], (ROWS,), scatter_name("half", 1), np.zeros(ROWS, H))
    assert not bits(got).any()


# ---- 3. INDEX_BACK_TILES ----------------------------------------------------------------------------------------------------------------------------------
def tiles_cases():
    out = [(data((len(i), 8), 2), i, h) for h, s in BOUNDARY for i in [boundary_indices(h, s)]]
    g, idx, _ = hot_case()
    return out + [(g, idx, ROWS)]


@pytest.mark.parametrize("dtype", [F, H], ids=["fp32", "half"])
def test_back_tiles_key(backend, ref_lib, dtype):
    """fp32 and half backward at INDEX_BACK_TILES 0 and 1: the same bits; index_scatter_add_kernel at 0 only (a half command then keeps its fp32 images)"""
    L = backend
    assert L.tune_get(TILES) == 1 and L.tune_get(KEY) == 1
    old = "index_select_back|nnc::index_scatter_add_kernel"
    for g, idx, h_rows in tiles_cases():
        g = g.astype(dtype)
        s0, n0 = counts(L)
        (r, on), names = records(L, lambda: execute(L, BWD, [g, None, idx], fill((h_rows, 8), dtype)))
        assert r == 0 and names == [scatter_name("half", 8) if dtype == H else scatter_name("float", 4)], names
        assert counts(L) == ((s0, n0 + 2) if dtype == H else (s0, n0))
        with key_off(L, TILES):
            s0, n0 = counts(L)
            (r, off), names = records(L, lambda: execute(L, BWD, [g, None, idx], fill((h_rows, 8), dtype)))
            assert r == 0 and names == [old], names
            assert counts(L) == ((s0 + 2, n0) if dtype == H else (s0, n0))
        same(on, off, "INDEX_BACK_TILES 1 against 0, %d rows" % h_rows)
        want = ref_run(ref_lib, BWD, [g, None, idx], [np.zeros((h_rows, 8), dtype)])[0].astype(dtype)
        same(on, want, "against the reference")


def test_fp32_scatter_add_scalar_instance(backend, ref_lib):
    """fp32 columns that are no multiple of four: the scalar instance of the tile kernel, the bits of the reference"""
    L = backend
    g = data((len(IDX), 3), 1, F)
    (r, got), names = records(L, lambda: execute(L, BWD, [g, None, IDX], fill((ROWS, 3), F)))
    assert r == 0 and names == [scatter_name("float", 1)], names
    same(got, ref_run(ref_lib, BWD, [g, None, IDX], [np.zeros((ROWS, 3), F)])[0], "against the reference")


# ---- 4. pad -----------------------------------------------------------------------------------------------------------------------------------------------
PADS = [  # shape, begin, end, vector instance for (zero, replicate)
    ((5,), (2,), (3,), (1, 1)), ((3, 4), (1, 0), (0, 2), (1, 1)), ((2, 3, 4), (0, 1, 2), (1, 0, 1), (1, 1)), ((2, 3, 4, 5), (1, 1, 0, 2), (0, 2, 1, 1), (1, 1)),  # test_pad's
    ((2, 3, 4, 16), (0, 1, 1, 8), (0, 0, 1, 8), (8, 1)),   # whole vectors on the innermost axis: the vector instance for zero; a replicated edge is one element
    ((2, 3, 4, 16), (0, 1, 1, 0), (0, 1, 0, 0), (8, 8)),   # nothing padded on the innermost axis: the vector instance for both
    ((2, 3, 4, 16), (0, 0, 0, 4), (0, 0, 0, 4), (1, 1)),   # begin[3] is no multiple of 8
]


@pytest.mark.parametrize("pad_type", [0, 1], ids=["zero", "replicate"])
@pytest.mark.parametrize("shape,begin,end,w", PADS, ids=["x".join(map(str, p[0])) + "+" + "".join(map(str, p[1])) + "+" + "".join(map(str, p[2])) for p in PADS])
def test_pad(backend, ref_lib, pad_type, shape, begin, end, w):
    a = data(shape, 6)
    oshape = tuple(d + b + e for d, b, e in zip(shape, begin, end))
    cmd = nnc.CMD_PAD("PAD_FORWARD", pad_type, begin, end)
    name = "pad_forw|nnc::pad_forw_kernel<half,%d,%s>" % (w[pad_type], "replicate" if pad_type else "zero")
    got = check(backend, cmd, [a], oshape, name, reference(ref_lib, ("pad", pad_type, shape, begin, end), cmd, [a], oshape))
    if pad_type == 0:
        inner = tuple(slice(b, b + d) for b, d in zip(begin, shape))
        rest = got.copy()
        rest[inner] = 0
        assert not bits(rest).any(), "zero fill is +0"
        g = data(oshape, 7)
        cmd = nnc.CMD_PAD("PAD_BACKWARD", pad_type, begin, end)
        check(backend, cmd, [g], shape, "pad_back|nnc::pad_back_kernel<half,%d>" % w[0], reference(ref_lib, ("crop", shape, begin, end), cmd, [g], shape))
        if w[0] == 8:  # one element off 16 bytes: the scalar instances
            check(backend, cmd, [g], shape, "pad_back|nnc::pad_back_kernel<half,1>", reference(ref_lib, ("crop", shape, begin, end), cmd, [g], shape), True)
    if w[pad_type] == 8:
        cmd = nnc.CMD_PAD("PAD_FORWARD", pad_type, begin, end)
        check(backend, cmd, [a], oshape, "pad_forw|nnc::pad_forw_kernel<half,1,%s>" % ("replicate" if pad_type else "zero"), reference(ref_lib, ("pad", pad_type, shape, begin, end), cmd, [a], oshape), True)


# ---- 5. kept routes ---------------------------------------------------------------------------------------------------------------------------------------
def test_keys_are_on(backend):
    assert backend.tune_get(KEY) == 1 and backend.tune_get(TILES) == 1


def staged(L, fn, halves, what):
    """fn() -> (return value, output): success, `halves` tensors through fp32 images, none handed over as halves, no record of a half instance"""
    s0, n0 = counts(L)
    (r, got), names = records(L, fn)
    assert r == 0, (what, r)
    assert counts(L) == (s0 + halves, n0), (what, counts(L), (s0, n0))
    assert not any("<half" in x for x in names), (what, names)
    return got


def test_kept_routes(backend, ref_lib):
    L = backend
    cols = 8
    a, g = data((ROWS, cols)), data((len(IDX), cols), 1)
    want_b = reference(ref_lib, ("gather", cols), FWD, [a, IDX], (len(IDX), cols))
    want_h = reference(ref_lib, ("scatter", cols, "idx"), BWD, [g, None, IDX], (ROWS, cols))

    def into_a_view():  # b is a view: rows of `cols` elements at a stride of cols + 8
        (at, it) = make_tensors(L, nnc.GPU_MEMORY, [a, IDX])
        (parent,) = make_tensors(L, nnc.GPU_MEMORY, [fill((len(IDX), cols + 8))])
        r = L.cmd_exec(FWD, nnc.NO_HINT, 0, [at, it], [parent.view((len(IDX), cols), (cols + 8, 1), 0)])
        return r, parent.numpy()

    got = staged(L, into_a_view, 2, "a view of b")
    same(got[:, :cols], want_b, "a view of b")
    same(got[:, cols:], fill((len(IDX), 8)), "what lies between the view's rows")
    for cmd, ins, oshape, want in ((FWD, [a, IDX], (len(IDX), cols), want_b), (BWD, [g, None, IDX], (ROWS, cols), want_h)):
        got = staged(L, lambda: execute(L, cmd, ins, fill(oshape), flags=nnc.ACCUMULATE_OUTPUT), 2, "ACCUMULATE_OUTPUT")
        same(got, want, "ACCUMULATE_OUTPUT")
    got = staged(L, lambda: execute(L, BWD, [g, None, IDX], fill((ROWS, cols), F)), 1, "half g into fp32 h")
    same(got, ref_run(ref_lib, BWD, [g, None, IDX], [np.zeros((ROWS, cols), F)])[0], "half g into fp32 h")
    # pad under accumulation keeps its fp32 images too
    cmd = nnc.CMD_PAD("PAD_FORWARD", 0, (0, 1), (1, 0))
    got = staged(L, lambda: execute(L, cmd, [a], fill((ROWS + 1, cols + 1)), flags=nnc.ACCUMULATE_OUTPUT), 2, "pad, ACCUMULATE_OUTPUT")
    same(got, reference(ref_lib, ("pad-acc",), cmd, [a], (ROWS + 1, cols + 1)), "pad, ACCUMULATE_OUTPUT")
