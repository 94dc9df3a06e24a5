"""Gradient clipping and the NaN check on dense CCV_16F gradients without fp32 images (ccv_amd/csrc/grad_ops.h; tunable GRAD_HALF_NATIVE): whole-tensor
REDUCE_NORM2_FORWARD and REDUCE_ISNAN_FORWARD, MUL_FORWARD of a half tensor by a one-element tensor.

Every accepted case is held to
  (a) nnc_mi355x_debug_half_counts: the native count rises by the number of half tensors handed over, the staged count does not move;
  (b) the launch records: one launch of grad_reduce_kernel up to GRAD_ONE_WG_MAX elements, that and grad_fold_kernel above, exactly one of ew_map_kernel<GScale> for MUL;
  (c) two runs agree bit for bit.
NORM2 numerics:
  1. coverage, exact: zeros and ONE element v -> exactly |v| (a dropped element reads 0, a doubled one sqrt(2) |v|), v at every edge of the kernel's geometry;
  2. order-free: integer-valued halves with S = sum x^2 < 2^20: every fp32 partial sum is exact in any order, so |got - sqrt(S)| <= 2 x 2^-24 sqrt(S) (sqrtf, and
     S -> float64 sqrt) and got is bit for bit the GRAD_HALF_NATIVE = 0 result;
  3. general data: U(-2, 2) halves; n non-negative exact terms summed in fp32 in ANY order have a relative error of at most (n - 1) 2^-24, the square root halves
     it and adds one rounding: the bound (n + 2) 2^-24 want (+ 2^-11 want + 2^-24 for a half result) holds for the native route, the key-off route and the
     reference's CPU backend alike.  Loose at large n by construction: 1 and 2 carry the sharpness (test_wrong_expectations_break_the_bounds).
Outputs are pre-filled with 3.
"""
import os
import re
import numpy as np
import pytest
from ccv_amd import nnc
from harness import make_tensors
from test_mbconv_half import counts, records, key_off, bits, within, ref_run, aliased

F, H, D, I = np.float32, np.float16, np.float64, np.int32
KEY = "GRAD_HALF_NATIVE"
U = 2.0 ** -24

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccv_amd", "csrc", "grad_ops.h")
with open(_HDR) as _f:
    _TEXT = _f.read()
ONE_WG, THREADS, TILE = (int(re.search(r"constexpr int %s = (\d+);" % k, _TEXT).group(1)) for k in ("GRAD_ONE_WG_MAX", "GRAD_THREADS", "GRAD_TILE"))
WG = TILE * THREADS * 8  # elements a workgroup of the first stage takes

BIG = max(ONE_WG, 2 * WG) + WG // 2 + 3
SHAPE4, SHAPE2 = (3, 5, 7, 11), (37, 29)
SHAPES = [(1,), (7,), (8,), (9,), (ONE_WG - 1,), (ONE_WG,), (ONE_WG + 1,), (BIG,), SHAPE4, SHAPE2]
CASES = [(s, m) for s in SHAPES for m in (False, True)]
IDS = ["%s%s" % ("x".join(map(str, s)), "-misaligned" if m else "") for s, m in CASES]
with open(os.path.join(os.path.dirname(_HDR), "ew_map.h")) as _f:
    _EW = _f.read()
EW_WG = 8 * int(re.search(r"constexpr int EW_THREADS = (\d+);", _EW).group(1)) * int(re.search(r"constexpr int EW_TILE = (\d+);", _EW).group(1))  # halves per workgroup of ew_map_kernel
# MUL: every size of the list, and two whole workgroups of the map with no partial one and no tail
MUL_CASES = CASES + [((2 * EW_WG,), False), ((2 * EW_WG,), True)]
MUL_IDS = ["%s%s" % ("x".join(map(str, s)), "-misaligned" if m else "") for s, m in MUL_CASES]


def geometry(n, misaligned):
    """grad_geometry restated: (head, vectors, tail, workgroups of the first stage)"""
    head = min(n, 7 if misaligned else 0)
    nv = (n - head) // 8
    tiles = -(-nv // (TILE * THREADS))
    return head, nv, n - head - 8 * nv, 1 if n <= ONE_WG else max(tiles, 1)


def test_the_large_case_takes_three_workgroups_a_partial_one_and_a_tail():
    for mis in (False, True):
        head, nv, tail, blocks = geometry(BIG, mis)
        assert BIG > ONE_WG and blocks >= 3 and nv % (TILE * THREADS) != 0 and 1 <= tail <= 7, (head, nv, tail, blocks)
    assert geometry(ONE_WG, False)[3] == 1 and geometry(ONE_WG + 1, False)[3] >= 2 and geometry(ONE_WG + 1, True)[3] >= 2
    assert 4 * BIG < 2 ** 20  # check 2: S < 2^20


def positions(n, misaligned):
    """the first and last element, the last of the vector body and the first of the tail, both sides of the head, of every workgroup (and trip) boundary of the
    first stage and of the one-workgroup threshold"""
    head, nv, tail, _ = geometry(n, misaligned)
    p = {0, n - 1, head - 1, head, head + 8 * nv - 1, head + 8 * nv, ONE_WG - 1, ONE_WG}
    for k in range(1, n // WG + 2):
        p |= {head + k * WG - 1, head + k * WG}
    return sorted(i for i in p if 0 <= i < n)


_DATA = {}


def data(shape, kind):
    """'uniform': U(-2, 2) halves; 'ints': integer-valued halves in {-2 .. 2}.  Made once per (shape, kind), read-only"""
    key = (tuple(shape), kind)
    if key not in _DATA:
        rng = np.random.default_rng(7000 + 13 * int(np.prod(shape)) + len(shape) + (kind == "ints"))
        x = ((rng.random(shape) - 0.5) * 4).astype(H) if kind == "uniform" else rng.integers(-2, 3, shape).astype(H)
        x.setflags(write=False)
        _DATA[key] = x
    return _DATA[key]


def tensor(L, x, misaligned=False):
    if misaligned and x.dtype == H and x.size > 0:
        (t,) = aliased(L, [x], 1)
        assert t.ptr % 16 == 2
        return t
    (t,) = make_tensors(L, nnc.GPU_MEMORY, [x])
    assert t.ptr % 16 == 0
    return t


def same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert np.array_equal(bits(a) if a.dtype != I else a, bits(b) if b.dtype != I else b), "%s: %s against %s" % (what, a.ravel()[:4], b.ravel()[:4])


def reduce_cmd(op, nd):
    return (nnc.CMD_REDUCE_NORM2_FORWARD if op == "norm2" else nnc.CMD_REDUCE_ISNAN_FORWARD)(*range(nd))


def reduce_run(L, op, x, odt, misaligned=False, flags=0):
    out = tensor(L, np.full((1,) * x.ndim, 3, odt))
    r = L.cmd_exec(reduce_cmd(op, x.ndim), nnc.NO_HINT, flags, [tensor(L, x, misaligned)], [out])
    assert r == 0, (op, x.shape, r)
    return out.numpy()


def reduce_names(op, n, misaligned):
    tag = {"norm2": "NORM2", "isnan": "ISNAN"}[op]
    names = ["grad_%s|nnc::grad_reduce_kernel<%s>" % (op, tag)]
    return names if geometry(n, misaligned)[3] == 1 else names + ["grad_%s|nnc::grad_fold_kernel<%s>" % (op, tag)]


def accepted(L, fn, tensors, names_want, what):
    """checks (a) - (c) on fn() -> array; -> (the native result, the key-off result)"""
    s0, n0 = counts(L)
    got, names = records(L, fn)
    assert counts(L) == (s0, n0 + tensors), (what, counts(L), (s0, n0), tensors)  # (a)
    assert names == names_want, (what, names, names_want)  # (b)
    same(got, fn(), "%s, two runs" % what)  # (c)
    with key_off(L, KEY):
        s0, n0 = counts(L)
        off, names = records(L, fn)
        s1, n1 = counts(L)
        assert s1 > s0 and n1 == n0, (what, (s1, n1), (s0, n0))
        assert not any("grad_" in x for x in names), (what, names)
    return got, off


def staged(L, fn, what):
    """fn() -> array on today's route: half tensors through fp32 images, none handed over, no kernel of grad_ops.h"""
    s0, n0 = counts(L)
    got, names = records(L, fn)
    s1, n1 = counts(L)
    assert s1 > s0 and n1 == n0, (what, (s1, n1), (s0, n0))
    assert not any("grad_" in x for x in names), (what, names)
    return got


def norm_bound(n, want, odt):
    return (n + 2) * U * want + (2.0 ** -11 * want + U if odt == H else 0)


_REF = {}


def reference(ref, key, cmd, ins, outs):
    if key not in _REF:
        _REF[key] = ref_run(ref, cmd, ins, outs)
    return _REF[key]


# ---- NORM2 ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,mis", CASES, ids=IDS)
def test_norm2_coverage_is_exact(backend, shape, mis):
    """check 1, and (a) - (c) on its first command"""
    L, n = backend, int(np.prod(shape))
    first = True
    for pos in positions(n, mis):
        for v in (1.5, -3.0):
            x = np.zeros(n, H)
            x[pos] = v
            x = x.reshape(shape)
            for odt in (F, H):
                fn = lambda: reduce_run(L, "norm2", x, odt, mis)
                got = accepted(L, fn, 1 + (odt == H), reduce_names("norm2", n, mis), "NORM2 %s" % (shape,))[0] if first and odt == F else fn()
                assert got.dtype == odt and got.shape == (1,) * len(shape) and float(got.ravel()[0]) == abs(v), (shape, mis, pos, v, odt, got)
        first = False


@pytest.mark.parametrize("shape,mis", CASES, ids=IDS)
def test_norm2_of_integers_is_order_free(backend, shape, mis):
    """check 2"""
    L, n = backend, int(np.prod(shape))
    x = data(shape, "ints")
    S = float((x.astype(D) ** 2).sum())
    assert S < 2 ** 20
    for odt in (F, H):
        got, off = accepted(L, lambda: reduce_run(L, "norm2", x, odt, mis), 1 + (odt == H), reduce_names("norm2", n, mis), "NORM2 of integers %s" % (shape,))
        want = np.sqrt(S)
        err, bound = abs(float(got.ravel()[0]) - want), 2 * U * want + (2.0 ** -11 * want + U if odt == H else 0)
        print("NORM2 of integers", shape, mis, odt.__name__, "error / bound", err / max(bound, 1e-300))
        assert err <= bound, (shape, mis, odt, got, want)
        same(got, off, "NORM2 of integers %s against the key at 0" % (shape,))


@pytest.mark.parametrize("shape,mis", CASES, ids=IDS)
def test_norm2_general(backend, ref_lib, shape, mis):
    """check 3: the native route, the key-off route and the reference's CPU backend on the widened input inside one bound"""
    L, n = backend, int(np.prod(shape))
    x = data(shape, "uniform")
    want = float(np.sqrt((x.astype(D) ** 2).sum()))
    ref = reference(ref_lib, ("norm2", shape), reduce_cmd("norm2", len(shape)), [x], [np.zeros((1,) * len(shape), F)])[0]
    for odt in (F, H):
        got, off = accepted(L, lambda: reduce_run(L, "norm2", x, odt, mis), 1 + (odt == H), reduce_names("norm2", n, mis), "NORM2 %s" % (shape,))
        b = norm_bound(n, want, odt)
        for what, r in (("native", got), ("key off", off), ("reference", ref.astype(odt))):
            err = abs(float(r.ravel()[0]) - want)
            print("NORM2", shape, mis, odt.__name__, what, "error / bound", err / max(b, 1e-300))
            assert err <= b, (what, shape, mis, odt, r, want)


def test_wrong_expectations_break_the_bounds(backend):
    """an expectation with ONE element left out fails check 1 and check 2"""
    L = backend
    x = np.zeros(BIG, H)
    x[BIG - 1] = 1.5
    got = float(reduce_run(L, "norm2", x, F).ravel()[0])
    assert got == 1.5 and got != 0.0 and got != float(F(np.sqrt(2.0) * 1.5))
    for shape in [(9,), (BIG,)]:
        x = data(shape, "ints")
        got = float(reduce_run(L, "norm2", x, F).ravel()[0])
        S = float((x.astype(D) ** 2).sum())
        k = int(np.flatnonzero(x.ravel())[-1])
        for wrong in (np.sqrt(S - float(x.ravel()[k]) ** 2), np.sqrt(S + float(x.ravel()[k]) ** 2)):
            assert abs(got - np.sqrt(S)) <= 2 * U * np.sqrt(S) and not abs(got - wrong) <= 2 * U * wrong, (shape, got, wrong)


# ---- ISNAN ----------------------------------------------------------------------------------------------------------------------------------------------------
SPECIAL = np.array([0x7c00, 0xfc00, 0x7bff, 0xfbff, 0x0000, 0x8000, 0x0001, 0x8001], np.uint16)  # +-Inf, +-65504, +-0, the smallest subnormals: no NaN
NANS = (0x7e00, 0xfe00, 0x7c01, 0xffff)


def isnan_base(shape):
    n = int(np.prod(shape))
    x = bits(data(shape, "uniform")).ravel().copy()
    at = np.unique(np.linspace(0, n - 1, min(n, 3 * len(SPECIAL))).astype(int))
    x[at] = SPECIAL[np.arange(len(at)) % len(SPECIAL)]
    assert not np.isnan(x.view(H)).any()
    return x


@pytest.mark.parametrize("shape,mis", CASES, ids=IDS)
def test_isnan(backend, ref_lib, shape, mis):
    L, n = backend, int(np.prod(shape))
    base = isnan_base(shape)
    cmd = reduce_cmd("isnan", len(shape))
    run = lambda xb: reduce_run(L, "isnan", xb.view(H).reshape(shape), I, mis)
    oshape = (1,) * len(shape)

    def full_check(xb, want, what):
        got, off = accepted(L, lambda: run(xb), 1, reduce_names("isnan", n, mis), what)
        ref = ref_run(ref_lib, cmd, [xb.view(H).reshape(shape)], [np.full(oshape, 3, I)])[0]
        for r in (got, off, ref):
            assert r.dtype == I and r.shape == oshape and int(r.ravel()[0]) == want, (what, r, want)

    full_check(base, 0, "ISNAN %s without a NaN" % (shape,))
    pos = positions(n, mis)
    for k, pattern in enumerate(NANS):
        for p in pos:
            xb = base.copy()
            xb[p] = pattern
            if p == pos[(k * 3) % len(pos)]:
                full_check(xb, 1, "ISNAN %s, 0x%04x at %d" % (shape, pattern, p))
            else:
                got = run(xb)
                assert got.dtype == I and int(got.ravel()[0]) == 1, (shape, mis, hex(pattern), p, got)


# ---- MUL by a one-element tensor --------------------------------------------------------------------------------------------------------------------------------
SCALAR_F = F(0.3136)  # no half: halfway between the halves 0.31372 and 0.31348
MUL_NAMES = ["grad_mul|nnc::ew_map_kernel<GScale>"]


def mul_run(L, p, x, s, first, in_place, mis=False, flags=0):
    """(p a) b with the scalar s as a (first) or b; -> the half output"""
    tx, ts = tensor(L, x, mis), tensor(L, s)
    out = tx.alias(x.shape, 0) if in_place else tensor(L, np.full(x.shape, 3, H), mis)
    assert not in_place or out.ptr == tx.ptr
    r = L.cmd_exec(nnc.CMD_MUL_FORWARD(p), nnc.NO_HINT, flags, [ts, tx] if first else [tx, ts], [out])
    assert r == 0, r
    return out.numpy()


def mul_bound(want):
    return 2.0 ** -11 * np.abs(want) + U + 2 * U * np.abs(want)


def test_the_fp32_scalar_is_no_half():
    """rounding the scalar to half first changes at least a tenth of the results: bit equality with the key-off route shows the kernel did not narrow it"""
    x = data((BIG,), "uniform").astype(D)
    for p in (1.0, 0.7):
        true, narrowed = (D(F(p)) * x * D(SCALAR_F)).astype(H), (D(F(p)) * x * D(H(SCALAR_F))).astype(H)
        assert (bits(true) != bits(narrowed)).mean() >= 0.1


@pytest.mark.parametrize("in_place", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("sdt", [F, H], ids=["f32-scalar", "f16-scalar"])
@pytest.mark.parametrize("first", [False, True], ids=["large-first", "large-second"])
@pytest.mark.parametrize("shape,mis", MUL_CASES, ids=MUL_IDS)
def test_mul_by_a_scalar(backend, ref_lib, shape, mis, first, sdt, in_place):
    L = backend
    x = data(shape, "uniform")
    s = np.array([SCALAR_F if sdt == F else H(-1.3779296875)], sdt)
    if x.size == 1 and sdt == H:  # two half tensors of ONE shape: bcast_ops.h's rows come first and still take what they took
        got, names = records(L, lambda: mul_run(L, 0.7, x, s, first, in_place, mis))
        assert names == ["bcast_mul_fwd|nnc::ew_map_kernel"], names
        want = D(F(0.7)) * x.astype(D) * D(s[0])
        within(got, want, mul_bound(want), "MUL of two one-element halves")
        return
    for p in (1.0, 0.7):
        what = "MUL(%g) %s, scalar %s %s%s%s" % (p, shape, sdt.__name__, "first" if first else "second", ", in place" if in_place else "", ", misaligned" if mis else "")
        got, off = accepted(L, lambda: mul_run(L, p, x, s, first, in_place, mis), 2 + (sdt == H), MUL_NAMES, what)
        want = D(F(p)) * x.astype(D) * D(s[0])
        assert got.dtype == H and got.shape == x.shape
        same(got, off, "%s, against the key at 0" % what)
        within(got, want, mul_bound(want), what)
        ref = reference(ref_lib, ("mul", shape, p, sdt, first), nnc.CMD_MUL_FORWARD(p), [s, x] if first else [x, s], [np.zeros(shape, F)])[0]
        within(ref, want, 2 * U * np.abs(want), "%s, the reference in fp32" % what)


# ---- the sequences the trainer issues -----------------------------------------------------------------------------------------------------------------------------
GRADS = [(9,), (ONE_WG + 1,), SHAPE4]


def clip(L, grads, max_norm):
    """the commands of ccv_cnnp_model_parameters_clip_grad_norm on half gradients; -> the clipped gradients"""
    gt = [tensor(L, g) for g in grads]
    total, norm2, maxn = tensor(L, np.zeros(1, F)), tensor(L, np.full(1, 3, F)), tensor(L, np.full(1, 3, F))
    run = lambda cmd, ins, outs: L.cmd_exec(cmd, nnc.NO_HINT, 0, ins, outs)
    for g, t in zip(grads, gt):
        assert run(nnc.CMD_REDUCE_NORM2_FORWARD(), [t], [norm2]) == 0
        assert run(nnc.CMD_MUL_FORWARD(1), [norm2, norm2], [norm2]) == 0
        assert run(nnc.CMD_ADD_FORWARD(1, 1), [total, norm2], [total]) == 0
    assert run(nnc.CMD_EWSQRT_FORWARD(), [total], [total]) == 0
    assert run(nnc.CMD_SET_FORWARD(max_norm), [], [maxn]) == 0
    assert run(nnc.CMD_EWDIV_FORWARD(), [maxn, total], [total]) == 0
    assert run(nnc.CMD_CLAMP_FORWARD(float("nan"), 1), [total], [total]) == 0
    for g, t in zip(grads, gt):
        assert run(nnc.CMD_MUL_FORWARD(1), [t, total], [t.alias(g.shape, 0)]) == 0
    return [t.numpy() for t in gt]


DEPTH = 64


def test_clip_sequence(backend):
    """Composed bound.  A sum of non-negative terms in which no term passes through more than d additions is within d u of the exact sum, whatever the data.  In
    grad_ops.h a square passes through at most 8 additions inside its vector, one per trip (<= GRAD_ONE_WG_MAX / WG = 8), 3 folding the lane's accumulators, 6 in the
    wave's tree, 3 across the waves, and above the threshold one per pass of the fold, 2, 6 and 15 more there: fewer than DEPTH = 64 for every tensor below 2^26
    elements (test_the_depth_covers_these_sizes), where (n + 2) u of check 3 allows 131 075.  So a norm is within (DEPTH / 2 + 1) u, its square within
    (DEPTH + 3) u, the sum of three adds 2, the root halves that and adds one, the division one: the scale is within (DEPTH / 2 + 5) u of min(1, max_norm / norm);
    the in-place MUL adds two fp32 roundings and the store's one to half."""
    L = backend
    grads = [data(s, "uniform") for s in GRADS]
    norm = float(np.sqrt(sum((g.astype(D) ** 2).sum() for g in grads)))
    for max_norm, clipped in ((10.0, True), (1000.0, False)):
        assert (norm > max_norm) == clipped
        s0, n0 = counts(L)
        got, names = records(L, lambda: clip(L, grads, max_norm))
        s1, n1 = counts(L)
        assert s1 == s0 and n1 == n0 + 3 * len(grads), ((s1, n1), (s0, n0))  # per gradient: the norm's input, the scale's input and output
        assert sum("grad_reduce_kernel<NORM2>" in x for x in names) == 3 and sum("grad_fold_kernel<NORM2>" in x for x in names) == 1 and sum(x == MUL_NAMES[0] for x in names) == 3, names
        scale = min(1.0, D(F(max_norm)) / norm)
        for g, c in zip(grads, got):
            want = g.astype(D) * scale
            within(c, want, 2.0 ** -11 * np.abs(want) + U + (DEPTH / 2 + 5 + 2) * U * np.abs(want), "the clipped gradient %s" % (g.shape,))
            if not clipped:
                same(c, g, "a gradient under max_norm keeps its bits")
        after = float(np.sqrt(sum((c.astype(D) ** 2).sum() for c in got)))
        assert after <= max_norm * (1 + 2.0 ** -10), (after, max_norm)


def test_the_depth_covers_these_sizes():
    for shape in GRADS:
        n = int(np.prod(shape))
        blocks = geometry(n, False)[3]
        trips = -(-n // WG) if blocks == 1 else 1
        fold = 0 if blocks == 1 else -(-blocks // (4 * 1024)) + 2 + 6 + 15
        assert 8 + trips + 3 + 6 + 3 + fold < DEPTH, (shape, trips, fold)


def test_nan_check_sequence(backend):
    """REDUCE_ISNAN -> EWSUM into an int32 accumulator over the gradients (ccv_cnnp_model_parameter_gradients_isnan)"""
    L = backend
    for with_nan in (False, True):
        grads = [data(s, "uniform") for s in GRADS]
        if with_nan:
            g = grads[-1].copy()
            g.ravel()[g.size // 2] = np.nan
            grads[-1] = g

        def run():
            acc, flag = tensor(L, np.zeros(1, I)), tensor(L, np.full(1, 3, I))
            for g in grads:
                cmd = nnc.CMD_REDUCE_ISNAN_FORWARD(*range(g.ndim))
                assert L.cmd_exec(cmd, nnc.NO_HINT, 0, [tensor(L, g)], [flag]) == 0
                assert L.cmd_exec(nnc.CMD_EWSUM_FORWARD(), nnc.NO_HINT, 0, [acc, flag], [acc]) == 0
            return acc.numpy()
        s0, n0 = counts(L)
        acc = run()
        assert counts(L) == (s0, n0 + len(grads))
        assert acc.dtype == I and int(acc[0]) == int(with_nan), acc


# ---- kept routes ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_keep_the_route(backend):
    L = backend
    rows, cols = 37, 29
    x = data((rows, cols), "uniform")
    want = float(np.sqrt((x.astype(D) ** 2).sum()))

    def view_of_x():  # rows of `cols` elements at a stride of cols + 8
        parent = np.full((rows, cols + 8), 5, H)
        parent[:, :cols] = x
        return tensor(L, parent).view((rows, cols), (cols + 8, 1), 0)

    def norm2_of_view():
        out = tensor(L, np.full((1, 1), 3, F))
        assert L.cmd_exec(reduce_cmd("norm2", 2), nnc.NO_HINT, 0, [view_of_x()], [out]) == 0
        return out.numpy()
    got = staged(L, norm2_of_view, "NORM2 of a view")
    assert abs(float(got[0, 0]) - want) <= norm_bound(x.size, want, F)

    def isnan_of_view():
        out = tensor(L, np.full((1, 1), 3, I))
        assert L.cmd_exec(reduce_cmd("isnan", 2), nnc.NO_HINT, 0, [view_of_x()], [out]) == 0
        return out.numpy()
    assert int(staged(L, isnan_of_view, "ISNAN of a view")[0, 0]) == 0

    def mul_of_view():
        out = tensor(L, np.full((rows, cols), 3, H))
        assert L.cmd_exec(nnc.CMD_MUL_FORWARD(0.7), nnc.NO_HINT, 0, [view_of_x(), tensor(L, np.array([SCALAR_F]))], [out]) == 0
        return out.numpy()
    w = D(F(0.7)) * x.astype(D) * D(SCALAR_F)
    within(staged(L, mul_of_view, "MUL of a view"), w, mul_bound(w), "MUL of a view")

    # CCV_NNC_ACCUMULATE_OUTPUT: the native kernels do not take it.  On the kept route these three rows WRITE their result (cmd_bcast.cpp's exec functions do not
    # read the flag, as the reference's CPU rows do not): the pre-filled 3 is gone, and the value is held to the same bounds as everywhere else
    ACC = nnc.ACCUMULATE_OUTPUT
    for odt in (F, H):
        got = staged(L, lambda: reduce_run(L, "norm2", x, odt, flags=ACC), "NORM2 with ACCUMULATE_OUTPUT")
        assert got.dtype == odt and abs(float(got[0, 0]) - want) <= norm_bound(x.size, want, odt), (odt, got, want)
    xn = x.copy()
    xn[rows // 2, cols // 2] = np.nan
    for xi, flag in ((x, 0), (xn, 1)):
        got = staged(L, lambda: reduce_run(L, "isnan", xi, I, flags=ACC), "ISNAN with ACCUMULATE_OUTPUT")
        assert got.dtype == I and int(got[0, 0]) == flag, (got, flag)
    w = D(F(0.7)) * x.astype(D) * D(SCALAR_F)
    for in_place in (False, True):
        got = staged(L, lambda: mul_run(L, 0.7, x, np.array([SCALAR_F]), False, in_place, flags=ACC), "MUL with ACCUMULATE_OUTPUT")
        within(got, w, mul_bound(w), "MUL with ACCUMULATE_OUTPUT%s" % (", in place" if in_place else ""))

    # mul_planes.h's pattern at N = C = 1 (a 4-d map of one image and one channel by a 4-d one-element tensor of its type): with MUL_PLANES at 0 it keeps the
    # generic kernels on fp32 images, as that key says
    m, sm = data((1, 1, 8, 8), "uniform"), data((1, 1, 1, 1), "uniform")

    def plane_scale():
        tm, ts, to = make_tensors(L, nnc.GPU_MEMORY, [m, sm, np.full(m.shape, 3, H)], "NCHW")
        assert L.cmd_exec(nnc.CMD_MUL_FORWARD(0.7), nnc.NO_HINT, 0, [tm, ts], [to]) == 0
        return to.numpy()
    wm = D(F(0.7)) * m.astype(D) * sm.astype(D)
    with key_off(L, "MUL_PLANES"):
        within(staged(L, plane_scale, "the plane-scale pattern with MUL_PLANES at 0"), wm, mul_bound(wm), "the plane-scale pattern with MUL_PLANES at 0")
    got, names = records(L, plane_scale)
    assert any("mul_planes" in n for n in names) and not any("grad_" in n for n in names), names
    within(got, wm, mul_bound(wm), "the plane-scale pattern")

    # a two-element output: the norm along one axis
    y = data((2, ONE_WG // 4 + 5), "uniform")

    def rows_norm2():
        out = tensor(L, np.full((2, 1), 3, F))
        assert L.cmd_exec(nnc.CMD_REDUCE_NORM2_FORWARD(1), nnc.NO_HINT, 0, [tensor(L, y)], [out]) == 0
        return out.numpy()
    got = staged(L, rows_norm2, "NORM2 along one axis")
    for r in range(2):
        w = float(np.sqrt((y[r].astype(D) ** 2).sum()))
        assert abs(float(got[r, 0]) - w) <= norm_bound(y.shape[1], w, F), (r, got, w)

    def rows_isnan():
        out = tensor(L, np.full((2, 1), 3, I))
        assert L.cmd_exec(nnc.CMD_REDUCE_ISNAN_FORWARD(1), nnc.NO_HINT, 0, [tensor(L, y)], [out]) == 0
        return out.numpy()
    assert not staged(L, rows_isnan, "ISNAN along one axis").any()

    # MUL of [N, C] by [C]
    c = data((cols,), "uniform")

    def by_a_row():
        out = tensor(L, np.full((rows, cols), 3, H))
        assert L.cmd_exec(nnc.CMD_MUL_FORWARD(0.7), nnc.NO_HINT, 0, [tensor(L, x), tensor(L, c)], [out]) == 0
        return out.numpy()
    w = D(F(0.7)) * x.astype(D) * c.astype(D)
    within(staged(L, by_a_row, "MUL of [N, C] by [C]"), w, mul_bound(w), "MUL of [N, C] by [C]")

    # the key at 0 (every accepted case above runs it too)
    with key_off(L, KEY):
        got = staged(L, lambda: reduce_run(L, "norm2", x, F), "NORM2 with the key at 0")
    assert abs(float(got[0, 0]) - want) <= norm_bound(x.size, want, F)


def test_a_key_above_one_is_the_threshold(backend):
    """GRAD_HALF_NATIVE > 1: the one-workgroup threshold in elements (the sweep of tools/grad_half_bench.py).  The results stay inside the bounds, the launches follow"""
    L = backend
    two, one = ["grad_norm2|nnc::grad_reduce_kernel<NORM2>", "grad_norm2|nnc::grad_fold_kernel<NORM2>"], ["grad_norm2|nnc::grad_reduce_kernel<NORM2>"]
    try:
        for key, shape, names_want in ((2, (3 * WG + 5,), two), (2 * ONE_WG, (ONE_WG + 1,), one), (1, (ONE_WG + 1,), two), (1, (3 * WG + 5,), one if 3 * WG + 5 <= ONE_WG else two)):
            L.tune_set(KEY, key)
            x = data(shape, "ints")
            S = float((x.astype(D) ** 2).sum())
            got, names = records(L, lambda: reduce_run(L, "norm2", x, F))
            assert names == names_want, (key, shape, names)
            assert abs(float(got[0]) - np.sqrt(S)) <= 2 * U * np.sqrt(S), (key, shape, got, S)
    finally:
        L.tune_set(KEY, 1)


def test_tune_key_round_trips(backend):
    L = backend
    assert L.tune_get(KEY) == 1
    L.tune_set(KEY, 0)
    try:
        assert L.tune_get(KEY) == 0
    finally:
        L.tune_set(KEY, 1)
    assert L.tune_get(KEY) == 1
