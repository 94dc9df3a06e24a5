"""Parity of the broadcasting map / reduce rows (ccv_amd/csrc/cmd_bcast.cpp) at the edges of their kernels: every broadcast pattern,
absent operands, outputs that are views, both sides of the two-stage reduction threshold, and the int flag REDUCE_ISNAN carries as a
float subnormal.

Two references: the reference's CPU backend where it implements the case (it asserts equal shapes on most element-wise rows), and a
float64 numpy statement of the operation.  Bounds are derived, never tuned:
  moves / selections          bit-exact
  one-rounding maps           |got - f64| <= 2 eps32 sum|terms|   (room for an fma contraction either way)
  sums of T terms             |got - f64| <= T eps32 S, S = the same f64 expression on absolute values: the worst case of ANY summation order,
                              so one bound serves the serial kernel and the two-stage one
  expf / logf / sqrtf         twice the reference CPU backend's own largest deviation from float64 on these inputs, at least 2 ulp
"""
import numpy as np
import pytest
from ccv_amd import nnc
from harness import exec_on

F, D = np.float32, np.float64
EPS = float(np.finfo(F).eps)
NAN = float("nan")

FULL = (3, 6, 5, 4)
# (a shape, b shape): an extent-1 axis in each position and on either operand, 4-d against 4-d, 3-d, 1-d and the scalar-like (1,)
PAIRS = [((3, 1, 5, 4), (1, 6, 1, 4)),
         ((1, 6, 5, 4), FULL), ((3, 1, 5, 4), FULL), ((3, 6, 1, 4), FULL), ((3, 6, 5, 1), FULL),
         (FULL, (1, 6, 5, 4)), (FULL, (3, 1, 5, 4)), (FULL, (3, 6, 1, 4)), (FULL, (3, 6, 5, 1)),
         (FULL, (6, 5, 4)), (FULL, (6, 1, 4)), (FULL, (1, 5, 1)), (FULL, (4,)), (FULL, (1,)), ((1,), FULL), (FULL, FULL)]
PAIR_IDS = ["%s*%s" % ("x".join(map(str, a)), "x".join(map(str, b))) for a, b in PAIRS]


def rnd(shape, seed, lo=-1.0, hi=1.0):
    return (np.random.default_rng(seed).random(shape) * (hi - lo) + lo).astype(F)


def gpu(L, cmd, ins, outs):
    r, res = exec_on(L, nnc.GPU_MEMORY, cmd, nnc.NO_HINT, 0, ins, outs)
    assert r == 0, "backend returned %d" % r
    return res


def cpu(ref, cmd, ins, outs):
    r, res = exec_on(ref, nnc.CPU_MEMORY, cmd, nnc.NO_HINT, 0, ins, outs, backend=nnc.BACKEND_CPU_REF)
    assert r == 0, "reference returned %d" % r
    return res


def within(x, f64, bound, what=""):
    err = np.abs(np.asarray(x, D) - f64)
    bad = ~(err <= bound)
    assert not bad.any(), "%s: %d elements off, worst error %.3e against a bound of %.3e" % (what, int(bad.sum()), float(err[bad].max()), float(np.asarray(bound + 0 * err)[bad].min()))


def reduce_to(x, shape):
    """x (the full broadcast shape) summed over the axes on which the right-aligned `shape` has extent 1."""
    padded = (1,) * (x.ndim - len(shape)) + tuple(shape)
    axes = tuple(i for i in range(x.ndim) if padded[i] == 1 and x.shape[i] != 1)
    return (x.sum(axis=axes, keepdims=True) if axes else x).reshape(shape)


def sum_bound(full, shape, s_abs):
    """T eps S for T > 1 terms per output, the one-rounding bound 2 eps S where nothing is folded."""
    t = int(np.prod(full)) // int(np.prod(shape))
    return max(t, 2) * EPS * s_abs


def fwd_f64(op, p, q, a, b):
    a, b = a.astype(D), (None if b is None else b.astype(D))
    if b is None:
        return D(F(p)) * a, np.abs(D(F(p)) * a)
    if op == "ADD":
        return D(F(p)) * a + D(F(q)) * b, np.abs(D(F(p)) * a) + np.abs(D(F(q)) * b)
    return D(F(p)) * a * b, np.abs(D(F(p)) * a * b)


def fwd_cmd(op, p, q):
    return nnc.CMD_ADD_FORWARD(p, q) if op == "ADD" else nnc.CMD_MUL_FORWARD(p)


def bwd_cmd(op, p, q):
    return nnc.CMD_ADD_BACKWARD(p, q) if op == "ADD" else nnc.CMD_MUL_BACKWARD(p)


# ---- ADD / MUL forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("op", ["ADD", "MUL"])
def test_add_mul_forward_broadcast(backend, ref_lib, op, pair):
    a, b = rnd(pair[0], 1), rnd(pair[1], 2)
    p, q = 0.7, -1.3
    full = np.broadcast_shapes(*pair)
    want64, mag = fwd_f64(op, p, q, a, b)
    want64, mag = np.broadcast_to(want64, full), np.broadcast_to(mag, full)
    got = gpu(backend, fwd_cmd(op, p, q), [a, b], [np.full(full, 9, F)])[0]
    ref = cpu(ref_lib, fwd_cmd(op, p, q), [a, b], [np.full(full, 9, F)])[0]
    within(got, want64, 2 * EPS * mag, "kernel")
    within(ref, want64, 2 * EPS * mag, "reference")


@pytest.mark.parametrize("op", ["ADD", "MUL"])
def test_add_mul_forward_without_second_input(backend, ref_lib, op):
    """b absent: the FScale path, c = p * a (a broadcast into c)."""
    for ashape, cshape in ((FULL, FULL), ((3, 1, 5, 1), FULL)):
        a = rnd(ashape, 3)
        want64, mag = fwd_f64(op, 0.7, 0.0, a, None)
        got = gpu(backend, fwd_cmd(op, 0.7, 0.0), [a, None], [np.full(cshape, 9, F)])[0]
        within(got, np.broadcast_to(want64, cshape), 2 * EPS * np.broadcast_to(mag, cshape), "kernel")
        if ashape == cshape:
            ref = cpu(ref_lib, fwd_cmd(op, 0.7, 0.0), [a, None], [np.full(cshape, 9, F)])[0]  # (the reference asserts q == 0 without b)
            within(ref, want64, 2 * EPS * mag, "reference")


@pytest.mark.parametrize("op", ["ADD", "MUL"])
def test_add_mul_forward_into_a_strided_view(backend, op):
    """The output is a (3, 6, 5, 4) window of a (3, 6, 5, 8) buffer: the window takes the result, every byte around it stays."""
    L = backend
    a, b = rnd((3, 1, 5, 4), 4), rnd((1, 6, 1, 4), 5)
    base = rnd((3, 6, 5, 8), 6, 10, 20)
    at, bt, ct = [L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_32F, x.shape, 0), x) for x in (a, b, base)]
    view = ct.view(FULL, (240, 40, 8, 1), 3)
    assert L.cmd_exec(fwd_cmd(op, 0.7, -1.3), nnc.NO_HINT, 0, [at, bt], [view]) == 0
    out = ct.numpy()
    want64, mag = fwd_f64(op, 0.7, -1.3, a, b)
    within(out[..., 3:7], want64, 2 * EPS * mag, "window")
    keep = np.ones(base.shape, bool)
    keep[..., 3:7] = False
    assert np.array_equal(out[keep].view(np.uint32), base[keep].view(np.uint32))


@pytest.mark.parametrize("op", ["ADD", "MUL"])
def test_five_dimensional_tensor_is_invalid(backend, op):
    """More than 4 axes: CCV_NNC_EXEC_INVALID, no result (the output keeps its contents).  Nothing further runs on the tensor."""
    a = rnd((2, 2, 2, 2, 2), 7)
    r, res = exec_on(backend, nnc.GPU_MEMORY, fwd_cmd(op, 1, 1), nnc.NO_HINT, 0, [a, a], [np.full(a.shape, 9, F)])
    assert r == nnc.EXEC_INVALID
    assert np.array_equal(res[0], np.full(a.shape, 9, F))


# ---- ADD / MUL backward -----------------------------------------------------------------------------------------------------------
def bwd_f64(op, p, q, g, a, b, full):
    """(da, |da| sums, db, |db| sums) in float64; for MUL g None = ones of the full shape."""
    g64 = np.ones(full, D) if g is None else g.astype(D)
    p, q = D(F(p)), D(F(q))
    if op == "ADD" and g is None:  # the contract is the reference's: without g the outputs are FILLED with p and q, nothing is folded (add_cpu_ref.c:202-209)
        return np.full(a.shape, p), np.full(a.shape, abs(p)), np.full(b.shape, q), np.full(b.shape, abs(q))
    if op == "ADD":
        ta, tb = p * g64, q * g64
    else:
        ta, tb = p * g64 * np.broadcast_to(b.astype(D), full), p * g64 * np.broadcast_to(a.astype(D), full)
    return reduce_to(ta, a.shape), reduce_to(np.abs(ta), a.shape), reduce_to(tb, b.shape), reduce_to(np.abs(tb), b.shape)


def check_backward(backend, ref_lib, op, a, b, g, full, what=(0, 1)):
    p, q = 0.7, -1.3
    da64, sa, db64, sb = bwd_f64(op, p, q, g, a, b, full)
    ins = [g] if op == "ADD" else [g, a, b]
    outs = [np.full(a.shape, 9, F) if 0 in what else None, np.full(b.shape, 9, F) if 1 in what else None]
    got = gpu(backend, bwd_cmd(op, p, q), ins, outs)
    res = [got, cpu(ref_lib, bwd_cmd(op, p, q), ins, outs)]
    for who, r in zip(("kernel", "reference"), res):
        if 0 in what:
            within(r[0], da64, sum_bound(full, a.shape, sa), who + " da")
        if 1 in what:
            within(r[1], db64, sum_bound(full, b.shape, sb), who + " db")
    return got


@pytest.mark.parametrize("with_g", [True, False], ids=["g", "no-g"])
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("op", ["ADD", "MUL"])
def test_add_mul_backward_broadcast(backend, ref_lib, op, pair, with_g):
    a, b = rnd(pair[0], 11), rnd(pair[1], 12)
    full = np.broadcast_shapes(*pair)
    g = rnd(full, 13) if with_g else None
    both = check_backward(backend, ref_lib, op, a, b, g, full)
    if op == "ADD" and not with_g:  # the fill path: exactly p and q
        assert np.array_equal(both[0], np.full(a.shape, F(0.7))) and np.array_equal(both[1], np.full(b.shape, F(-1.3)))
    only_a = check_backward(backend, ref_lib, op, a, b, g, full, what=(0,))
    only_b = check_backward(backend, ref_lib, op, a, b, g, full, what=(1,))
    assert only_a[1] is None and only_b[0] is None
    assert np.array_equal(only_a[0], both[0]) and np.array_equal(only_b[1], both[1])  # (deterministic: the same kernel either way)


R_CASES = [4095, 4096, 4096 * 3 + 5]  # either side of REDUCE_TWO_STAGE_MIN; the last one leaves a short final slice


@pytest.mark.parametrize("with_g", [True, False], ids=["g", "no-g"])
@pytest.mark.parametrize("R", R_CASES)
@pytest.mark.parametrize("op", ["ADD", "MUL"])
def test_backward_reduction_at_the_two_stage_threshold(backend, ref_lib, op, R, with_g):
    """da folds exactly R elements per output (axis 1 of (3, R, 2)); for MUL its second operand b = (1, R, 2) is itself broadcast on the
    KEPT axis 0.  db = (1, R, 2) folds 3 (the serial kernel) with a broadcast on the reduced axis."""
    a, b = rnd((3, 1, 2), 21), rnd((1, R, 2), 22)
    full = (3, R, 2)
    g = rnd(full, 23) if with_g else None
    check_backward(backend, ref_lib, op, a, b, g, full)


@pytest.mark.parametrize("R", R_CASES)
def test_backward_reduction_into_a_view(backend, R):
    """MUL backward, da a (3, 1, 2) window (strides 4, 2, 1; offset 1) of a 12-element buffer: both reduce paths store through the
    output's own strides and leave the rest of the buffer alone."""
    L = backend
    a, b, g = rnd((3, 1, 2), 31), rnd((1, R, 2), 32), rnd((3, R, 2), 33)
    base = rnd((3, 4), 34, 10, 20)
    gt, at, bt, ct = [L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_32F, x.shape, 0), x) for x in (g, a, b, base)]
    view = ct.view((3, 1, 2), (4, 2, 1), 1)
    assert L.cmd_exec(nnc.CMD_MUL_BACKWARD(0.7), nnc.NO_HINT, 0, [gt, at, bt], [view]) == 0
    out = ct.numpy()
    da64, sa, _, _ = bwd_f64("MUL", 0.7, 0, g, a, b, (3, R, 2))
    within(out[:, 1:3], da64.reshape(3, 2), R * EPS * sa.reshape(3, 2), "window")
    assert np.array_equal(out[:, [0, 3]].view(np.uint32), base[:, [0, 3]].view(np.uint32))


# ---- REDUCE_SUM / REDUCE_MEAN backward ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_g", [True, False], ids=["g", "no-g"])
@pytest.mark.parametrize("axes", [(0,), (3,), (1, 2), (0, 1, 2, 3)], ids=str)
@pytest.mark.parametrize("name", ["SUM", "MEAN"])
def test_reduce_sum_mean_backward(backend, ref_lib, name, axes, with_g):
    """h = g broadcast back (SUM: a move) or g / count (MEAN: one rounding after the rounding of 1 / count).  g absent: ones, the count taken
    from the command's axes."""
    shape = FULL
    gshape = tuple(1 if i in axes else d for i, d in enumerate(shape))
    cnt = int(np.prod([shape[i] for i in axes]))
    g = rnd(gshape, 41) if with_g else None
    cmd = (nnc.CMD_REDUCE_SUM_BACKWARD if name == "SUM" else nnc.CMD_REDUCE_MEAN_BACKWARD)(*axes)
    g64 = np.broadcast_to(np.ones(gshape, D) if g is None else g.astype(D), shape)
    want64 = g64 if name == "SUM" else g64 / cnt
    got = gpu(backend, cmd, [g], [np.full(shape, 9, F)])[0]
    ref = cpu(ref_lib, cmd, [g], [np.full(shape, 9, F)])[0]
    if name == "SUM":
        assert np.array_equal(got.view(np.uint32), want64.astype(F).view(np.uint32))
        assert np.array_equal(ref.view(np.uint32), want64.astype(F).view(np.uint32))
    else:
        within(got, want64, 2 * EPS * np.abs(want64), "kernel")
        within(ref, want64, 2 * EPS * np.abs(want64), "reference")


# ---- EWDIV ------------------------------------------------------------------------------------------------------------------------
def test_ewdiv_forward(backend, ref_lib):
    a, b = rnd(FULL, 51), rnd(FULL, 52, 0.5, 2.0)
    for ins in ([a, b], [None, b]):
        want64 = (1.0 if ins[0] is None else a.astype(D)) / b.astype(D)
        got = gpu(backend, nnc.CMD_EWDIV_FORWARD(), ins, [np.full(FULL, 9, F)])[0]
        ref = cpu(ref_lib, nnc.CMD_EWDIV_FORWARD(), ins, [np.full(FULL, 9, F)])[0]
        within(got, want64, 2 * EPS * np.abs(want64), "kernel")
        within(ref, want64, 2 * EPS * np.abs(want64), "reference")
    # b broadcast (the reference asserts equal shapes: numpy alone)
    for bshape in ((1, 6, 1, 4), (4,), (1,)):
        bb = rnd(bshape, 53, 0.5, 2.0)
        want64 = a.astype(D) / bb.astype(D)
        got = gpu(backend, nnc.CMD_EWDIV_FORWARD(), [a, bb], [np.full(FULL, 9, F)])[0]
        within(got, want64, 2 * EPS * np.abs(want64), "kernel, b %s" % (bshape,))


@pytest.mark.parametrize("with_g", [True, False], ids=["g", "no-g"])
@pytest.mark.parametrize("what", [(0,), (1,), (0, 1)], ids=["ha", "hb", "both"])
def test_ewdiv_backward(backend, ref_lib, what, with_g):
    """inputs (g, a, b, c = a / b) -> ha = g / b (one rounding), hb = -g c / b (two)."""
    a, b = rnd(FULL, 54), rnd(FULL, 55, 0.5, 2.0)
    c = (a / b).astype(F)
    g = rnd(FULL, 56) if with_g else None
    g64 = np.ones(FULL, D) if g is None else g.astype(D)
    ha64, hb64 = g64 / b.astype(D), -g64 * c.astype(D) / b.astype(D)
    outs = [np.full(FULL, 9, F) if 0 in what else None, np.full(FULL, 9, F) if 1 in what else None]
    for who, res in (("kernel", gpu(backend, nnc.CMD_EWDIV_BACKWARD(), [g, a, b, c], outs)), ("reference", cpu(ref_lib, nnc.CMD_EWDIV_BACKWARD(), [g, a, b, c], outs))):
        if 0 in what:
            within(res[0], ha64, 2 * EPS * np.abs(ha64), who + " ha")
        if 1 in what:
            within(res[1], hb64, 2 * EPS * np.abs(hb64), who + " hb")


# ---- EWEXP / EWLOG / EWSQRT ---------------------------------------------------------------------------------------------------------
def ulps(x, f64):
    return np.abs(np.asarray(x, D) - f64) / np.spacing(np.abs(f64).astype(F)).astype(D)


@pytest.mark.parametrize("name", ["EXP", "LOG", "SQRT"])
def test_ew_exp_log_sqrt(backend, ref_lib, name):
    """Forward: the kernel may deviate from float64 by twice what the reference CPU backend itself deviates on these inputs, and at least
    2 ulp.  Backward is a one-rounding map of f32 inputs: exp h = g b, log h = g / a, sqrt h = 0.5 g / b; g absent = ones."""
    n = 5000
    if name == "EXP":
        a = rnd((n,), 61, -10, 10)
    else:
        a = np.exp(rnd((n,), 62, np.log(1e-3), np.log(1e3)).astype(D)).astype(F)   # log-uniform over [1e-3, 1e3]
    a = np.clip(a, F(-10), F(10)) if name == "EXP" else np.clip(a, F(1e-3), F(1e3))
    f64 = {"EXP": np.exp, "LOG": np.log, "SQRT": np.sqrt}[name](a.astype(D))
    fwd = nnc.generic_cmd("EW%s_FORWARD" % name)
    got = gpu(backend, fwd, [a], [np.full(a.shape, 9, F)])[0]
    ref = cpu(ref_lib, fwd, [a], [np.full(a.shape, 9, F)])[0]
    ref_ulp = float(ulps(ref, f64).max())
    # measured on these inputs: the reference CPU backend deviates 0.500 ulp for exp, log and sqrt alike (it evaluates in double and rounds once, so
    # it is the correctly rounded result); twice that is 1 ulp, so the floor of 2 ulp is the bound in force.  (The kernels measured 0.501 / 0.673 /
    # 0.500 ulp on the emulator's libm.  On the MI355X logf measured 2.235 ulp and failed this test: EWLOG forward now takes the logarithm in double.)
    assert ref_ulp <= 0.5 + 1e-9
    bound = max(2.0, 2 * ref_ulp)
    got_ulp = float(ulps(got, f64).max())
    print("%s: reference %.3f ulp, kernel %.3f ulp" % (name, ref_ulp, got_ulp))
    assert got_ulp <= bound
    # backward
    b = ref
    bwd = nnc.generic_cmd("EW%s_BACKWARD" % name)
    for g in (rnd(a.shape, 63), None):
        g64 = np.ones(a.shape, D) if g is None else g.astype(D)
        ins = [g, a, b]
        want64 = {"EXP": g64 * b.astype(D), "LOG": g64 / a.astype(D), "SQRT": 0.5 * g64 / b.astype(D)}[name]
        got = gpu(backend, bwd, ins, [np.full(a.shape, 9, F)])[0]
        refb = cpu(ref_lib, bwd, ins, [np.full(a.shape, 9, F)])[0]
        within(got, want64, 2 * EPS * np.abs(want64), "kernel backward")
        within(refb, want64, 2 * EPS * np.abs(want64), "reference backward")
        if name == "EXP" and g is None:
            assert np.array_equal(got.view(np.uint32), b.view(np.uint32))  # a copy


# ---- CLAMP ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(-0.25, NAN), (NAN, 0.5), (-0.25, 0.5)], ids=["min", "max", "both"])
def test_clamp(backend, ref_lib, lo, hi):
    """NaN is the builder's "no bound".  Inputs sit exactly on each bound: forward keeps them, backward zeroes them (b >= hi, b <= lo)."""
    a = rnd((4, 5, 6, 3), 71)
    a.flat[::7] = F(-0.25)
    a.flat[3::11] = F(0.5)
    a.flat[5::13] = np.nextafter(F(0.5), F(0))
    a.flat[6::17] = np.nextafter(F(-0.25), F(0))
    want = a.copy()
    if not np.isnan(lo):
        want = np.maximum(want, F(lo))
    if not np.isnan(hi):
        want = np.minimum(want, F(hi))
    got = gpu(backend, nnc.CMD_CLAMP_FORWARD(lo, hi), [a], [np.full(a.shape, 9, F)])[0]
    ref = cpu(ref_lib, nnc.CMD_CLAMP_FORWARD(lo, hi), [a], [np.full(a.shape, 9, F)])[0]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(ref.view(np.uint32), want.view(np.uint32))
    b = want
    inside = np.ones(a.shape, bool)
    if not np.isnan(lo):
        inside &= b > F(lo)
    if not np.isnan(hi):
        inside &= b < F(hi)
    assert (b[~inside] == (F(lo) if np.isnan(hi) else F(hi))).any()  # (the on-the-bound inputs are there)
    for g in (rnd(a.shape, 72), None):
        wantb = np.where(inside, np.ones(a.shape, F) if g is None else g, F(0))
        got = gpu(backend, nnc.CMD_CLAMP_BACKWARD(lo, hi), [g, None, b], [np.full(a.shape, 9, F)])[0]
        assert np.array_equal(got.view(np.uint32), wantb.view(np.uint32))
        if g is not None:  # (the reference reads g's shape before it tests g for NULL, ew_cpu_ref.c:1364: without g it is numpy alone)
            ref = cpu(ref_lib, nnc.CMD_CLAMP_BACKWARD(lo, hi), [g, None, b], [np.full(a.shape, 9, F)])[0]
            assert np.array_equal(ref.view(np.uint32), wantb.view(np.uint32))


# ---- MASKED_FILL ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mshape", [(4, 5, 6), (1, 5, 6), (4, 5, 1)], ids=["same", "leading", "last"])
@pytest.mark.parametrize("mdt", [F, np.int32], ids=["f32-mask", "i32-mask"])
def test_masked_fill(backend, ref_lib, mdt, mshape):
    """c = (mask == eq) ? fill : a, backward h = (mask == eq) ? 0 : g; the fill value is one that a already holds."""
    a, g = rnd((4, 5, 6), 81), rnd((4, 5, 6), 82)
    mask = (np.random.default_rng(83).integers(0, 3, mshape)).astype(mdt)
    fill = float(a.flat[7])
    hit = np.broadcast_to(mask == 2, a.shape)
    assert hit.any() and not hit.all()
    for cmd, ins, want in ((nnc.CMD_MASKED_FILL_FORWARD(2, fill), [a, mask], np.where(hit, F(fill), a)),
                           (nnc.CMD_MASKED_FILL_BACKWARD(2, fill), [g, a, mask], np.where(hit, F(0), g))):
        got = gpu(backend, cmd, ins, [np.full(a.shape, 9, F)])[0]
        ref = cpu(ref_lib, cmd, ins, [np.full(a.shape, 9, F)])[0]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(ref.view(np.uint32), want.view(np.uint32))


# ---- REDUCE_ISNAN -----------------------------------------------------------------------------------------------------------------
def two_stage_slices(R, n, cus=256):
    """The slicing of bcast_reduce restated: (slices, elements per slice), or None below the two-stage threshold."""
    if R < 4096:
        return None
    slices = (4 * cus + n - 1) // n
    slices = max(1, min(slices, (R + 2047) // 2048, 65535))
    per = (R + slices - 1) // slices
    return (R + per - 1) // per, per


@pytest.mark.parametrize("dt", [F, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("R", [1000, 6000, 4096 * 3 + 5])
def test_reduce_isnan(backend, ref_lib, R, dt):
    """int32 output, exactly 0 or 1.  The flag rides through a float max-reduction as the subnormal with bit pattern 1: a flushed subnormal,
    or a slice whose partial is dropped, loses it.  One NaN at the first / last element of the reduced sub-space, at the last element of a
    slice and the first of the next (for the small size: around the middle); only row 1 of 3 holds it."""
    sl = two_stage_slices(R, 3)
    assert (sl is None) == (R < 4096) and (sl is None or sl[0] >= 2)
    per = sl[1] if sl else R // 2
    x = rnd((3, R), 91).astype(dt)
    cmd = nnc.CMD_REDUCE_ISNAN_FORWARD(1)
    for pos in (None, 0, R - 1, per - 1, per, (sl[0] - 1) * per if sl else R // 3):
        a = x.copy()
        if pos is not None:
            a[1, pos] = np.nan
        want = np.array([[0], [0 if pos is None else 1], [0]], np.int32)
        got = gpu(backend, cmd, [a], [np.full((3, 1), 9, np.int32)])[0]
        assert got.dtype == np.int32 and np.array_equal(got, want), "NaN at %s: %s" % (pos, got.ravel())
        if dt == F:
            ref = cpu(ref_lib, cmd, [a], [np.full((3, 1), 9, np.int32)])[0]
            assert np.array_equal(ref, want)


# ---- element-wise MIN / MAX backward, REDUCE_NORM2 backward -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["MIN", "MAX"])
def test_min_max_backward_ties_and_broadcast_gradient(backend, ref_lib, name):
    """(g, a, b) -> (ha, hb): the smaller (larger) operand takes g, a tie gives it to both -- selections, bit-exact."""
    shape = (4, 5, 6, 3)
    a, b = rnd(shape, 101), rnd(shape, 102)
    b.flat[::3] = a.flat[::3]
    less = a < b if name == "MIN" else a > b
    tie = a == b
    cmd = nnc.generic_cmd(name + "_BACKWARD")
    for g in (rnd(shape, 103), rnd((1, 1, 1, 3), 104), rnd((1,), 105)):
        gb = np.broadcast_to(g, shape)
        ha, hb = np.where(less | tie, gb, F(0)), np.where(~less | tie, gb, F(0))
        got = gpu(backend, cmd, [g, a, b], [np.full(shape, 9, F), np.full(shape, 9, F)])
        assert np.array_equal(got[0].view(np.uint32), ha.view(np.uint32)) and np.array_equal(got[1].view(np.uint32), hb.view(np.uint32))
        if g.shape == shape:  # (the reference reads g with the outputs' shape)
            ref = cpu(ref_lib, cmd, [g, a, b], [np.full(shape, 9, F), np.full(shape, 9, F)])
            assert np.array_equal(ref[0], ha) and np.array_equal(ref[1], hb)


def test_reduce_norm2_backward_ties_and_broadcast_gradient(backend, ref_lib):
    """h = g a / b with g and b = |a|_2 of the reduced shape broadcast back: two roundings.  Elements of equal magnitude in one reduced
    sub-space must receive gradients of equal magnitude, bit for bit."""
    shape, axes = (4, 5, 6, 3), (1, 2)
    a = rnd(shape, 111)
    a[:, 0, 0, :] = -a[:, 4, 5, :]
    rshape = (4, 1, 1, 3)
    b = np.sqrt((a.astype(D) ** 2).sum(axis=axes, keepdims=True)).astype(F)
    cmd = nnc.CMD_REDUCE_NORM2_BACKWARD(*axes)
    for g in (rnd(rshape, 112), None):
        g64 = np.ones(rshape, D) if g is None else g.astype(D)
        want64 = g64 * a.astype(D) / b.astype(D)
        got = gpu(backend, cmd, [g, a, b], [np.full(shape, 9, F)])[0]
        ref = cpu(ref_lib, cmd, [g, a, b], [np.full(shape, 9, F)])[0]
        within(got, want64, 2 * EPS * np.abs(want64), "kernel")
        within(ref, want64, 2 * EPS * np.abs(want64), "reference")
        assert np.array_equal(got[:, 0, 0, :].view(np.uint32), (-got[:, 4, 5, :]).view(np.uint32))
