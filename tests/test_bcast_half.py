"""Broadcast arithmetic on dense CCV_16F tensors without fp32 images (ccv_amd/csrc/bcast_ops.h; tunable BCAST_HALF_NATIVE): ADD, same-shape MUL, SCALAR_MUL,
REDUCE_SUM and REDUCE_MEAN, forward and backward, on shapes that are flat, a period ([I][R][Cc] against [I][Cc]) or runs ([Q][M][L] against [M]).

Expectations are float64 numpy on the widened half inputs, with p, q, s as the float32 the command carries.  Bounds are derived, not tuned (u = 2^-24):
  a stored half                 2^-11 |want| + 2^-24
  a one-rounding map            2 u S, S = the expression on absolute values; 3 u S for ADD (two products and a sum)
  a sum of R terms              (R + 2) u S
The reference's CPU backend runs every case on the widened inputs and must meet the fp32 part of the bound alone (the bound is not too tight);
test_wrong_expectations_break_the_bounds shows it is not too loose.  The maps with one fp32 rounding or none (SCALAR_MUL, MUL and its gradients, ADD with
p = q = 1, the flat gradients of ADD, the REDUCE_* backward broadcasts) carry the bits of the route with the key at 0.
"""
import os
import re
import numpy as np
import pytest
from ccv_amd import nnc
from harness import exec_on, make_tensors
from test_mbconv_half import counts, records, key_off, bits, within, ref_run, aliased

F, H, D = np.float32, np.float16, np.float64
KEY = "BCAST_HALF_NATIVE"
U = 2.0 ** -24
P, Q, S = 0.7, -1.3, 0.3
P64, Q64, S64 = D(F(P)), D(F(Q)), D(F(S))

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccv_amd", "csrc", "chan_sums.h")
with open(_HDR) as _f:
    _TEXT = _f.read()
SLICE, SHORT = (int(re.search(r"constexpr int %s = (\d+);" % k, _TEXT).group(1)) for k in ("CHAN_RUN_SLICE", "CHAN_SHORT_PLANE"))

_DATA = {}


def data(shape, seed=0):
    """U(-2, 2) exact halves, made once per (shape, seed), read-only"""
    key = (tuple(shape), seed)
    if key not in _DATA:
        rng = np.random.default_rng(1000 + seed + 7 * int(np.prod(shape)) + len(shape))
        x = ((rng.random(shape) - 0.5) * 4).astype(H)
        x.setflags(write=False)
        _DATA[key] = x
    return _DATA[key]


def stored(want):
    return 2.0 ** -11 * np.abs(want) + 2.0 ** -24


def run(L, cmd, ins, outs, flags=0):
    r, res = exec_on(L, nnc.GPU_MEMORY, cmd, nnc.NO_HINT, flags, ins, outs)
    assert r == 0, "backend returned %d" % r
    return res


def native(L, fn):
    """fn() with no half tensor staged through an fp32 image"""
    s0, n0 = counts(L)
    out = fn()
    s1, n1 = counts(L)
    assert s1 == s0 and n1 > n0, "staged %d, native %d" % (s1 - s0, n1 - n0)
    return out


def fill(shape):
    return np.full(shape, 3, H)


def same_bits(a, b, what):
    assert np.array_equal(bits(a), bits(b)), "%s: %d elements differ from the fp32-image route" % (what, int((bits(a) != bits(b)).sum()))


def pad(small, nd):
    return (1,) * (nd - len(small)) + tuple(small)


def reduced_axes(big, small):
    sp = pad(small, len(big))
    return tuple(k for k in range(len(big)) if sp[k] == 1 and big[k] > 1)


# ---- the operations in float64 --------------------------------------------------------------------------------------------------------------------------
def add_want(a, b, p=P64, q=Q64):
    a, b = a.astype(D), b.astype(D)
    return p * a + q * b, np.abs(p * a) + np.abs(q * b)


def sum_want(x, small, scale):
    """(want, S, R): the sum of scale * x over the axes on which `small` is 1, in small's shape"""
    axes = reduced_axes(x.shape, small)
    t = scale * x.astype(D)
    want, s = t.sum(axis=axes, keepdims=True).reshape(small), np.abs(t).sum(axis=axes, keepdims=True).reshape(small)
    return want, s, x.size // want.size


def check_map(L, ref, cmd, ins, shape, want, s, k, what, off_bits):
    """One map command on the native route, against float64, the reference and (off_bits) the bits of the key-off route."""
    got = native(L, lambda: run(L, cmd, ins, [fill(shape)]))[0]
    assert got.dtype == H
    within(got, want, stored(want) + k * U * s, what)
    r = ref_run(ref, cmd, ins, [np.zeros(shape, H)])[0]
    within(r, want, k * U * s, what + ", reference")
    with key_off(L, KEY):
        off = run(L, cmd, ins, [fill(shape)])[0]
    within(off, want, stored(want) + k * U * s, what + ", fp32 images")
    if off_bits:
        same_bits(got, off, what)
    return got


def check_sum(L, ref, cmd, ins, small, want, s, R, what):
    got = native(L, lambda: run(L, cmd, ins, [fill(small)]))[0]
    assert got.dtype == H
    within(got, want, stored(want) + (R + 2) * U * s, what)
    again = run(L, cmd, ins, [fill(small)])[0]
    assert np.array_equal(bits(got), bits(again)), what + ": two runs differ"
    r = ref_run(ref, cmd, ins, [np.zeros(small, H)])[0]
    within(r, want, (R + 2) * U * s, what + ", reference")
    with key_off(L, KEY):
        off = run(L, cmd, ins, [fill(small)])[0]
    within(off, want, stored(want) + (R + 2) * U * s, what + ", fp32 images")


def check_broadcast_case(L, ref, big, small):
    """Every command of the issue on one (big, small) pair: ADD forward with the small operand second and first, ADD backward (both outputs, each alone, the
    small one in either slot), REDUCE_SUM / REDUCE_MEAN forward over the axes that give `small`, and their backward."""
    x, sm, g = data(big), data(small, 1), data(big, 2)
    tag = "%s against %s" % (list(big), list(small))
    # ADD forward
    want, s = add_want(x, sm)
    check_map(L, ref, nnc.CMD_ADD_FORWARD(P, Q), [x, sm], big, want, s, 3, "ADD, small second, " + tag, False)
    want, s = add_want(sm, x)
    check_map(L, ref, nnc.CMD_ADD_FORWARD(P, Q), [sm, x], big, want, s, 3, "ADD, small first, " + tag, False)
    want, s = add_want(x, sm, 1.0, 1.0)
    check_map(L, ref, nnc.CMD_ADD_FORWARD(1, 1), [x, sm], big, want, s, 3, "ADD p = q = 1, " + tag, True)
    # ADD backward: da = p g (flat), db = q sum g
    bwd = nnc.CMD_ADD_BACKWARD(P, Q)
    wa, sa = P64 * g.astype(D), np.abs(P64 * g.astype(D))
    wb, sb, R = sum_want(g, small, Q64)
    da, db = native(L, lambda: run(L, bwd, [g], [fill(big), fill(small)]))
    within(da, wa, stored(wa) + 2 * U * sa, "ADD backward, large, " + tag)
    within(db, wb, stored(wb) + (R + 2) * U * sb, "ADD backward, small, " + tag)
    ra, rb = ref_run(ref, bwd, [g], [np.zeros(big, H), np.zeros(small, H)])
    within(ra, wa, 2 * U * sa, "ADD backward, large, reference, " + tag)
    within(rb, wb, (R + 2) * U * sb, "ADD backward, small, reference, " + tag)
    with key_off(L, KEY):
        oa, ob = run(L, bwd, [g], [fill(big), fill(small)])
    same_bits(da, oa, "ADD backward, large, " + tag)
    within(ob, wb, stored(wb) + (R + 2) * U * sb, "ADD backward, small, fp32 images, " + tag)
    a_only, none = native(L, lambda: run(L, bwd, [g], [fill(big), None]))
    assert none is None and np.array_equal(bits(a_only), bits(da))
    none, b_only = native(L, lambda: run(L, bwd, [g], [None, fill(small)]))
    assert none is None and np.array_equal(bits(b_only), bits(db))
    ws, ss, _ = sum_want(g, small, P64)  # the small operand was a: da = p sum g, db = q g
    da2, db2 = native(L, lambda: run(L, bwd, [g], [fill(small), fill(big)]))
    within(da2, ws, stored(ws) + (R + 2) * U * ss, "ADD backward, small first, " + tag)
    wq = Q64 * g.astype(D)
    within(db2, wq, stored(wq) + 2 * U * np.abs(wq), "ADD backward, large second, " + tag)
    # REDUCE_SUM / REDUCE_MEAN over the axes that give `small`
    axes = reduced_axes(big, small)
    for name, scale in (("SUM", 1.0), ("MEAN", 1.0 / R)):
        fwd, back = getattr(nnc, "CMD_REDUCE_%s_FORWARD" % name)(*axes), getattr(nnc, "CMD_REDUCE_%s_BACKWARD" % name)(*axes)
        want, s, _ = sum_want(x, small, scale)
        check_sum(L, ref, fwd, [x], small, want, s, R, "REDUCE_%s, %s" % (name, tag))
        wh = np.broadcast_to(scale * sm.astype(D).reshape(pad(small, len(big))), big)
        check_map(L, ref, back, [sm], big, wh, np.abs(wh), 2, "REDUCE_%s backward, %s" % (name, tag), True)


# ---- flat -------------------------------------------------------------------------------------------------------------------------------------------------
def flat_exec(L, cmd, ins, n_out, mode):
    """ins: half arrays or None -> the half outputs.  "misaligned": every tensor starts 2 bytes past a 16-byte boundary; "inplace": output 0 is input 0."""
    if mode == "misaligned":
        ts = aliased(L, [x for x in ins if x is not None] + [fill(ins[0].shape) for _ in range(n_out)], 1)
        assert all(t.ptr % 16 == 2 for t in ts)
        it = iter(ts)
        tin = [None if x is None else next(it) for x in ins]
        tout = list(it)
    else:
        tin = make_tensors(L, nnc.GPU_MEMORY, list(ins))
        tout = make_tensors(L, nnc.GPU_MEMORY, [fill(ins[0].shape) for _ in range(n_out)])
        if mode == "inplace":
            tout[0] = tin[0]
    assert L.cmd_exec(cmd, nnc.NO_HINT, 0, tin, tout) == 0
    return [t.numpy() for t in tout]


@pytest.mark.parametrize("size", [5, 3240, 3243, "misaligned", "inplace"], ids=str)
def test_flat(backend, ref_lib, size):
    """5 elements are a tail alone, 3240 are 405 whole vectors, 3243 add a tail of three; misaligned: 3240 elements on bases one element off 16-byte alignment
    (the scalar loop); inplace: the output is input 0 (what the host issues for ADD and SCALAR_MUL)."""
    L = backend
    mode = size if isinstance(size, str) else ""
    n = 3240 if mode else size
    a, b, g = data((3243,))[:n], data((3243,), 1)[:n], data((3243,), 2)[:n]
    a64, b64, g64 = a.astype(D), b.astype(D), g.astype(D)
    cases = [  # command, inputs, wanted outputs, S per output, rounding count k, same bits as the key-off route
        ("SCALAR_MUL", nnc.CMD_SCALAR_MUL_FORWARD(S), [a], [S64 * a64], 2, True),
        ("SCALAR_MUL backward", nnc.CMD_SCALAR_MUL_BACKWARD(S), [g], [S64 * g64], 2, True),
        ("ADD", nnc.CMD_ADD_FORWARD(P, Q), [a, b], [P64 * a64 + Q64 * b64], 3, False),
        ("ADD p = q = 1", nnc.CMD_ADD_FORWARD(1, 1), [a, b], [a64 + b64], 3, True),
        ("ADD one operand", nnc.CMD_ADD_FORWARD(P, 0), [a, None], [P64 * a64], 2, True),
        ("ADD backward", nnc.CMD_ADD_BACKWARD(P, Q), [g], [P64 * g64, Q64 * g64], 2, True),
        ("MUL", nnc.CMD_MUL_FORWARD(P), [a, b], [P64 * a64 * b64], 2, True),
        ("MUL backward", nnc.CMD_MUL_BACKWARD(P), [g, a, b], [P64 * g64 * b64, P64 * g64 * a64], 2, True),
        ("REDUCE_SUM of nothing", nnc.CMD_REDUCE_SUM_FORWARD(0), [a], [a64], 2, True),
        ("REDUCE_MEAN backward of nothing", nnc.CMD_REDUCE_MEAN_BACKWARD(0), [g], [g64], 2, True),
    ]
    for what, cmd, ins, wants, k, same in cases:
        if mode == "inplace" and len(wants) > 1:  # (a second output would read the input the first one has replaced, on either route)
            continue
        s_abs = [np.abs(P64 * a64) + np.abs(Q64 * b64)] if what == "ADD" else [np.abs(a64) + np.abs(b64)] if what == "ADD p = q = 1" else [np.abs(w) for w in wants]
        gots = native(L, lambda: flat_exec(L, cmd, ins, len(wants), mode))
        for got, want, s in zip(gots, wants, s_abs):
            assert got.dtype == H
            within(got, want, stored(want) + k * U * s, what)
        refs = ref_run(ref_lib, cmd, ins, [np.zeros(n, H) for _ in wants])
        for r, want, s in zip(refs, wants, s_abs):
            within(r, want, k * U * s, what + ", reference")
        with key_off(L, KEY):
            s0, n0 = counts(L)
            offs = flat_exec(L, cmd, ins, len(wants), mode)
            s1, n1 = counts(L)
            assert n1 == n0 and s1 > s0, what
        for got, off, want, s in zip(gots, offs, wants, s_abs):
            within(off, want, stored(want) + k * U * s, what + ", fp32 images")
            if same:
                same_bits(got, off, what)
    # MUL backward, each gradient alone
    cmd = nnc.CMD_MUL_BACKWARD(P)
    da, none = native(L, lambda: run(L, cmd, [g, a, b], [fill(n), None]))
    none2, db = native(L, lambda: run(L, cmd, [g, a, b], [None, fill(n)]))
    assert none is None and none2 is None
    assert np.array_equal(bits(da), bits(((F(P) * g.astype(F)) * b.astype(F)).astype(H))) and np.array_equal(bits(db), bits(((F(P) * g.astype(F)) * a.astype(F)).astype(H)))


# ---- period: big [I][R][Cc], small [I][Cc] -------------------------------------------------------------------------------------------------------------------
PERIOD = [
    ((2, 3, 5, 8), (8,)),                # I = 1, R = 30, Cc = 8: one vector per row
    ((3, 5, 5, 8), (3, 1, 1, 8)),        # NHWC map against one value per (image, channel): I = 3, R = 25
    ((67, 24), (24,)),                   # R = 67: past colsum_plan's 64-row slice floor
    ((3, 5), (5,)),                      # Cc = 5: the scalar instance
    ((3, 3, 5), (3, 1, 5)),              # ... with I = 3
    ((3, 67, 8), (3, 1, 8)),             # I = 3, R = 67
    ((3, 24), (1, 24)),                  # R = 3, three vectors per row
    ((3, 2056), (2056,)),                # 257 vectors per row: more than one column tile of 256 lanes
    ((3, 3, 2056), (3, 1, 2056)),        # ... with I = 3
    ((1, 24), (24,)),                    # R = 1: nothing is broadcast, flat
]


@pytest.mark.parametrize("big,small", PERIOD, ids=["%s-%s" % ("x".join(map(str, b)), "x".join(map(str, s))) for b, s in PERIOD])
def test_period(backend, ref_lib, big, small):
    if np.prod(big) == np.prod(small):  # flat: the sums have nothing to add up; ADD alone
        x, sm = data(big), data(small, 1)
        want, s = add_want(x, sm)
        check_map(backend, ref_lib, nnc.CMD_ADD_FORWARD(P, Q), [x, sm], big, want, s, 3, "ADD, R = 1", False)
        return
    check_broadcast_case(backend, ref_lib, big, small)


def test_period_misaligned(backend):
    """Cc = 8 on bases one element off 16-byte alignment: the scalar instance, the same values."""
    L = backend
    big, small = (2, 3, 5, 8), (8,)
    x, sm = data(big), data(small, 1)
    want, s = add_want(x, sm)
    xt, st, ot = aliased(L, [x, sm, fill(big)], 1)
    assert all(t.ptr % 16 == 2 for t in (xt, st, ot))
    native(L, lambda: L.cmd_exec(nnc.CMD_ADD_FORWARD(P, Q), nnc.NO_HINT, 0, [xt, st], [ot]))
    within(ot.numpy(), want, stored(want) + 3 * U * s, "ADD, misaligned")
    (gt,) = aliased(L, [sm], 1)
    (ht,) = aliased(L, [fill(big)], 1)
    native(L, lambda: L.cmd_exec(nnc.CMD_REDUCE_SUM_BACKWARD(0, 1, 2), nnc.NO_HINT, 0, [gt], [ht]))
    assert np.array_equal(bits(ht.numpy()), bits(np.broadcast_to(sm, big)))
    (dt,) = aliased(L, [fill(small)], 1)
    native(L, lambda: L.cmd_exec(nnc.CMD_REDUCE_SUM_FORWARD(0, 1, 2), nnc.NO_HINT, 0, [xt], [dt]))
    w, sa, R = sum_want(x, small, 1.0)
    within(dt.numpy(), w, stored(w) + (R + 2) * U * sa, "REDUCE_SUM, misaligned")


# ---- run: big [Q][M][L], small [M] ---------------------------------------------------------------------------------------------------------------------------
RUN = [
    ((2, 3, 5, 7), (1, 3, 1, 1)),        # NCHW map against one value per channel: Q = 2, M = 3, L = 35 (runs start unaligned from the second on)
    ((2, 3, 5, 7), (2, 3, 1, 1)),        # ... per (image, channel): Q = 1, M = 6
    ((5, 64), (5, 1)),                   # [A][B] against [A][1], L = 64
    ((3, 3, 2), (1, 3, 1)),              # L = 2
    ((3, 7), (3, 1)),                    # L = 7
    ((3, 3, 8), (1, 3, 1)),              # L = 8: a vector per run
    ((3, 5, 7), (1,)),                   # a one-element small: Q = M = 1, one run of the whole tensor
    ((3, 3, SHORT), (1, 3, 1)),          # the longest plane the sums give sixteen lanes each
    ((3, 3, SHORT + 1), (1, 3, 1)),      # one above: a wave per plane
    ((SLICE - 1,), (1,)),                # one below the slicing constant
    ((3, SLICE), (3, 1)),                # at it: M = 3, not sliced
    ((SLICE + 8,), (1,)),                # eight above: two slices
    ((3, 3, SLICE + 8), (1, 3, 1)),      # ... with Q = M = 3
    ((3, 4100), (1,)),                   # the sum of a whole tensor to one value
    ((3, 4100), (1, 1)),
]


@pytest.mark.parametrize("big,small", RUN, ids=["%s-%s" % ("x".join(map(str, b)), "x".join(map(str, s))) for b, s in RUN])
def test_run(backend, ref_lib, big, small):
    check_broadcast_case(backend, ref_lib, big, small)


# ---- bounds, overflow ---------------------------------------------------------------------------------------------------------------------------------------
def test_wrong_expectations_break_the_bounds(backend):
    """q dropped, a sum that misses its last row, a mean divided by the wrong count: each breaks its bound."""
    L = backend
    big, small = (67, 24), (24,)
    x, sm = data(big), data(small, 1)
    got = run(L, nnc.CMD_ADD_FORWARD(P, Q), [x, sm], [fill(big)])[0]
    want, s = add_want(x, sm)
    within(got, want, stored(want) + 3 * U * s, "ADD")
    with pytest.raises(AssertionError):
        within(got, P64 * x.astype(D), stored(want) + 3 * U * s, "ADD, q dropped")
    got = run(L, nnc.CMD_REDUCE_SUM_FORWARD(0), [x], [fill((1, 24))])[0]
    want, s, R = sum_want(x, (1, 24), 1.0)
    within(got, want, stored(want) + (R + 2) * U * s, "REDUCE_SUM")
    with pytest.raises(AssertionError):
        within(got, x[:-1].astype(D).sum(axis=0, keepdims=True), stored(want) + (R + 2) * U * s, "REDUCE_SUM, last row missing")
    got = run(L, nnc.CMD_REDUCE_MEAN_FORWARD(0), [x], [fill((1, 24))])[0]
    want, s, R = sum_want(x, (1, 24), 1.0 / 67)
    within(got, want, stored(want) + (R + 2) * U * s, "REDUCE_MEAN")
    with pytest.raises(AssertionError):
        within(got, want * 67 / 66, stored(want) + (R + 2) * U * s, "REDUCE_MEAN, wrong count")


def test_sum_overflow_is_infinity(backend):
    """A column of 40 values of 60000 sums to 2.4e6: +inf in half, on both routes; the fp32 partials do not overflow on the way."""
    L = backend
    x = np.full((40, 8), 60000, H)
    got = native(L, lambda: run(L, nnc.CMD_REDUCE_SUM_FORWARD(0), [x], [fill((1, 8))]))[0]
    assert np.isposinf(got).all(), got
    planes = native(L, lambda: run(L, nnc.CMD_REDUCE_SUM_FORWARD(1), [np.ascontiguousarray(x.T)], [fill((8, 1))]))[0]
    assert np.isposinf(planes).all(), planes
    with key_off(L, KEY):
        off = run(L, nnc.CMD_REDUCE_SUM_FORWARD(0), [x], [fill((1, 8))])[0]
    assert np.isposinf(off).all(), off


# ---- routes -------------------------------------------------------------------------------------------------------------------------------------------------
def test_routes(backend):
    """One case of each command.  Key at 1: no tensor staged, the used tensors native, the launch records hold the bcast_* names and no conversion.  Key at 0: the
    old counts come back and no bcast_* record."""
    L = backend
    assert L.tune_get(KEY) == 1
    L.dll.nnc_mi355x_last_kernel_name.restype = nnc.C.c_char_p
    big, small = (2, 3, 5, 8), (8,)
    x, y, sm, g = data(big), data(big, 3), data(small, 1), data(big, 2)
    steps = [  # command, inputs, outputs, half tensors used, a kernel of the launch records
        (nnc.CMD_SCALAR_MUL_FORWARD(S), [x], [fill(big)], 2, "bcast_scalar_mul|nnc::ew_map_kernel"),
        (nnc.CMD_SCALAR_MUL_BACKWARD(S), [g], [fill(big)], 2, "bcast_scalar_mul|nnc::ew_map_kernel"),
        (nnc.CMD_ADD_FORWARD(P, Q), [x, sm], [fill(big)], 3, "bcast_add_fwd|nnc::bcast_period_kernel"),
        (nnc.CMD_ADD_FORWARD(P, Q), [x, y], [fill(big)], 3, "bcast_add_fwd|nnc::ew_map_kernel"),
        (nnc.CMD_ADD_BACKWARD(P, Q), [g], [fill(big), fill(small)], 3, "bcast_add_bwd|nnc::chan_reduce_rows_kernel"),
        (nnc.CMD_MUL_FORWARD(P), [x, y], [fill(big)], 3, "bcast_mul_fwd|nnc::ew_map_kernel"),
        (nnc.CMD_MUL_BACKWARD(P), [g, x, y], [fill(big), fill(big)], 5, "bcast_mul_bwd|nnc::ew_map_kernel"),
        (nnc.CMD_REDUCE_SUM_FORWARD(0, 1, 2), [x], [fill(small)], 2, "bcast_reduce_fwd|nnc::chan_reduce_rows_kernel"),
        (nnc.CMD_REDUCE_SUM_BACKWARD(0, 1, 2), [sm], [fill(big)], 2, "bcast_reduce_bwd|nnc::bcast_period_kernel"),
        (nnc.CMD_REDUCE_MEAN_FORWARD(2, 3), [x], [fill((2, 3, 1, 1))], 2, "bcast_reduce_fwd|nnc::chan_reduce_short_planes_kernel"),
        (nnc.CMD_REDUCE_MEAN_BACKWARD(2, 3), [data((2, 3, 1, 1), 1)], [fill(big)], 2, "bcast_reduce_bwd|nnc::bcast_run_kernel"),
        (nnc.CMD_REDUCE_MEAN_FORWARD(1, 2), [x], [fill((2, 1, 1, 8))], 2, "bcast_reduce_fwd|nnc::rows_image_sum_kernel"),
    ]
    for cmd, ins, outs, halves, kernel in steps:
        s0, n0 = counts(L)
        _, names = records(L, lambda: run(L, cmd, ins, outs))
        assert counts(L) == (s0, n0 + halves), (kernel, counts(L), (s0, n0))
        assert kernel in names and all(x.startswith("bcast_") for x in names), names
        assert not any("half_up_kernel" in x or "half_down_kernel" in x for x in names), names
        last = L.dll.nnc_mi355x_last_kernel_name().decode()  # a literal of the library, alive after the launcher has returned
        assert last in ("bcast_flat", "bcast_period", "bcast_run", "bcast_sum"), last
        with key_off(L, KEY):
            s0, n0 = counts(L)
            _, names = records(L, lambda: run(L, cmd, ins, outs))
            assert counts(L) == (s0 + halves, n0), (kernel, counts(L), (s0, n0))
            assert not any(x.startswith("bcast_") for x in names), names


def test_sum_routes_at_the_plane_lengths(backend):
    """Which kernel sums a run, by its length alone: sixteen lanes per plane up to CHAN_SHORT_PLANE elements, a wave per plane above, slices above CHAN_RUN_SLICE
    where the planes are few.  The launch records name the kernel that ran."""
    L = backend
    L.dll.nnc_mi355x_last_kernel_name.restype = nnc.C.c_char_p
    for big, small, kernel in (((3, 3, SHORT), (1, 3, 1), "chan_reduce_short_planes_kernel"), ((3, 3, SHORT + 1), (1, 3, 1), "chan_reduce_planes_kernel"),
                               ((SLICE - 1,), (1,), "chan_reduce_planes_kernel"), ((3, SLICE), (3, 1), "chan_reduce_planes_kernel"),
                               ((SLICE + 8,), (1,), "chan_reduce_plane_slices_kernel"), ((3, 3, SLICE + 8), (1, 3, 1), "chan_reduce_plane_slices_kernel")):
        x = data(big)
        _, names = records(L, lambda: native(L, lambda: run(L, nnc.CMD_REDUCE_SUM_FORWARD(*reduced_axes(big, small)), [x], [fill(small)])))
        assert names == ["bcast_reduce_fwd|nnc::" + kernel], (big, names)
        assert L.dll.nnc_mi355x_last_kernel_name() == b"bcast_sum"


def form(L, big, small, is_sum):
    """bcast_ops.h's form of a pair of shapes (host arithmetic only): 0 refused, 1 flat, 2 period, 3 run"""
    f = L.dll.nnc_mi355x_debug_bcast_form
    f.restype, f.argtypes = nnc.C.c_int, [nnc.C.POINTER(nnc.C.c_int), nnc.C.POINTER(nnc.C.c_int), nnc.C.c_int]
    arr = lambda d: (nnc.C.c_int * 4)(*pad(d, 4))
    return f(arr(big), arr(small), int(is_sum))


def test_forms_and_the_image_limit_of_the_sums(backend):
    """The plan's forms for the shapes of this file, and period form with more images than a grid dimension holds: the maps have no limit on I and stay
    native, the per-image sums (the images are a grid dimension of rows_image_sum) are refused from 65 536 images on."""
    L = backend
    for big, small in PERIOD[:-1]:
        assert form(L, big, small, False) == 2 and form(L, big, small, True) == 2, (big, small)
    for big, small in RUN:
        assert form(L, big, small, False) == 3 and form(L, big, small, True) == 3, (big, small)
    assert form(L, (1, 24), (24,), False) == 1 and form(L, (3, 4, 5, 6), (3, 1, 5, 1), False) == 0 and form(L, (3, 4, 5, 6), (3, 1, 5, 1), True) == 0
    assert form(L, (65535, 2, 8), (65535, 1, 8), True) == 2 and form(L, (65536, 2, 8), (65536, 1, 8), True) == 0
    assert form(L, (65536, 2, 8), (65536, 1, 8), False) == 2 and form(L, (65536, 2, 8), (8,), True) == 2  # (I = 1: chan_reduce_rows)
    assert form(L, (65536, 32768), (32768,), False) == 0  # 2^31 elements


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------------
def staged(L, fn, halves):
    s0, n0 = counts(L)
    out, names = records(L, fn)
    assert counts(L) == (s0 + halves, n0), (counts(L), (s0, n0))
    assert not any(x.startswith("bcast_") for x in names), names
    return out


def test_refusals_keep_their_route_and_their_results(backend):
    L = backend
    # an output view: a [6, 4] window of [6, 10]
    a, b = data((6, 4)), data((4,), 1)
    want, s = add_want(a, b)
    at, bt, ct = make_tensors(L, nnc.GPU_MEMORY, [a, b, np.full((6, 10), 5, H)])
    view = ct.view((6, 4), (10, 1), 3)
    assert staged(L, lambda: L.cmd_exec(nnc.CMD_ADD_FORWARD(P, Q), nnc.NO_HINT, 0, [at, bt], [view]), 3) == 0
    out = ct.numpy()
    within(out[:, 3:7], want, stored(want) + 3 * U * s, "an output view")
    assert (out[:, :3] == 5).all() and (out[:, 7:] == 5).all()
    # ACCUMULATE_OUTPUT: the bits of the key-off route
    x, y = data((67, 24)), data((24,), 1)
    with key_off(L, KEY):
        off = run(L, nnc.CMD_ADD_FORWARD(P, Q), [x, y], [fill((67, 24))], nnc.ACCUMULATE_OUTPUT)[0]
    got = staged(L, lambda: run(L, nnc.CMD_ADD_FORWARD(P, Q), [x, y], [fill((67, 24))], nnc.ACCUMULATE_OUTPUT), 3)[0]
    same_bits(got, off, "ACCUMULATE_OUTPUT")
    # neither operand has the output's shape
    a, b = data((3, 1, 5, 4)), data((1, 6, 1, 4), 1)
    want, s = add_want(a, b)
    got = staged(L, lambda: run(L, nnc.CMD_ADD_FORWARD(P, Q), [a, b], [fill((3, 6, 5, 4))]), 3)[0]
    within(got, want, stored(want) + 3 * U * s, "(3, 1, 5, 4) + (1, 6, 1, 4)")
    # four alternating groups
    a, b = data((3, 4, 5, 6)), data((3, 1, 5, 1), 1)
    want, s = add_want(a, b)
    got = staged(L, lambda: run(L, nnc.CMD_ADD_FORWARD(P, Q), [a, b], [fill((3, 4, 5, 6))]), 3)[0]
    within(got, want, stored(want) + 3 * U * s, "[3, 1, 5, 1]")
    w, sa, R = sum_want(a, (3, 1, 5, 1), 1.0)
    got = staged(L, lambda: run(L, nnc.CMD_REDUCE_SUM_FORWARD(1, 3), [a], [fill((3, 1, 5, 1))]), 2)[0]
    within(got, w, stored(w) + (R + 2) * U * sa, "REDUCE_SUM to [3, 1, 5, 1]")
    # MUL by a broadcast operand the plane-scale kernels do not take
    a, b = data((2, 3, 7, 7)), data((1, 3, 1, 1), 1)
    want = P64 * a.astype(D) * b.astype(D)
    got = staged(L, lambda: run(L, nnc.CMD_MUL_FORWARD(P), [a, b], [fill((2, 3, 7, 7))]), 3)[0]
    within(got, want, stored(want) + 2 * U * np.abs(want), "MUL [2, 3, 7, 7] by [1, 3, 1, 1]")
    # backward without g (ones)
    da, db = staged(L, lambda: run(L, nnc.CMD_ADD_BACKWARD(P, Q), [None], [fill((6, 4)), fill((6, 4))]), 2)
    assert np.array_equal(bits(da), bits(np.full((6, 4), F(P), F).astype(H))) and np.array_equal(bits(db), bits(np.full((6, 4), F(Q), F).astype(H)))
    h = staged(L, lambda: run(L, nnc.CMD_REDUCE_SUM_BACKWARD(0), [None], [fill((6, 4))]), 1)[0]
    assert (h == 1).all()
    # half and fp32 tensors in one command
    a, b = data((6, 4)), data((4,), 1).astype(F)
    want, s = add_want(a, b)
    got = staged(L, lambda: run(L, nnc.CMD_ADD_FORWARD(P, Q), [a, b], [fill((6, 4))]), 2)[0]
    within(got, want, stored(want) + 3 * U * s, "half + fp32")
    L.stream_wait(None)
