"""CMUL_FORWARD / CMUL_BACKWARD (rotary position embeddings) on dense CCV_16F tensors without fp32 images (ccv_amd/csrc/cmul_ops.h; tunable CMUL_HALF_NATIVE).

Every accepted case is held to five checks:
  (a) nnc_mi355x_debug_half_counts: the native count rises by the number of half tensors handed over, the staged count does not move;
  (b) bit for bit the same command under CMUL_HALF_NATIVE = 0 (the fp32 kernel between conversions);
  (c) against the float64 value: |got - want| <= 2^-11 |want| + 2^-24 + T 2^-24 S, with S the same expression on absolute values (cabs_terms), reduced as the
      output is, and T = 2 x the number of elements summed per output -- one rounding to half, the half subnormal floor, the fp32 sum.  The same assertion is made
      on the reference's CPU result for the widened inputs, rounded by .astype(float16): the bound holds for the reference alone;
  (d) two runs agree bit for bit;
  (e) exactly one launch record per requested output, of the expected instance of cmul_half_map_kernel / cmul_half_reduce_kernel.
Inputs are U(-2, 2) exact halves from a fixed seed; outputs are pre-filled with 3.
"""
import os
import re
import numpy as np
import pytest
from ccv_amd import nnc
from harness import make_tensors
from test_mbconv_half import counts, records, key_off, bits, ref_run, aliased, within
from test_parity_detect import cx, interleave, cabs_terms, reduce_to, CMUL_PAIRS

F, H, D = np.float32, np.float16, np.float64
KEY = "CMUL_HALF_NATIVE"
FWD, BWD = nnc.CMD_CMUL_FORWARD(), nnc.CMD_CMUL_BACKWARD()
MODES = {0: "MUL", 1: "MUL_CONJ", 2: "CONJ", 3: "SUM"}

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccv_amd", "csrc", "cmul_ops.h")
with open(_HDR) as _f:
    _TEXT = _f.read()
THREADS, TILE = (int(re.search(r"constexpr int %s = (\d+);" % k, _TEXT).group(1)) for k in ("CMUL_THREADS", "CMUL_TILE"))

ROTARY = ((2, 5, 3, 16), (1, 5, 1, 16))
PLAIN2D = ((20, 10), (20, 10))  # the reference's own half case
BIG = ((3, 7, 5, 88), (1, 7, 1, 88))
PAIRS = [((2,), (2,)), ((6,), (6,)), PLAIN2D, ROTARY, ((5, 3, 8), (5, 1, 8)), ((3, 4, 5, 24), (3, 4, 5, 24))] + list(CMUL_PAIRS) + [BIG]
CASES = [(p, swap) for p in PAIRS for swap in (False, True)]
IDS = ["%s*%s%s" % ("x".join(map(str, p[0])), "x".join(map(str, p[1])), "-swapped" if s else "") for p, s in CASES]


def test_the_large_case_takes_more_than_one_workgroup_and_a_partial_one():
    vectors = int(np.prod(BIG[0])) // 8
    assert BIG[0][-1] % 8 == 0 and vectors > TILE * THREADS and vectors % (TILE * THREADS) != 0


_DATA = {}


def data(shape, seed):
    """U(-2, 2) exact halves, made once per (shape, seed), read-only"""
    key = (tuple(shape), seed)
    if key not in _DATA:
        rng = np.random.default_rng(5000 + seed + 7 * int(np.prod(shape)) + len(shape))
        x = ((rng.random(shape) - 0.5) * 4).astype(H)
        x.setflags(write=False)
        _DATA[key] = x
    return _DATA[key]


def fill(shape, dtype=H):
    return None if shape is None else np.full(shape, 3, dtype)


def same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert np.array_equal(bits(a), bits(b)), "%s: %d of %d elements differ" % (what, int((bits(a) != bits(b)).sum()), a.size)


def bound(want, S, T):
    return 2.0 ** -11 * np.abs(want) + 2.0 ** -24 + T * 2.0 ** -24 * S


def execute(L, cmd, ins, outs, misaligned=False, flags=0):
    """half arrays one element off a 16-byte boundary where asked; -> (return value, outputs)"""
    def tensor(x):
        if x is None:
            return None
        if misaligned and x.dtype == H:
            (t,) = aliased(L, [x], 1)
            assert t.ptr % 16 == 2
            return t
        (t,) = make_tensors(L, nnc.GPU_MEMORY, [x])
        assert t.ptr % 16 == 0
        return t
    it, ot = [tensor(x) for x in ins], [tensor(x) for x in outs]
    r = L.cmd_exec(cmd, nnc.NO_HINT, flags, it, ot)
    return r, [None if t is None else t.numpy() for t in ot]


def unit_like(x):
    """(1, 0) pairs: cabs_terms(x, unit) is |x|, element by element"""
    u = np.zeros(x.shape, D)
    u[..., 0::2] = 1
    return u


def forward_want(a, b):
    """(want, S, T, mode) of c = a b"""
    full = np.broadcast_shapes(a.shape, b.shape)
    return np.broadcast_to(interleave(cx(a) * cx(b)), full), np.broadcast_to(cabs_terms(a, b), full), 2, 0


def backward_want(g, own_shape, other, full):
    """(want, S, T, mode) of one gradient: g conj(other) summed over the axes the output is 1 on; without g conj(other) when the two operands have one shape, and
    the plain sum of other when they have not (the reference's broadcasting branch)"""
    pad = lambda s: (1,) * (len(full) - len(s)) + tuple(s)
    plain = pad(own_shape) == pad(other.shape)
    ob = np.broadcast_to(other, full)
    if g is not None:
        t, s, mode = interleave(cx(g) * np.conj(cx(ob))), cabs_terms(g, ob), 1
    elif plain:
        t, s, mode = interleave(np.conj(cx(ob))), cabs_terms(ob, unit_like(ob)), 2
    else:
        t, s, mode = ob.astype(D), cabs_terms(ob, unit_like(ob)), 3
    return reduce_to(t, own_shape), reduce_to(s, own_shape), 2 * (int(np.prod(full)) // int(np.prod(own_shape))), mode


def kernel_name(row, mode, oshape, full, misaligned):
    form = "map" if int(np.prod(oshape)) == int(np.prod(full)) else "reduce"
    w = 8 if oshape[-1] % 8 == 0 and not misaligned else 2
    return "%s|nnc::cmul_half_%s_kernel<%s,%d>" % (row, form, MODES[mode], w)


_REF = {}


def reference(ref, key, cmd, ins, oshapes):
    """half(reference(float(x))) per output: computed once per case, read-only"""
    if key not in _REF:
        res = ref_run(ref, cmd, ins, [None if s is None else np.zeros(s, H) for s in oshapes])
        res = [None if r is None else r.astype(H) for r in res]
        for r in res:
            if r is not None:
                r.setflags(write=False)
        _REF[key] = res
    return _REF[key]


def check(L, ref, key, cmd, row, ins, oshapes, expect, full, misaligned=False):
    """checks (a) - (e) on one command.  expect: per output None or (want, S, T, mode)"""
    what = "%s %s -> %s%s" % (row, [None if x is None else list(x.shape) for x in ins], [None if s is None else list(s) for s in oshapes], ", misaligned" if misaligned else "")
    tensors = sum(x is not None for x in ins) + sum(s is not None for s in oshapes)
    names_want = [kernel_name(row, e[3], s, full, misaligned) for e, s in zip(expect, oshapes) if e is not None]
    run = lambda: execute(L, cmd, ins, [fill(s) for s in oshapes], misaligned)
    s0, n0 = counts(L)
    (r, got), names = records(L, run)
    assert r == 0, (what, r)
    assert counts(L) == (s0, n0 + tensors), (what, counts(L), (s0, n0))  # (a)
    assert names == names_want and all("cmul_half" in x for x in names), (what, names, names_want)  # (e)
    with key_off(L, KEY):
        s0, n0 = counts(L)
        (r, off), names = records(L, run)
        assert r == 0 and counts(L) == (s0 + tensors, n0), (what, r, counts(L), (s0, n0))
        assert not any("cmul_half" in x for x in names), (what, names)
    refs = reference(ref, key, cmd, ins, oshapes)
    r, again = run()
    for k, e in enumerate(expect):
        if e is None:
            assert got[k] is None
            continue
        want, S, T, _ = e
        same(got[k], off[k], "%s, output %d against the key at 0" % (what, k))  # (b)
        b = bound(want, S, T)
        print(what, "output", k, "worst error / bound", float((np.abs(got[k].astype(D) - want) / b).max()), "reference", float((np.abs(refs[k].astype(D) - want) / b).max()))
        within(got[k], want, b, "%s, output %d" % (what, k))  # (c)
        within(refs[k], want, b, "%s, output %d, the reference" % (what, k))
        same(got[k], again[k], "%s, output %d, two runs" % (what, k))  # (d)
    return got


def operands(pair, swap):
    sa, sb = (pair[1], pair[0]) if swap else pair
    return data(sa, 1), data(sb, 2), np.broadcast_shapes(sa, sb)


def forward(L, ref, pair, swap, misaligned=False):
    a, b, full = operands(pair, swap)
    return check(L, ref, ("fwd", pair, swap), FWD, "cmul_forw", [a, b], [full], [forward_want(a, b)], full, misaligned)[0]


def backward(L, ref, pair, swap, with_g, which, misaligned=False):
    """which: the outputs requested, a pair of flags"""
    a, b, full = operands(pair, swap)
    g = data(full, 3) if with_g else None
    oshapes = [a.shape if which[0] else None, b.shape if which[1] else None]
    expect = [backward_want(g, a.shape, b, full) if which[0] else None, backward_want(g, b.shape, a, full) if which[1] else None]
    return check(L, ref, ("bwd", pair, swap, with_g, which), BWD, "cmul_back", [g, a, b], oshapes, expect, full, misaligned)


# ---- 1. the shapes ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair,swap", CASES, ids=IDS)
def test_forward(backend, ref_lib, pair, swap):
    forward(backend, ref_lib, pair, swap)


@pytest.mark.parametrize("with_g", [True, False], ids=["g", "no-g"])
@pytest.mark.parametrize("pair,swap", CASES, ids=IDS)
def test_backward(backend, ref_lib, pair, swap, with_g):
    """both outputs, then each alone: the same bits"""
    both = backward(backend, ref_lib, pair, swap, with_g, (True, True))
    for k, which in enumerate(((True, False), (False, True))):
        one = backward(backend, ref_lib, pair, swap, with_g, which)
        same(one[k], both[k], "output %d alone" % k)


# ---- 2. two bytes past a 16-byte boundary: the pair instance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [ROTARY, PLAIN2D], ids=["rotary", "20x10"])
def test_misaligned(backend, ref_lib, pair):
    got = forward(backend, ref_lib, pair, False, True)
    same(got, forward(backend, ref_lib, pair, False), "forward, against the aligned tensors")
    for with_g in (True, False):
        got = backward(backend, ref_lib, pair, False, with_g, (True, True), True)
        for x, y in zip(got, backward(backend, ref_lib, pair, False, with_g, (True, True))):
            same(x, y, "backward, against the aligned tensors")


# ---- 3. in place, no elements, the key ------------------------------------------------------------------------------------------------------------------------------
def test_forward_in_place(backend, ref_lib):
    """c in a's memory, the rotary pattern: native, the bits of the out-of-place command"""
    L = backend
    a, b, full = operands(ROTARY, False)
    want = forward(L, ref_lib, ROTARY, False)

    def run():
        ta, tb = make_tensors(L, nnc.GPU_MEMORY, [a, b])
        tc = ta.alias(a.shape, 0)
        assert tc.ptr == ta.ptr
        return L.cmd_exec(FWD, nnc.NO_HINT, 0, [ta, tb], [tc]), tc.numpy()
    s0, n0 = counts(L)
    (r, got), names = records(L, run)
    assert r == 0 and counts(L) == (s0, n0 + 3), (r, counts(L), (s0, n0))
    assert names == [kernel_name("cmul_forw", 0, full, full, False)], names
    same(got, want, "in place against out of place")
    with key_off(L, KEY):
        r, off = run()
        assert r == 0
    same(got, off, "in place, against the key at 0")


def test_no_elements(backend):
    """tensors of no elements: success, nothing is launched"""
    L = backend

    def run():
        ts = [t.alias((0,), 0) for t in make_tensors(L, nnc.GPU_MEMORY, [np.zeros(8, H)] * 3)]
        return L.cmd_exec(FWD, nnc.NO_HINT, 0, ts[:2], ts[2:])
    r, names = records(L, run)
    assert r == 0 and names == [], (r, names)


def test_key_is_on(backend):
    assert backend.tune_get(KEY) == 1


# ---- 4. kept routes -----------------------------------------------------------------------------------------------------------------------------------------------
def staged(L, fn, what):
    """fn() -> (return value, output): success, half tensors through fp32 images, none handed over as halves, no record of a half instance"""
    s0, n0 = counts(L)
    (r, got), names = records(L, fn)
    assert r == 0, (what, r)
    s1, n1 = counts(L)
    assert s1 > s0 and n1 == n0, (what, (s1, n1), (s0, n0))
    assert not any("cmul_half" in x for x in names), (what, names)
    return got


def test_kept_routes(backend, ref_lib):
    L = backend
    a, b, full = operands(ROTARY, False)
    want, S, T, _ = forward_want(a, b)
    bd = bound(want, S, T)
    rows, cols = int(np.prod(full[:-1])), full[-1]

    def into_a_view():  # c is a view: rows of `cols` elements at a stride of cols + 8
        ta, tb = make_tensors(L, nnc.GPU_MEMORY, [a, b])
        (parent,) = make_tensors(L, nnc.GPU_MEMORY, [fill(full[:-1] + (cols + 8,))])
        strides = tuple(int(np.prod(full[i + 1:-1])) * (cols + 8) for i in range(len(full) - 1)) + (1,)
        return L.cmd_exec(FWD, nnc.NO_HINT, 0, [ta, tb], [parent.view(full, strides, 0)]), parent.numpy()

    got = staged(L, into_a_view, "a view of c")
    within(got[..., :cols], want, bd, "a view of c")
    same(got[..., cols:], fill(full[:-1] + (8,)), "what lies between the view's rows")
    got = staged(L, lambda: execute(L, FWD, [a, b], [fill(full)], flags=nnc.ACCUMULATE_OUTPUT), "ACCUMULATE_OUTPUT")[0]
    within(got, want, bd, "ACCUMULATE_OUTPUT")
    got = staged(L, lambda: execute(L, FWD, [a, b.astype(F)], [fill(full)]), "b in fp32")[0]
    assert got.dtype == H
    within(got, want, bd, "b in fp32")

    # a reduce-form output over an input's memory: db = the sum over axis 0 of g conj(a), written over g's first slab.  (Every output element is the sum of the
    # elements of g at its own position in every slab: the fp32 kernel's lane reads them before it writes.)
    pa, pb = (3, 4, 5, 6), (1, 4, 5, 6)
    a2, b2, g2 = data(pa, 1), data(pb, 2), data(pa, 3)
    want, S, T, _ = backward_want(g2, pb, a2, pa)

    def over_g():
        tg, ta, tb = make_tensors(L, nnc.GPU_MEMORY, [g2, a2, b2])
        db = tg.alias(pb, 0)
        return L.cmd_exec(BWD, nnc.NO_HINT, 0, [tg, ta, tb], [None, db]), db.numpy()
    got = staged(L, over_g, "db over g")
    within(got, want, bound(want, S, T), "db over g")
