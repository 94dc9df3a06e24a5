"""LAYER_NORM, RMSNORM and plain SOFTMAX, forward and backward, on CCV_16F maps without fp32 images (ccv_amd/csrc/row_ops.h; tunable ROW_HALF_NATIVE):
every used tensor half ("hh"), or the maps half and the parameters and statistics fp32 ("hf").

Every result is stated in float64 numpy on the inputs as the command sees them: halves widened, and for the backward commands the statistics as STORED
(the float64 forward statistics rounded to the type of the statistics tensors).  Bounds are derived, not tuned.  With u = 2^-24:
  * the one rounding to half of a stored value: 2^-11 |want| + 2^-24 (fp32 outputs: nothing, their last rounding is in E below);
  * an fp32 sum of R terms: R u sum|terms|; every other fp32 operation: u |result| (expf: 16 u |result|, as tests/test_mbconv_half.py allows the device's);
  * E, the fp32 error of an output, is these propagated to first order through the expression, in float64:
      mean          dm   = (n + 2) u sum|a| / n
      var           dvar = (n + 4) u var                           (d var / d mean is zero at the mean; the centring w = a - mean adds 2 u var)
      inv_std       dis  = inv_std^3 dvar / 2 + 3 u inv_std        (fma, square root, division)
      y = w inv_std dy   = inv_std (dm + u |w|) + |w| dis + u |y|   (RMSNORM: dm = 0, w = a)
      b             E    = |scale| dy + 2 u (|y scale| + |bias|)
      backward      ah, gss carry 2 u each; ds1 = (n + 2) u sum|gss|, ds2 = (n + 4) u sum|ah gss|,
                    E(h) = 4 u (|gss| + (|s1| + |ah s2|) / n) + (ds1 + |ah| ds2) / n
                    E(dscale) = (rows + 4) u sum_rows |ah g|,  E(dbias) = rows u sum_rows |g|
      softmax       E(b) = (n + 40) u b  (the subtraction, expf, the sum of n positive terms, the reciprocal and the product)
                    E(h) = |b| (n + 1) u sum|g b| + 3 u (|g| + |s|) |b|
The reference's CPU backend runs every case on the widened inputs and must meet the fp32 form (E alone): the bound is not too tight.  A deliberately wrong
expectation -- the variance taken around zero, epsilon dropped, softmax without the max -- breaks it on these inputs: it is not too loose
(test_wrong_expectations_break_the_bounds).
Inputs: a = U(-4, 4) plus a per-row offset in +-8 (no row has a variance near zero), g = U(-2, 2), scale around 1, bias around 0, epsilon = 0.1 (large enough
to show in a half output); one softmax row holds +60000 and -60000 and overflows without the max subtraction.
"""
import os
import re
import numpy as np
import pytest
from ccv_amd import nnc
from harness import make_tensors
from test_mbconv_half import aliased, bits, counts, key_off, records, ref_run, within

F, H, D = np.float32, np.float16, np.float64
U = 2.0 ** -24
KEY = "ROW_HALF_NATIVE"
EPS = 0.1
_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccv_amd", "csrc", "row_ops.h")
with open(_HDR) as _f:
    _TEXT = _f.read()
WAVE_MAX, REG_MAX, CHUNK_ROWS = (int(re.search(r"constexpr int %s = (\d+);" % k, _TEXT).group(1)) for k in ("ROW_WAVE_MAX", "ROW_REG_MAX", "ROW_CHUNK_ROWS"))
NS = [1, 7, 8, 64, 520, 523, WAVE_MAX, WAVE_MAX + 8, REG_MAX]
ROWS = [1, 5, CHUNK_ROWS + 3]
COMBOS = {"hh": H, "hf": F}  # the type of the parameters and statistics
FAMILIES = ["layernorm_affine", "layernorm_plain", "rmsnorm"]


def form(n):
    return "wg" if n > WAVE_MAX else "wave"


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------------
_DATA = {}


def data(rows, n):
    """a, g (half), scale, bias (float64 values that are exact halves)"""
    if (rows, n) not in _DATA:
        rng = np.random.default_rng(1000 * rows + n)
        a = ((rng.random((rows, n)) - 0.5) * 8 + (rng.random((rows, 1)) - 0.5) * 16).astype(H)
        g = ((rng.random((rows, n)) - 0.5) * 4).astype(H)
        scale = (1 + (rng.random((1, n)) - 0.5) * 0.5).astype(H)
        bias = ((rng.random((1, n)) - 0.5) * 0.5).astype(H)
        for x in (a, g, scale, bias):
            x.setflags(write=False)
        _DATA[(rows, n)] = (a, g, scale, bias)
    return _DATA[(rows, n)]


# ---- expectations: (want, E) in float64 -----------------------------------------------------------------------------------------------------------------
def norm_forward(a, scale, bias, center, eps=EPS, centred_variance=True):
    a = a.astype(D)
    n = a.shape[1]
    e = D(F(eps))
    mean = a.mean(axis=1, keepdims=True) if center else np.zeros((a.shape[0], 1))
    dm = (n + 2) * U * np.abs(a).sum(axis=1, keepdims=True) / n if center else 0.0
    w = a - mean
    var = (w * w).mean(axis=1, keepdims=True) if centred_variance else (a * a).mean(axis=1, keepdims=True)
    istd = 1 / np.sqrt(var + e)
    dis = istd ** 3 * (n + 4) * U * var / 2 + 3 * U * istd
    y = w * istd
    dy = istd * (dm + U * np.abs(w)) + np.abs(w) * dis + U * np.abs(y)
    sc = 1.0 if scale is None else scale.astype(D)
    bi = 0.0 if bias is None else bias.astype(D)
    b = y * sc + bi
    out = {"b": (b, np.abs(sc) * dy + 2 * U * (np.abs(y * sc) + np.abs(bi))), "inv_std": (istd, dis)}
    if center:
        out["mean"] = (mean, dm + 0 * mean)
    return out


def norm_backward(g, a, scale, mean, istd, center):
    """mean, istd: as stored (float64 values of the stored numbers)"""
    g, a = g.astype(D), a.astype(D)
    rows, n = a.shape
    sc = 1.0 if scale is None else scale.astype(D)
    ah = (a - (mean if center else 0.0)) * istd
    gss = g * sc * istd
    s1 = gss.sum(axis=1, keepdims=True) if center else np.zeros((rows, 1))
    s2 = (ah * gss).sum(axis=1, keepdims=True)
    ds1 = (n + 2) * U * np.abs(gss).sum(axis=1, keepdims=True) if center else 0.0
    ds2 = (n + 4) * U * np.abs(ah * gss).sum(axis=1, keepdims=True)
    h = gss - (s1 + ah * s2) / n
    eh = 4 * U * (np.abs(gss) + (np.abs(s1) + np.abs(ah * s2)) / n) + (ds1 + np.abs(ah) * ds2) / n
    return {"h": (h, eh), "dscale": ((ah * g).sum(axis=0, keepdims=True), (rows + 4) * U * np.abs(ah * g).sum(axis=0, keepdims=True)),
            "dbias": (g.sum(axis=0, keepdims=True), rows * U * np.abs(g).sum(axis=0, keepdims=True))}


def softmax_forward(a, subtract_max=True):
    a = a.astype(D)
    n = a.shape[-1]
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(a - (a.max(axis=-1, keepdims=True) if subtract_max else 0.0))
        b = e / e.sum(axis=-1, keepdims=True)
    return b, (n + 40) * U * b


def softmax_backward(g, b):
    g, b = g.astype(D), b.astype(D)
    n = b.shape[-1]
    s = (g * b).sum(axis=-1, keepdims=True)
    return (g - s) * b, np.abs(b) * (n + 1) * U * np.abs(g * b).sum(axis=-1, keepdims=True) + 3 * U * (np.abs(g) + np.abs(s)) * np.abs(b)


def bound(want, e, dtype):
    return 2.0 ** -11 * np.abs(want) + 2.0 ** -24 + e if dtype == H else e


def check(got, want, what, names=None):
    for k in (names or want):
        x, (w, e) = got[k], want[k]
        within(x.reshape(w.shape), w, bound(w, e, x.dtype), "%s %s" % (what, k))


# ---- the commands -----------------------------------------------------------------------------------------------------------------------------------------
def family_of(fam):
    """-> (center, affine, forward command, backward command)"""
    if fam == "rmsnorm":
        return False, True, nnc.CMD_NORM("RMSNORM_FORWARD", EPS, 0, 1), nnc.CMD_NORM("RMSNORM_BACKWARD", EPS, 0, 1)
    affine = int(fam.endswith("affine"))
    return True, bool(affine), nnc.CMD_NORM("LAYER_NORM_FORWARD", EPS, affine, 1), nnc.CMD_NORM("LAYER_NORM_BACKWARD", EPS, affine, 1)


def place(L, arrays, mode):
    """device tensors; "unaligned": dense aliases that start one element past a 16-byte boundary"""
    if mode == "unaligned":
        idx = [i for i, x in enumerate(arrays) if x is not None]
        ts = aliased(L, [arrays[i] for i in idx], 1)
        assert all(t.ptr % 16 == t.np_dtype.itemsize for t in ts)
        out = [None] * len(arrays)
        for i, t in zip(idx, ts):
            out[i] = t
        return out
    return make_tensors(L, nnc.GPU_MEMORY, arrays)


def run_forward(L, fam, a, scale, bias, pt, mode="plain", flags=0, expect_ret=0):
    """-> {"b", "mean", "inv_std"} as the command left them.  mode "inplace": b = a"""
    center, affine, fwd, _ = family_of(fam)
    rows, n = a.shape
    ins = [a] + ([scale.astype(pt)] + ([bias.astype(pt)] if center else []) if affine else [])
    outs = [np.full((rows, n), 3, H)] + ([np.full((rows, 1), 3, pt)] if center else []) + [np.full((rows, 1), 3, pt)]
    it, ot = place(L, ins, mode), place(L, outs, mode)
    if mode == "inplace":
        ot[0] = it[0]
    r = L.cmd_exec(fwd, nnc.NO_HINT, flags, it, ot)
    assert r == expect_ret, "backend returned %d" % r
    res = [t.numpy() for t in ot]
    return dict(zip(["b", "mean", "inv_std"] if center else ["b", "inv_std"], res))


def backward_io(fam, g, a, scale, mean, istd, pt, want=("h", "dscale", "dbias"), unused=None):
    """input and output arrays of the backward command, the output names; `unused`: an array for the slots the command does not read"""
    center, affine, _, _ = family_of(fam)
    rows, n = a.shape
    st = lambda x: x.astype(pt).reshape(rows, 1)
    if fam == "rmsnorm":
        ins, names = [g, unused, a, scale.astype(pt), unused, st(istd)], ["h", "dscale"]
    elif affine:
        ins, names = [g, unused, unused, a, scale.astype(pt), unused, unused, st(mean), st(istd)], ["h", "dscale", "dbias"]
    else:
        ins, names = [g, unused, unused, a, unused, st(mean), st(istd)], ["h", "dscale", "dbias"]
    outs = [np.full((rows, n), 3, H) if "h" in want else None] + [np.full((1, n), 3, pt) if k in want else None for k in names[1:]]
    return ins, outs, names


def run_backward(L, fam, g, a, scale, mean, istd, pt, mode="plain", flags=0, **kw):
    _, _, _, bwd = family_of(fam)
    ins, outs, names = backward_io(fam, g, a, scale, mean, istd, pt, **kw)
    it, ot = place(L, ins, mode), place(L, outs, mode)
    if mode == "inplace":
        ot[0] = it[0]
    r = L.cmd_exec(bwd, nnc.NO_HINT, flags, it, ot)
    assert r == 0, "backend returned %d" % r
    return {k: t.numpy() for k, t in zip(names, ot) if t is not None}


def stored_stats(fam, a, pt):
    """the forward statistics as a tensor of type pt holds them (float64 values)"""
    f = norm_forward(a, None, None, family_of(fam)[0])
    mean = f["mean"][0].astype(pt).astype(D) if "mean" in f else None
    return mean, f["inv_std"][0].astype(pt).astype(D)


def same_bits(x, y, what):
    assert x.dtype == y.dtype and np.array_equal(bits(x), bits(y)), "%s differs in %d elements" % (what, int((bits(x) != bits(y)).sum()))


# ---- 1. values --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("fam", FAMILIES)
def test_norm_half(backend, ref_lib, fam, combo, n, rows):
    """n: 1, 7 scalar only; 8 one vector; 64; 520 whole vectors; 523 odd -- every row after the first is unaligned: the scalar route; ROW_WAVE_MAX the longest
    wave-form row; + 8 the first workgroup-form one; ROW_REG_MAX the longest served.  rows: 1; 5 a partial last workgroup in the wave form; one chunk + 3:
    two chunks of the backward plan, the second partial."""
    L, pt = backend, COMBOS[combo]
    center, affine, fwd, bwd = family_of(fam)
    a, g, scale, bias = data(rows, n)
    sc, bi = (scale if affine else None), (bias if affine and center else None)
    want = norm_forward(a, sc, bi, center)
    got = run_forward(L, fam, a, scale, bias, pt)
    assert got["b"].dtype == H and got["inv_std"].dtype == pt
    check(got, want, "%s %s forward" % (fam, combo))
    mean, istd = stored_stats(fam, a, pt)
    wantb = norm_backward(g, a, sc, mean, istd, center)
    gotb = run_backward(L, fam, g, a, scale, mean, istd, pt)
    check(gotb, wantb, "%s %s backward" % (fam, combo), list(gotb))
    if combo == "hh":  # the reference on the widened inputs, once per case: the fp32 form
        ins = [a] + ([scale] + ([bias] if center else []) if affine else [])
        outs = [np.zeros((rows, n), F)] + [np.zeros((rows, 1), F)] * (2 if center else 1)
        ref = dict(zip(["b", "mean", "inv_std"] if center else ["b", "inv_std"], ref_run(ref_lib, fwd, ins, outs)))
        check(ref, {k: (w, e + U * np.abs(w)) for k, (w, e) in want.items()}, fam + " forward, reference")
        bi_, bo_, names = backward_io(fam, g, a, scale, mean, istd, H)
        if not affine:  # (the reference has no parameter gradients without parameters)
            bo_, names = bo_[:1], names[:1]
        ref ={k: x for k, x in zip(names, ref_run(ref_lib, bwd, bi_, [None if x is None else np.zeros(x.shape, F) for x in bo_]))}
        check(ref, {k: (w, e + U * np.abs(w)) for k, (w, e) in wantb.items()}, fam + " backward, reference", names)


def softmax_data(rows, n):
    a, g, _, _ = data(rows, n)
    a = a.copy()
    if n >= 2:
        a[rows // 2, 0], a[rows // 2, n - 1] = 60000, -60000
    return a, g


def run_softmax(L, a, g=None, mode="plain", flags=0):
    """forward: a -> b; backward (g given): g, _, b = a -> h"""
    ins = [a] if g is None else [g, None, a]
    it, ot = place(L, ins, mode), place(L, [np.full(a.shape, 3, H)], mode)
    if mode == "inplace":
        ot[0] = it[0]
    cmd = nnc.generic_cmd("SOFTMAX_FORWARD" if g is None else "SOFTMAX_BACKWARD")
    r = L.cmd_exec(cmd, nnc.NO_HINT, flags, it, ot)
    assert r == 0, "backend returned %d" % r
    return ot[0].numpy()


@pytest.mark.parametrize("rows", ROWS + ["1-d"], ids=str)
@pytest.mark.parametrize("n", NS)
def test_softmax_half(backend, ref_lib, n, rows):
    """The shapes of test_norm_half and one 1-d tensor (a single row); one row holds +60000 and -60000."""
    L = backend
    a, g = softmax_data(1 if rows == "1-d" else rows, n)
    if rows == "1-d":
        a, g = a.reshape(n), g.reshape(n)
    want, e = softmax_forward(a)
    got = run_softmax(L, a)
    assert got.dtype == H
    within(got, want, bound(want, e, H), "softmax forward")
    b = want.astype(H)
    wanth, eh = softmax_backward(g, b)
    goth = run_softmax(L, b, g)
    within(goth, wanth, bound(wanth, eh, H), "softmax backward")
    ref = ref_run(ref_lib, nnc.generic_cmd("SOFTMAX_FORWARD"), [a], [np.zeros(a.shape, H)])[0]
    within(ref, want, e + U * np.abs(want), "softmax forward, reference")
    ref = ref_run(ref_lib, nnc.generic_cmd("SOFTMAX_BACKWARD"), [g, None, b], [np.zeros(a.shape, H)])[0]
    within(ref, wanth, eh + U * np.abs(wanth), "softmax backward, reference")


@pytest.mark.parametrize("n", [520, WAVE_MAX + 8])
@pytest.mark.parametrize("combo", list(COMBOS))
def test_layer_norm_variants(backend, combo, n):
    """A one-element scale and bias; h alone; the parameter gradients alone -- each against the bounds, the partial commands bit for bit the full one."""
    L, pt = backend, COMBOS[combo]
    rows, fam = CHUNK_ROWS + 3, "layernorm_affine"
    a, g, scale, bias = data(rows, n)
    s1, b1 = scale[:, :1], bias[:, :1]
    check(run_forward(L, fam, a, s1, b1, pt), norm_forward(a, s1, b1, True), "one-element scale, forward")
    mean, istd = stored_stats(fam, a, pt)
    want1 = norm_backward(g, a, s1, mean, istd, True)
    check(run_backward(L, fam, g, a, s1, mean, istd, pt, want=("h",)), want1, "one-element scale, backward", ["h"])
    want = norm_backward(g, a, scale, mean, istd, True)
    full = run_backward(L, fam, g, a, scale, mean, istd, pt)
    check(full, want, "backward")
    (only_h, names_h) = records(L, lambda: run_backward(L, fam, g, a, scale, mean, istd, pt, want=("h",)))
    assert list(only_h) == ["h"] and len(names_h) == 1, names_h  # no fold
    same_bits(only_h["h"], full["h"], "h alone")
    (only_p, names_p) = records(L, lambda: run_backward(L, fam, g, a, scale, mean, istd, pt, want=("dscale", "dbias")))
    assert sorted(only_p) == ["dbias", "dscale"] and len(names_p) == 2, names_p
    same_bits(only_p["dscale"], full["dscale"], "dscale alone")
    same_bits(only_p["dbias"], full["dbias"], "dbias alone")
    only_b = run_backward(L, fam, g, a, scale, mean, istd, pt, want=("dbias",))
    same_bits(only_b["dbias"], full["dbias"], "dbias without dscale")


def test_wrong_expectations_break_the_bounds():
    """The bounds are not too loose: the variance around zero, epsilon dropped and softmax without the max each leave them on these inputs."""
    rows, n = 5, 64
    a, g, scale, bias = data(rows, n)
    good = norm_forward(a, scale, bias, True)
    for what, wrong in (("variance around zero", norm_forward(a, scale, bias, True, centred_variance=False)), ("no epsilon", norm_forward(a, scale, bias, True, eps=0.0))):
        for k in ("b", "inv_std"):
            w, e = good[k]
            assert (np.abs(wrong[k][0] - w) > 2 * bound(w, e, H)).any(), (what, k)
    good = norm_forward(a, scale, None, False)
    wrong = norm_forward(a, scale, None, False, eps=0.0)
    assert (np.abs(wrong["b"][0] - good["b"][0]) > 2 * bound(good["b"][0], good["b"][1], H)).any()
    sa, _ = softmax_data(rows, n)
    w, e = softmax_forward(sa)
    assert not (np.abs(softmax_forward(sa, subtract_max=False)[0] - w) <= bound(w, e, H)).all()


# ---- 2. unaligned bases -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("fam", FAMILIES)
def test_unaligned_bases(backend, fam, combo):
    """Every tensor starts one element past a 16-byte boundary: the scalar route.  dscale and dbias involve no sum across lanes -- a column's terms are added
    row by row inside a chunk, then chunk by chunk -- and carry the bits of the aligned run; b, the statistics and h depend on sums over a row, whose order
    follows the lanes' columns, and only meet the bounds."""
    L, pt = backend, COMBOS[combo]
    center, affine, _, _ = family_of(fam)
    rows, n = CHUNK_ROWS + 3, 520
    a, g, scale, bias = data(rows, n)
    sc, bi = (scale if affine else None), (bias if affine and center else None)
    check(run_forward(L, fam, a, scale, bias, pt, "unaligned"), norm_forward(a, sc, bi, center), fam + " unaligned forward")
    mean, istd = stored_stats(fam, a, pt)
    got = run_backward(L, fam, g, a, scale, mean, istd, pt, "unaligned")
    check(got, norm_backward(g, a, sc, mean, istd, center), fam + " unaligned backward", list(got))
    plain = run_backward(L, fam, g, a, scale, mean, istd, pt)
    for k in got:
        if k != "h":
            same_bits(got[k], plain[k], "%s unaligned %s" % (fam, k))


def test_softmax_unaligned_bases(backend):
    L = backend
    a, g = softmax_data(5, 520)
    want, e = softmax_forward(a)
    within(run_softmax(L, a, mode="unaligned"), want, bound(want, e, H), "softmax unaligned forward")
    b = want.astype(H)
    wanth, eh = softmax_backward(g, b)
    within(run_softmax(L, b, g, mode="unaligned"), wanth, bound(wanth, eh, H), "softmax unaligned backward")


# ---- 3. in place, 4. twice -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [523, 520, WAVE_MAX + 8])
@pytest.mark.parametrize("fam", FAMILIES)
def test_in_place_and_twice(backend, fam, n):
    """b = a and h = g carry the bits of the out-of-place run; two runs carry the same bits, dscale / dbias over two chunks included."""
    L, pt = backend, H
    rows = CHUNK_ROWS + 3
    a, g, scale, bias = data(rows, n)
    first = run_forward(L, fam, a, scale, bias, pt)
    for other, what in ((run_forward(L, fam, a, scale, bias, pt), "twice"), (run_forward(L, fam, a, scale, bias, pt, "inplace"), "in place")):
        for k in first:
            same_bits(other[k], first[k], "%s forward %s %s" % (fam, what, k))
    mean, istd = stored_stats(fam, a, pt)
    first = run_backward(L, fam, g, a, scale, mean, istd, pt)
    for other, what in ((run_backward(L, fam, g, a, scale, mean, istd, pt), "twice"), (run_backward(L, fam, g, a, scale, mean, istd, pt, "inplace"), "in place")):
        for k in first:
            same_bits(other[k], first[k], "%s backward %s %s" % (fam, what, k))


@pytest.mark.parametrize("n", [523, 520, WAVE_MAX + 8])
def test_softmax_in_place_and_twice(backend, n):
    L = backend
    a, g = softmax_data(5, n)
    first = run_softmax(L, a)
    same_bits(run_softmax(L, a), first, "softmax forward twice")
    same_bits(run_softmax(L, a, mode="inplace"), first, "softmax forward in place")
    firsth = run_softmax(L, first, g)
    same_bits(run_softmax(L, first, g), firsth, "softmax backward twice")
    ins = place(L, [g, None, first], "plain")
    assert L.cmd_exec(nnc.generic_cmd("SOFTMAX_BACKWARD"), nnc.NO_HINT, 0, ins, [ins[0]]) == 0  # h = g
    same_bits(ins[0].numpy(), firsth, "softmax backward in place")


# ---- 5. routes ------------------------------------------------------------------------------------------------------------------------------------------------
def _norm_steps(L, fam, combo, n):
    """[(what, call, half tensors named by the row, launch records expected)]"""
    pt = COMBOS[combo]
    center, affine, _, _ = family_of(fam)
    rows = CHUNK_ROWS + 3
    a, g, scale, bias = data(rows, n)
    mean, istd = stored_stats(fam, a, pt)
    nstat, nscale = (2 if center else 1), (1 if affine else 0)
    nbias = 1 if affine and center else 0
    nd = 2 if center else 1  # dscale, dbias
    hh = combo == "hh"
    tag = "layernorm" if center else "rmsnorm"
    return [("%s_fwd" % tag, lambda: run_forward(L, fam, a, scale, bias, pt), 2 + (nstat + nscale + nbias if hh else 0), 1, (nstat + nscale + nbias if pt == H else 0)),
            ("%s_bwd" % tag, lambda: run_backward(L, fam, g, a, scale, mean, istd, pt), 3 + (nstat + nscale + nd if hh else 0), 2, (nstat + nscale + nd if pt == H else 0))]


@pytest.mark.parametrize("n", [520, 523, WAVE_MAX + 8])
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("fam", FAMILIES)
def test_routes(backend, fam, combo, n):
    """No half tensor named by the row gets an fp32 image and all of them are counted native; the launch records hold the rows_* kernel of the right type and
    form (and the fold for the parameter gradients), no conversion; with the key at 0 every half tensor is staged again, no rows_* kernel runs and the result
    still meets the bounds."""
    L = backend
    center, affine, _, _ = family_of(fam)
    a, g, scale, bias = data(CHUNK_ROWS + 3, n)
    sc, bi = (scale if affine else None), (bias if affine and center else None)
    mean, istd = stored_stats(fam, a, COMBOS[combo])
    wants = [norm_forward(a, sc, bi, center), norm_backward(g, a, sc, mean, istd, center)]
    for (tag, call, halves, launches, _), want in zip(_norm_steps(L, fam, combo, n), wants):
        s0, n0 = counts(L)
        got, names = records(L, call)
        assert counts(L) == (s0, n0 + halves), (tag, counts(L), (s0, n0), halves)
        assert len(names) == launches and names[0].startswith("rows_%s_%s|nnc::rows::%s" % (tag, combo, form(n))), names
        assert all(x.startswith("rows_") for x in names) and not any("half_up" in x or "half_down" in x for x in names), names
        with key_off(L, KEY):
            s0, n0 = counts(L)
            off, names = records(L, call)
            assert counts(L) == (s0 + halves, n0), (tag, counts(L), (s0, n0), halves)
            assert not any(x.startswith("rows_") for x in names), names
        check(off, want, "%s %s, fp32 images" % (tag, combo), list(off))


@pytest.mark.parametrize("n", [520, 523, WAVE_MAX + 8])
def test_routes_softmax(backend, n):
    L = backend
    a, g = softmax_data(5, n)
    want, e = softmax_forward(a)
    b = want.astype(H)
    wanth, eh = softmax_backward(g, b)
    for tag, call, halves, w, ee in (("fwd", lambda: run_softmax(L, a), 2, want, e), ("bwd", lambda: run_softmax(L, b, g), 3, wanth, eh)):
        s0, n0 = counts(L)
        _, names = records(L, call)
        assert counts(L) == (s0, n0 + halves)
        assert len(names) == 1 and names[0].startswith("rows_softmax_%s_h|nnc::rows::%s" % (tag, form(n))), names
        with key_off(L, KEY):
            s0, n0 = counts(L)
            off, names = records(L, call)
            assert counts(L) == (s0 + halves, n0) and not any(x.startswith("rows_") for x in names), names
        within(off, w, bound(w, ee, H), "softmax %s, fp32 images" % tag)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_keep_their_route(backend):
    """A dense view, a strided view, CCV_NNC_ACCUMULATE_OUTPUT and a row of ROW_REG_MAX + 8 elements keep the fp32 images and what the command returned before;
    an fp32 tensor in an unused slot of the backward command does NOT refuse."""
    L = backend
    fam, pt = "layernorm_affine", H
    rows, n = 5, 520
    a, g, scale, bias = data(rows, n)
    want = norm_forward(a, scale, bias, True)
    fwd = family_of(fam)[2]
    arrays = [a, scale, bias, np.full((rows, n), 3, H), np.full((rows, 1), 3, H), np.full((rows, 1), 3, H)]
    # a dense view: staged, right
    ts = make_tensors(L, nnc.GPU_MEMORY, arrays)
    ts[0] = ts[0].view((rows, n), (n, 1), 0)
    s0, n0 = counts(L)
    r, names = records(L, lambda: L.cmd_exec(fwd, nnc.NO_HINT, 0, ts[:3], ts[3:]))
    assert r == 0 and counts(L) == (s0 + 6, n0) and not any(x.startswith("rows_") for x in names), names
    check(dict(zip(["b", "mean", "inv_std"], [t.numpy() for t in ts[3:]])), want, "a dense view")
    # a strided view: refused by the fp32 kernel underneath, as it was
    ts = make_tensors(L, nnc.GPU_MEMORY, arrays)
    (wide,) = make_tensors(L, nnc.GPU_MEMORY, [np.ones((rows, n + 8), H)])
    s0, n0 = counts(L)
    r = L.cmd_exec(fwd, nnc.NO_HINT, 0, [wide.view((rows, n), (n + 8, 1), 0)] + ts[1:3], ts[3:])
    assert r == -1 and counts(L) == (s0 + 6, n0)
    # ACCUMULATE_OUTPUT: staged; the same bits as with the key at 0
    s0, n0 = counts(L)
    got = run_forward(L, fam, a, scale, bias, pt, flags=nnc.ACCUMULATE_OUTPUT)
    assert counts(L) == (s0 + 6, n0)
    with key_off(L, KEY):
        off = run_forward(L, fam, a, scale, bias, pt, flags=nnc.ACCUMULATE_OUTPUT)
    for k in got:
        same_bits(got[k], off[k], "ACCUMULATE_OUTPUT " + k)
    # n = ROW_REG_MAX + 8: staged, right
    big = REG_MAX + 8
    a2, g2, scale2, bias2 = data(2, big)
    s0, n0 = counts(L)
    got, names = records(L, lambda: run_forward(L, fam, a2, scale2, bias2, pt))
    assert counts(L) == (s0 + 6, n0) and not any(x.startswith("rows_") for x in names), names
    check(got, norm_forward(a2, scale2, bias2, True), "n = ROW_REG_MAX + 8")
    sa, _ = softmax_data(2, big)
    s0, n0 = counts(L)
    got = run_softmax(L, sa)
    assert counts(L) == (s0 + 2, n0)
    w, e = softmax_forward(sa)
    within(got, w, bound(w, e, H), "softmax, n = ROW_REG_MAX + 8")
    # an fp32 tensor in the unused slots: native all the same
    mean, istd = stored_stats(fam, a, pt)
    s0, n0 = counts(L)
    got, names = records(L, lambda: run_backward(L, fam, g, a, scale, mean, istd, pt, unused=np.zeros((rows, n), F)))
    assert counts(L) == (s0, n0 + 8) and names[0].startswith("rows_layernorm_bwd_hh|"), names
    check(got, norm_backward(g, a, scale, mean, istd, True), "fp32 tensors in unused slots")
    L.stream_wait(None)


def test_half_parameters_beside_fp32_statistics(backend):
    """Half maps, half scale and bias, fp32 statistics: the all-half row's mask meets an fp32 tensor and refuses, the maps-only row takes the command -- the
    two parameters get their small fp32 images, the maps do not."""
    L = backend
    rows, n = 5, 520
    a, g, scale, bias = data(rows, n)
    ts = make_tensors(L, nnc.GPU_MEMORY, [a, scale, bias, np.full((rows, n), 3, H), np.full((rows, 1), 3, F), np.full((rows, 1), 3, F)])
    s0, n0 = counts(L)
    r, names = records(L, lambda: L.cmd_exec(family_of("layernorm_affine")[2], nnc.NO_HINT, 0, ts[:3], ts[3:]))
    assert r == 0 and counts(L) == (s0 + 2, n0 + 2), (counts(L), (s0, n0))
    assert len(names) == 1 and names[0].startswith("rows_layernorm_fwd_hf|nnc::rows::wave"), names
    check(dict(zip(["b", "mean", "inv_std"], [t.numpy() for t in ts[3:]])), norm_forward(a, scale, bias, True), "half parameters, fp32 statistics")


def test_tuning_key_is_listed(backend):
    assert backend.tune_get(KEY) == 1
