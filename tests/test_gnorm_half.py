"""GROUP_NORM forward and backward on dense CCV_16F maps without fp32 images (ccv_amd/csrc/group_ops.h; tunable GNORM_HALF_NATIVE): the planar layout
(NCHW with the groups on axis 1, [N, C] maps) and the interleaved one (NHWC with the groups on axis 3); every used tensor half ("hh"), or the maps half and
the parameters and statistics fp32 ("hf").

Every result is stated in float64 numpy on the inputs as the command sees them: halves widened, and for the backward command the statistics as STORED.
Everything is computed on the canonical view [N][G][cg][P] of a map (P = H W pixels), whatever the layout.  Bounds are derived with the formulas in the
docstring of tests/test_rows_half.py, not tuned: n = cg P is the block size, the parameter gradients are sums of N P terms, u = 2^-24, and a value stored as
half adds 2^-11 |want| + 2^-24.  The reference's CPU backend runs each case on the widened inputs and must meet the fp32 part alone: the bound is not too
tight; deliberately wrong expectations break it (test_wrong_expectations_break_the_bounds): it is not too loose.
Inputs: a = U(-4, 4) plus a per-statistic offset in +-8 (no block has a variance near zero; epsilon is the ~1e-45 both reference backends read, see
cmd_groupnorm.cpp), g = U(-2, 2), scale around 1, bias around 0, all exact halves.
"""
import os
import re
import numpy as np
import pytest
from ccv_amd import nnc
from harness import make_tensors
from test_mbconv_half import aliased, bits, counts, key_off, records, ref_run, within
from test_rows_half import bound, same_bits

F, H, D = np.float32, np.float16, np.float64
U = 2.0 ** -24
KEY = "GNORM_HALF_NATIVE"
_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccv_amd", "csrc", "group_ops.h")
with open(_HDR) as _f:
    _TEXT = _f.read()
REG_MAX, SLICE_MAX, SLICE_MIN, INTER_SLICE_MIN, TARGET_WGS, LANE = (int(re.search(r"constexpr int %s = (\d+);" % k, _TEXT).group(1)) for k in ("GN_REG_MAX", "GN_SLICE_MAX", "GN_SLICE_MIN", "GN_INTER_SLICE_MIN", "GN_TARGET_WGS", "GN_LANE"))
COMBOS = {"hh": H, "hf": F}  # the type of the parameters and statistics


# ---- shapes: (layout, N, C, G, H, W) ---------------------------------------------------------------------------------------------------------------------
def slice_plan(units, length, quantum, min_per, max_per):
    """group_ops.h slice_plan: (slices, per)"""
    want = max(1, -(-TARGET_WGS // max(units, 1)))
    per = max(-(-length // want), min_per)
    per = -(-per // quantum) * quantum
    if max_per:
        per = min(per, max_per)
    return max(1, -(-length // per)), per


def map_plan(lay, N, C, G, HW):
    if lay == "nhwc":
        return slice_plan(N, HW, 1, -(-INTER_SLICE_MIN // C), 0)
    return slice_plan(N * G, C // G * HW, LANE, SLICE_MIN, SLICE_MAX)


def planar(case, affine):
    """Every statistic owns one contiguous run: NCHW and [N, C] maps -- and NHWC maps of a single pixel, or of one group when no per-channel parameter
    asks for the channels to be told apart."""
    lay, N, C, G, Hh, W = case
    return lay != "nhwc" or Hh * W == 1 or (G == 1 and not affine)


def form(case, affine):
    lay, N, C, G, Hh, W = case
    return "reg" if planar(case, affine) and C // G * Hh * W <= REG_MAX else "split"


def layout_tag(case, affine):
    return "planar" if planar(case, affine) else "inter"


_HW_BELOW, _HW_AT, _HW_ABOVE = (23, 89), (32, 64), (3, 683)  # with cg = 8: n = GN_REG_MAX - 8, GN_REG_MAX, GN_REG_MAX + 8 at the default
CASES = [
    ("nchw", 1, 4, 2, 1, 1),      # C < 8, a single pixel: n = 2
    ("nchw", 3, 8, 8, 5, 7),      # instance norm; 35-element planes: every plane after the first starts unaligned
    ("nchw", 3, 12, 3, 5, 7),     # cg = 4, three groups
    ("nchw", 1, 20, 2, 8, 8),     # cg = 10, whole vectors
    ("nchw", 3, 16, 1, 8, 8),     # one group, cg = 16
    ("nchw", 1, 8, 2, 33, 33),    # n = 4356: no multiple of 8
    ("nchw", 1, 16, 2) + _HW_BELOW,  # the longest runs of the reg form ...
    ("nchw", 1, 16, 2) + _HW_AT,
    ("nchw", 1, 16, 2) + _HW_ABOVE,  # ... and the first of the split form: nine slices, the last one of 8 elements
    ("nchw", 1, 8, 2, 65, 65),    # n = 16 900: split, scalar
    ("nc", 3, 12, 3, 1, 1),       # an [N, C] map
    ("nhwc", 1, 4, 2, 1, 1),      # a single pixel row, C < 8
    ("nhwc", 3, 8, 8, 5, 7),      # instance norm
    ("nhwc", 3, 12, 3, 5, 7),     # cg = 4: C no multiple of 8, the scalar instance
    ("nhwc", 1, 40, 4, 8, 8),     # cg = 10: a 16-byte vector straddles two groups
    ("nhwc", 3, 16, 1, 8, 8),     # one group
    ("nhwc", 1, 16, 2, 33, 33),   # three pixel slices, the last one partial
    ("nhwc", 1, 2056, 8, 1, 2),   # more than 256 channel vectors: a lane walks two columns
    ("nhwc", 1, 16, 2, 25, 41),   # ... the last one a single pixel row
]
assert _HW_AT[0] * _HW_AT[1] * 8 == REG_MAX or REG_MAX != 16384
assert map_plan("nchw", 1, 16, 2, 2049) == (9, 2048) or (SLICE_MIN, TARGET_WGS) != (2048, 1024)
assert map_plan("nhwc", 1, 16, 2, 1089) == (3, 512) or (INTER_SLICE_MIN, TARGET_WGS) != (8192, 1024)


def case_id(c):
    return "%s-%dx%dg%d-%dx%d" % c


def to_canon(x, case):
    lay, N, C, G, Hh, W = case
    if lay == "nhwc":
        return x.reshape(N, Hh * W, G, C // G).transpose(0, 2, 3, 1)
    return x.reshape(N, G, C // G, Hh * W)


def from_canon(xc, case):
    lay, N, C, G, Hh, W = case
    if lay == "nhwc":
        return np.ascontiguousarray(xc.transpose(0, 3, 1, 2)).reshape(N, Hh, W, C)
    return np.ascontiguousarray(xc).reshape((N, C) if lay == "nc" else (N, C, Hh, W))


def stat_shape(case):
    lay, N, C, G, Hh, W = case
    return {"nchw": (N, G, 1, 1), "nhwc": (N, 1, 1, G), "nc": (N, G)}[lay]


def param_shape(case):
    lay, N, C, G, Hh, W = case
    return {"nchw": (1, C, 1, 1), "nhwc": (1, 1, 1, C), "nc": (1, C)}[lay]


def cmds(case, affine):
    lay, N, C, G, Hh, W = case
    axis, reduce_axes = {"nchw": (1, (2, 3)), "nhwc": (3, (1, 2)), "nc": (1, ())}[lay]
    return tuple(nnc.CMD_GROUP_NORM(k, axis, G, 1e-5, affine, *reduce_axes) for k in ("GROUP_NORM_FORWARD", "GROUP_NORM_BACKWARD"))


def epsilon(case):
    """what the commands read: the reduce count seen as a float"""
    return {"nchw": 2, "nhwc": 2, "nc": 0}[case[0]] * 2.0 ** -149


# ---- inputs, canonical -----------------------------------------------------------------------------------------------------------------------------------
_DATA = {}


def data(case, offset=None):
    """a, g [N][G][cg][P], scale, bias [1][G][cg][1]: halves"""
    key = (case, offset)
    if key not in _DATA:
        lay, N, C, G, Hh, W = case
        cg, P = C // G, Hh * W
        rng = np.random.default_rng(abs(hash(case[1:])) % 2 ** 31 + len(lay))
        base = (rng.random((N, G, 1, 1)) - 0.5) * 16 if offset is None else offset
        a = ((rng.random((N, G, cg, P)) - 0.5) * 8 + base).astype(H)
        g = ((rng.random((N, G, cg, P)) - 0.5) * 4).astype(H)
        scale = (1 + (rng.random((1, G, cg, 1)) - 0.5) * 0.5).astype(H)
        bias = ((rng.random((1, G, cg, 1)) - 0.5) * 0.5).astype(H)
        for x in (a, g, scale, bias):
            x.setflags(write=False)
        _DATA[key] = (a, g, scale, bias)
    return _DATA[key]


# ---- expectations: {name: (want, E)} in float64, canonical ----------------------------------------------------------------------------------------------
def gn_forward(a, scale, bias, eps, centred_variance=True):
    a = a.astype(D)
    n = a.shape[2] * a.shape[3]
    mean = a.mean(axis=(2, 3), keepdims=True)
    dm = (n + 2) * U * np.abs(a).sum(axis=(2, 3), keepdims=True) / n
    var = ((a - mean) ** 2).mean(axis=(2, 3), keepdims=True) if centred_variance else (a * a).mean(axis=(2, 3), keepdims=True)
    w = a - mean
    istd = 1 / np.sqrt(var + eps)
    dis = istd ** 3 * (n + 4) * U * var / 2 + 3 * U * istd
    y = w * istd
    dy = istd * (dm + U * np.abs(w)) + np.abs(w) * dis + U * np.abs(y)
    sc = 1.0 if scale is None else scale.astype(D)
    bi = 0.0 if bias is None else bias.astype(D)
    return {"b": (y * sc + bi, np.abs(sc) * dy + 2 * U * (np.abs(y * sc) + np.abs(bi))), "mean": (mean, dm + 0 * mean), "inv_std": (istd, dis)}


def gn_backward(g, a, scale, mean, istd, centred=True):
    """mean, istd: as stored (float64 values of the stored numbers), [N][G][1][1]"""
    g, a = g.astype(D), a.astype(D)
    N, G, cg, P = a.shape
    n, rows = cg * P, N * P
    sc = 1.0 if scale is None else scale.astype(D)
    ah = (a - (mean if centred else 0.0)) * istd
    gss = g * sc * istd
    s1 = gss.sum(axis=(2, 3), keepdims=True)
    s2 = (ah * gss).sum(axis=(2, 3), keepdims=True)
    ds1 = (n + 2) * U * np.abs(gss).sum(axis=(2, 3), keepdims=True)
    ds2 = (n + 4) * U * np.abs(ah * gss).sum(axis=(2, 3), keepdims=True)
    h = gss - (s1 + ah * s2) / n
    eh = 4 * U * (np.abs(gss) + (np.abs(s1) + np.abs(ah * s2)) / n) + (ds1 + np.abs(ah) * ds2) / n
    return {"h": (h, eh), "dscale": ((ah * g).sum(axis=(0, 3), keepdims=True), (rows + 4) * U * np.abs(ah * g).sum(axis=(0, 3), keepdims=True)),
            "dbias": (g.sum(axis=(0, 3), keepdims=True), rows * U * np.abs(g).sum(axis=(0, 3), keepdims=True))}


def canon_of(x, k, case):
    lay, N, C, G, Hh, W = case
    if k in ("b", "h"):
        return to_canon(x, case)
    return x.reshape(N, G, 1, 1) if k in ("mean", "inv_std") else x.reshape(1, G, C // G, 1)


def check(got, want, case, what, names=None):
    for k in (names or got):
        x, (w, e) = got[k], want[k]
        within(canon_of(x, k, case), w, bound(w, e, x.dtype), "%s %s" % (what, k))


# ---- the commands ---------------------------------------------------------------------------------------------------------------------------------------
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


def forward_io(case, affine, pt):
    a, _, scale, bias = data(case)
    ins = [from_canon(a, case)] + ([x.astype(pt).reshape(param_shape(case)) for x in (scale, bias)] if affine else [])
    outs = [np.full(ins[0].shape, 3, H), np.full(stat_shape(case), 3, pt), np.full(stat_shape(case), 3, pt)]
    return ins, outs


def run_forward(L, case, affine, pt, mode="plain", flags=0, io=None):
    """-> {"b", "mean", "inv_std"} as the command left them.  mode "inplace": b = a"""
    ins, outs = io or forward_io(case, affine, pt)
    it, ot = place(L, ins, mode), place(L, outs, mode)
    if mode == "inplace":
        ot[0] = it[0]
    r = L.cmd_exec(cmds(case, affine)[0], nnc.NO_HINT, flags, it, ot)
    assert r == 0, "backend returned %d" % r
    return dict(zip(["b", "mean", "inv_std"], [t.numpy() for t in ot]))


def stored_stats(case, pt):
    """the forward statistics as a tensor of type pt holds them (float64 values), canonical"""
    f = gn_forward(data(case)[0], None, None, epsilon(case))
    return f["mean"][0].astype(pt).astype(D), f["inv_std"][0].astype(pt).astype(D)


def backward_io(case, affine, pt, want=("h", "dscale", "dbias"), unused=None):
    a, g, scale, _ = data(case)
    mean, istd = (x.astype(pt).reshape(stat_shape(case)) for x in stored_stats(case, pt))
    gl, al = from_canon(g, case), from_canon(a, case)
    if affine:
        ins = [gl, unused, unused, al, scale.astype(pt).reshape(param_shape(case)), unused, unused, mean, istd]
        names = ["h", "dscale", "dbias"]
    else:  # (the reference has no parameter gradients without parameters)
        ins, names = [gl, unused, unused, al, unused, mean, istd], ["h"]
    outs = [np.full(al.shape, 3, H) if "h" in want else None] + [np.full(param_shape(case), 3, pt) if k in want else None for k in names[1:]]
    return ins, outs, names


def run_backward(L, case, affine, pt, mode="plain", flags=0, **kw):
    ins, outs, names = backward_io(case, affine, pt, **kw)
    it, ot = place(L, ins, mode), place(L, outs, mode)
    if mode == "inplace":
        ot[0] = it[0]
    r = L.cmd_exec(cmds(case, affine)[1], nnc.NO_HINT, flags, it, ot)
    assert r == 0, "backend returned %d" % r
    return {k: t.numpy() for k, t in zip(names, ot) if t is not None}


def wants(case, affine, pt):
    a, g, scale, bias = data(case)
    mean, istd = stored_stats(case, pt)
    return gn_forward(a, scale if affine else None, bias if affine else None, epsilon(case)), gn_backward(g, a, scale if affine else None, mean, istd)


# ---- 1. values ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [1, 0], ids=["affine", "plain"])
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gnorm_half(backend, ref_lib, case, combo, affine):
    """Forward; backward with every gradient, with h alone and with the parameter gradients alone.  The parameter gradients alone carry the bits of the full
    command (the same sums and fold); h alone does where the full command takes the same form."""
    L, pt = backend, COMBOS[combo]
    lay = case[0]
    wf, wb = wants(case, affine, pt)
    got = run_forward(L, case, affine, pt)
    assert got["b"].dtype == H and got["mean"].dtype == pt and got["inv_std"].dtype == pt
    check(got, wf, case, "%s forward" % combo)
    full = run_backward(L, case, affine, pt)
    check(full, wb, case, "%s backward" % combo)
    only_h = run_backward(L, case, affine, pt, want=("h",))
    assert list(only_h) == ["h"]
    check(only_h, wb, case, "%s backward, h alone" % combo)
    if affine:
        if form(case, affine) == "split":
            same_bits(only_h["h"], full["h"], "h alone")
        only_p = run_backward(L, case, affine, pt, want=("dscale", "dbias"))
        assert sorted(only_p) == ["dbias", "dscale"]
        for k in only_p:
            same_bits(only_p[k], full[k], k + " alone")
        only_s = run_backward(L, case, affine, pt, want=("dscale",))
        same_bits(only_s["dscale"], full["dscale"], "dscale without dbias")
    else:
        same_bits(only_h["h"], full["h"], "h, plain")
    if combo == "hh":  # the reference on the widened inputs, once per case: the fp32 form
        fmt = "NHWC" if lay == "nhwc" else "NCHW"
        fwd, bwd = cmds(case, affine)
        ins, outs = forward_io(case, affine, H)
        ref = dict(zip(["b", "mean", "inv_std"], ref_run(ref_lib, fwd, ins, [np.zeros(x.shape, F) for x in outs], fmt)))
        check(ref, {k: (w, e + U * np.abs(w)) for k, (w, e) in wf.items()}, case, "forward, reference")
        bi_, bo_, names = backward_io(case, affine, H)
        ref = dict(zip(names, ref_run(ref_lib, bwd, bi_, [np.zeros(x.shape, F) for x in bo_], fmt)))
        check(ref, {k: (w, e + U * np.abs(w)) for k, (w, e) in wb.items()}, case, "backward, reference")


def test_wrong_expectations_break_the_bounds():
    """The bounds are not too loose: the variance around zero, the statistics of the wrong group for a vector that straddles two groups, and dscale without
    centring each leave them; so do serially accumulated raw fp32 moments at a large offset, where a two-pass fp32 variance keeps a margin above 1000."""
    case = ("nhwc", 1, 40, 4, 8, 8)
    a, g, scale, bias = data(case)
    eps = epsilon(case)
    good = gn_forward(a, scale, bias, eps)

    w, e = good["b"]
    wrong = gn_forward(a, scale, bias, eps, centred_variance=False)
    assert (np.abs(wrong["b"][0] - w) > 2 * bound(w, e, H)).any(), "variance around zero"
    ad = a.astype(D)
    mean, istd = ad.mean(axis=(2, 3)), 1 / ad.std(axis=(2, 3))  # [N][G]
    gw = np.array([(8 * (c // 8)) // 10 for c in range(40)]).reshape(4, 10)  # every channel takes the group its 8-channel vector STARTS in
    wrong_b = (ad - mean[:, gw][..., None]) * istd[:, gw][..., None] * scale.astype(D) + bias.astype(D)
    assert (np.abs(wrong_b - w) > 2 * bound(w, e, H)).any(), "the wrong group"
    mean, istd = stored_stats(case, H)
    goodb = gn_backward(g, a, scale, mean, istd)
    wrongb = gn_backward(g, a, scale, mean, istd, centred=False)
    w, e = goodb["dscale"]
    assert (np.abs(wrongb["dscale"][0] - w) > 2 * bound(w, e, H)).any()
    # a = 512 + U(-4, 4), n = 16 900, fp32
    big = ("nchw", 1, 8, 2, 65, 65)
    a = data(big, offset=512.0)[0]
    f = gn_forward(a, None, None, 0.0)
    w, e = f["inv_std"]
    x = a.astype(F)[0, 0].ravel()
    n = x.size
    m32 = F(x.sum(dtype=F) / F(n))
    two_pass = F(1) / np.sqrt(F(((x - m32) ** 2).sum(dtype=F) / F(n)))
    assert abs(D(two_pass) - w[0, 0, 0, 0]) * 1000 < e[0, 0, 0, 0]
    s1, s2 = np.cumsum(x, dtype=F)[-1], np.cumsum(x * x, dtype=F)[-1]
    raw = F(1) / np.sqrt(np.maximum(F(s2 / F(n)) - F(s1 / F(n)) ** 2, F(1e-30)))
    assert not abs(D(raw) - w[0, 0, 0, 0]) <= e[0, 0, 0, 0]


@pytest.mark.parametrize("case", [("nchw", 1, 8, 2, 65, 65), ("nhwc", 1, 16, 2, 33, 33)], ids=case_id)
def test_large_offset(backend, case):
    """a = 512 + U(-4, 4), "hf": saved_inv_std (and the rest) within the derived bound -- a guard against E[x^2] - mean^2, not a proof of the formula."""
    L = backend
    a = data(case, offset=512.0)[0]
    al = from_canon(a, case)
    got = run_forward(L, case, 0, F, io=([al], [np.full(al.shape, 3, H), np.full(stat_shape(case), 3, F), np.full(stat_shape(case), 3, F)]))
    check(got, gn_forward(a, None, None, epsilon(case)), case, "offset 512")


# ---- 2. unaligned bases, 3. in place, 4. twice ---------------------------------------------------------------------------------------------------------------
SOME = [("nchw", 1, 20, 2, 8, 8), ("nchw", 1, 16, 2) + _HW_ABOVE, ("nhwc", 1, 40, 4, 8, 8), ("nhwc", 1, 16, 2, 33, 33)]  # reg, planar split, inter, inter in three slices


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("case", SOME, ids=case_id)
def test_unaligned_bases(backend, case, combo):
    """Every tensor starts one element past a 16-byte boundary: the scalar instances."""
    L, pt = backend, COMBOS[combo]
    wf, wb = wants(case, 1, pt)
    check(run_forward(L, case, 1, pt, "unaligned"), wf, case, "unaligned forward")
    check(run_backward(L, case, 1, pt, "unaligned"), wb, case, "unaligned backward")
    check(run_backward(L, case, 1, pt, "unaligned", want=("h",)), wb, case, "unaligned backward, h alone")


@pytest.mark.parametrize("case", SOME, ids=case_id)
def test_in_place_and_twice(backend, case):
    """b = a and h = g carry the bits of the out-of-place run; two runs carry the same bits."""
    L, pt = backend, H
    first = run_forward(L, case, 1, pt)
    for other, what in ((run_forward(L, case, 1, pt), "twice"), (run_forward(L, case, 1, pt, "inplace"), "in place")):
        for k in first:
            same_bits(other[k], first[k], "forward %s %s" % (what, k))
    for want in (("h", "dscale", "dbias"), ("h",)):
        first = run_backward(L, case, 1, pt, want=want)
        for other, what in ((run_backward(L, case, 1, pt, want=want), "twice"), (run_backward(L, case, 1, pt, "inplace", want=want), "in place")):
            for k in first:
                same_bits(other[k], first[k], "backward %s %s" % (what, k))


# ---- 5. routes ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [1, 0], ids=["affine", "plain"])
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("case", SOME, ids=case_id)
def test_routes(backend, case, combo, affine):
    """No half tensor named by the row gets an fp32 image and all of them are counted native; the launch records hold only gnorm_* kernels of the expected
    layout and form, in the stated number, and no conversion; with the key at 0 every half tensor is staged again, no gnorm_ label appears and the result still
    meets the bounds."""
    L, pt = backend, COMBOS[combo]
    f, hh = form(case, affine), combo == "hh"
    wf, wb = wants(case, affine, pt)
    nparam = 2 if affine else 0
    steps = [("fwd", lambda: run_forward(L, case, affine, pt), 2 + (2 + nparam if hh else 0), 1 if f == "reg" else 2, f, wf),
             ("bwd", lambda: run_backward(L, case, affine, pt), 3 + (2 + (3 if affine else 0) if hh else 0), 3 if affine or f == "split" else 1, "split" if affine else f, wb),
             ("bwd", lambda: run_backward(L, case, affine, pt, want=("h",)), 3 + (2 + (1 if affine else 0) if hh else 0), 1 if f == "reg" else 3, f, wb)]
    if affine:
        steps.append(("bwd", lambda: run_backward(L, case, affine, pt, want=("dscale", "dbias")), 2 + (5 if hh else 0), 2, "split", wb))
    for tag, call, halves, launches, fm, want in steps:
        s0, n0 = counts(L)
        got, names = records(L, call)
        assert counts(L) == (s0, n0 + halves), (tag, counts(L), (s0, n0), halves)
        assert len(names) == launches, names
        assert all(x.startswith("gnorm_%s_%s|nnc::gnorm::%s_%s" % (tag, combo, layout_tag(case, affine), fm)) for x in names), names
        assert not any("half_up" in x or "half_down" in x for x in names), names
        with key_off(L, KEY):
            s0, n0 = counts(L)
            off, names = records(L, call)
            assert counts(L) == (s0 + halves, n0), (tag, counts(L), (s0, n0), halves)
            assert not any(x.startswith("gnorm_") for x in names), names
        check(off, want, case, "%s %s, fp32 images" % (tag, combo))


def test_tuning_key_is_listed(backend):
    assert backend.tune_get(KEY) == 1


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_keep_their_route(backend):
    """H-only reduction, a dense view, a strided view, CCV_NNC_ACCUMULATE_OUTPUT and a parameter tensor of one element keep the fp32 images and what the
    command returned before; an fp32 tensor in an unused slot of the backward command does NOT refuse."""
    L, pt = backend, H
    case = ("nchw", 1, 20, 2, 8, 8)
    wf, wb = wants(case, 1, pt)
    fwd = cmds(case, 1)[0]
    ins, outs = forward_io(case, 1, pt)

    def staged(call, halves=6, ret=0):
        s0, n0 = counts(L)
        r, names = records(L, call)
        assert r == ret and counts(L) == (s0 + halves, n0) and not any(x.startswith("gnorm_") for x in names), (r, names, counts(L), (s0, n0))

    # H-only reduction: one statistic per (image, group, column)
    rng = np.random.default_rng(5)
    a2 = ((rng.random((3, 12, 4, 4)) - 0.5) * 8).astype(H)
    t2 = make_tensors(L, nnc.GPU_MEMORY, [a2, np.full(a2.shape, 3, H), np.full((3, 3, 1, 4), 3, H), np.full((3, 3, 1, 4), 3, H)])
    hcmd = nnc.CMD_GROUP_NORM("GROUP_NORM_FORWARD", 1, 3, 1e-5, 0, 2)
    staged(lambda: L.cmd_exec(hcmd, nnc.NO_HINT, 0, t2[:1], t2[1:]), halves=4)
    blk = a2.astype(D).reshape(3, 3, 4, 4, 4)
    wantb = (blk - blk.mean(axis=(2, 3), keepdims=True)) / blk.std(axis=(2, 3), keepdims=True)
    assert np.abs(t2[1].numpy().astype(D).reshape(blk.shape) - wantb).max() < 4e-3
    # a dense view: staged, right
    ts = make_tensors(L, nnc.GPU_MEMORY, ins + outs)
    ts[0] = ts[0].view(ins[0].shape, (20 * 64, 64, 8, 1), 0)
    staged(lambda: L.cmd_exec(fwd, nnc.NO_HINT, 0, ts[:3], ts[3:]))
    check(dict(zip(["b", "mean", "inv_std"], [t.numpy() for t in ts[3:]])), wf, case, "a dense view")
    # a strided view: refused by the fp32 kernel underneath, as it was
    ts = make_tensors(L, nnc.GPU_MEMORY, ins + outs)
    (wide,) = make_tensors(L, nnc.GPU_MEMORY, [np.ones((1, 20, 8, 16), H)])
    staged(lambda: L.cmd_exec(fwd, nnc.NO_HINT, 0, [wide.view(ins[0].shape, (20 * 128, 128, 16, 1), 0)] + ts[1:3], ts[3:]), ret=-1)
    # ACCUMULATE_OUTPUT: staged; the same bits as with the key at 0
    s0, n0 = counts(L)
    got = run_forward(L, case, 1, pt, flags=nnc.ACCUMULATE_OUTPUT)
    assert counts(L) == (s0 + 6, n0)
    with key_off(L, KEY):
        off = run_forward(L, case, 1, pt, flags=nnc.ACCUMULATE_OUTPUT)
    for k in got:
        same_bits(got[k], off[k], "ACCUMULATE_OUTPUT " + k)
    # a scale and a bias of one element: staged, the same bits as with the key at 0
    one = [ins[0], np.full((1, 1, 1, 1), 1.25, H), np.full((1, 1, 1, 1), 0.5, H)]
    ts = make_tensors(L, nnc.GPU_MEMORY, one + outs)
    staged(lambda: L.cmd_exec(fwd, nnc.NO_HINT, 0, ts[:3], ts[3:]))
    with key_off(L, KEY):
        to = make_tensors(L, nnc.GPU_MEMORY, one + outs)
        assert L.cmd_exec(fwd, nnc.NO_HINT, 0, to[:3], to[3:]) == 0
    for x, y in zip(ts[3:], to[3:]):
        same_bits(x.numpy(), y.numpy(), "one-element parameters")
    # an fp32 tensor in the unused slots: native all the same
    s0, n0 = counts(L)
    got, names = records(L, lambda: run_backward(L, case, 1, pt, unused=np.zeros(ins[0].shape, F)))
    assert counts(L) == (s0, n0 + 8) and names[0].startswith("gnorm_bwd_hh|"), names
    check(got, wb, case, "fp32 tensors in unused slots")
    L.stream_wait(None)


def test_half_parameters_beside_fp32_statistics(backend):
    """Half maps, half scale and bias, fp32 statistics: the all-half row's mask meets an fp32 tensor and refuses, the maps-only row takes the command -- the
    two parameters get their small fp32 images, the maps do not."""
    L = backend
    case = ("nhwc", 1, 40, 4, 8, 8)
    ins, outs = forward_io(case, 1, H)
    ts = make_tensors(L, nnc.GPU_MEMORY, ins + [outs[0], outs[1].astype(F), outs[2].astype(F)])
    s0, n0 = counts(L)
    r, names = records(L, lambda: L.cmd_exec(cmds(case, 1)[0], nnc.NO_HINT, 0, ts[:3], ts[3:]))
    assert r == 0 and counts(L) == (s0 + 2, n0 + 2), (counts(L), (s0, n0))
    assert len(names) == 2 and all(x.startswith("gnorm_fwd_hf|nnc::gnorm::inter_split") for x in names), names
    check(dict(zip(["b", "mean", "inv_std"], [t.numpy() for t in ts[3:]])), wants(case, 1, F)[0], case, "half parameters, fp32 statistics")
