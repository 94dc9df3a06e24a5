"""The element-wise legs of an MBConv block on CCV_16F tensors without fp32 images: the five activation families and dropout as halves
(cmd_act_opt.cpp, cmd_ew.cpp; tunable ACT_HALF_NATIVE), and MUL of an activation tensor by one value per (image, channel) -- the
squeeze-excite scale -- on the plane-scale kernels of mul_planes.h in half and fp32 (tunable MUL_PLANES).

Every operation is stated in float64 numpy on the half-rounded inputs; the reference's CPU backend runs the same command on the widened
inputs where it implements it, and must meet the fp32 form of the same bound.  Bounds are derived, not tuned:
  half output of a one-rounding map   |got - want| <= 2^-11 |want| + 2^-24 + 2^-19 S
      S = the sum of the magnitudes of the expression's terms; 2^-11 |want| is one rounding to half, 2^-24 the half subnormal floor,
      2^-19 S sixteen fp32 ulps for the device's expf / tanhf / erff
  half sum over R elements            2^-11 |want| + 2^-24 + R 2^-24 sum|terms|
  fp32 sum over R elements            R 2^-24 sum|terms|
  pure multiplies (MUL forward, the large operand's gradient, leaky ReLU, dropout): bit for bit the route with the tuning key at 0 -- the fp32
      value is the same before the one rounding.
The transcendental activations are also compared with the key-off route and the number of differing elements is printed, not asserted.
"""
import contextlib
import ctypes
import zlib
import numpy as np
import pytest
from ccv_amd import nnc
from harness import exec_on, make_tensors

F, H, D = np.float32, np.float16, np.float64
ACT_KEY, MUL_KEY = "ACT_HALF_NATIVE", "MUL_PLANES"


def counts(L):
    """(half tensors staged through fp32 images, half tensors handed to kernels as halves) so far"""
    a, b = ctypes.c_long(), ctypes.c_long()
    L.dll.nnc_mi355x_debug_half_counts(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def records(L, fn):
    L.profile_enable(1)
    try:
        out = fn()
        L.stream_wait(None)
        names = [r[0] for r in L.profile_records()]
    finally:
        L.profile_enable(0)
    return out, names


@contextlib.contextmanager
def key_off(L, name):
    L.tune_set(name, 0)
    try:
        yield
    finally:
        L.tune_set(name, 1)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint16 if x.dtype == H else np.uint32)


def within(got, want, bound, what):
    err = np.abs(np.asarray(got, D) - want)
    bad = ~(err <= bound)
    assert not bad.any(), "%s: %d elements off, worst error / bound %.3f" % (what, int(bad.sum()), float((err[bad] / np.maximum(np.asarray(bound + 0 * err)[bad], 1e-300)).max()))


def half_bound(want, s):
    return 2.0 ** -11 * np.abs(want) + 2.0 ** -24 + 2.0 ** -19 * s


def run(L, cmd, ins, outs, fmt="NHWC", flags=0):
    r, res = exec_on(L, nnc.GPU_MEMORY, cmd, nnc.NO_HINT, flags, ins, outs, fmt)
    assert r == 0, "backend returned %d" % r
    return res


def ref_run(ref, cmd, ins, outs, fmt="NHWC"):
    up = lambda xs: [None if x is None else (x.astype(F) if x.dtype == H else x) for x in xs]
    r, res = exec_on(ref, nnc.CPU_MEMORY, cmd, nnc.NO_HINT, 0, up(ins), up(outs), fmt, backend=nnc.BACKEND_CPU_REF)
    assert r == 0, "reference returned %d" % r
    return res


# ---- activations --------------------------------------------------------------------------------------------------------------------
def _erf(x):
    import math
    return np.vectorize(math.erf)(x)


K, CC = np.sqrt(2.0 / np.pi), 0.044715
SLOPE = 0.2


def act_forward(name, a):
    """(want, S) in float64"""
    if name == "SIGMOID":
        w = 1.0 / (1.0 + np.exp(-a)); return w, np.abs(w)
    if name == "TANH":
        w = np.tanh(a); return w, np.abs(w)
    if name == "SWISH":
        w = a / (1.0 + np.exp(-a)); return w, np.abs(w)
    if name == "GELU":
        e = _erf(a * np.sqrt(0.5)); return 0.5 * a * (1 + e), 0.5 * np.abs(a) * (1 + np.abs(e))
    if name == "GELU_TANH":
        t = np.tanh(K * (a + CC * a ** 3)); return 0.5 * a * (1 + t), 0.5 * np.abs(a) * (1 + np.abs(t))
    w = np.where(a >= 0, a, D(F(SLOPE)) * a); return w, np.abs(w)


def act_backward(name, g, a, b):
    """(want, S) in float64; b = the forward output (used by sigmoid, tanh, leaky ReLU), a the forward input (the others)"""
    ag = np.abs(g)
    if name == "SIGMOID":
        return g * b * (1 - b), ag * (np.abs(b) + b * b)
    if name == "TANH":
        return g * (1 - b * b), ag * (1 + b * b)
    if name == "SWISH":
        y = 1.0 / (1.0 + np.exp(-a)); return g * (a * (y - y * y) + y), ag * (np.abs(a) * (y + y * y) + y)
    if name == "GELU":
        cdf, pdf = 0.5 * (1 + _erf(a * np.sqrt(0.5))), np.exp(-0.5 * a * a) * K
        return g * (cdf + a * pdf), ag * (0.5 + np.abs(cdf - 0.5) + np.abs(a) * pdf)
    if name == "GELU_TANH":
        t = np.tanh(K * (a + CC * a ** 3))
        left, f = 0.5 * (1 + t), 0.5 * a * K * (1 + 3 * CC * a * a)
        return g * (left + f * (1 - t * t)), ag * (0.5 + 0.5 * np.abs(t) + np.abs(f) * (1 + t * t))
    return np.where(b >= 0, g, D(F(SLOPE)) * g), ag


def act_cmds(name):
    if name.startswith("GELU"):
        return nnc.CMD_GELU_FORWARD(int(name.endswith("TANH"))), nnc.CMD_GELU_BACKWARD(int(name.endswith("TANH")))
    if name == "LEAKY_RELU":
        return nnc.CMD_LEAKY_RELU_FORWARD(SLOPE), nnc.CMD_LEAKY_RELU_BACKWARD(SLOPE)
    return nnc.generic_cmd(name + "_FORWARD"), nnc.generic_cmd(name + "_BACKWARD")


ACTS = ["SIGMOID", "TANH", "SWISH", "GELU", "GELU_TANH", "LEAKY_RELU"]
_ACT_DATA = {}


def act_data(n):
    if n not in _ACT_DATA:
        rng = np.random.default_rng(100 + n)
        a, g = ((rng.random(n) - 0.5) * 16).astype(H), ((rng.random(n) - 0.5) * 4).astype(H)
        a[:5] = np.array([8, -8, 0, 0.5, -0.5], H)[:n]
        a.setflags(write=False); g.setflags(write=False)
        _ACT_DATA[n] = (a, g)
    return _ACT_DATA[n]


def aliased(L, arrays, off):
    """Each array as a dense tensor that starts `off` elements into a larger allocation."""
    out = []
    for x in arrays:
        buf = np.full(x.size + 8, 7, x.dtype)
        buf[off:off + x.size] = x.ravel()
        (t,) = make_tensors(L, nnc.GPU_MEMORY, [buf])
        out.append(t.alias(x.shape, off))
    return out


def act_exec(L, cmd, ins, n, misaligned):
    """ins: half arrays or None -> the half output.  misaligned: the INPUTS start 2 bytes past a 16-byte boundary (the scalar path)."""
    if not misaligned:
        return run(L, cmd, ins, [np.full(n, 3, H)])[0]
    ts = aliased(L, [x for x in ins if x is not None], 1)
    assert all(t.ptr % 16 == 2 for t in ts)
    it = iter(ts)
    tin = [None if x is None else next(it) for x in ins]
    (out,) = make_tensors(L, nnc.GPU_MEMORY, [np.full(n, 3, H)])
    assert L.cmd_exec(cmd, nnc.NO_HINT, 0, tin, [out]) == 0
    return out.numpy()


@pytest.mark.parametrize("size", [3240, 3243, 5, "3240-misaligned"], ids=str)
@pytest.mark.parametrize("name", ACTS)
def test_activation_half(backend, ref_lib, name, size):
    """3240 elements are 405 whole vectors of 8 halves; 3243 add a tail of three; 5 are a tail alone; the alias's inputs start 2 bytes past a
    16-byte boundary, so all of its 3240 elements take the scalar loop."""
    L = backend
    mis = isinstance(size, str)
    n = 3240 if mis else size
    a, g = act_data(3243)
    a, g = a[:n], g[:n]
    fwd, bwd = act_cmds(name)
    from_output = name in ("SIGMOID", "TANH", "LEAKY_RELU")
    want, s = act_forward(name, a.astype(D))
    s0, n0 = counts(L)
    got, names = records(L, lambda: act_exec(L, fwd, [a], n, mis))
    assert counts(L) == (s0, n0 + 2)
    assert got.dtype == H
    within(got, want, half_bound(want, s), name + " forward")
    ref = ref_run(ref_lib, fwd, [a], [np.zeros(n, H)])[0]
    within(ref, want, 2.0 ** -23 * np.abs(want) + 2.0 ** -19 * s, name + " forward, reference")
    b = want.astype(H)
    wantb, sb = act_backward(name, g.astype(D), a.astype(D), b.astype(D))
    ins = [g, None, b] if from_output else [g, a, None]
    s0, n0 = counts(L)
    gotb = act_exec(L, bwd, ins, n, mis)
    assert counts(L) == (s0, n0 + 3)
    within(gotb, wantb, half_bound(wantb, sb), name + " backward")
    refb = ref_run(ref_lib, bwd, ins, [np.zeros(n, H)])[0]
    within(refb, wantb, 2.0 ** -23 * np.abs(wantb) + 2.0 ** -19 * sb, name + " backward, reference")
    with key_off(L, ACT_KEY):
        s0, n0 = counts(L)
        off_f, off_b = act_exec(L, fwd, [a], n, mis), act_exec(L, bwd, ins, n, mis)
        s1, n1 = counts(L)
        assert n1 == n0 and s1 == s0 + 5
    within(off_f, want, half_bound(want, s), name + " forward, fp32 images")
    if name == "LEAKY_RELU":
        assert np.array_equal(bits(got), bits(off_f)) and np.array_equal(bits(gotb), bits(off_b))
        assert np.array_equal(bits(got), bits(np.where(a >= 0, a, (a.astype(F) * F(SLOPE)).astype(H))))
    else:
        print("%s n=%s: %d forward / %d backward elements differ from the fp32-image route" % (name, size, int((bits(got) != bits(off_f)).sum()), int((bits(gotb) != bits(off_b)).sum())))


def test_activation_backward_without_gradient_keeps_fp32_images(backend):
    """SIGMOID_BACKWARD without g (ones): staged as before, h = b (1 - b)."""
    L = backend
    a, _ = act_data(3243)
    b = act_forward("SIGMOID", a.astype(D))[0].astype(H)
    s0, n0 = counts(L)
    got = run(L, nnc.generic_cmd("SIGMOID_BACKWARD"), [None, None, b], [np.full(b.shape, 3, H)])[0]
    s1, n1 = counts(L)
    assert n1 == n0 and s1 == s0 + 2
    bd = b.astype(D)
    within(got, bd * (1 - bd), half_bound(bd * (1 - bd), bd + bd * bd), "sigmoid backward, no g")


def test_routes_swish_and_dropout(backend):
    """Native: the staged count stays, the native count grows by the half tensors handed over (swish 2 / 3, dropout 2 / 2); key at 0: the other way round."""
    L = backend
    a, g = act_data(3243)
    a, g = a[:3240], g[:3240]
    n = a.size
    at, gt, bt, ht, mask = make_tensors(L, nnc.GPU_MEMORY, [a, g, np.zeros(n, H), np.zeros(n, H), np.zeros(n // 2, H)])
    drop_f = nnc.CMD_DROPOUT_FORWARD(0.4)
    drop_b = nnc.CMD_DROPOUT_FORWARD(0.4)
    drop_b.cmd = nnc.CMD["DROPOUT_BACKWARD"]
    steps = [(nnc.generic_cmd("SWISH_FORWARD"), [at], [bt], 2), (nnc.generic_cmd("SWISH_BACKWARD"), [gt, at], [ht], 3),
             (drop_f, [at], [bt, mask], 2), (drop_b, [gt, None, None, None, mask], [ht], 2)]
    for cmd, ins, outs, k in steps:
        s0, n0 = counts(L)
        assert L.cmd_exec(cmd, nnc.NO_HINT, 0, ins, outs) == 0
        assert counts(L) == (s0, n0 + k)
    with key_off(L, ACT_KEY):
        for cmd, ins, outs, k in steps:
            s0, n0 = counts(L)
            assert L.cmd_exec(cmd, nnc.NO_HINT, 0, ins, outs) == 0
            assert counts(L) == (s0 + k, n0)
    L.stream_wait(None)


# ---- dropout ------------------------------------------------------------------------------------------------------------------------
def _dropout_data():
    rng = np.random.default_rng(7)
    n = 4104
    a = (np.exp(rng.random(n) * np.log(64.0)) / 16).astype(H) * np.where(rng.random(n) < 0.5, H(-1), H(1))   # 2^-4 <= |a| <= 4
    g = (np.exp(rng.random(n) * np.log(64.0)) / 16).astype(H) * np.where(rng.random(n) < 0.5, H(-1), H(1))
    assert (np.abs(a) >= H(2.0 ** -4)).all()
    return a, g


def test_dropout_half(backend):
    L = backend
    a, g = _dropout_data()
    n, p = a.size, 0.4
    inv_p = F(1) / (F(1) - F(p))
    at, gt, bt, ht, mask = make_tensors(L, nnc.GPU_MEMORY, [a, g, np.full(n, 3, H), np.full(n, 3, H), np.zeros(n // 2, H)])
    fwd = nnc.CMD_DROPOUT_FORWARD(p)
    bwd = nnc.CMD_DROPOUT_FORWARD(p)
    bwd.cmd = nnc.CMD["DROPOUT_BACKWARD"]
    s0, n0 = counts(L)
    assert L.cmd_exec(fwd, nnc.NO_HINT, 0, [at], [bt, mask]) == 0
    assert L.cmd_exec(bwd, nnc.NO_HINT, 0, [gt, None, None, None, mask], [ht]) == 0
    assert counts(L) == (s0, n0 + 4)
    b, h, m = bt.numpy(), ht.numpy(), mask.numpy().view(np.uint8)[:n]
    kept = (a.astype(F) * inv_p).astype(H)
    dropped = b == 0
    assert np.array_equal(m != 0, dropped) and set(np.unique(m)) <= {0, 1}
    assert np.array_equal(bits(b[~dropped]), bits(kept[~dropped])) and np.array_equal(bits(b[dropped]), np.zeros(int(dropped.sum()), np.uint16))
    assert abs(int(dropped.sum()) - n * p) <= 6 * np.sqrt(n * p * (1 - p)), int(dropped.sum())
    assert np.array_equal(h == 0, dropped)
    assert np.array_equal(bits(h[~dropped]), bits((g.astype(F) * inv_p).astype(H)[~dropped]))


def test_dropout_half_entirety(backend):
    L = backend
    a, g = _dropout_data()
    n, p = a.size, 0.4
    inv_p = F(1) / (F(1) - F(p))
    at, gt, bt, ht, mask = make_tensors(L, nnc.GPU_MEMORY, [a, g, np.full(n, 3, H), np.full(n, 3, H), np.zeros(n // 2, H)])
    fwd = nnc.CMD_DROPOUT_FORWARD(p, 1)
    bwd = nnc.CMD_DROPOUT_FORWARD(p, 1)
    bwd.cmd = nnc.CMD["DROPOUT_BACKWARD"]
    seen = set()
    for _ in range(4):
        s0, n0 = counts(L)
        assert L.cmd_exec(fwd, nnc.NO_HINT, 0, [at], [bt, mask]) == 0
        assert L.cmd_exec(bwd, nnc.NO_HINT, 0, [gt, None, None, None, mask], [ht]) == 0
        assert counts(L) == (s0, n0 + 4)
        b, h, decision = bt.numpy(), ht.numpy(), int(mask.numpy().view(np.int32)[0])
        assert decision in (0, 1)
        seen.add(decision)
        if decision:
            assert not b.any() and not h.any()
        else:
            assert np.array_equal(bits(b), bits((a.astype(F) * inv_p).astype(H))) and np.array_equal(bits(h), bits((g.astype(F) * inv_p).astype(H)))
    print("entirety decisions seen:", sorted(seen))


# ---- MUL by a per-(image, channel) vector ------------------------------------------------------------------------------------------
P_MUL = 0.7
NCHW_SHAPES = [(2, 3, 7, 7), (2, 3, 1, 3), (1, 1, 8, 8), (2, 5, 8, 8), (1, 2, 56, 56), (1, 1, 112, 112)]
NHWC_SHAPES = [((2, 7, 7, 8), (F, H)), ((1, 1, 3, 24), (F, H)), ((2, 4, 4, 16), (F, H)), ((2, 4, 4, 4), (F,))]
MUL_CASES = [("NCHW", s, dt) for s in NCHW_SHAPES for dt in (F, H)] + [("NHWC", s, dt) for s, dts in NHWC_SHAPES for dt in dts]
_MUL_DATA = {}


def small_shape(fmt, shape):
    return (shape[0], shape[1], 1, 1) if fmt == "NCHW" else (shape[0], 1, 1, shape[3])


def mul_data(fmt, shape, dt):
    key = (fmt, shape, dt)
    if key not in _MUL_DATA:
        rng = np.random.default_rng(zlib.crc32(repr((fmt, shape)).encode()))
        mk = lambda s: ((rng.random(s) - 0.5) * 4).astype(dt)
        x, s, g = mk(shape), mk(small_shape(fmt, shape)), mk(shape)
        p = D(F(P_MUL))
        x64, s64, g64 = x.astype(D), s.astype(D), g.astype(D)
        axes = (2, 3) if fmt == "NCHW" else (1, 2)
        d = dict(x=x, s=s, g=g, c=p * x64 * s64, dx=p * g64 * s64, ds=(p * g64 * x64).sum(axis=axes, keepdims=True),
                 ds_abs=np.abs(p * g64 * x64).sum(axis=axes, keepdims=True), R=shape[axes[0]] * shape[axes[1]])
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _MUL_DATA[key] = d
    return _MUL_DATA[key]


def map_bound(want, dt):
    return half_bound(want, np.abs(want)) if dt == H else 2.0 ** -22 * np.abs(want)  # fp32: two roundings, p x and the product


def sum_bound(d, dt):
    b = d["R"] * 2.0 ** -24 * d["ds_abs"]
    return 2.0 ** -11 * np.abs(d["ds"]) + 2.0 ** -24 + b if dt == H else b


def mul_forward(L, d, fmt, first, flags=0):
    ins = [d["s"], d["x"]] if first else [d["x"], d["s"]]
    return run(L, nnc.CMD_MUL_FORWARD(P_MUL), ins, [np.full(d["x"].shape, 3, d["x"].dtype)], fmt, flags)[0]


def mul_backward(L, d, fmt, first, what=("dx", "ds")):
    """-> (dx, ds), None where not asked for; the outputs are pre-filled with 3"""
    dt = d["x"].dtype
    ins = [d["g"], d["s"], d["x"]] if first else [d["g"], d["x"], d["s"]]
    ox = np.full(d["x"].shape, 3, dt) if "dx" in what else None
    os_ = np.full(d["s"].shape, 3, dt) if "ds" in what else None
    res = run(L, nnc.CMD_MUL_BACKWARD(P_MUL), ins, [os_, ox] if first else [ox, os_], fmt)
    return (res[1], res[0]) if first else (res[0], res[1])


@pytest.mark.parametrize("first", [False, True], ids=["small-second", "small-first"])
@pytest.mark.parametrize("fmt,shape,dt", MUL_CASES, ids=["%s-%s-%s" % (f, "x".join(map(str, s)), "f16" if dt == H else "f32") for f, s, dt in MUL_CASES])
def test_mul_planes(backend, ref_lib, fmt, shape, dt, first):
    L = backend
    d = mul_data(fmt, shape, dt)
    half = dt == H
    # forward
    s0, n0 = counts(L)
    c, names = records(L, lambda: mul_forward(L, d, fmt, first))
    assert counts(L) == ((s0, n0 + 3) if half else (s0, n0))
    assert any("mul_planes_fwd" in x for x in names), names
    assert c.dtype == dt
    within(c, d["c"], map_bound(d["c"], dt), "forward")
    # backward: both outputs, twice; then each alone
    s0, n0 = counts(L)
    (dx, ds), names = records(L, lambda: mul_backward(L, d, fmt, first))
    assert counts(L) == ((s0, n0 + 5) if half else (s0, n0))
    assert any("mul_planes_back" in x for x in names), names
    within(dx, d["dx"], map_bound(d["dx"], dt), "gradient of the large operand")
    within(ds, d["ds"], sum_bound(d, dt), "gradient of the small operand")
    dx2, ds2 = mul_backward(L, d, fmt, first)
    assert np.array_equal(bits(dx), bits(dx2)) and np.array_equal(bits(ds), bits(ds2))
    (dx_only, none), names_x = records(L, lambda: mul_backward(L, d, fmt, first, what=("dx",)))
    assert none is None and np.array_equal(bits(dx_only), bits(dx)) and any("mul_planes_back" in x for x in names_x), names_x
    (none, ds_only), names_s = records(L, lambda: mul_backward(L, d, fmt, first, what=("ds",)))
    assert none is None and np.array_equal(bits(ds_only), bits(ds)) and any("mul_planes_back" in x for x in names_s), names_s
    # the generic route: no such launch record, half tensors staged; forward and the large operand's gradient carry the same bits
    with key_off(L, MUL_KEY):
        s0, n0 = counts(L)
        (c0, (dx0, ds0)), names0 = records(L, lambda: (mul_forward(L, d, fmt, first), mul_backward(L, d, fmt, first)))
        s1, n1 = counts(L)
    assert not any("mul_planes" in x for x in names0), names0
    assert n1 == n0 and s1 == (s0 + 8 if half else s0)
    assert np.array_equal(bits(c), bits(c0)) and np.array_equal(bits(dx), bits(dx0))
    within(ds0, d["ds"], sum_bound(d, dt), "gradient of the small operand, generic route")
    # the reference's CPU backend on the widened inputs
    up = lambda x: x.astype(F)
    ins = [d["s"], d["x"]] if first else [d["x"], d["s"]]
    rc = ref_run(ref_lib, nnc.CMD_MUL_FORWARD(P_MUL), ins, [np.zeros(shape, F)], fmt)[0]
    within(rc, d["c"], 2.0 ** -22 * np.abs(d["c"]), "forward, reference")
    rb = ref_run(ref_lib, nnc.CMD_MUL_BACKWARD(P_MUL), [d["g"]] + ins, [np.zeros(i.shape, F) for i in ins], fmt)
    within(rb[1] if first else rb[0], d["dx"], 2.0 ** -22 * np.abs(d["dx"]), "large gradient, reference")
    within(rb[0] if first else rb[1], d["ds"], (d["R"] + 2) * 2.0 ** -24 * d["ds_abs"], "small gradient, reference")


@pytest.mark.parametrize("dt", [F, H], ids=["f32", "f16"])
def test_mul_plane_too_large_keeps_the_generic_route(backend, dt):
    """(1, 1, 256, 257): a plane of 65 792 elements is refused; the command runs as before."""
    L = backend
    d = mul_data("NCHW", (1, 1, 256, 257), dt)
    s0, n0 = counts(L)
    (c, (dx, ds)), names = records(L, lambda: (mul_forward(L, d, "NCHW", False), mul_backward(L, d, "NCHW", False)))
    s1, n1 = counts(L)
    assert not any("mul_planes" in x for x in names), names
    assert n1 == n0 and s1 == (s0 + 8 if dt == H else s0)
    within(c, d["c"], map_bound(d["c"], dt), "forward")
    within(dx, d["dx"], map_bound(d["dx"], dt), "large gradient")
    within(ds, d["ds"], sum_bound(d, dt), "small gradient")


def test_mul_refused_half_commands_are_staged_as_before(backend):
    """NHWC with C = 12 (no whole 8-channel vectors), an output that is a view, ACCUMULATE_OUTPUT: fp32 images as before, right results.  (The fp32
    images of the C = 12 command are themselves the pattern -- three 4-channel vectors -- so the fp32 command underneath may take the plane-scale
    kernels; a view or an accumulation is refused in either type.)"""
    L = backend
    # C = 12
    d = mul_data("NHWC", (2, 3, 3, 12), H)
    s0, n0 = counts(L)
    c, (dx, ds) = mul_forward(L, d, "NHWC", False), mul_backward(L, d, "NHWC", False)
    assert counts(L) == (s0 + 8, n0)
    within(c, d["c"], map_bound(d["c"], H), "C = 12 forward")
    within(dx, d["dx"], map_bound(d["dx"], H), "C = 12 large gradient")
    within(ds, d["ds"], sum_bound(d, H), "C = 12 small gradient")
    # the output a (2, 3, 7, 7) window of a (2, 3, 7, 9) buffer
    d = mul_data("NCHW", (2, 3, 7, 7), H)
    base = np.full((2, 3, 7, 9), 5, H)
    xt, st, ct = make_tensors(L, nnc.GPU_MEMORY, [d["x"], d["s"], base], "NCHW")
    view = ct.view((2, 3, 7, 7), (189, 63, 9, 1), 1)
    s0, n0 = counts(L)
    r, names = records(L, lambda: L.cmd_exec(nnc.CMD_MUL_FORWARD(P_MUL), nnc.NO_HINT, 0, [xt, st], [view]))
    assert r == 0 and counts(L) == (s0 + 3, n0) and not any("mul_planes" in x for x in names), names
    out = ct.numpy()
    within(out[..., 1:8], d["c"], map_bound(d["c"], H), "view")
    assert (out[..., 0] == 5).all() and (out[..., 8] == 5).all()
    # ACCUMULATE_OUTPUT
    with key_off(L, MUL_KEY):
        want = mul_forward(L, d, "NCHW", False, nnc.ACCUMULATE_OUTPUT)
    s0, n0 = counts(L)
    got, names = records(L, lambda: mul_forward(L, d, "NCHW", False, nnc.ACCUMULATE_OUTPUT))
    assert counts(L) == (s0 + 3, n0) and not any("mul_planes" in x for x in names), names
    assert np.array_equal(bits(got), bits(want))


def test_tuning_keys_are_listed(backend):
    assert backend.tune_get(ACT_KEY) == 1 and backend.tune_get(MUL_KEY) == 1
