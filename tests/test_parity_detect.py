"""Parity of the detection / signal rows (ccv_amd/csrc/cmd_detect.cpp): NMS, CMUL, ROI_ALIGN and the LSSC compression, against the
reference's CPU backend and a numpy statement of each operation.

NMS and LSSC are moves and selections: bit-exact.  CMUL and ROI_ALIGN are sums: |got - f64| <= T eps32 S with T the largest number
of terms that meets in one output and S the same float64 expression on absolute values -- the worst case of any summation order, which
is what the atomics of ROI_ALIGN backward need.
"""
import numpy as np
import pytest
from ccv_amd import nnc
from harness import exec_on

F, D, H = np.float32, np.float64, np.float16
EPS = float(np.finfo(F).eps)
FLT_MAX = np.finfo(F).max


def gpu(L, cmd, ins, outs, fmt="NHWC"):
    r, res = exec_on(L, nnc.GPU_MEMORY, cmd, nnc.NO_HINT, 0, ins, outs, fmt)
    assert r == 0, "backend returned %d" % r
    return res


def cpu(ref, cmd, ins, outs, fmt="NHWC"):
    r, res = exec_on(ref, nnc.CPU_MEMORY, cmd, nnc.NO_HINT, 0, ins, outs, fmt, backend=nnc.BACKEND_CPU_REF)
    assert r == 0, "reference returned %d" % r
    return res


def within(x, f64, bound, what=""):
    err = np.abs(np.asarray(x, D) - f64)
    bad = ~(err <= bound)
    assert not bad.any(), "%s: %d elements off, worst error %.3e" % (what, int(bad.sum()), float(err[bad].max()))


def same_f32(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))


# ---- NMS --------------------------------------------------------------------------------------------------------------------------
def nms_numpy(a, thr):
    """One image (m, d): rows by descending score, a greedy sweep in float32 (the reference's expression order), survivors' first five columns
    moved to the front, -FLT_MAX in the score column behind them; c = the original index of each surviving row, then -1."""
    m, d = a.shape
    order = np.argsort(-a[:, 0], kind="stable")
    b = a[order].copy()
    c = order.astype(np.int32)
    thr = F(thr)
    for x in range(m):
        if b[x, 0] == -FLT_MAX:
            continue
        y = np.arange(x + 1, m)
        y = y[b[y, 0] != -FLT_MAX]
        if not len(y):
            continue
        x1, y1, w1, h1 = b[x, 1], b[x, 2], b[x, 3], b[x, 4]
        x2, y2, w2, h2 = b[y, 1], b[y, 2], b[y, 3], b[y, 4]
        xd = np.maximum(F(0), np.minimum(x1 + w1, x2 + w2) - np.maximum(x1, x2))
        yd = np.maximum(F(0), np.minimum(y1 + h1, y2 + h2) - np.maximum(y1, y2))
        inter = xd * yd
        with np.errstate(invalid="ignore", divide="ignore"):
            iou = inter / (w1 * h1 + w2 * h2 - inter)
        b[y[iou >= thr], 0] = -FLT_MAX
    keep = np.nonzero(b[:, 0] != -FLT_MAX)[0]
    for dst, src in enumerate(keep):
        if dst != src:
            b[dst, :5] = b[src, :5]
            c[dst] = c[src]
    b[len(keep):, 0] = -FLT_MAX
    c[len(keep):] = -1
    return b, c, len(keep)


def nms_boxes(n, m, d, seed):
    """Distinct scores (a shuffled linspace); boxes dense enough that some are suppressed at either threshold, plus -- for m > 2 -- one exact
    duplicate (always suppressed) and one far-away box (always survives) in every image."""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, m, d), F)
    side = max(1.0, 0.6 * np.sqrt(m))
    for i in range(n):
        a[i, :, 0] = rng.permutation(np.linspace(0.05, 0.95, m)).astype(F)
        a[i, :, 1:3] = rng.uniform(0, side, (m, 2))
        a[i, :, 3:5] = rng.uniform(0.6, 1.2, (m, 2))
        a[i, :, 5:] = rng.uniform(-1, 1, (m, d - 5))
        if m > 2:
            a[i, 1, 1:5] = a[i, 0, 1:5]
            a[i, 2, 1:3] = 1000.0
    return a


@pytest.mark.parametrize("d", [5, 6, 7])
@pytest.mark.parametrize("m", [1, 2, 255, 256, 257, 700])
def test_nms_forward(backend, ref_lib, m, d):
    """(m, d) and (n, m, d) with n = 1, 3 at thresholds 0.3 and 0.7.  b against the reference CPU backend, bit for bit and in full (the survivor
    prefix's five moved columns, the columns it leaves where the sort put them, the -FLT_MAX markers) and against the numpy statement.
    c against the numpy statement: the reference's selection-sort branch (d != 5, or a view) swaps its index column once per COLUMN of every row it
    moves (nms_cpu_ref.c:128-136), d times: an even d swaps it back, its c is wrong, and only for d = 5 and 7 is c also compared with it."""
    for n, thr in ((0, 0.3), (0, 0.7), (1, 0.7), (3, 0.3), (3, 0.7)):
        a = nms_boxes(max(n, 1), m, d, 100 * m + 10 * d + n)
        if n == 0:
            a = a[0]
        cshape = a.shape[:-1]
        cmd = nnc.CMD_NMS_FORWARD(thr)
        got = gpu(backend, cmd, [a], [np.full(a.shape, 9, F), np.full(cshape, 9, np.int32)])
        ref = cpu(ref_lib, cmd, [a], [np.full(a.shape, 9, F), np.full(cshape, 9, np.int32)])
        assert same_f32(got[0], ref[0]), "b differs from the reference (n %d, threshold %g)" % (n, thr)
        for i in range(max(n, 1)):
            img = a[i] if n else a
            wb, wc, survivors = nms_numpy(img, thr)
            if m > 2:
                assert 0 < survivors < m
            gb, gc = (got[0][i], got[1][i]) if n else (got[0], got[1])
            assert same_f32(gb, wb) and np.array_equal(gc, wc), "image %d of %d, threshold %g" % (i, n, thr)
        if d != 6:
            assert np.array_equal(got[1], ref[1])


def test_nms_forward_on_a_view(backend, ref_lib):
    """The input is a (300, 5) window of a (300, 9) tensor (row pitch 9 > d), the output rows a window of pitch 7; the columns around them stay."""
    L = backend
    m, d = 300, 5
    big = np.random.default_rng(5).uniform(-1, 1, (m, 9)).astype(F)
    a = nms_boxes(1, m, d, 77)[0]
    big[:, 2:7] = a
    obase = np.full((m, 7), 5, F)
    bt = L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_32F, big.shape, 0), big)
    ot = L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_32F, obase.shape, 0), obase)
    ct = L.tensor(nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc.CCV_32S, (m,), 0), np.full(m, 9, np.int32))
    assert L.cmd_exec(nnc.CMD_NMS_FORWARD(0.3), nnc.NO_HINT, 0, [bt.view((m, d), (9, 1), 2)], [ot.view((m, d), (7, 1), 1), ct]) == 0
    wb, wc, survivors = nms_numpy(a, 0.3)
    assert 0 < survivors < m
    out = ot.numpy()
    assert same_f32(out[:, 1:6], wb) and np.array_equal(ct.numpy(), wc)
    assert same_f32(out[:, [0, 6]], obase[:, [0, 6]])
    ref = cpu(ref_lib, nnc.CMD_NMS_FORWARD(0.3), [a], [np.zeros_like(a), np.zeros(m, np.int32)])
    assert same_f32(ref[0], wb) and np.array_equal(ref[1], wc)


@pytest.mark.parametrize("kind", ["all-survive", "one-suppressed", "half-suppressed", "one-survives"])
@pytest.mark.parametrize("n,m,d", [(0, 257, 5), (3, 40, 6)])
def test_nms_backward(backend, ref_lib, kind, n, m, d):
    """The forward's c routes the gradient rows back: b = 0, b[c[x]] = g[x]; the rows of suppressed boxes stay zero."""
    rng = np.random.default_rng(m)
    a = np.zeros((max(n, 1), m, d), F)
    for i in range(a.shape[0]):
        a[i, :, 0] = rng.permutation(np.linspace(0.05, 0.95, m)).astype(F)
        a[i, :, 1] = np.arange(m) * 10      # disjoint boxes ...
        a[i, :, 3:5] = 1
        if kind == "one-suppressed":
            a[i, 7, 1] = a[i, 3, 1]
        elif kind == "half-suppressed":
            a[i, 1::2, 1] = a[i, :m - 1:2, 1]   # ... paired up
        elif kind == "one-survives":
            a[i, :, 1] = 0
    if n == 0:
        a = a[0]
    cshape = a.shape[:-1]
    fwd = gpu(backend, nnc.CMD_NMS_FORWARD(0.5), [a], [np.zeros_like(a), np.zeros(cshape, np.int32)])
    c = fwd[1]
    want_survivors = {"all-survive": m, "one-suppressed": m - 1, "half-suppressed": (m + 1) // 2, "one-survives": 1}[kind]
    assert ((c >= 0).sum(axis=-1) == want_survivors).all()
    g = rng.uniform(-1, 1, a.shape).astype(F)
    ins = [g, None, None, None, c]
    got = gpu(backend, nnc.CMD_NMS_BACKWARD(0.5), ins, [np.full(a.shape, 9, F)])[0]
    ref = cpu(ref_lib, nnc.CMD_NMS_BACKWARD(0.5), ins, [np.full(a.shape, 9, F)])[0]
    want = np.zeros(a.shape, F)
    g3, c2, w3 = g.reshape(-1, m, d), c.reshape(-1, m), want.reshape(-1, m, d)
    for i in range(c2.shape[0]):
        alive = c2[i] >= 0
        w3[i, c2[i][alive]] = g3[i, alive]
    assert same_f32(got, want) and same_f32(ref, want)
    suppressed = np.ones(c2.shape, bool)
    for i in range(c2.shape[0]):
        suppressed[i, c2[i][c2[i] >= 0]] = False
    assert (got.reshape(-1, m, d)[suppressed] == 0).all()


# ---- CMUL -------------------------------------------------------------------------------------------------------------------------
def cx(x):
    x = x.astype(D)
    return x[..., 0::2] + 1j * x[..., 1::2]


def interleave(z):
    out = np.zeros(z.shape[:-1] + (2 * z.shape[-1],), D)
    out[..., 0::2], out[..., 1::2] = z.real, z.imag
    return out


def cabs_terms(x, y):
    """The same complex product on absolute values: re and im each collect |x0 y0| + |x1 y1| resp. |x0 y1| + |x1 y0|."""
    x, y = np.abs(x.astype(D)), np.abs(y.astype(D))
    x0, x1, y0, y1 = x[..., 0::2], x[..., 1::2], y[..., 0::2], y[..., 1::2]
    return interleave((x0 * y0 + x1 * y1) + 1j * (x0 * y1 + x1 * y0))


def reduce_to(x, shape):
    padded = (1,) * (x.ndim - len(shape)) + tuple(shape)
    axes = tuple(i for i in range(x.ndim) if padded[i] == 1 and x.shape[i] != 1)
    return (x.sum(axis=axes, keepdims=True) if axes else x).reshape(shape)


def rnd(shape, seed, dt=F):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(dt)


def cmul_bound(dt, T, S, f64):
    """T eps32 S for the fp32 kernel; halves are computed in fp32 and rounded once more on the way out (2^-11 relative)."""
    b = T * EPS * S
    return b if dt == F else b + 2.0 ** -11 * (np.abs(f64) + b)


CMUL_PAIRS = [((3, 4, 5, 6), (3, 4, 5, 6)), ((1, 4, 5, 6), (3, 4, 5, 6)), ((3, 1, 5, 6), (3, 4, 5, 6)), ((3, 4, 1, 6), (3, 4, 5, 6)),
              ((3, 4, 5, 6), (1, 1, 5, 6)), ((3, 4, 5, 6), (6,)), ((3, 1, 5, 6), (1, 4, 1, 6))]


@pytest.mark.parametrize("dt", [F, H], ids=["f32", "f16"])
@pytest.mark.parametrize("pair", CMUL_PAIRS, ids=lambda p: "%s*%s" % ("x".join(map(str, p[0])), "x".join(map(str, p[1]))))
def test_cmul_forward(backend, ref_lib, pair, dt):
    a, b = rnd(pair[0], 1, dt), rnd(pair[1], 2, dt)
    full = np.broadcast_shapes(*pair)
    want64 = np.broadcast_to(interleave(cx(a) * cx(b)), full)
    S = np.broadcast_to(cabs_terms(a, b), full)
    got = gpu(backend, nnc.CMD_CMUL_FORWARD(), [a, b], [np.full(full, 9, dt)])[0]
    assert got.dtype == dt
    within(got, want64, cmul_bound(dt, 2, S, want64), "kernel")
    if dt == F:
        ref = cpu(ref_lib, nnc.CMD_CMUL_FORWARD(), [a, b], [np.full(full, 9, dt)])[0]
        within(ref, want64, 2 * EPS * S, "reference")


@pytest.mark.parametrize("dt", [F, H], ids=["f32", "f16"])
@pytest.mark.parametrize("with_g", [True, False], ids=["g", "no-g"])
@pytest.mark.parametrize("pair", CMUL_PAIRS, ids=lambda p: "%s*%s" % ("x".join(map(str, p[0])), "x".join(map(str, p[1]))))
def test_cmul_backward(backend, ref_lib, pair, with_g, dt):
    """da = sum over a's broadcast axes of g conj(b), db likewise with a.  Without g: conj of the other operand when nothing is broadcast, and -- the
    contract is the reference's broadcasting branch (cmul_cpu_ref.c:372-420) -- the PLAIN sum of the other operand when something is.  The pairs
    reduce over no axis, one axis and two axes."""
    a, b = rnd(pair[0], 3, dt), rnd(pair[1], 4, dt)
    full = np.broadcast_shapes(*pair)
    plain = pair[0] == pair[1]
    g = rnd(full, 5, dt) if with_g else None
    res = [("kernel", gpu(backend, nnc.CMD_CMUL_BACKWARD(), [g, a, b], [np.full(a.shape, 9, dt), np.full(b.shape, 9, dt)]))]
    if dt == F:
        res.append(("reference", cpu(ref_lib, nnc.CMD_CMUL_BACKWARD(), [g, a, b], [np.full(a.shape, 9, dt), np.full(b.shape, 9, dt)])))
    for k, (own, other) in enumerate(((a, b), (b, a))):
        ob = np.broadcast_to(other, other.shape)
        if with_g:
            t = interleave(cx(g) * np.conj(np.broadcast_to(cx(ob), cx(g).shape)))
            s = cabs_terms(g, np.broadcast_to(ob, full))
            per = 2
        elif plain:
            t, s, per = interleave(np.conj(cx(ob))), np.abs(ob.astype(D)), 1
        else:
            t, s, per = np.broadcast_to(ob.astype(D), full), np.abs(np.broadcast_to(ob.astype(D), full)), 1
        want64, S = reduce_to(np.broadcast_to(t, full), own.shape), reduce_to(np.broadcast_to(s, full), own.shape)
        T = max(2, per * (int(np.prod(full)) // own.size))
        for who, r in res:
            within(r[k], want64, cmul_bound(dt if who == "kernel" else F, T, S, want64), "%s d%s" % (who, "ab"[k]))
    # one output at a time
    for what in (0, 1):
        outs = [np.full(a.shape, 9, dt) if what == 0 else None, np.full(b.shape, 9, dt) if what == 1 else None]
        one = gpu(backend, nnc.CMD_CMUL_BACKWARD(), [g, a, b], outs)
        if with_g or plain or pair[1 - what] == full:  # (without g the reference's "nothing is broadcast" test looks only at the outputs requested)
            assert np.array_equal(one[what], res[0][1][what])


# ---- ROI_ALIGN --------------------------------------------------------------------------------------------------------------------
def roi_weights(h, w, a_n, rois, c_n, pool_h, pool_w):
    """W[(n, y, x), (n % a_n, iy, ix)]: the weight of every map element in every output cell, and the number of (sample, tap) contributions behind
    it.  Sample coordinates and bilinear weights are part of the operation's definition and follow the reference's float32 expressions
    (roi_align_cpu_ref.c:20-47, 182-185); what the bound covers is the sum."""
    W = np.zeros((c_n, pool_h, pool_w, a_n, h, w), D)
    K = np.zeros(W.shape, np.int64)
    samples = np.zeros((c_n, pool_h, pool_w), np.int64)
    b_n = rois.shape[0]
    for n in range(c_n):
        r = rois[n % b_n]
        roi_x, roi_y, roi_w, roi_h = F(r[0] * F(w)), F(r[1] * F(h)), F(r[2] * F(w)), F(r[3] * F(h))
        bin_h, bin_w = int(np.ceil(F(roi_h / F(pool_h)))), int(np.ceil(F(roi_w / F(pool_w))))
        scale_y, scale_x = F(roi_h / F(bin_h * pool_h)), F(roi_w / F(bin_w * pool_w))
        for y in range(pool_h):
            ys = [F(D(roi_y) + (by + y * bin_h + 0.5) * D(scale_y) - 0.5) for by in range(bin_h)]
            ys = [(ay, int(np.floor(ay))) for ay in ys]
            ys = [(ay, iy) for ay, iy in ys if not (iy + 1 < 0 or iy > h - 1)]
            for x in range(pool_w):
                xs = [F(D(roi_x) + (bx + x * bin_w + 0.5) * D(scale_x) - 0.5) for bx in range(bin_w)]
                xs = [(ax, int(np.floor(ax))) for ax in xs]
                xs = [(ax, ix) for ax, ix in xs if not (ix + 1 < 0 or ix > w - 1)]
                count = len(ys) * len(xs)
                samples[n, y, x] = count
                for ay, iy in ys:
                    ry = F(ay - F(iy))
                    iy0, iy1 = min(max(iy, 0), h - 1), min(max(iy + 1, 0), h - 1)
                    for ax, ix in xs:
                        rx = F(ax - F(ix))
                        ix0, ix1 = min(max(ix, 0), w - 1), min(max(ix + 1, 0), w - 1)
                        for jy, jx, cw in ((iy0, ix0, F(F(1 - ry) * F(1 - rx))), (iy0, ix1, F(F(1 - ry) * rx)), (iy1, ix0, F(ry * F(1 - rx))), (iy1, ix1, F(ry * rx))):
                            W[n, y, x, n % a_n, jy, jx] += D(cw) / count
                            K[n, y, x, n % a_n, jy, jx] += 1
    return W, K, samples


ROIS = np.array([[0.10, 0.15, 0.55, 0.62],     # inside the map
                 [-0.20, 0.60, 0.70, 0.80],    # partly outside on the left and below: samples dropped from the average
                 [0.40, 0.30, 0.02, 0.03]], F)  # degenerate: narrower than a pool cell


@pytest.mark.parametrize("pool", [(1, 1), (2, 3), (7, 7)], ids=lambda p: "%dx%d" % p)
@pytest.mark.parametrize("ch", [1, 5])
@pytest.mark.parametrize("a_n,b_n", [(1, 1), (2, 1), (1, 3), (2, 3), (2, 6), (6, 3)])
def test_roi_align(backend, ref_lib, a_n, b_n, ch, pool):
    """The command's contract is c_n == max(a_n, b_n) (the reference asserts it), so the two modulo wraps are met with n % a_n at (2, 3) and
    (2, 6), n % b_n at (2, 1) and (6, 3); the last two have an output batch of 6.  NHWC against the reference and numpy, NCHW against numpy
    (the reference's CPU backend reads NHWC strides only).  T = samples per cell x 4 taps forward, the number of contributions that meet in one
    map element backward."""
    h, w = 9, 11
    c_n = max(a_n, b_n)
    rois = np.concatenate([ROIS, ROIS[::-1] * F(0.9)])[:b_n]
    a = rnd((a_n, h, w, ch), 7)
    g = rnd((c_n, pool[0], pool[1], ch), 8)
    W, K, samples = roi_weights(h, w, a_n, rois, c_n, *pool)
    if b_n >= 3:
        assert (samples == 0).any() or (samples < samples.max()).any()   # (the partly-outside region did drop samples)
    want64 = np.einsum("nyxaij,aijk->nyxk", W, a.astype(D))
    S = np.einsum("nyxaij,aijk->nyxk", W, np.abs(a.astype(D)))
    T = max(4, int(samples.max()) * 4)
    back64 = np.einsum("nyxaij,nyxk->aijk", W, g.astype(D))
    Sb = np.einsum("nyxaij,nyxk->aijk", W, np.abs(g.astype(D)))
    Tb = max(1, int(K.sum(axis=(0, 1, 2)).max()))
    fwd, bwd = nnc.CMD_ROI_ALIGN_FORWARD(*pool), nnc.CMD_ROI_ALIGN_BACKWARD(*pool)
    got = gpu(backend, fwd, [a, rois], [np.full(g.shape, 9, F)])[0]
    ref = cpu(ref_lib, fwd, [a, rois], [np.full(g.shape, 9, F)])[0]
    within(got, want64, T * EPS * S, "kernel forward")
    within(ref, want64, T * EPS * S, "reference forward")
    got = gpu(backend, bwd, [g, None, rois], [np.full(a.shape, 9, F)])[0]
    ref = cpu(ref_lib, bwd, [g, None, rois], [np.full(a.shape, 9, F)])[0]
    within(got, back64, Tb * EPS * Sb, "kernel backward")
    within(ref, back64, Tb * EPS * Sb, "reference backward")
    nchw = lambda t: np.ascontiguousarray(t.transpose(0, 3, 1, 2))
    got = gpu(backend, fwd, [nchw(a), rois], [np.full(nchw(g).shape, 9, F)], "NCHW")[0]
    within(got, nchw(want64), T * EPS * nchw(S), "kernel forward, NCHW")
    got = gpu(backend, bwd, [nchw(g), None, rois], [np.full(nchw(a).shape, 9, F)], "NCHW")[0]
    within(got, nchw(back64), Tb * EPS * nchw(Sb), "kernel backward, NCHW")


def test_roi_align_output_batch_must_be_the_larger_input_batch(backend):
    """a_n = 2, b_n = 3 into an output batch of 6: not max(a_n, b_n) -- CCV_NNC_EXEC_INVALID, nothing written."""
    a, g = rnd((2, 9, 11, 5), 7), np.full((6, 2, 3, 5), 9, F)
    r, res = exec_on(backend, nnc.GPU_MEMORY, nnc.CMD_ROI_ALIGN_FORWARD(2, 3), nnc.NO_HINT, 0, [a, ROIS], [g])
    assert r == nnc.EXEC_INVALID and np.array_equal(res[0], g)


# ---- LSSC -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("hw", [(4, 4), (5, 7), (8, 12), (1, 1)], ids=lambda p: "%dx%d" % p)
def test_lssc(backend, ref_lib, hw, ch):
    """4 x 4 blocks of halves -> (min, max, 2 x 16 bits of indices): the compressed words and the decompressed tensor bit-identical to the reference
    CPU backend.  Ragged blocks (5 x 7, 1 x 1), a constant block (min == max), a block holding the largest finite half, negative values.  The
    first two words of a block are the block's min and max (numpy), and a constant block comes back exactly."""
    h, w = hw
    n = 2
    rng = np.random.default_rng(h * 10 + w + ch)
    a = rng.uniform(-3, 3, (n, ch, h, w)).astype(H)
    a[0, 0, :4, :4] = H(1.375)                 # constant block
    a[1, ch - 1, 0, 0] = H(65504)             # largest finite half
    if h > 4:
        a[1, 0, 4:, :] = -np.abs(a[1, 0, 4:, :])  # an all-negative block row
    bh, bw = (h + 3) // 4, (w + 3) // 4
    bshape = (n, ch, bh, bw * 4)
    fwd, bwd = nnc.CMD_COMPRESSION_LSSC_FORWARD(), nnc.CMD_COMPRESSION_LSSC_BACKWARD()
    got = gpu(backend, fwd, [a], [np.zeros(bshape, H)], "NCHW")[0]
    ref = cpu(ref_lib, fwd, [a], [np.zeros(bshape, H)], "NCHW")[0]
    assert np.array_equal(got.view(np.uint16), ref.view(np.uint16))
    for by in range(bh):
        for bx in range(bw):
            blk = a[:, :, by * 4:by * 4 + 4, bx * 4:bx * 4 + 4].reshape(n, ch, -1)
            assert np.array_equal(got[:, :, by, bx * 4], blk.min(axis=-1)) and np.array_equal(got[:, :, by, bx * 4 + 1], blk.max(axis=-1))
    back = gpu(backend, bwd, [ref], [np.full(a.shape, 9, H)], "NCHW")[0]
    rback = cpu(ref_lib, bwd, [ref], [np.full(a.shape, 9, H)], "NCHW")[0]
    assert np.array_equal(back.view(np.uint16), rback.view(np.uint16))
    assert np.array_equal(back[0, 0, :4, :4], a[0, 0, :4, :4])
    assert back[1, ch - 1, 0, 0] == H(65504)
