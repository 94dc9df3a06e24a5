"""RMSPROP, ADAM, ADAMW and LAMB on CCV_16F tensors without fp32 images (ccv_amd/csrc/optim.h; tunable OPT_HALF_NATIVE): every tensor half ("hh"),
half gradients into fp32 parameters and state ("hf"), fp32 gradients into half parameters and state ("fh").

Every result is stated in float64 numpy on the inputs as the command sees them (the half ones rounded to half).  Bounds are derived, not tuned:
  half output   |got - want| <= 2^-11 |want| + 2^-24 + 2^-19 S
  fp32 output   |got - want| <= 2^-19 S
      S = the output's expression with every term replaced by its magnitude (cancellation does not shrink it); 2^-11 |want| is the one rounding to
      half, 2^-24 the half subnormal floor, 2^-19 S thirty-two fp32 ulps for the dozen fp32 roundings of the expression and the bias corrections
      1 / (1 - beta^step), which the host computes in fp32 (1 - 0.98^3 loses four bits to cancellation).
The reference's CPU backend runs the same command on the widened inputs and must meet the fp32 form.
Against the route with the tuning key at 0 (fp32 images, the fp32 instance of the same kernels) every output carries the same bits: the expression is
shared, division and square root are correctly rounded on both routes, and each stored value is rounded to fp32 before the store narrows it.
"""
import ctypes
import os
import re
import numpy as np
import pytest
from ccv_amd import nnc
from harness import make_tensors
from test_mbconv_half import aliased, bits, counts, half_bound, key_off, records, ref_run, within

F, H, D = np.float32, np.float16, np.float64
KEY = "OPT_HALF_NATIVE"
_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccv_amd", "csrc", "optim.h")
with open(_HDR) as _f:
    TILE = int(re.search(r"constexpr int OPT_TILE = (\d+);", _f.read()).group(1))  # elements of one workgroup's tile
SIZES = [1, 5, 8, 3240, 3243, TILE + 3, 2 * TILE + 11]
OPTS = ["RMSPROP", "ADAM", "ADAM_AMS", "ADAMW", "ADAMW_AMS", "LAMB"]
COMBOS = {"hh": (H, H), "hf": (H, F), "fh": (F, H)}  # (type of g, type of the parameter and state tensors)

f = lambda x: D(F(x))  # a command parameter as the kernel sees it
STEP, RATE, B1, B2, DECAY, EPS, SCALE = 3, 0.002, 0.9, 0.98, 0.01, 1e-6, 0.5
R_RATE, R_DECAY, R_ALPHA, R_MOM, R_EPS = 0.001, 0.0005, 0.9, 0.9, 1e-4


def command(opt, decay=DECAY):
    if opt == "RMSPROP":
        return nnc.CMD_RMSPROP_FORWARD(R_RATE, R_DECAY, R_ALPHA, R_MOM, R_EPS, scale=SCALE)
    cmd = nnc.CMD_ADAM_FORWARD(STEP, RATE, B1, B2, decay, EPS, amsgrad=int(opt.endswith("AMS")), scale=SCALE, decoupled=opt.startswith("ADAMW"))
    if opt == "LAMB":
        cmd.cmd = nnc.CMD["LAMB_FORWARD"]  # lamb's parameters are adam's without amsgrad
    return cmd


def arity(opt):
    return (5, 4) if opt.endswith("AMS") else (4, 3)


_RAW = {}


def raw(n):
    """g, a, m, v, vm in fp32 as tests/test_parity_act_opt.py draws them: magnitudes around 1, velocities 0.01 U(0, 1)"""
    if n not in _RAW:
        rng = np.random.default_rng(500 + n)
        sym = lambda s: ((rng.random(n, dtype=F) - 0.5) * 2 * s).astype(F)
        _RAW[n] = (sym(1.0), sym(1.0), sym(0.1), rng.random(n, dtype=F) * F(0.01), rng.random(n, dtype=F) * F(0.02))
    return _RAW[n]


def inputs(opt, combo, n, zero=None):
    tg, tp = COMBOS[combo]
    g, a, m, v, vm = raw(n)
    xs = [g.astype(tg), a.astype(tp), m.astype(tp), v.astype(tp), vm.astype(tp)][:arity(opt)[0]]
    if zero == "a":
        xs[1] = np.zeros(n, tp)
    if zero == "g":  # no gradient and no momentum: with decay 0 the update is zero everywhere
        xs[0], xs[2] = np.zeros(n, tg), np.zeros(n, tp)
    for x in xs:
        x.setflags(write=False)
    return xs


def expect(opt, xs, decay=DECAY):
    """[(want, S)] per output (b, n, u[, um]) in float64"""
    g, a, m, v = (x.astype(D) for x in xs[:4])
    ab = np.abs
    if opt == "RMSPROP":
        grad, sg = f(SCALE) * g + f(R_DECAY) * a, f(SCALE) * ab(g) + f(R_DECAY) * ab(a)
        vel, sv = f(R_ALPHA) * v + (1 - f(R_ALPHA)) * grad * grad, f(R_ALPHA) * ab(v) + (1 - f(R_ALPHA)) * sg * sg
        den = np.sqrt(vel) + f(R_EPS)
        mom, sm = f(R_MOM) * m + grad / den, f(R_MOM) * ab(m) + sg / den
        return [(a - f(R_RATE) * mom, ab(a) + f(R_RATE) * sm), (mom, sm), (vel, sv)]
    dec = f(decay)
    c1, c2 = 1 / (1 - f(B1) ** STEP), 1 / (1 - f(B2) ** STEP)
    decoupled = opt.startswith("ADAMW")
    grad, sg = f(SCALE) * g, f(SCALE) * ab(g)
    if opt.startswith("ADAM") and not decoupled:
        grad, sg = grad + dec * a, sg + dec * ab(a)
    mom, sm = f(B1) * m + (1 - f(B1)) * grad, f(B1) * ab(m) + (1 - f(B1)) * sg
    vel, sv = f(B2) * v + (1 - f(B2)) * grad * grad, f(B2) * ab(v) + (1 - f(B2)) * sg * sg
    if opt == "LAMB":
        den = np.sqrt(vel * c2) + f(EPS)
        upd, su = mom * c1 / den + a * dec, sm * c1 / den + ab(a) * dec
        wn, un = np.sqrt((a * a).sum()), np.sqrt((upd * upd).sum())
        trust = wn / un if wn > 0 and un > 0 else 1.0
        return [(a - f(RATE) * trust * upd, ab(a) + f(RATE) * trust * su), (mom, sm), (vel, sv)]
    outs = [None, (mom, sm), (vel, sv)]
    if opt.endswith("AMS"):
        vm = xs[4].astype(D)
        vmh = np.maximum(vm, vel * c2)
        outs.append((vmh, np.maximum(ab(vm), sv * c2)))
        den = np.sqrt(vmh) + f(EPS)
    else:
        den = np.sqrt(vel * c2) + f(EPS)
    base, sb = (a - f(RATE) * dec * a, ab(a) + f(RATE) * dec * ab(a)) if decoupled else (a, ab(a))
    outs[0] = (base - mom * f(RATE) * c1 / den, sb + sm * f(RATE) * c1 / den)
    return outs


def execute(L, opt, xs, mode="plain", flags=0, decay=DECAY):
    """-> the outputs (b, n, u[, um]) of the command on fresh tensors.  "inplace": b = a, n = m, u = v, um = vm, as the host issues the command;
    "unaligned": every tensor a dense alias that starts one element past a 16-byte boundary."""
    nin, nout = arity(opt)
    tp = xs[1].dtype
    n = xs[0].size
    if mode == "unaligned":
        ins = aliased(L, xs, 1)
        outs = aliased(L, [np.full(n, 3, tp) for _ in range(nout)], 1)
        assert all(t.ptr % 16 == t.np_dtype.itemsize for t in ins + outs)
    else:
        ins = make_tensors(L, nnc.GPU_MEMORY, xs)
        outs = ins[1:] if mode == "inplace" else make_tensors(L, nnc.GPU_MEMORY, [np.full(n, 3, tp) for _ in range(nout)])
    r = L.cmd_exec(command(opt, decay), nnc.NO_HINT, flags, ins, outs)
    assert r == 0, "backend returned %d" % r
    return [t.numpy() for t in outs]


def check(opt, got, want, what):
    for k, (x, (w, s)) in enumerate(zip(got, want)):
        bound = half_bound(w, s) if x.dtype == H else 2.0 ** -19 * s
        within(x, w, bound, "%s %s output %d" % (opt, what, k))


def same_bits(xs, ys, what):
    for k, (x, y) in enumerate(zip(xs, ys)):
        assert x.dtype == y.dtype and np.array_equal(bits(x), bits(y)), "%s: output %d differs in %d elements" % (what, k, int((bits(x) != bits(y)).sum()))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("opt", OPTS)
def test_optimizer_half(backend, ref_lib, opt, combo, n):
    """1, 5: the scalar loop alone; 8: one vector; 3240: whole vectors; 3243: a tail of three; one tile + 3 and two tiles + 11: more than one workgroup."""
    xs = inputs(opt, combo, n)
    want = expect(opt, xs)
    got = execute(backend, opt, xs)
    assert all(x.dtype == COMBOS[combo][1] for x in got)
    check(opt, got, want, combo)
    ref = ref_run(ref_lib, command(opt), xs, [np.zeros(n, F) for _ in range(arity(opt)[1])])
    for k, (x, (w, s)) in enumerate(zip(ref, want)):
        within(x, w, 2.0 ** -19 * s, "%s reference output %d" % (opt, k))


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("opt", OPTS)
def test_unaligned_bases_take_the_scalar_route(backend, opt, combo):
    n = 3243
    xs = inputs(opt, combo, n)
    got = execute(backend, opt, xs, "unaligned")
    check(opt, got, expect(opt, xs), combo + " unaligned")
    if opt != "LAMB":  # (LAMB's norms are summed in another order on the scalar route: b may differ in the last bit)
        same_bits(got, execute(backend, opt, xs), opt + " unaligned against aligned")


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("opt", OPTS)
def test_in_place_gives_the_same_bits(backend, opt, combo):
    n = 2 * TILE + 11
    xs = inputs(opt, combo, n)
    same_bits(execute(backend, opt, xs, "inplace"), execute(backend, opt, xs), "%s %s in place" % (opt, combo))


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("opt", OPTS)
def test_same_bits_as_the_fp32_image_route(backend, opt, combo):
    L = backend
    n = 2 * TILE + 11
    xs = inputs(opt, combo, n)
    native, native_in_place = execute(L, opt, xs), execute(L, opt, xs, "inplace")
    with key_off(L, KEY):
        staged, staged_in_place = execute(L, opt, xs), execute(L, opt, xs, "inplace")
    same_bits(native, staged, "%s %s against fp32 images" % (opt, combo))
    same_bits(native_in_place, staged_in_place, "%s %s in place against fp32 images" % (opt, combo))


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("opt", OPTS)
def test_routes(backend, opt, combo):
    """No half tensor gets an fp32 image, the half ones are counted native, the launch records hold the typed kernel and nothing else; with the key at 0
    every half tensor is staged again and the fp32 instance runs."""
    L = backend
    n = 3243
    xs = inputs(opt, combo, n)
    nin, nout = arity(opt)
    halves = {"hh": nin + nout, "hf": 1, "fh": nin - 1 + nout}[combo]
    name = "optim_" + opt.replace("_AMS", "").lower()
    s0, n0 = counts(L)
    _, names = records(L, lambda: execute(L, opt, xs))
    assert counts(L) == (s0, n0 + halves)
    assert any(x.startswith("%s_%s|" % (name, combo)) for x in names), names
    assert all(x.startswith("optim_") for x in names) and not any("half_up" in x or "half_down" in x for x in names), names
    with key_off(L, KEY):
        s0, n0 = counts(L)
        _, names = records(L, lambda: execute(L, opt, xs))
        assert counts(L) == (s0 + halves, n0)
        assert any(x.startswith(name + "_ff|") for x in names) and not any(x.startswith("%s_%s|" % (name, combo)) for x in names), names


@pytest.mark.parametrize("combo", list(COMBOS))
def test_lamb_edges(backend, combo):
    """Five tiles + 77 elements: several workgroups' partial pairs; all-zero parameters (|w| = 0) and a zero update (no gradient, no momentum, no decay:
    |update| = 0) take trust = 1; two runs carry the same bits."""
    L = backend
    n = 5 * TILE + 77
    xs = inputs("LAMB", combo, n)
    got = execute(L, "LAMB", xs)
    check("LAMB", got, expect("LAMB", xs), combo + " five tiles")
    same_bits(got, execute(L, "LAMB", xs), "LAMB twice")
    with key_off(L, KEY):
        same_bits(got, execute(L, "LAMB", xs), "LAMB against fp32 images")
    zs = inputs("LAMB", combo, 3243, zero="a")
    got = execute(L, "LAMB", zs)
    want = expect("LAMB", zs)
    check("LAMB", got, want, combo + " zero parameters")
    upd = -want[0][0] / f(RATE)  # trust = 1: b = -rate update
    assert np.abs(upd).max() > 0
    zs = inputs("LAMB", combo, 3243, zero="g")
    got = execute(L, "LAMB", zs, decay=0.0)
    check("LAMB", got, expect("LAMB", zs, decay=0.0), combo + " zero update")
    assert np.array_equal(bits(got[0]), bits(zs[1])) and not got[1].any()


def test_refusals_keep_their_route(backend):
    """A view, CCV_NNC_ACCUMULATE_OUTPUT, state tensors of two types: fp32 images as before, and what the command returned before."""
    L = backend
    n = 3240
    xs = inputs("RMSPROP", "hh", n)
    want = expect("RMSPROP", xs)
    plain = execute(L, "RMSPROP", xs)
    cmd = command("RMSPROP")
    # a dense view: staged, the same result
    ts = make_tensors(L, nnc.GPU_MEMORY, list(xs) + [np.full(n, 3, H) for _ in range(3)])
    ts[1] = ts[1].view((n,), (1,), 0)
    s0, n0 = counts(L)
    r, names = records(L, lambda: L.cmd_exec(cmd, nnc.NO_HINT, 0, ts[:4], ts[4:]))
    assert r == 0 and counts(L) == (s0 + 7, n0) and any(x.startswith("optim_rmsprop_ff|") for x in names), names
    same_bits([t.numpy() for t in ts[4:]], plain, "a dense view")
    # a strided view is refused by the fp32 kernel underneath, as it was
    base = make_tensors(L, nnc.GPU_MEMORY, [np.ones((4, 8), H)])[0]
    small = make_tensors(L, nnc.GPU_MEMORY, [np.ones((4, 6), H) for _ in range(6)])
    s0, n0 = counts(L)
    r = L.cmd_exec(cmd, nnc.NO_HINT, 0, [small[0], base.view((4, 6), (8, 1), 1), small[1], small[2]], small[3:])
    assert r == -1 and counts(L) == (s0 + 7, n0)
    # ACCUMULATE_OUTPUT
    s0, n0 = counts(L)
    got = execute(L, "RMSPROP", xs, flags=nnc.ACCUMULATE_OUTPUT)
    assert counts(L) == (s0 + 7, n0)
    with key_off(L, KEY):
        same_bits(got, execute(L, "RMSPROP", xs, flags=nnc.ACCUMULATE_OUTPUT), "ACCUMULATE_OUTPUT")
    # g, a, v, b, u half; m, n fp32
    g, a, m, v = xs
    ts = make_tensors(L, nnc.GPU_MEMORY, [g, a, m.astype(F), v, np.full(n, 3, H), np.full(n, 3, F), np.full(n, 3, H)])
    s0, n0 = counts(L)
    r, names = records(L, lambda: L.cmd_exec(cmd, nnc.NO_HINT, 0, ts[:4], ts[4:]))
    assert r == 0 and counts(L) == (s0 + 5, n0) and any(x.startswith("optim_rmsprop_ff|") for x in names), names
    check("RMSPROP", [t.numpy() for t in ts[4:]], want, "state tensors of two types")
    L.stream_wait(None)


def test_tuning_key_is_listed(backend):
    assert backend.tune_get(KEY) == 1
