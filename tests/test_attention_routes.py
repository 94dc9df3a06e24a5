"""Which kernel family every SCALED_DOT_PRODUCT_ATTENTION command reaches (ccv_amd/csrc/cmd_attention.cpp: sdpa_route_half / sdpa_route_fp32), row by row: the
names that must and must not appear in the profile records, whether half tensors went through fp32 images, and the results against float64 -- the forward within
3e-3 / 2e-3 (tests/test_attention_heads.py), the half gradients within 5e-3 of the tensor's largest value (tests/test_attention.py) and, where the any-head-size
kernels computed them, within the per-element bound of tests/test_attention_heads_back.py, the fp32 gradients within 1e-4 of the tensor's largest value.  The rows are the places where two route decisions meet: the backward's own kernels against the kernel of its
forward re-run, the decode kernel's row and key thresholds, the any-head-size key at 0 / 1 / 2, absent gradients, rows that are not whole 16-byte chunks."""
import numpy as np
import pytest
from ccv_amd import nnc
from harness import exec_on
from test_attention import close, sdpa_cmd
from test_attention_heads import attention64, tensors
from test_attention_heads_back import check, gradients64
from test_mbconv_half import counts, records

F, H, D64 = np.float32, np.float16, np.float64
FWD, BWD = "SCALED_DOT_PRODUCT_ATTENTION_FORWARD", "SCALED_DOT_PRODUCT_ATTENTION_BACKWARD"
SMALL = dict(B=1, R=33, C=40, Hq=2, Hk=1)
DECODE = dict(B=1, R=2, C=256, Hq=4, Hk=2)  # 4 packed rows a key head, the default key threshold of SDPA_F16_DECODE
ANYD_BWD = ("sdpa_bwd_anyd_dq_f16_kernel", "sdpa_bwd_anyd_dkv_f16_kernel")


def with_keys(lib, keys, fn):
    before = {name: lib.tune_get(name) for name in keys}
    try:
        for name, value in keys.items():
            lib.tune_set(name, value)
        return fn()
    finally:
        for name, value in before.items():
            lib.tune_set(name, value)


def expect(names, must, must_not):
    for m, times in must.items():
        assert sum(m in n for n in names) == times, (m, times, names)
    for m in must_not:
        assert not any(m in n for n in names), (m, names)


FORWARD_ROWS = [
    # id, D, Dv, shape, keys, {name: records}, absent, fp32 images
    ("f16", 48, 64, SMALL, {}, {"sdpa_forw_f16_kernel": 1}, ("sdpa_fwd_anyd", "sdpa_decode"), False),
    ("anyd", 8, 32, SMALL, {}, {"sdpa_fwd_anyd_f16_kernel": 1}, ("sdpa_forw_f16", "sdpa_decode"), False),
    ("anyd-key-0", 8, 32, SMALL, {"SDPA_F16_ANYD": 0}, {"sdpa_forw_mfma_kernel": 1}, ("_f16_kernel",), True),
    ("decode", 64, 64, DECODE, {}, {"sdpa_decode_f16_kernel": 1}, ("sdpa_forw_f16", "sdpa_fwd_anyd"), False),
    ("decode-255-keys", 64, 64, dict(DECODE, C=255), {}, {"sdpa_forw_f16_kernel": 1}, ("sdpa_decode", "sdpa_fwd_anyd"), False),
    ("decode-34-rows", 64, 64, dict(DECODE, R=17), {}, {"sdpa_forw_f16_kernel": 1}, ("sdpa_decode", "sdpa_fwd_anyd"), False),
]


@pytest.mark.parametrize("row", FORWARD_ROWS, ids=[r[0] for r in FORWARD_ROWS])
def test_forward_route(backend, row):
    _, Dq, Dv, s, keys, must, must_not, images = row
    B, R, C, Hq, Hk = s["B"], s["R"], s["C"], s["Hq"], s["Hk"]
    q, k, v, _ = tensors(np.random.default_rng(61), B, R, C, Hq, Hk, Dq, Dv, None)
    cmd = sdpa_cmd(FWD, float(1.0 / np.sqrt(Dq)), True)
    staged = counts(backend)[0]
    (r, got), names = with_keys(backend, keys, lambda: records(backend, lambda: exec_on(backend, nnc.GPU_MEMORY, cmd, nnc.NO_HINT, 0, [q, k, v], [np.full((B, R, Hq, Dv), 3, H), np.zeros((B, Hq, R), F)])))
    assert r == 0
    expect(names, must, must_not)
    assert (counts(backend)[0] > staged) == images
    want, lse, seen = attention64(q, k, v, None, True)
    assert seen.all()
    np.testing.assert_allclose(got[0].astype(D64), want, rtol=0, atol=3e-3)
    np.testing.assert_allclose(got[1], lse, rtol=2e-3, atol=2e-3)


def test_forward_rows_that_are_not_whole_chunks_go_through_fp32_images(backend):
    """q is a view into a wider tensor: its row stride, 2 * 48 + 4 halves, is no multiple of 8"""
    B, R, C, Hq, Hk, Dq, Dv = 1, 33, 40, 2, 1, 48, 64
    q, k, v, _ = tensors(np.random.default_rng(62), B, R, C, Hq, Hk, Dq, Dv, None)
    pitch = Hq * Dq + 4
    wide = np.zeros((B, R, pitch), H)
    wide[:, :, :Hq * Dq] = q.reshape(B, R, Hq * Dq)
    par = lambda a: nnc.tensor_param(nnc.GPU_MEMORY, nnc.NHWC, nnc._NP_DT[np.dtype(a.dtype)], a.shape, 0)
    wt, kt, vt = [backend.tensor(par(a), a) for a in (wide, k, v)]
    ot = backend.tensor(par(np.zeros((B, R, Hq, Dv), H)), np.full((B, R, Hq, Dv), 3, H))
    cmd = sdpa_cmd(FWD, float(1.0 / np.sqrt(Dq)), False)
    staged = counts(backend)[0]
    r, names = records(backend, lambda: backend.cmd_exec(cmd, nnc.NO_HINT, 0, [wt.view((B, R, Hq, Dq), (R * pitch, pitch, Dq, 1), 0), kt, vt], [ot]))
    assert r == 0
    expect(names, {}, ("_f16_kernel",))
    assert counts(backend)[0] > staged
    np.testing.assert_allclose(ot.numpy().astype(D64), attention64(q, k, v, None, False)[0], rtol=0, atol=3e-3)


HALF_BACKWARD_ROWS = [
    # id, D, Dv, shape, keys, {name: records}, absent, fp32 images
    ("anyd-behind-f16-forward", 48, 64, SMALL, {}, {ANYD_BWD[0]: 1, ANYD_BWD[1]: 1, "sdpa_forw_f16_kernel": 1}, ("sdpa_fwd_anyd_f16_kernel", "sdpa_dq_f16_kernel", "sdpa_dkv_f16_kernel"), False),
    ("anyd-key-2", 48, 64, SMALL, {"SDPA_F16_ANYD": 2}, {ANYD_BWD[0]: 1, ANYD_BWD[1]: 1, "sdpa_fwd_anyd_f16_kernel": 1}, ("sdpa_forw_f16_kernel", "sdpa_dq_f16_kernel", "sdpa_dkv_f16_kernel"), False),
    ("anyd-key-0", 48, 64, SMALL, {"SDPA_F16_ANYD": 0}, {"sdpa_forw_mfma_kernel": 1}, ("sdpa_dq_mfma_kernel", "sdpa_dkv_mfma_kernel", "_f16_kernel"), True),
    ("decode-shape", 64, 64, DECODE, {}, {"sdpa_forw_f16_kernel": 1, "sdpa_dq_f16_kernel": 1, "sdpa_dkv_f16_kernel": 1}, ("sdpa_decode", "anyd"), False),
]


@pytest.mark.parametrize("row", HALF_BACKWARD_ROWS, ids=[r[0] for r in HALF_BACKWARD_ROWS])
def test_half_backward_route(backend, row):
    _, Dq, Dv, s, keys, must, must_not, images = row
    B, R, C, Hq, Hk = s["B"], s["R"], s["C"], s["Hq"], s["Hk"]
    rng = np.random.default_rng(63)
    q, k, v, _ = tensors(rng, B, R, C, Hq, Hk, Dq, Dv, None)
    g = (rng.random((B, R, Hq, Dv), dtype=F) - F(0.5)).astype(H)
    scale = float(1.0 / np.sqrt(Dq))
    cmd = sdpa_cmd(BWD, scale, True)
    staged = counts(backend)[0]
    (r, got), names = with_keys(backend, keys, lambda: records(backend, lambda: exec_on(backend, nnc.GPU_MEMORY, cmd, nnc.NO_HINT, 0, [g, None, None, q, k, v], [np.full(a.shape, 3, H) for a in (q, k, v)])))
    assert r == 0
    expect(names, must, must_not)
    assert (counts(backend)[0] > staged) == images
    if ANYD_BWD[0] in must:  # (the per-element bound is derived from the rounding points of these kernels)
        check((B, R, C, Hq, Hk, Dq, Dv, True, None), got, g, q, k, v, None, scale)
    for a, w in zip(got, gradients64(g, q, k, v, None, True, scale)[0]):
        close(a.astype(F), w, tol=5e-3)


FP32_BACKWARD_ROWS = [
    # id, D, Dv, gradients asked for, {name: records}, absent
    ("dq-alone-on-the-matrix-cores", 32, 40, (True, True, True), {"sdpa_dq_mfma_kernel": 1}, ("sdpa_dkv_mfma_kernel", "sdpa_forw_mfma_kernel")),
    ("one-gradient-per-pass", 96, 96, (True, True, True), {"sdpa_forw_mfma_kernel": 1, "sdpa_dq_mfma_kernel": 1, "sdpa_dkv_mfma_kernel": 1}, ()),  # (both passes in one record)
    ("dk-alone", 96, 96, (False, True, False), {"sdpa_forw_mfma_kernel": 1, "sdpa_dkv_mfma_kernel": 1}, ("sdpa_dq_mfma_kernel",)),
]


@pytest.mark.parametrize("row", FP32_BACKWARD_ROWS, ids=[r[0] for r in FP32_BACKWARD_ROWS])
def test_fp32_backward_route(backend, row):
    _, Dq, Dv, ask, must, must_not = row
    B, R, C, Hq, Hk = SMALL["B"], SMALL["R"], SMALL["C"], SMALL["Hq"], SMALL["Hk"]
    rng = np.random.default_rng(64)
    g, q, k, v = [rng.random(s, dtype=F) - F(0.5) for s in ((B, R, Hq, Dv), (B, R, Hq, Dq), (B, C, Hk, Dq), (B, C, Hk, Dv))]
    scale = float(1.0 / np.sqrt(Dq))
    cmd = sdpa_cmd(BWD, scale, True)
    staged = counts(backend)[0]
    (r, got), names = records(backend, lambda: exec_on(backend, nnc.GPU_MEMORY, cmd, nnc.NO_HINT, 0, [g, None, None, q, k, v], [np.full(a.shape, 3, F) if want else None for a, want in zip((q, k, v), ask)]))
    assert r == 0
    expect(names, must, must_not)
    assert counts(backend)[0] == staged
    want, _ = gradients64(g, q, k, v, None, True, scale)
    for a, w, asked in zip(got, want, ask):
        assert (a is not None) == asked
        if asked:
            close(a, w)
