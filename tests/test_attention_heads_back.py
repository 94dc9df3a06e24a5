"""SCALED_DOT_PRODUCT_ATTENTION_BACKWARD on CCV_16F tensors at the head sizes sdpa_dq_f16_kernel / sdpa_dkv_f16_kernel refuse (D, Dv in 8s up to 256:
sdpa_bwd_anyd_dq_f16_kernel / sdpa_bwd_anyd_dkv_f16_kernel, ccv_amd/csrc/sdpa_anyd_f16_back.h; tunable SDPA_F16_ANYD), against the closed-form float64 gradients of
the same half values (the formulas of tests/test_attention.py).  Two bounds, both asserted: close(tol=5e-3) of test_attention.py, and a per-element bound from the
kernels' rounding points -- u = 2^-11 (one rounding to half), t = 2^-25 (half the spacing of half subnormals):
    p_err = u p + t                                   p rounded to half in its registers
    ds_err = u |ds| + t + p u sum_d |g| |o|           ds rounded to half; delta comes from the half-rounded forward output
    dv_bound = sum_x p_err |g| + u |dv|               the stored gradient is rounded once more
    dq_bound = scale sum_y ds_err |k| + u |dq|,  dk_bound = scale sum_x ds_err |q| + u |dk|
|got - want| <= 2 bound element-wise; the factor 2 covers fp32 accumulation, exp2 and the fp32 log-sum-exp, each orders of magnitude below u."""
import numpy as np
import pytest
from ccv_amd import nnc
from harness import exec_on
from test_attention import close, sdpa_cmd
from test_attention_heads import tensors
from test_mbconv_half import counts, records

F, H, D64 = np.float32, np.float16, np.float64
NEW, OLD = ("sdpa_bwd_anyd_dq_f16_kernel", "sdpa_bwd_anyd_dkv_f16_kernel"), ("sdpa_dq_f16_kernel", "sdpa_dkv_f16_kernel")
U, T = 2.0 ** -11, 2.0 ** -25


def gradients64(g, q, k, v, mask, causal, scale):
    """float64 ((dq, dk, dv), their per-element bounds)"""
    B, R, Hq, _ = q.shape
    C, Hk, ratio = k.shape[1], k.shape[2], q.shape[2] // k.shape[2]
    q64, g64 = q.astype(D64), g.astype(D64)
    kr, vr = np.repeat(k, ratio, axis=2).astype(D64), np.repeat(v, ratio, axis=2).astype(D64)
    s = np.einsum("brhd,bchd->bhrc", q64, kr) * scale
    if mask is not None:
        s = s + mask.astype(D64)
    if causal:
        s = np.where(np.arange(C)[None, :] < np.arange(R)[:, None] - R + C + 1, s, -np.inf)
    seen = np.isfinite(s).any(-1)
    with np.errstate(invalid="ignore"):
        p = np.exp(s - np.where(seen, s.max(-1), 0.0)[..., None])
    p = np.where(np.isfinite(s), p, 0.0)
    p = p / np.where(seen, p.sum(-1), 1.0)[..., None]
    dp = np.einsum("brhd,bchd->bhrc", g64, vr)
    ds = p * (dp - (p * dp).sum(-1, keepdims=True))
    heads = lambda a: a.reshape(B, C, Hk, ratio, a.shape[-1]).sum(3)
    dq = scale * np.einsum("bhrc,bchd->brhd", ds, kr)
    dk = heads(scale * np.einsum("bhrc,brhd->bchd", ds, q64))
    dv = heads(np.einsum("bhrc,brhd->bchd", p, g64))
    go = np.einsum("brhd,brhd->bhr", np.abs(g64), np.abs(np.einsum("bhrc,bchd->brhd", p, vr)))
    p_err = U * p + T
    ds_err = U * np.abs(ds) + T + p * U * go[..., None]
    bounds = (scale * np.einsum("bhrc,bchd->brhd", ds_err, np.abs(kr)) + U * np.abs(dq),
              heads(scale * np.einsum("bhrc,brhd->bchd", ds_err, np.abs(q64))) + U * np.abs(dk),
              heads(np.einsum("bhrc,brhd->bchd", p_err, np.abs(g64))) + U * np.abs(dv))
    return (dq, dk, dv), bounds


def problem(case, seed=51):
    B, R, C, Hq, Hk, Dq, Dv, causal, mask_shape = case
    rng = np.random.default_rng(seed)
    q, k, v, mask = tensors(rng, B, R, C, Hq, Hk, Dq, Dv, mask_shape)
    g = (rng.random((B, R, Hq, Dv), dtype=F) - F(0.5)).astype(H)
    scale = float(1.0 / np.sqrt(Dq))
    return (g, q, k, v, mask), sdpa_cmd("SCALED_DOT_PRODUCT_ATTENTION_BACKWARD", scale, causal), scale


def backward(backend, cmd, g, q, k, v, mask, ask=(True, True, True)):
    outs = [np.full(a.shape, 3, H) if want else None for a, want in zip((q, k, v), ask)]
    return records(backend, lambda: exec_on(backend, nnc.GPU_MEMORY, cmd, nnc.NO_HINT, 0, [g, None, None, q, k, v] + ([mask] if mask is not None else []), outs))


def check(case, got, g, q, k, v, mask, scale):
    want, bounds = gradients64(g, q, k, v, mask, case[7], scale)
    for name, a, w, bound in zip(("dq", "dk", "dv"), got, want, bounds):
        err = np.abs(a.astype(D64) - w)
        print(case, name, "worst |err| / bound", float((err / bound).max()), "worst |err|", float(err.max()))
    for a, w, bound in zip(got, want, bounds):
        close(a.astype(F), w, tol=5e-3)
        assert (np.abs(a.astype(D64) - w) <= 2 * bound).all()


CASES = [
    # B, R, C, Hq, Hk, D, Dv, causal, mask
    (2, 33, 37, 2, 2, 24, 8, False, (1, 2)),     # a padded reduction chunk, one 8-wide output group, a mask
    (1, 40, 70, 2, 1, 40, 40, True, None),       # grouped heads summed into one key head, ragged causal blocks, a partial output tile
    (1, 37, 20, 2, 2, 40, 40, True, None),       # R > C: the first rows see no key
    (1, 131, 140, 2, 2, 80, 80, False, None),    # two workgroups in the row grid and in the key grid, several waves
    (1, 20, 33, 1, 1, 136, 72, False, (1, 1)),   # D > 128 and not in 16s
    (1, 70, 150, 2, 1, 160, 160, True, (1, 1)),
    (1, 37, 65, 1, 1, 256, 256, False, None),    # the largest instance; one gradient per pass
]
ROUTED = (2, 150, 170, 4, 2, 64, 64, True, None)  # a shape of sdpa_dq_f16_kernel / sdpa_dkv_f16_kernel


@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_half_backward_at_every_head_size(backend, case):
    tens, cmd, scale = problem(case)
    staged = counts(backend)[0]
    (r, got), names = backward(backend, cmd, *tens)
    assert r == 0
    assert all(any(n in rec for rec in names) for n in NEW) and not any(o in rec for rec in names for o in OLD), names
    assert counts(backend)[0] == staged
    check(case, got, *tens, scale)


@pytest.mark.parametrize("ask", [(True, False, False), (False, True, False), (False, False, True), (False, True, True)], ids=["dq", "dk", "dv", "dk+dv"])
def test_absent_gradients_leave_the_others_bit_for_bit(backend, ask):
    tens, cmd, _ = problem(CASES[1])
    (r0, full), _ = backward(backend, cmd, *tens)
    (r1, part), _ = backward(backend, cmd, *tens, ask=ask)
    assert r0 == 0 and r1 == 0
    for a, b, want in zip(full, part, ask):
        assert (b is None) if not want else (a.view(np.uint16) == b.view(np.uint16)).all()


def test_routing_by_the_key(backend):
    tens, cmd, scale = problem(ROUTED)
    (r, _), names = backward(backend, cmd, *tens)
    assert r == 0 and all(any(o in rec for rec in names) for o in OLD) and not any(n in rec for rec in names for n in NEW), names
    key = backend.tune_get("SDPA_F16_ANYD")
    try:
        backend.tune_set("SDPA_F16_ANYD", 2)  # the new kernels on the same tensors
        (r, got), names = backward(backend, cmd, *tens)
        assert r == 0 and all(any(n in rec for rec in names) for n in NEW) and not any(o in rec for rec in names for o in OLD), names
        check(ROUTED, got, *tens, scale)
        backend.tune_set("SDPA_F16_ANYD", 0)  # the former route: a shape of the new kernels goes through fp32 images again
        tens, cmd, _ = problem(CASES[1])
        staged = counts(backend)[0]
        (r, _), names = backward(backend, cmd, *tens)
        assert r == 0 and not any(n in rec for rec in names for n in NEW + OLD), names
        assert counts(backend)[0] > staged
    finally:
        backend.tune_set("SDPA_F16_ANYD", key)
