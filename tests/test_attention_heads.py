"""SCALED_DOT_PRODUCT_ATTENTION_FORWARD on CCV_16F tensors at the head sizes sdpa_forw_f16_kernel refuses (D, Dv in 8s up to 256: sdpa_fwd_anyd_f16_kernel,
ccv_amd/csrc/sdpa_anyd_f16.h; tunable SDPA_F16_ANYD) and the head projection in half, against float64 attention of the same half values.  Tolerances: 3e-3 on the
output and 2e-3 on the log-sum-exp, those of tests/test_attention.py and of the reference's own GPU test for half attention (cublas.tests.c:2816)."""
import numpy as np
import pytest
from ccv_amd import nnc
from harness import exec_on
from test_attention import sdpa_cmd
from test_mbconv_half import counts, records

F, H, D64 = np.float32, np.float16, np.float64
NEW, OLD = "sdpa_fwd_anyd_f16_kernel", "sdpa_forw_f16_kernel"


def attention64(q, k, v, mask, causal):
    """float64 (output [B, R, Hq, Dv], log-sum-exp [B, Hq, R], rows that see a key [B, Hq, R]); the bottom-right causal triangle, 0 for a row that sees no key"""
    ratio, R, C = q.shape[2] // k.shape[2], q.shape[1], k.shape[1]
    s = np.einsum("brhd,bchd->bhrc", q.astype(D64), np.repeat(k, ratio, axis=2).astype(D64)) / np.sqrt(q.shape[3])
    if mask is not None:
        s = s + mask.astype(D64)
    if causal:
        s = np.where(np.arange(C)[None, :] < np.arange(R)[:, None] - R + C + 1, s, -np.inf)
    seen = np.isfinite(s).any(-1)
    m = np.where(seen, s.max(-1), 0.0)[..., None]
    p = np.exp(s - m)
    l = p.sum(-1, keepdims=True)
    o = np.einsum("bhrc,bchd->brhd", p / np.where(l > 0, l, 1.0), np.repeat(v, ratio, axis=2).astype(D64))
    with np.errstate(divide="ignore"):
        return o, (np.log(l) + m)[..., 0], seen


def tensors(rng, B, R, C, Hq, Hk, Dq, Dv, mask_shape):
    q, k, v = [(rng.random(s, dtype=F) - F(0.5)).astype(H) for s in ((B, R, Hq, Dq), (B, C, Hk, Dq), (B, C, Hk, Dv))]
    mask = None if mask_shape is None else ((rng.random(mask_shape + (R, C), dtype=F) - F(0.5)) * F(2)).astype(H)
    return q, k, v, mask


CASES = [
    # B, R, C, Hq, Hk, D, Dv, causal, mask
    (2, 33, 37, 2, 2, 24, 8, False, (1, 2)),     # smallest tiles, one 8-wide output group, a mask
    (1, 40, 70, 2, 1, 40, 40, True, None),       # padded last reduction chunk, partial output tile, grouped heads, ragged causal blocks
    (1, 37, 20, 2, 2, 40, 40, True, None),       # R > C: the first rows see no key
    (1, 131, 97, 2, 2, 80, 80, False, None),     # several waves, two workgroups
    (1, 20, 33, 1, 1, 136, 72, False, (1, 1)),   # D > 128 and not in 16s
    (1, 70, 150, 2, 1, 160, 160, True, (1, 1)),
    (1, 37, 65, 1, 1, 256, 256, False, None),    # the largest instance
]


@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_half_forward_at_every_head_size(backend, case):
    B, R, C, Hq, Hk, Dq, Dv, causal, mask_shape = case
    q, k, v, mask = tensors(np.random.default_rng(41), B, R, C, Hq, Hk, Dq, Dv, mask_shape)
    cmd = sdpa_cmd("SCALED_DOT_PRODUCT_ATTENTION_FORWARD", float(1.0 / np.sqrt(Dq)), causal)
    staged = counts(backend)[0]
    (r, got), names = records(backend, lambda: exec_on(backend, nnc.GPU_MEMORY, cmd, nnc.NO_HINT, 0, [q, k, v] + ([mask] if mask is not None else []), [np.full((B, R, Hq, Dv), 3, H), np.zeros((B, Hq, R), F)]))
    assert r == 0
    assert any(NEW in n for n in names) and not any(OLD in n for n in names), names
    assert counts(backend)[0] == staged
    want, lse, seen = attention64(q, k, v, mask, causal)
    print(case, "worst output error", float(np.abs(got[0].astype(D64) - want).max()), "worst lse error", float(np.abs(got[1][seen] - lse[seen]).max()))
    np.testing.assert_allclose(got[0].astype(D64), want, rtol=0, atol=3e-3)
    np.testing.assert_allclose(got[1][seen], lse[seen], rtol=2e-3, atol=2e-3)
    assert (got[0][~seen.transpose(0, 2, 1)] == 0).all() and np.isneginf(got[1][~seen]).all()


def test_shapes_of_the_first_half_kernel_keep_it(backend):
    B, R, C, Hq, Hk, Dq, Dv = 2, 150, 70, 4, 2, 64, 64
    q, k, v, _ = tensors(np.random.default_rng(42), B, R, C, Hq, Hk, Dq, Dv, None)
    cmd = sdpa_cmd("SCALED_DOT_PRODUCT_ATTENTION_FORWARD", float(1.0 / np.sqrt(Dq)), True)
    (r, got), names = records(backend, lambda: exec_on(backend, nnc.GPU_MEMORY, cmd, nnc.NO_HINT, 0, [q, k, v], [np.zeros((B, R, Hq, Dv), H)]))
    assert r == 0 and any(OLD in n for n in names) and not any(NEW in n for n in names), names
    np.testing.assert_allclose(got[0].astype(D64), attention64(q, k, v, None, True)[0], rtol=0, atol=3e-3)


def test_head_projection_in_half(backend):
    """every tensor CCV_16F: the attention output lands in outputs[2] as halves, the projection is a half GEMM_FORWARD -- no fp32 images"""
    B, R, C, Hh, Dq, Dv = 2, 21, 17, 2, 40, 40
    rng = np.random.default_rng(43)
    q, k, v, _ = tensors(rng, B, R, C, Hh, Hh, Dq, Dv, None)
    w, bias = (rng.random((Hh * Dv, Hh * Dv), dtype=F) - F(0.5)).astype(H), (rng.random(Hh * Dv, dtype=F) - F(0.5)).astype(H)
    cmd = sdpa_cmd("SCALED_DOT_PRODUCT_ATTENTION_FORWARD", float(1.0 / np.sqrt(Dq)), False)
    staged = counts(backend)[0]
    r, got = exec_on(backend, nnc.GPU_MEMORY, cmd, nnc.NO_HINT, 0, [q, k, v, None, w, bias], [np.zeros((B, R, Hh * Dv), H), np.zeros((B, Hh, R), F), np.zeros((B, R, Hh, Dv), H)])
    assert r == 0
    assert counts(backend)[0] == staged
    np.testing.assert_allclose(got[2].astype(D64), attention64(q, k, v, None, False)[0], rtol=0, atol=3e-3)
    want = got[2].astype(D64).reshape(B, R, Hh * Dv) @ w.astype(D64).T + bias.astype(D64)
    # one rounding of the result to half (2^-11 relative) with a factor of two for the 80-term fp32 accumulation
    np.testing.assert_allclose(got[0].astype(D64), want, rtol=0, atol=2.0 ** -10 * float(np.abs(want).max()))
