"""SCALED_DOT_PRODUCT_ATTENTION_FORWARD on CCV_16F tensors with few query rows against many keys on sdpa_decode_f16_kernel / sdpa_decode_fold_kernel
(ccv_amd/csrc/sdpa_decode_f16.h; tunables SDPA_F16_DECODE, SDPA_DECODE_SPLITS), against float64 attention of the same half values.  Tolerances: those of
tests/test_attention_heads.py, 3e-3 on the output and 2e-3 on the log-sum-exp."""
import numpy as np
import pytest
from ccv_amd import nnc
from harness import exec_on
from test_attention import sdpa_cmd
from test_attention_heads import attention64, tensors
from test_mbconv_half import counts, records

F, H, D64 = np.float32, np.float16, np.float64
NEW, FOLD, FORMER = "sdpa_decode_f16_kernel", "sdpa_decode_fold_kernel", ("sdpa_forw_f16_kernel", "sdpa_fwd_anyd_f16_kernel")


def run(lib, cmd, ins, outs, decode=1, splits=0):
    """The command with the two tuning keys at `decode` and `splits` (None: as they are; restored afterwards); returns ((status, outputs), launch records)."""
    keys = lib.tune_get("SDPA_F16_DECODE"), lib.tune_get("SDPA_DECODE_SPLITS")
    if decode is not None:
        lib.tune_set("SDPA_F16_DECODE", decode)
    lib.tune_set("SDPA_DECODE_SPLITS", splits)
    try:
        return records(lib, lambda: exec_on(lib, nnc.GPU_MEMORY, cmd, nnc.NO_HINT, 0, ins, outs))
    finally:
        lib.tune_set("SDPA_F16_DECODE", keys[0])
        lib.tune_set("SDPA_DECODE_SPLITS", keys[1])


CASES = [
    # B, R, C, Hq, Hk, D, Dv, causal, mask, splits
    (1, 1, 37, 2, 2, 24, 8, False, None, 1),       # one row, one ragged block, the direct store, an 8-wide output group
    (1, 1, 37, 2, 2, 24, 8, False, None, 4),       # more splits than key blocks: empty splits, waves without a block
    (2, 1, 300, 8, 1, 64, 64, False, None, 3),     # eight heads packed on one key head, uneven splits and waves, two batch items
    (1, 4, 150, 8, 2, 40, 40, True, None, 2),      # 16 packed rows with four causal limits, a padded reduction chunk, a partial output tile
    (1, 3, 2, 2, 2, 40, 40, True, None, 0),        # R > C: the first row sees no key; splits chosen by the launch
    (1, 4, 70, 8, 1, 64, 32, True, (1, 1), 2),     # exactly 32 packed rows, a broadcast mask
    (1, 2, 200, 2, 1, 136, 72, False, (1, 2), 4),  # D above 128 and not in 16s, a mask per head
    (1, 1, 130, 1, 1, 256, 256, False, None, 2),   # the largest instance
]


@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_decode_forward_matches_float64(backend, case):
    B, R, C, Hq, Hk, Dq, Dv, causal, mask_shape, splits = case
    q, k, v, mask = tensors(np.random.default_rng(51), B, R, C, Hq, Hk, Dq, Dv, mask_shape)
    cmd = sdpa_cmd("SCALED_DOT_PRODUCT_ATTENTION_FORWARD", float(1.0 / np.sqrt(Dq)), causal)
    ins, outs = [q, k, v] + ([mask] if mask is not None else []), [np.full((B, R, Hq, Dv), 3, H), np.zeros((B, Hq, R), F)]
    staged = counts(backend)[0]
    (r, got), names = run(backend, cmd, ins, outs, splits=splits)
    assert r == 0
    assert any(NEW in n for n in names) and not any(f in n for n in names for f in FORMER), names
    assert any(FOLD in n for n in names) == (splits > 1), names
    assert counts(backend)[0] == staged
    want, lse, seen = attention64(q, k, v, mask, causal)
    print(case, "worst output error", float(np.abs(got[0].astype(D64) - want).max()), "worst lse error", float(np.abs(got[1][seen] - lse[seen]).max(initial=0)))
    np.testing.assert_allclose(got[0].astype(D64), want, rtol=0, atol=3e-3)
    np.testing.assert_allclose(got[1][seen], lse[seen], rtol=2e-3, atol=2e-3)
    assert (got[0][~seen.transpose(0, 2, 1)] == 0).all() and np.isneginf(got[1][~seen]).all()
    if splits == 3:  # the fold has no atomics: the same tensors give the same bits
        (_, again), _ = run(backend, cmd, ins, outs, splits=splits)
        assert (again[0].view(np.uint16) == got[0].view(np.uint16)).all() and (again[1].view(np.uint32) == got[1].view(np.uint32)).all()


def test_other_shapes_and_the_backward_keep_their_kernels(backend):
    def names_of(shape, decode, name="SCALED_DOT_PRODUCT_ATTENTION_FORWARD"):
        B, R, C, Hq, Hk, Dq, Dv = shape
        q, k, v, _ = tensors(np.random.default_rng(52), B, R, C, Hq, Hk, Dq, Dv, None)
        cmd = sdpa_cmd(name, float(1.0 / np.sqrt(Dq)), False)
        if name.endswith("BACKWARD"):
            ins, outs = [np.ones((B, R, Hq, Dv), H), None, None, q, k, v], [np.zeros_like(q), np.zeros_like(k), np.zeros_like(v)]
        else:
            ins, outs = [q, k, v], [np.zeros((B, R, Hq, Dv), H)]
        (r, _), names = run(backend, cmd, ins, outs, decode=decode)
        assert r == 0
        return names

    decode_shape = (1, 1, 70, 4, 2, 64, 64)
    assert any(NEW in n for n in names_of(decode_shape, 1))
    for shape, decode in (((1, 33, 70, 1, 1, 64, 64), 1), (decode_shape, 0)):  # 33 packed rows; the key at 0
        names = names_of(shape, decode)
        assert any("sdpa_forw_f16_kernel" in n for n in names) and not any("sdpa_decode" in n for n in names), names
    names = names_of((1, 20, 33, 1, 1, 136, 72), None)  # the key at its default
    assert any("sdpa_fwd_anyd_f16_kernel" in n for n in names) and not any("sdpa_decode" in n for n in names), names
    names = names_of(decode_shape, 1, "SCALED_DOT_PRODUCT_ATTENTION_BACKWARD")
    assert names and not any("sdpa_decode" in n for n in names), names
