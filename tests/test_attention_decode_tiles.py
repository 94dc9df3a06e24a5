"""SCALED_DOT_PRODUCT_ATTENTION_FORWARD on CCV_16F tensors with 33 .. 256 packed rows per key head on sdpa_decode_tiles_f16_kernel / sdpa_decode_fold_kernel
(ccv_amd/csrc/sdpa_decode_tiles_f16.h; tunables SDPA_DECODE_TILES, SDPA_F16_DECODE, SDPA_DECODE_SPLITS), against float64 attention of the same half values.
Tolerances: those of tests/test_attention_heads.py, 3e-3 on the output and 2e-3 on the log-sum-exp."""
import numpy as np
import pytest
from ccv_amd import nnc
from harness import exec_on
from test_attention_decode import FOLD, FORMER, attention64, counts, records, sdpa_cmd, tensors

F, H, D64 = np.float32, np.float16, np.float64
NEW, ONE_TILE = "sdpa_decode_tiles_f16_kernel", "sdpa_decode_f16_kernel"


def run(lib, cmd, ins, outs, tiles, decode=1, splits=0):
    """The command with the three tuning keys at `tiles`, `decode` and `splits` (restored afterwards); returns ((status, outputs), launch records)."""
    new = dict(SDPA_DECODE_TILES=tiles, SDPA_F16_DECODE=decode, SDPA_DECODE_SPLITS=splits)
    old = {k: lib.tune_get(k) for k in new}
    for k in new:
        lib.tune_set(k, new[k])
    try:
        return records(lib, lambda: exec_on(lib, nnc.GPU_MEMORY, cmd, nnc.NO_HINT, 0, ins, outs))
    finally:
        for k in old:
            lib.tune_set(k, old[k])


CASES = [
    # B, R, C, Hq, Hk, D, Dv, causal, mask, splits
    (1, 33, 37, 1, 1, 24, 8, False, None, 1),        # the second tile holds one row; one ragged block; the direct store; an 8-wide output
    (1, 33, 37, 1, 1, 24, 8, False, None, 4),        # more splits than blocks: empty splits
    (1, 5, 150, 8, 1, 40, 40, True, None, 2),        # 40 rows; a padded reduction chunk; a partial output tile
    (1, 5, 150, 16, 2, 40, 40, True, None, 2),       # M = 40 with ratio 8: every wave's rows share causal limits with a neighbour
    (2, 8, 70, 16, 2, 64, 32, False, (1, 1), 2),     # exactly 64 rows: T = 2 is full; two batches; two key heads; a broadcast mask
    (1, 3, 100, 32, 1, 64, 64, False, (1, 32), 3),   # 96 rows: T = 4 with one empty tile; uneven splits; a mask per head
    (1, 16, 130, 8, 1, 64, 64, True, None, 0),       # exactly 128 rows; splits chosen by the launch
    (1, 65, 33, 2, 1, 32, 32, True, None, 2),        # 130 rows: two row groups, the second nearly empty; rows whose visible range ends before the second block
    (1, 40, 2, 1, 1, 40, 40, True, None, 1),         # R > C: the first 38 rows see no key
    (1, 33, 130, 1, 1, 256, 256, False, None, 2),    # the largest instance: LDS and register budget
    (1, 2, 200, 32, 1, 136, 72, False, None, 2),     # D above 128 and not in 16s
]


@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_decode_tiles_forward_matches_float64(backend, case):
    B, R, C, Hq, Hk, Dq, Dv, causal, mask_shape, splits = case
    q, k, v, mask = tensors(np.random.default_rng(61), B, R, C, Hq, Hk, Dq, Dv, mask_shape)
    cmd = sdpa_cmd("SCALED_DOT_PRODUCT_ATTENTION_FORWARD", float(1.0 / np.sqrt(Dq)), causal)
    ins, outs = [q, k, v] + ([mask] if mask is not None else []), [np.full((B, R, Hq, Dv), 3, H), np.zeros((B, Hq, R), F)]
    staged = counts(backend)[0]
    (r, got), names = run(backend, cmd, ins, outs, 8, splits=splits)
    assert r == 0
    assert any(NEW in n for n in names) and not any(f in n for n in names for f in FORMER + (ONE_TILE,)), names
    assert any(FOLD in n for n in names) == (splits > 1), names  # (splits 0: five blocks are one split by the launch's rule)
    assert counts(backend)[0] == staged
    want, lse, seen = attention64(q, k, v, mask, causal)
    print(case, "worst output error", float(np.abs(got[0].astype(D64) - want).max()), "worst lse error", float(np.abs(got[1][seen] - lse[seen]).max(initial=0)))
    np.testing.assert_allclose(got[0].astype(D64), want, rtol=0, atol=3e-3)
    np.testing.assert_allclose(got[1][seen], lse[seen], rtol=2e-3, atol=2e-3)
    assert (got[0][~seen.transpose(0, 2, 1)] == 0).all() and np.isneginf(got[1][~seen]).all()
    if splits == 3:  # no atomics anywhere: the same tensors give the same bits
        (_, again), _ = run(backend, cmd, ins, outs, 8, splits=splits)
        assert (again[0].view(np.uint16) == got[0].view(np.uint16)).all() and (again[1].view(np.uint32) == got[1].view(np.uint32)).all()


def test_the_key_bounds_the_rows_and_other_commands_keep_their_kernels(backend):
    def names_of(shape, tiles, decode=1, name="SCALED_DOT_PRODUCT_ATTENTION_FORWARD"):
        B, R, C, Hq, Hk, Dq, Dv = shape
        q, k, v, _ = tensors(np.random.default_rng(62), B, R, C, Hq, Hk, Dq, Dv, None)
        cmd = sdpa_cmd(name, float(1.0 / np.sqrt(Dq)), False)
        if name.endswith("BACKWARD"):
            ins, outs = [np.ones((B, R, Hq, Dv), H), None, None, q, k, v], [np.zeros_like(q), np.zeros_like(k), np.zeros_like(v)]
        else:
            ins, outs = [q, k, v], [np.zeros((B, R, Hq, Dv), H)]
        (r, _), names = run(backend, cmd, ins, outs, tiles, decode=decode)
        assert r == 0
        return names

    def former(names):
        return any("sdpa_forw_f16_kernel" in n for n in names) and not any("sdpa_decode" in n for n in names)

    assert backend.tune_get("SDPA_DECODE_TILES") == 1
    names = names_of((1, 34, 256, 1, 1, 64, 64), 1, decode=256)  # both keys at their defaults
    assert former(names), names
    names = names_of((1, 64, 70, 1, 1, 64, 64), 2)
    assert any(NEW in n for n in names) and not any(f in n for n in names for f in FORMER), names
    names = names_of((1, 65, 70, 1, 1, 64, 64), 2)
    assert former(names), names
    names = names_of((1, 32, 70, 1, 1, 64, 64), 8)
    assert any(ONE_TILE in n for n in names) and not any(NEW in n for n in names), names
    names = names_of((1, 64, 70, 1, 1, 64, 64), 8, decode=71)  # C below SDPA_F16_DECODE
    assert former(names), names
    names = names_of((1, 64, 70, 1, 1, 64, 64), 8, name="SCALED_DOT_PRODUCT_ATTENTION_BACKWARD")
    assert names and not any("sdpa_decode" in n for n in names), names
