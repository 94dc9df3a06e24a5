"""The register-resident Winograd kernels (wino_fused.h: six instantiations -- 4 x 4, 2 x 8, 8 x 2 tile groups, each plain and with the ReLU mask --
and wino_wgrad_fused.h) at the smallest shapes that reach each of them and cross every hand-over inside them: an even and an odd number of 8-channel
chunks (the item -> next-item hand-over sits in an item's last two trips), two blocks of 32 output channels with the second one ragged, two images.
Runtime behaviour only: results are held to the via-HBM Winograd path (algorithm 1) at the tolerance tests/test_parity_ops.py holds either of the
two to the reference with (1e-4 relative; absolute 1e-5 forward, 2e-5 of the tensor's scale backward).  Runs on the CPU HIP emulator in the `not gpu`
tier and on the MI355X in the `gpu` tier."""
import numpy as np
import pytest
from ccv_amd import nnc
from harness import exec_on

F = np.float32
HINT = nnc.HINT((1, 1), (1, 1))
GEOMS = [(9, 9, "4x4"), (6, 33, "2x8"), (33, 6, "8x2")]  # 3 x 3 / 2 x 9 / 9 x 2 tiles: the group shape with the least padding


def srnd(rng, *shape, scale=1.0):
    return ((rng.random(shape, dtype=F) - 0.5) * 2 * scale).astype(F)


def _inputs(h, w, c, k, seed=0):
    rng = np.random.default_rng(seed)
    a = np.maximum(srnd(rng, 2, h, w, c), 0)  # a rectified map: the mask of the data gradient
    return a, srnd(rng, k, 3, 3, c, scale=1.0 / (9 * c)), srnd(rng, k, scale=0.5), srnd(rng, 2, h, w, k)


def _forward(lib, algo, relu, a, wt, bias, k):
    cmd = nnc.CMD_CONVOLUTION_FORWARD(1, k, 3, 3, a.shape[3])
    cmd.algorithm = (nnc.CONV_ALGO_FUSE_RELU | algo) if relu else algo
    r, (out,) = exec_on(lib, nnc.GPU_MEMORY, cmd, HINT, 0, [a, wt] + ([bias] if bias is not None else []), [np.full(a.shape[:3] + (k,), 7, F)])
    assert r == 0
    return out


def _backward(lib, algo, mask, g, a, wt):
    cmd = nnc.CMD_CONVOLUTION_BACKWARD(1, wt.shape[0], 3, 3, a.shape[3])
    cmd.algorithm = (nnc.CONV_ALGO_FUSE_RELU | algo) if mask else algo
    r, out = exec_on(lib, nnc.GPU_MEMORY, cmd, HINT, 0, [g, a, wt], [np.full_like(a, 3), np.zeros_like(wt), np.zeros(wt.shape[0], F)])
    assert r == 0
    return out


def _close_fwd(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5)


def _close_bwd(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-5 * max(1.0, float(np.abs(want).max())))


@pytest.mark.parametrize("k", [32, 40])
@pytest.mark.parametrize("c", [16, 24])
@pytest.mark.parametrize("geom", GEOMS, ids=[x[2] for x in GEOMS])
def test_fused_forward_and_data_gradient_against_via_hbm(backend, geom, c, k):
    """wino_fused_kernel<GH, GW> forward with and without bias and ReLU, <GH, GW, 0, true> / plain as the data gradient with and without the mask."""
    h, w, _ = geom
    a, wt, bias, g = _inputs(h, w, c, k)
    for relu in (False, True):
        for b in (bias, None):
            got = _forward(backend, 2, relu, a, wt, b, k)
            assert backend.dll.nnc_mi355x_last_kernel_name().decode() == "conv_fwd_wino_fused"
            _close_fwd(got, _forward(backend, 1, relu, a, wt, b, k))
            assert not relu or ((got >= 0).all() and (got == 0).any())
    for mask in (False, True):
        got = _backward(backend, 2, mask, g, a, wt)
        assert backend.dll.nnc_mi355x_last_kernel_name().decode() == "conv_dgrad_wino_fused"
        want = _backward(backend, 1, mask, g, a, wt)
        for i in range(3):
            _close_bwd(got[i], want[i])
        assert not mask or (got[0][a <= 0] == 0).all()


@pytest.mark.parametrize("geom", GEOMS, ids=[x[2] for x in GEOMS])
def test_fused_filter_gradient_against_via_hbm(backend, geom):
    """wino_wgrad_fused_kernel (C % 64 == 0, K % 32 == 0) with the bias gradient from the same pass."""
    h, w, _ = geom
    a, wt, _, g = _inputs(h, w, 64, 32, seed=1)
    cmd = nnc.CMD_CONVOLUTION_BACKWARD(1, 32, 3, 3, 64)
    res = {}
    for algo in (2, 1):
        cmd.algorithm = algo
        r, out = exec_on(backend, nnc.GPU_MEMORY, cmd, HINT, 0, [g, a, wt], [None, np.zeros_like(wt), np.zeros(32, F)])
        assert r == 0
        if algo == 2:
            assert backend.dll.nnc_mi355x_last_kernel_name().decode() == "conv_wgrad_wino_fused"
        res[algo] = out
    _close_bwd(res[2][1], res[1][1])
    _close_bwd(res[2][2], res[1][2])


@pytest.mark.parametrize("geom", GEOMS, ids=[x[2] for x in GEOMS])
def test_fused_kernels_twice_on_a_dirty_workspace(backend, geom):
    """The same commands twice in one process behind a larger convolution that leaves the workspace full of other values: whatever a kernel keeps
    or recomputes per item is set up again by every launch -- the two runs are EQUAL, and close to the via-HBM path."""
    h, w, _ = geom
    a, wt, bias, g = _inputs(h, w, 24, 40, seed=2)
    runs = []
    for _ in range(2):
        big = _inputs(21, 23, 32, 64, seed=9)
        _forward(backend, 1, False, big[0], big[1], big[2], 64)  # V and M of 2 x 36 tiles x 96 channels over the same scratch
        runs.append((_forward(backend, 2, True, a, wt, bias, 40), _backward(backend, 2, True, g, a, wt), _backward(backend, 2, False, g, a, wt)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for j in (1, 2):
        for i in range(3):
            assert np.array_equal(runs[0][j][i], runs[1][j][i]), (j, i)
    _close_fwd(runs[0][0], _forward(backend, 1, True, a, wt, bias, 40))
    want = _backward(backend, 1, True, g, a, wt)
    for i in range(3):
        _close_bwd(runs[0][1][i], want[i])
