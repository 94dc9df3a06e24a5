"""Every route of the convolution commands (ccv_amd/csrc/cmd_conv.cpp) at the smallest size that still takes it, plain and under
NNC_MI355X_CONV_ALGO_FUSE_RELU: the route taken, the ReLU / mask identities bit for bit, and that one command leaves nothing behind for the next.
The cases are tests/conv_route_cases.py's (tools/conv_snapshot.py prints the same commands' routes and output hashes for a given build of the library).
The convolution paths use no floating-point atomics, so results are reproducible run to run and bit equality is demanded throughout.
Runs on the CPU HIP emulator in the `not gpu` tier and on the MI355X in the `gpu` tier."""
import numpy as np
import pytest
import conv_route_cases as crc

# The route of every plain command -- the last kernel name, or (name, launches of wino_outgrad_both_kernel / wino_input_kernel<true>, half tensors staged
# as fp32 images / handed on as halves) where a counter moves -- recorded on the commit BEFORE the per-call context replaced the thread-local flags
# (tools/conv_snapshot.py --routes) and read against the routing rules of cmd_conv.cpp.  The FUSE_RELU command takes the same route unless "<key>+relu"
# says otherwise.  Emulator and MI355X agree on every entry.
EXPECTED = {
    'c8_k8_5x5': {  # C < 16: no fused kernel; C < 32: the backend's own choice is the implicit GEMM
        'fwd/-1': 'conv_fwd', 'fwd/0': 'conv_fwd', 'fwd/1': 'conv_fwd_wino', 'fwd/2': 'conv_fwd_wino',
        'dx': 'conv_dgrad', 'dw': 'conv_wgrad', 'all': 'conv_dgrad',
    },
    'c16_k40_6x40': {  # (the filter gradient: C % 64 != 0 and C < 32, the implicit GEMM)
        'fwd/-1': 'conv_fwd_wino_fused', 'fwd/0': 'conv_fwd', 'fwd/1': 'conv_fwd_wino', 'fwd/2': 'conv_fwd_wino_fused',
        'dx': 'conv_dgrad_wino_fused', 'dw': 'conv_wgrad', 'all': 'conv_dgrad_wino_fused',
    },
    'c3_k16_9x9': {
        'fwd/-1': 'conv_fwd_c3', 'fwd/0': 'conv_fwd', 'fwd/1': 'conv_fwd_c3', 'fwd/2': 'conv_fwd_c3',
        'dx': 'conv_dgrad', 'dw': 'conv_wgrad_c3', 'all': 'conv_dgrad',
    },
    'c16_k32_7x7_1x1': {
        'fwd/-1': 'conv_fwd_pointwise', 'fwd/0': 'conv_fwd_pointwise', 'fwd/1': 'conv_fwd_pointwise', 'fwd/2': 'conv_fwd_pointwise',
        'dx': 'conv_dgrad_pointwise', 'dw': 'conv_wgrad_pointwise', 'all': 'conv_dgrad_pointwise',
    },
    'c6_k10_8x8': {
        'fwd/-1': 'conv_fwd', 'fwd/0': 'conv_fwd', 'fwd/1': 'conv_fwd', 'fwd/2': 'conv_fwd',
        'dx': 'conv_dgrad', 'dw': 'conv_wgrad', 'all': 'conv_dgrad',
    },
    'dw16_8x8': {  # (algorithm 0 keeps the grouped implicit GEMM; the filter gradient ends with the fold of its partials)
        'fwd/-1': 'conv_dw_fwd', 'fwd/0': 'conv_fwd', 'fwd/1': 'conv_dw_fwd', 'fwd/2': 'conv_dw_fwd',
        'dx': 'conv_dw_dgrad', 'dw': 'conv_dw_fold', 'all': 'conv_dw_dgrad',
    },
    'dw16_8x8_nchw': {
        'fwd/-1': 'conv_dw_fwd', 'fwd/0': 'conv_fwd', 'fwd/1': 'conv_dw_fwd', 'fwd/2': 'conv_dw_fwd',
        'dx': 'conv_dw_dgrad', 'dw': 'conv_dw_fold', 'all': 'conv_dw_dgrad',
    },
    'dw16_8x8_half_a': {  # fp32 images of the half tensors (a, b / g, a, h / g, a): the grouped implicit GEMM, never the depthwise kernels
        'fwd/-1': ('conv_fwd', (0, 0), (2, 0)), 'fwd/0': ('conv_fwd', (0, 0), (2, 0)), 'fwd/1': ('conv_fwd', (0, 0), (2, 0)), 'fwd/2': ('conv_fwd', (0, 0), (2, 0)),
        'dx': ('conv_dgrad', (0, 0), (3, 0)), 'dw': ('conv_wgrad', (0, 0), (2, 0)), 'all': ('conv_dgrad', (0, 0), (3, 0)),
    },
    'nchw_c8_k8_4x4_1x1': {  # (algorithm 0: through the layout kernels to the pointwise GEMM)
        'fwd/-1': 'conv1x1_nchw_fwd', 'fwd/0': 'conv_fwd_pointwise', 'fwd/1': 'conv1x1_nchw_fwd', 'fwd/2': 'conv1x1_nchw_fwd',
        'dx': 'conv1x1_nchw_dgrad', 'dw': 'conv1x1_nchw_wgrad', 'all': 'conv1x1_nchw_dgrad',
    },
    'nchw_c8_k8_6x6': {
        'fwd/-1': 'conv_fwd', 'fwd/0': 'conv_fwd', 'fwd/1': 'conv_fwd_wino', 'fwd/2': 'conv_fwd_wino',
        'dx': 'conv_dgrad', 'dw': 'conv_wgrad', 'all': 'conv_dgrad',
    },
    'half_c8_k8_6x6': {  # no tensor staged: the half-precision core reads the tensors where they lie
        'fwd/-1': 'conv_fwd_h', 'fwd/0': 'conv_fwd_h', 'fwd/1': 'conv_fwd_h', 'fwd/2': 'conv_fwd_h',
        'dx': 'conv_dgrad_h', 'dw': 'conv_wgrad_h', 'all': 'conv_dgrad_h',
    },
    'half_nchw_c8_k8_6x6_f16': {  # ... between half transposes (no fp32 image through half_stage.cpp on either branch)
        'fwd/-1': 'conv_fwd_h', 'fwd/0': 'conv_fwd_h', 'fwd/1': 'conv_fwd_h', 'fwd/2': 'conv_fwd_h',
        'dx': 'conv_dgrad_h', 'dw': 'conv_wgrad_h', 'all': 'conv_dgrad_h',
    },
    'half_nchw_c8_k8_6x6_f32': {
        'fwd/-1': 'conv_fwd', 'fwd/0': 'conv_fwd', 'fwd/1': 'conv_fwd_wino', 'fwd/2': 'conv_fwd_wino',
        'dx': 'conv_dgrad', 'dw': 'conv_wgrad', 'all': 'conv_dgrad',
    },
    'c8_k8_5x5_n3_algo1': {  # both gradients: wino_outgrad_both_kernel once, masked or not
        'dx': 'conv_dgrad_wino', 'dw': 'conv_wgrad_wino', 'all': ('conv_dgrad_wino', (1, 0), (0, 0)),
    },
    'c40_k40_6x40_algo2': {  # both gradients under the mask: the bits come from wino_input_kernel<true>; unmasked there is nothing to share
        'dx': 'conv_dgrad_wino_fused', 'dw': 'conv_wgrad_wino', 'all': 'conv_dgrad_wino_fused',
        'all+relu': ('conv_dgrad_wino_fused', (0, 1), (0, 0)),
    },
    'c8_k8_8x8_s2': {  # the parity classes run the forward implicit GEMM on the output gradient
        'dx': 'conv_fwd', 'dw': 'conv_wgrad', 'all': 'conv_fwd',
    },
}


def _route(x):
    return (x, (0, 0), (0, 0)) if isinstance(x, str) else x


def _bits(x):
    return x.view(np.uint16 if x.dtype == np.float16 else np.uint32)


@pytest.mark.parametrize("case", crc.CASES, ids=repr)
def test_routes_and_relu_identities(backend, case):
    """Per command of the case: plain, FUSE_RELU, plain again.
    Route: each of the three takes the recorded one.
    Forward: the FUSE_RELU output is np.maximum(0, plain output) bit for bit, fused epilogue or in-place pass.  The inputs hold exact and negative zeros
    and a filter of zeros, so the plain output holds exact zeros next to negative values (a contraction that accumulates from +0 gives no negative zero).
    Backward: with a rectified a that holds +0.0 and -0.0, the masked dx is where(a > 0, plain dx, 0) bit for bit; dw and dbias are the plain command's.
    No leak: the plain command run right behind the FUSE_RELU one repeats the first plain run bit for bit and moves the counters as the first did."""
    expected = EXPECTED[case.name]
    for key, kind, algo in crc.commands(case):
        route_plain, plain = crc.run(backend, case, kind, algo, False)
        route_relu, relu = crc.run(backend, case, kind, algo, True)
        route_again, again = crc.run(backend, case, kind, algo, False)
        assert route_plain == _route(expected[key]), (key, route_plain)
        assert route_relu == _route(expected.get(key + "+relu", expected[key])), (key, route_relu)
        assert route_again == route_plain, (key, route_again)
        assert len(plain) == len(relu) == len(again) == {"fwd": 1, "dx": 1, "dw": 1, "all": 3}[kind]
        for x, y in zip(plain, again):
            assert x.dtype == y.dtype and np.array_equal(_bits(x), _bits(y)), key
        if kind == "fwd":
            assert plain[0].dtype == case.act and (plain[0] == 0).any() and (plain[0] < 0).any() and (plain[0] > 0).any(), key
            want = np.maximum(0, plain[0])
            assert relu[0].dtype == want.dtype and np.array_equal(_bits(relu[0]), _bits(want)), key
        else:
            if kind != "dw":
                assert (plain[0][case.a <= 0] != 0).any(), key  # there is something to mask
                want = np.where(case.a > 0, plain[0], 0).astype(plain[0].dtype)
                assert np.array_equal(_bits(relu[0]), _bits(want)), key
            first = 0 if kind == "dw" else 1  # dw (and dbias)
            for x, y in zip(plain[first:], relu[first:]):
                assert np.array_equal(_bits(x), _bits(y)), key
