"""The slice plan of the column sums (ccv_amd/csrc/chan_sums.cpp) and the workspace figures derived from it, through nnc_mi355x_debug_colsum_plan: host
arithmetic only, nothing is launched.  Callers that keep data of their own behind the sums' partials size that head with colsum_workspace_bytes (one call)
or colsum_workspace_bound (any call with that many columns): the plan must cover the rows without an empty slice, the bytes must be the plan's, and the
bound must be their maximum -- reached, not merely above them.  Both tiers report 256 compute units, so the plans are the same."""
import ctypes as C
import pytest

ROWS = [0, 1, 63, 64, 65, 128, 129, 4096, 65537, 2**31 + 5]
COLS = [1, 3, 4, 63, 64, 65, 68, 1000, 4096, 16385, 300000]


def _plan(lib, rows, cols):
    f = lib.dll.nnc_mi355x_debug_colsum_plan
    f.restype, f.argtypes = None, [C.c_long, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    slices, rows_per_slice, nbytes, bound = C.c_long(), C.c_long(), C.c_size_t(), C.c_size_t()
    f(rows, cols, C.byref(slices), C.byref(rows_per_slice), C.byref(nbytes), C.byref(bound))
    return slices.value, rows_per_slice.value, nbytes.value, bound.value


@pytest.mark.parametrize("cols", COLS)
def test_colsum_plan_covers_the_rows_and_the_bound_is_its_maximum(backend, cols):
    reached = False
    for rows in ROWS:
        slices, rows_per_slice, nbytes, bound = _plan(backend, rows, cols)
        assert slices >= 1, (rows, cols)
        assert slices * rows_per_slice >= rows, (rows, cols, slices, rows_per_slice)
        if rows > 0:
            assert (slices - 1) * rows_per_slice < rows, (rows, cols, slices, rows_per_slice)  # no slice is empty
        assert nbytes == 4 * slices * cols, (rows, cols)
        assert nbytes <= bound, (rows, cols, nbytes, bound)
        reached = reached or nbytes == bound
    assert reached, (cols, bound)
