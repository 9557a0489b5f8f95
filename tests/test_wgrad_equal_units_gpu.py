"""GPU: the balanced grouped weight gradient at the smallest shape where the unit map has every kind of group - chunk_rows =
64 and groups of (0, 70, 200, 129) rows: an empty group (no unit), groups of two, four and three units, last units of 6, 8
and 1 rows (a partial last 32-row step each) - through every tile kernel that looks the map up (csrc/wgrad_dev.h: wgrad_unit)
at its smallest whole-tile shape: register-staged and LDS-DMA at N = K = 128, the 256 x 256 tile at N = K = 256.

Two forms, as the engine launches the experts: FC1 (A rows gathered through a_row_idx / 4) and FC2 (dC rows gathered through
c_row_idx / 4 and scaled by c_row_scale, with the fused bias gradient).  tests/test_contract_wgrad.py's run() does the work:
dW (and db) against a float64 product within kernel_contract's bounds for the grouped cases, guarded outputs and an exactly
sized sentinel-filled workspace, unchanged inputs, the launch signature, and the same bits from a second call under another
workspace fill."""
import pytest
import torch

import test_contract_wgrad as cw

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
COUNTS = [0, 70, 200, 129]
SLACK = 9                                       # rows past group_offsets[G] that belong to no group
CHUNK = 64

# kernel family, dtype, N = K, wgrad_set_dma, wgrad_set_big
CASES = [("staged", F16, 128, 0, 0), ("staged", BF16, 128, 0, 0), ("staged", F32, 128, 0, 0),
         ("dma", F16, 128, 2, 0), ("dma", BF16, 128, 2, 0), ("dma", F32, 128, 2, 0),
         ("big", F16, 256, None, 1), ("big", BF16, 256, None, 1)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    return _ops


def test_the_case_has_the_units_it_is_chosen_for(ops):
    import ctypes
    G, M = len(COUNTS), sum(COUNTS) + SLACK
    chunk, slots = ops.wgrad_plan(M, G, 2, True)
    assert chunk == CHUNK and slots >= 9
    off = [0, 0, 70, 270, 399]
    arr = (ctypes.c_int32 * 5)(*off)
    got = []
    for u in range(slots):
        g, b, e = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert ops.lib().m3_wgrad_unit_of(arr, G, chunk, u, ctypes.byref(g), ctypes.byref(b), ctypes.byref(e)) == 0
        got.append((g.value, e.value - b.value))
    assert got[:9] == [(1, 64), (1, 6), (2, 64), (2, 64), (2, 64), (2, 8), (3, 64), (3, 64), (3, 1)]
    assert all(x == (-1, 0) for x in got[9:])


@pytest.mark.parametrize("form", ["fc1", "fc2"])
@pytest.mark.parametrize("family,dtype,n,dma,big", CASES, ids=[f"{c[0]}-{str(c[1]).split('.')[1]}" for c in CASES])
def test_equal_units_every_tile_kernel(ops, family, dtype, n, dma, big, form):
    G, M = len(COUNTS), sum(COUNTS) + SLACK
    assert ops.wgrad_plan(M, G, 2, True)[0] == CHUNK
    kernel = family
    if form == "fc1":
        c_idx, c_scale, a_idx = cw._gathers(M, False, True, False, 1, 4, seed=8)
        kw = dict(a_idx=a_idx, a_div=4, want_db=False)
    else:
        c_idx, c_scale, a_idx = cw._gathers(M, True, False, True, 4, 1, seed=9)
        kw = dict(c_idx=c_idx, c_div=4, c_scale=c_scale, want_db=True)
        if not cw.has_instance(family, dtype, 1, 0, 1):          # no per-row factor for this dtype: the register-staged kernel takes it
            kernel = "staged"
    with cw.knobs(ops, dma, big):
        if family == "big":
            assert ops.wgrad_tile(n, n, dtype) == (256, 256)
        w = cw.run(ops, dtype, M, n, n, kernel=kernel, G=G, counts=COUNTS, splits=2, tag=f"equal_units/{family}/{dtype}/{form}", **kw)
    assert w < 1
