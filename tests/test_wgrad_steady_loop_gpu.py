"""GPU: the register-staged weight-gradient kernel's tile loop (csrc/wgrad_staged.hip: wgrad_tile_loop) at every row count at
which it takes another path.  The loop computes whole 32-row steps from bumped pointers and unselected LDS stores (16-bit
operands, the steps before a part's last, from the fifth step of a part on) and hands over to the clamped, zero-filling forms
two steps before the end; the remainder is one, two or three steps.  N = K = 128 (one output tile), wgrad_set_dma(0) and
wgrad_set_big(0), f16 / bf16 / f32 (fp32 keeps the clamped loop throughout).

tests/test_contract_wgrad.py's run() does the work: dW (and db) against a float64 product within kernel_contract's bounds,
guarded outputs and an exactly sized sentinel-filled workspace, unchanged inputs, the launch signature, and the same bits from
a second call under another workspace fill.  The operands are of order 1: a row added twice, a row left out or a tail row
that is not zeroed moves an output by about 1, far above a bound of a few 1e-4.

  plain rows, one part      M = 1 .. 289: parts of 1 - 10 steps, whole and partial last steps (every remainder, no / one /
                            two / three steady pairs, with and without a clamped pair behind them)
  plain rows, 2 and 3 parts M = 161, 225: inner parts end on a whole step, the last one on a one-row step
  grouped, balanced units   FC1 (A rows through a_row_idx / div) and FC2 (dC rows through c_row_idx / div, scaled by
                            c_row_scale, fused bias gradient), both gathers at once with and without the factor;
                            div = 1, 4 (a shift) and 3 (the general divide);
                            chunk_rows = 64 with groups of (0, 70, 200, 129) rows: units of one and two steps;
                            chunk_rows = 704 with groups of (0, 1030, 333, 3628) rows: units of 576, 454, 333, 5 x 640 and
                            428 rows - 11 to 20 steps, whole and partial last steps (6, 13 and 12 rows).

A gathered row's source row and factor come from an LDS table that is filled in pieces of 256 rows (8 steps), two slots: the
prologue makes the pieces 0 and 1, the loop over whole pieces (it runs while more than 10 steps are left) piece j + 2 while it
computes piece j.  The units of chunk64 lie inside piece 0; those of chunk704 span two pieces (333, 428, 454 rows: one turn
of the piece loop, the last piece ending on a partial step) and three (576, 640 rows: the third piece is written by the loop
into the slot of the first and read by the steps 16 - 19; at 640 rows the loop turns twice).  Both gathers at once keep two
row tables live, with the factor three arrays."""
import ctypes

import pytest
import torch

import test_contract_wgrad as cw

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F16, BF16, F32]
NK = 128
SLACK = 9                                       # rows past group_offsets[G] that belong to no group
PLAIN_M = [1, 32, 33, 64, 65, 96, 97, 128, 129, 161, 192, 225, 257, 289]
# name: (counts, splits, chunk_rows, (group, rows) of the live units in order)
SHAPES = {
    "chunk64": ([0, 70, 200, 129], 2, 64, [(1, 64), (1, 6), (2, 64), (2, 64), (2, 64), (2, 8), (3, 64), (3, 64), (3, 1)]),
    "chunk704": ([0, 1030, 333, 3628], 2, 704,
                 [(1, 576), (1, 454), (2, 333), (3, 640), (3, 640), (3, 640), (3, 640), (3, 640), (3, 428)]),
}
FORMS = {"fc1": (0, 1, 0), "fc2": (1, 0, 1)}                      # gathered dC rows, gathered A rows, per-row factor
BOTH = {"both": (1, 1, 0), "both_scaled": (1, 1, 1)}


def name(dtype):
    return str(dtype).split(".")[1]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("M", PLAIN_M)
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_plain_rows_one_part(ops, dtype, M):
    with cw.knobs(ops, 0, 0):
        assert cw.run(ops, dtype, M, NK, NK, kernel="staged", splits=1, tag=f"steady/plain/{dtype}/{M}") < 1


@pytest.mark.parametrize("M", [161, 225])
@pytest.mark.parametrize("splits", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_plain_rows_in_parts(ops, dtype, splits, M):
    with cw.knobs(ops, 0, 0):
        assert cw.run(ops, dtype, M, NK, NK, kernel="staged", splits=splits, tag=f"steady/parts/{dtype}/{M}/{splits}") < 1


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_shapes_have_the_units_they_are_chosen_for(ops, shape):
    counts, splits, chunk_want, units_want = SHAPES[shape]
    G, M = len(counts), sum(counts) + SLACK
    chunk, slots = ops.wgrad_plan(M, G, splits, True)
    assert chunk == chunk_want and slots >= len(units_want)
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    arr = (ctypes.c_int32 * (G + 1))(*off)
    got = []
    for u in range(slots):
        g, b, e = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert ops.lib().m3_wgrad_unit_of(arr, G, chunk, u, ctypes.byref(g), ctypes.byref(b), ctypes.byref(e)) == 0
        got.append((g.value, e.value - b.value))
    assert got[:len(units_want)] == units_want
    assert all(x == (-1, 0) for x in got[len(units_want):])


def grouped(ops, dtype, shape, flags, div, tag):
    counts, splits, chunk, _ = SHAPES[shape]
    G, M = len(counts), sum(counts) + SLACK
    assert ops.wgrad_plan(M, G, splits, True)[0] == chunk
    gc, ga, sc = flags
    c_div, a_div = (div if gc else 1), (div if ga else 1)
    c_idx, c_scale, a_idx = cw._gathers(M, gc, ga, sc, c_div, a_div, seed=8 + div)
    with cw.knobs(ops, 0, 0):
        return cw.run(ops, dtype, M, NK, NK, kernel="staged", G=G, counts=counts, splits=splits, c_idx=c_idx, c_div=c_div,
                      c_scale=c_scale, a_idx=a_idx, a_div=a_div, want_db=bool(gc), tag=f"steady/{tag}/{shape}/{dtype}/{div}")


@pytest.mark.parametrize("div", [1, 4, 3])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_grouped_units_fc1_and_fc2(ops, dtype, shape, form, div):
    assert grouped(ops, dtype, shape, FORMS[form], div, form) < 1


@pytest.mark.parametrize("div", [4, 3])
@pytest.mark.parametrize("form", list(BOTH))
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_grouped_units_both_gathers(ops, dtype, form, div):
    assert grouped(ops, dtype, "chunk704", BOTH[form], div, form) < 1
