"""GPU: the batched weight-gradient launch (m3_wgrad_multi, csrc/wgrad_multi.hip) on rows that end in a one-row step.  Its
tile loop is the register-staged kernel's (csrc/wgrad_staged.hip: wgrad_tile_loop); M = 33, 97 and 161 are 2, 4 and 6 steps of
32 rows whose last holds one row, cut into the plan's parts and into 3 (parts of one and two steps, at M = 33 an empty one).
The smallest batches tests/test_wgrad_multi.py builds: the single 8 x 8 problem and its three partial-tile problems.

Checked: bit for bit against the same problems issued one by one through ops.wgrad_tn on the register-staged kernel with
the same number of parts (the same loop over the same steps, the same slab order), and against a float64 product within
kernel_contract's bounds (tests/test_contract_wgrad.py: reference()).  Operands of order 1: a tail row that is not zeroed
or a row added twice moves an output by about 1."""
import pytest
import torch

import kernel_contract as kc
import test_contract_wgrad as cw
import test_wgrad_multi as wm

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("M", [33, 97, 161])
@pytest.mark.parametrize("parts", [0, 3])
@pytest.mark.parametrize("shapes", [wm.SMALL[1:2], wm.SMALL], ids=["one-8x8", "three"])
@pytest.mark.parametrize("dtype", wm.DTYPES, ids=lambda d: str(d).split(".")[1])
def test_multi_on_a_one_row_last_step(ops, dtype, shapes, parts, M):
    plan = ops.wgrad_multi_plan([(N, K, True) for N, K in shapes], M, dtype, parts)
    assert plan.allowed and plan.parts == (parts or plan.parts) and plan.parts >= 1
    cs = wm.case(M, shapes, dtype, seed=700)
    snap = kc.snapshot(**{f"dC{j}": c[0] for j, c in enumerate(cs)}, **{f"A{j}": c[1] for j, c in enumerate(cs)})
    dev = wm.dev()
    multi = [(torch.full((N, K), 3.0, device=dev), torch.full((N,), 3.0, device=dev)) for N, K in shapes]
    ops.wgrad_multi([(c[0], c[1], o[0], o[1], 0) for c, o in zip(cs, multi)], M, parts=parts)
    one = [(torch.full((N, K), 5.0, device=dev), torch.full((N,), 5.0, device=dev)) for N, K in shapes]
    with cw.knobs(ops, 0, 0):
        for c, o in zip(cs, one):
            ops.wgrad_tn(c[0], c[1], o[0], db=o[1], splits=plan.parts)
    torch.cuda.synchronize()
    kc.unchanged(snap)
    grp = torch.zeros(M, dtype=torch.long, device=dev)
    for j, ((N, K), c, m, o) in enumerate(zip(shapes, cs, multi, one)):
        assert kc.same_bits(m[0], o[0]) and kc.same_bits(m[1], o[1]), (j, (N, K))
        W, db, bW, bdb = cw.reference(c[0], c[1], N, K, 1, grp, M, plan.parts, dtype)
        assert kc.assert_within(m[0].view(1, N, K), W, bW, what=f"dW[{j}]") < 1
        assert kc.assert_within(m[1].view(1, N), db, bdb, what=f"db[{j}]") < 1
