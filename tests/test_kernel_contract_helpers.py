"""CPU: the checks of tests/kernel_contract.py have teeth.  A plain torch stand-in for a GEMM kernel (fp16 operands, fp32
arithmetic, + bias, GELU, one rounding to fp16 on the store) passes every check; each injected defect - the stray writes,
the wrong values confined to a few elements and the stale workspace read the GPU contract tests guard against - is caught,
and at least one of them passes the suite's older relative-L2 check, which is why the elementwise one exists."""
import pytest
import torch

import kernel_contract as kc

M, N, K, LD = 1000, 384, 384, 392
DEV = "cpu"


def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / 2 ** 0.5))


def gelu_grad64(x):
    return 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * torch.pi) ** 0.5


def rel(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def operands():
    g = torch.Generator().manual_seed(0)
    A = torch.randn(M, K, generator=g).half()
    B = (torch.randn(N, K, generator=g) * 0.05).half()
    bias = torch.randn(N, generator=g) * 0.1
    lin = A.double() @ B.double().t() + bias.double()
    ref = gelu64(lin)
    bound = kc.gemm_bound(A.double(), B.double(), ref, torch.float16, gain=gelu_grad64(lin).abs(),
                          extra=kc.U32 * lin.abs() + kc.gelu_eval_extra(lin))
    return A, B, bias, ref, bound


def kernel(A, B, bias, C, defect=None, c_row_idx=None, ws=None):
    """the stand-in: C[crow(m)] = fp16(GELU(A B^T + bias)) in fp32; `defect` injects one fault"""
    Kd = A.shape[1]
    acc = A.float() @ B.float().t()
    if defect == "k_slice":                                   # the last 8-wide K slice dropped for the first row tile
        acc[:128] -= A[:128, Kd - 8:].float() @ B[:, Kd - 8:].float().t()
    lin = acc + bias
    if defect == "bias_vec":                                  # bias lost from one 4-column vector of one row
        lin[517, 100:104] -= bias[100:104]
    if ws is not None:                                        # the per-column sum of the result goes through a workspace
        ws.copy_(lin.sum(0)[: ws.numel()])
        n = ws.numel() + (1 if defect == "ws_overread" else 0)
        lin[0, :n] += 0 * torch.as_strided(ws, (n,), (1,))
    out = torch.nn.functional.gelu(lin).half()
    rows = torch.arange(A.shape[0]) if c_row_idx is None else c_row_idx.clone()
    if defect == "scatter":                                   # one row lands on a destination it does not own
        rows[7] = C.shape[0] - 1
    C[rows] = out
    full = torch.as_strided(C, (C.shape[0] + 1, C.stride(0)), (C.stride(0), 1))
    if defect == "row_past_m":
        full[C.shape[0], 0] = 1.0
    if defect == "ld_pad":
        full[3, C.shape[1]] = 1.0


def run(operands, defect=None, scatter=False, ws=False):
    """returns (passes elementwise + guards, passes rel < 1e-3)"""
    A, B, bias, ref, bound = operands
    rows = M + 24 if scatter else M
    C, check = kc.guarded(rows, N, torch.float16, ld=LD, device=DEV)
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(1))[:M] if scatter else None
    W, wcheck = kc.guarded_ws(N - 8, device=DEV) if ws else (None, None)
    snap = kc.snapshot(A=A, B=B, bias=bias)
    kernel(A, B, bias, C, defect, perm, W)
    kc.unchanged(snap)
    got = C[perm] if scatter else C
    ok_rel = rel(got, ref) < 1e-3
    try:
        keep = None
        if scatter:
            mask = torch.ones(rows, dtype=torch.bool); mask[perm] = False
            keep = mask.nonzero().flatten()
        check(keep_rows=keep)
        if wcheck:
            wcheck()
        kc.assert_within(got, ref, bound)
    except AssertionError:
        return False, ok_rel
    return True, ok_rel


def test_the_clean_kernel_passes_every_check(operands):
    for kw in ({}, {"scatter": True}, {"ws": True}):
        assert run(operands, **kw) == (True, True), kw
    A, B, bias, ref, bound = operands
    C, _ = kc.guarded(M, N, torch.float16, ld=LD, device=DEV)
    kernel(A, B, bias, C)
    worst = kc.assert_within(C, ref, bound)
    assert 1e-2 < worst < 1, f"the bound is not tight enough to mean anything: worst err/bound {worst}"


@pytest.mark.parametrize("defect,kw", [("row_past_m", {}), ("ld_pad", {}), ("bias_vec", {}), ("k_slice", {}),
                                       ("scatter", {"scatter": True}), ("ws_overread", {"ws": True})])
def test_each_injected_defect_is_caught(operands, defect, kw):
    ok, _ = run(operands, defect, **kw)
    assert not ok, f"defect {defect} went unnoticed"


def test_relative_l2_alone_misses_defects_the_contract_catches(operands):
    missed = [d for d in ("row_past_m", "ld_pad", "bias_vec") if run(operands, d)[1]]
    assert "bias_vec" in missed and len(missed) == 3, missed


def test_guard_reports_the_first_bad_element():
    C, check = kc.guarded(5, 12, torch.float32, ld=16, device=DEV)
    C.fill_(0)
    check()
    torch.as_strided(C, (5, 16), (16, 1))[2, 13] = 0
    with pytest.raises(AssertionError, match=r"row 2, col 13.*row padding"):
        check()
    C2, check2 = kc.guarded(3, 4, torch.int32, device=DEV)
    C2[0] = 1
    with pytest.raises(AssertionError, match="does not own"):
        check2(keep_rows=[0])
    check2(keep_rows=[1, 2])
    assert C2.data_ptr() % kc.ALIGN == 0


def test_sentinels_are_nans_torch_does_not_produce():
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        s = kc.sentinel_like(torch.empty(1, dtype=dt))
        assert bool(torch.isnan(s).all())
        assert not kc.same_bits(s, torch.full((1,), float("nan"), dtype=dt))
        assert kc.same_bits(s, s.clone())
