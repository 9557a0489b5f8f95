"""The prologue of the LDS-DMA GEMM kernel (gemm_dma.hip) at the smallest shapes at which it can go wrong: the B pieces of
the first K slice leave before the tile's rows are known, the A pieces behind one round trip of every index, the per-row
factor through a shift or a 32-bit division, one slice / two slices / the benchmark's six, tiles whose rows and columns are
clamped, a group that is empty, has one row, ends inside a tile or fills one.

Every case states its kernel and epilogue kind and asserts them through m3_gemm_plan on the struct it launches - it cannot
pass on the register-staged kernel.  Outputs are guarded (tests/kernel_contract.py: nothing outside the owned rows may
change, rows past M / past the last group / not scattered to keep the sentinel) and compared elementwise with an fp64
reference computed on the host from the rounded operands, under kernel_contract.gemm_bound - the bound of the contract
tests, with the same terms per epilogue option."""
from ctypes import byref
from functools import lru_cache

import pytest
import torch

import kernel_contract as kc

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
F64 = torch.float64


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    return _ops


def rnd(*shape, dtype=F32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / 2 ** 0.5))


def gelu_grad64(x):
    return 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * torch.pi) ** 0.5


@lru_cache(maxsize=None)
def operands(dtype, a_rows, N, K, G):
    """(A [a_rows, K], B [G, N, K]) rounded to dtype, on the host, and their fp64 copies - made once per shape"""
    A = rnd(a_rows, K, dtype=dtype, seed=1)
    B = rnd(G, N, K, dtype=dtype, scale=0.06, seed=2)
    return A, B, A.to(F64), B.to(F64)


def run(ops, dtype, kind, M, N, K, *, counts=None, a_div=None, scatter=False, rs=None, bias=None, slack=0):
    """one m3_gemm_nt call of the stated kind; rs: None | "idx" | an integer row_scale_div.  counts: the groups' sizes
    (M = their sum + slack rows that belong to no group).  Returns the worst err / bound"""
    from m3vit_amd import _lib
    grouped = counts is not None
    G = len(counts) if grouped else 1
    Mv = sum(counts) if grouped else M                       # rows that are computed
    if grouped:
        M = Mv + slack
    bias = kind in ("gelu", "res") if bias is None else bias
    c_dtype = F32 if kind == "res" else dtype
    rows_c = M + 50 if scatter else M
    a_rows = M if a_div is None else (M + a_div - 1) // a_div + 3
    A, B, A64, B64 = operands(dtype, a_rows, N, K, G)
    gen = torch.Generator().manual_seed(1000 * M + N + K)
    a_idx = torch.randint(0, a_rows * a_div, (M,), generator=gen, dtype=torch.int32) if a_div is not None else None
    c_idx = torch.randperm(rows_c, generator=gen)[:M].to(torch.int32) if scatter else None
    arow = (a_idx.long() // a_div)[:Mv] if a_idx is not None else torch.arange(Mv)
    crow = c_idx.long()[:Mv] if c_idx is not None else torch.arange(Mv)
    grp = torch.repeat_interleave(torch.arange(G), torch.tensor(counts)) if grouped else torch.zeros(Mv, dtype=torch.long)
    off = ts = None
    if grouped:
        off = torch.tensor([sum(counts[:i]) for i in range(G + 1)], dtype=torch.int32)
        ts = torch.tensor([sum((c + 127) // 128 for c in counts[:i]) for i in range(G + 1)], dtype=torch.int32)
    bias_t = rnd(G, N, scale=0.1, seed=5) if bias else None
    gpre = rnd(rows_c, N, dtype=dtype, seed=6) if kind == "gpre" else None
    res = rnd(rows_c, N, seed=7) if kind == "res" else None
    rs_t = rs_idx = None
    rs_div = 1
    if rs is not None:
        if rs == "idx":
            rs_idx = torch.randint(0, rows_c, (M,), generator=gen, dtype=torch.int32)
            srow = rs_idx.long()[:Mv]
        else:
            rs_div, srow = rs, crow
        rs_t = torch.rand(rows_c // rs_div + 1, generator=gen) + 0.5
        srow = srow // rs_div

    dev = lambda t: t.cuda() if t is not None else None      # noqa: E731
    d = {k: dev(v) for k, v in dict(A=A, B=B, a_idx=a_idx, c_idx=c_idx, off=off, ts=ts, bias=bias_t, gpre=gpre, res=res,
                                    rs=rs_t, rs_idx=rs_idx).items()}
    C, c_check = kc.guarded(rows_c, N, c_dtype)
    pre, pre_check = kc.guarded(rows_c, N, dtype) if kind == "gelu" else (None, None)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    a = ops.GemmArgs()
    a.A, a.lda = d["A"].data_ptr(), K
    a.a_row_idx, a.a_row_div = ptr(d["a_idx"]), a_div or 1
    a.B, a.ldb = d["B"].data_ptr(), K
    a.C, a.ldc, a.c_dtype = C.data_ptr(), C.stride(0), ops.dt_code(c_dtype)
    a.c_row_idx = ptr(d["c_idx"])
    a.bias = ptr(d["bias"])
    a.pre_out, a.ld_pre = ptr(pre), (pre.stride(0) if pre is not None else 0)
    a.gelu_grad_pre, a.ld_gpre = ptr(d["gpre"]), (N if gpre is not None else 0)
    a.residual, a.ld_res = ptr(d["res"]), (N if res is not None else 0)
    a.act = ops.M3_ACT_GELU if kind == "gelu" else 0
    a.M, a.N, a.K, a.G = M, N, K, G
    a.group_offsets, a.tile_starts = ptr(d["off"]), ptr(d["ts"])
    a.dtype = ops.dt_code(dtype)
    a.row_scale, a.row_scale_div, a.row_scale_idx = ptr(d["rs"]), rs_div, ptr(d["rs_idx"])
    plan = ops.gemm_plan(a)
    assert (_lib.GEMM_KERNELS[plan.kernel], _lib.GEMM_EPILOGUES[plan.epilogue]) == ("dma", kind), \
        f"the case runs {_lib.GEMM_KERNELS[plan.kernel]} / {_lib.GEMM_EPILOGUES[plan.epilogue]}, not dma / {kind}"
    assert (plan.tile_m, plan.tile_n) == (128, 128)
    snap = kc.snapshot(**{k: v for k, v in d.items() if v is not None})
    ops.check(ops.lib().m3_gemm_nt(byref(a), ops._stream()), "m3_gemm_nt")
    torch.cuda.synchronize()
    kc.unchanged(snap)

    # fp64 on the host, slot by slot
    Ag = A64[arow]
    lin = torch.empty(Mv, N, dtype=F64)
    absacc = torch.empty_like(lin)
    for g in range(G):
        sel = (grp == g).nonzero().flatten()
        if sel.numel():
            lin[sel] = Ag[sel] @ B64[g].t()
            absacc[sel] = Ag[sel].abs() @ B64[g].abs().t()
    if bias_t is not None:
        lin = lin + bias_t.to(F64)[grp]
    v, gain, extra = lin, torch.ones_like(lin), kc.U32 * lin.abs()
    if kind == "gelu":
        v, gain = gelu64(lin), gelu_grad64(lin).abs()
        extra = extra * gain + kc.gelu_eval_extra(lin)
    if gpre is not None:
        p64 = gpre.to(F64)[crow]
        gg = gelu_grad64(p64)
        v = v * gg
        gain, extra = gain * gg.abs(), extra * gg.abs() + kc.gelu_eval_extra(p64) * lin.abs()
    if rs_t is not None:
        s = rs_t.to(F64)[srow].unsqueeze(1)
        v = v * s
        gain, extra = gain * s.abs(), extra * s.abs() + kc.U32 * v.abs()
    if res is not None:
        r64 = res.to(F64)[crow]
        extra = extra + kc.U32 * (v.abs() + r64.abs())
        v = v + r64
    bound = kc.gemm_bound(None, None, v, c_dtype, K=K, gain=gain, extra=extra, absacc=absacc)
    owned = torch.zeros(rows_c, dtype=torch.bool)
    owned[crow] = True
    keep = (~owned).nonzero().flatten()
    c_check(keep_rows=keep, what="C")
    worst = kc.assert_within(C[crow.cuda()], v, bound, what="C") if Mv else 0.0
    if pre is not None:
        pre_check(keep_rows=keep, what="pre_out")
        pre_bound = kc.gemm_bound(None, None, lin, dtype, K=K, extra=kc.U32 * lin.abs(), absacc=absacc)
        if Mv:
            worst = max(worst, kc.assert_within(pre[crow.cuda()], lin, pre_bound, what="pre_out"))
    return worst


# all four kinds in fp16, PLAIN and RES in bf16
KINDS = [(F16, "plain"), (F16, "gelu"), (F16, "gpre"), (F16, "res"), (BF16, "plain"), (BF16, "res")]
KIND_IDS = [f"{'f16' if d == F16 else 'bf16'}-{k}" for d, k in KINDS]


# dense: a one-row tile, a tile one row short, one row into a second tile; a clamped second column tile (136) and whole
# column tiles (384); one K slice (the loop runs on the prologue's slice alone), two, the benchmark's six
@pytest.mark.parametrize("K", [64, 128, 384])
@pytest.mark.parametrize("N", [136, 384])
@pytest.mark.parametrize("M", [1, 127, 129])
@pytest.mark.parametrize("dtype,kind", KINDS, ids=KIND_IDS)
def test_dense(ops, dtype, kind, M, N, K):
    assert run(ops, dtype, kind, M, N, K) < 1


# the per-row factor on dense rows: through row_scale_idx (the gate score's path), through row_scale_div = 197 (DropPath: one
# factor per image of 197 tokens - not a power of two, the 32-bit division; M = 400 spans three images and four row tiles)
# and = 1 (the shift by 0)
@pytest.mark.parametrize("K", [64, 384])
@pytest.mark.parametrize("M", [1, 127, 129, 400])
@pytest.mark.parametrize("rs", ["idx", 197, 1])
@pytest.mark.parametrize("dtype,kind", [(F16, "res"), (F16, "gpre"), (F16, "plain"), (BF16, "res")],
                         ids=["f16-res", "f16-gpre", "f16-plain", "bf16-res"])
def test_dense_row_factor(ops, dtype, kind, rs, M, K):
    assert run(ops, dtype, kind, M, 136, K, rs=rs) < 1


# grouped: an empty expert, a one-row expert, a group that ends inside its second tile, a full tile; 45 slack rows behind
# the last group.  The forms are the expert FFN's launches (FC1 forward: gathered A, GELU; FC2 input gradient: gathered A,
# GELU', gate score through row_scale_idx; FC2 forward: scattered C, bias; FC1 input gradient: scattered C) and the same
# options with the divisor that is not a power of two, on the other kinds and in bf16
COUNTS = (0, 1, 130, 128)
GROUPED = {
    "f16-gelu-gather4": (F16, "gelu", dict(a_div=4)),
    "f16-gelu-gather3": (F16, "gelu", dict(a_div=3)),
    "f16-gpre-gather4-rsidx": (F16, "gpre", dict(a_div=4, rs="idx")),
    "f16-gpre-gather3-rs197": (F16, "gpre", dict(a_div=3, rs=197)),
    "f16-plain-scatter-bias": (F16, "plain", dict(scatter=True, bias=True)),
    "f16-plain-scatter": (F16, "plain", dict(scatter=True)),
    "f16-plain-gather3-scatter-rs1": (F16, "plain", dict(a_div=3, scatter=True, rs=1)),
    "f16-res-gather4-rsidx": (F16, "res", dict(a_div=4, rs="idx")),
    "bf16-plain-gather4-scatter": (BF16, "plain", dict(a_div=4, scatter=True)),
    "bf16-res-gather3-rs197": (BF16, "res", dict(a_div=3, rs=197)),
}


@pytest.mark.parametrize("K", [64, 128, 384])
@pytest.mark.parametrize("N", [136, 384])
@pytest.mark.parametrize("form", list(GROUPED))
def test_grouped(ops, form, N, K):
    dtype, kind, opt = GROUPED[form]
    assert run(ops, dtype, kind, 0, N, K, counts=list(COUNTS), slack=45, **opt) < 1


def test_grouped_all_empty_but_one_row(ops):
    """one live row tile in the whole launch: every other workgroup of the grid leaves before it requests anything"""
    assert run(ops, F16, "gelu", 0, 136, 128, counts=[0, 0, 1, 0], slack=3, a_div=4) < 1
