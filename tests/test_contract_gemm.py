"""GPU contract tests of m3_gemm_nt, called through the C ABI with padded leading dimensions: every kernel path (register-
staged 128-row tiles with the generic and the staged epilogue and a K tail, fp32 160-row tiles, the LDS-DMA kernel in both
band orders, the 256 x 256 kernel with partial row and column tiles) crossed with every epilogue kind, dense and grouped
(empty groups, 128 / 129-row groups, slack rows past group_offsets[G], gathers with a non-power-of-two divisor, scatters
whose unmapped rows must stay untouched, G > 64).  Every output is guarded (tests/kernel_contract.py), compared
elementwise against fp64 under gemm_bound, and every input keeps its bits."""
from ctypes import byref

import pytest
import torch

import kernel_contract as kc

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
WORST = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    yield _ops
    if WORST:
        print("\nm3_gemm_nt worst err/bound:", max(WORST.values()), max(WORST, key=WORST.get))


def rnd(*shape, dtype=F32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def padded(rows, cols, ld, dtype, scale, seed):
    """an operand [rows, cols] inside rows of ld elements (the padding holds garbage the kernel must not read into C)"""
    full = rnd(rows, ld, dtype=dtype, scale=scale, seed=seed)
    return full[:, :cols]


def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / 2 ** 0.5))


def gelu_grad64(x):
    return 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * torch.pi) ** 0.5


def gemm_raw(ops, *, A, B, C, c_dtype, M, N, K, G=1, dtype, a_row_idx=None, a_row_div=1, c_row_idx=None, bias=None,
             pre=None, gpre=None, res=None, act=0, offsets=None, tile_starts=None, row_scale=None, row_scale_div=1,
             row_scale_idx=None):
    a = ops.GemmArgs()
    ptr = lambda t: t.data_ptr() if t is not None else None          # noqa: E731
    a.A, a.lda = A.data_ptr(), A.stride(0)
    a.a_row_idx, a.a_row_div = ptr(a_row_idx), a_row_div
    a.B, a.ldb = B.data_ptr(), B.stride(-2)
    a.C, a.ldc, a.c_dtype = C.data_ptr(), C.stride(0), ops.dt_code(c_dtype)
    a.c_row_idx = ptr(c_row_idx)
    a.bias = ptr(bias)
    a.pre_out, a.ld_pre = ptr(pre), (pre.stride(0) if pre is not None else 0)
    a.gelu_grad_pre, a.ld_gpre = ptr(gpre), (gpre.stride(0) if gpre is not None else 0)
    a.residual, a.ld_res = ptr(res), (res.stride(0) if res is not None else 0)
    a.act = act
    a.M, a.N, a.K, a.G = M, N, K, G
    a.group_offsets, a.tile_starts = ptr(offsets), ptr(tile_starts)
    a.dtype = ops.dt_code(dtype)
    a.row_scale, a.row_scale_div, a.row_scale_idx = ptr(row_scale), row_scale_div, ptr(row_scale_idx)
    ops.check(ops.lib().m3_gemm_nt(byref(a), ops._stream()), "m3_gemm_nt")


# path id: dtype, M, N, K, A row padding (elements), ldc, gemm_set_big mode (None: default)
PATHS = {
    "f32_staged_ldc+4": (F32, 333, 384, 64, 4, 388, None),
    "f32_tall160": (F32, 11000, 384, 64, 0, 384, None),
    "f16_staged_n132": (F16, 333, 132, 192, 8, 132, None),
    "bf16_staged_ldc+4": (BF16, 333, 384, 192, 8, 388, None),
    "f16_staged_ktail": (F16, 333, 256, 200, 0, 256, None),
    "f32_staged_ktail": (F32, 333, 256, 72, 0, 256, None),       # K * 4 B = two whole 128-byte slices + a 32-byte tail
    "bf16_staged_ktail": (BF16, 333, 256, 200, 0, 256, None),
    "f16_dma_band1_ldc+8": (F16, 1000, 384, 384, 8, 392, None),
    "bf16_dma_band4": (BF16, 300, 1536, 768, 0, 1536, 0),
    "f16_big_k512": (F16, 300, 384, 512, 0, 384, 1),
    "bf16_big_k1024_ldc+8": (BF16, 300, 384, 1024, 8, 392, 1),
}
EPIS = ["plain", "bias", "gelu", "gpre", "res", "res_inplace", "rs_idx_div1_res", "rs_idx_divk", "rs_div3_res", "f32c_gelu"]


def _slots(M, G, counts):
    """host routing of a grouped call: offsets / tile_starts [G+1] and the group of each slot"""
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    ts = [0]
    for c in counts:
        ts.append(ts[-1] + (c + 127) // 128)
    grp = torch.repeat_interleave(torch.arange(G), torch.tensor(counts))
    return (torch.tensor(off, dtype=torch.int32).cuda(), torch.tensor(ts, dtype=torch.int32).cuda(), grp.cuda(), off[-1])


def run_case(ops, dtype, M, N, K, apad, ldc, epi, *, G=1, counts=None, a_div=None, scatter=False, c_rows=None, seed=0):
    """one m3_gemm_nt call with every output guarded; returns the worst err / bound ratio"""
    f64 = torch.float64
    grouped = counts is not None
    if grouped:
        off, ts, grp, Mv = _slots(M, G, counts)
    else:
        off = ts = None
        grp, Mv = torch.zeros(M, dtype=torch.long, device="cuda"), M
    a_rows = M if a_div is None else (M + a_div - 1) // a_div + 3
    A = padded(a_rows, K, K + apad, dtype, 1.0, seed + 1)
    B = rnd(G, N, K, dtype=dtype, scale=0.06, seed=seed + 2)
    a_idx = None
    if a_div is not None:
        g = torch.Generator().manual_seed(seed + 3)
        a_idx = torch.randint(0, a_rows * a_div, (M,), generator=g, dtype=torch.int32).cuda()
    rows_c = M if c_rows is None else c_rows
    c_idx = None
    if scatter:
        g = torch.Generator().manual_seed(seed + 4)
        c_idx = torch.randperm(rows_c, generator=g)[:M].to(torch.int32).cuda()
    arow = (a_idx.long() // a_div)[:Mv] if a_idx is not None else torch.arange(Mv, device="cuda")
    crow = c_idx.long()[:Mv] if c_idx is not None else torch.arange(Mv, device="cuda")
    c_dtype = F32 if (dtype == F32 or epi in ("res", "res_inplace", "rs_idx_div1_res", "rs_div3_res", "f32c_gelu")) else dtype
    bias = rnd(G, N, scale=0.1, seed=seed + 5) if epi in ("bias", "gelu", "res", "rs_idx_div1_res", "rs_idx_divk", "f32c_gelu") else None
    act = ops.M3_ACT_GELU if epi in ("gelu", "f32c_gelu") else 0
    C, c_check = kc.guarded(rows_c, N, c_dtype, ld=ldc)
    pre, pre_check = kc.guarded(rows_c, N, dtype, ld=ldc) if epi == "gelu" else (None, None)
    gpre = padded(rows_c, N, ldc, dtype, 1.0, seed + 6) if epi == "gpre" else None
    res = None
    if epi in ("res", "rs_idx_div1_res", "rs_div3_res"):
        res = padded(rows_c, N, ldc, F32, 1.0, seed + 7)
    res0 = None
    if epi == "res_inplace":
        res0 = rnd(rows_c, N, seed=seed + 7)
        C.copy_(res0)
        res = C
    rs = rs_idx = None
    rs_div = 1
    if epi.startswith("rs_"):
        rs_div = {"rs_idx_div1_res": 1, "rs_idx_divk": 4, "rs_div3_res": 3}[epi]
        if "idx" in epi:
            g = torch.Generator().manual_seed(seed + 8)
            rs_idx = torch.randint(0, rows_c, (M,), generator=g, dtype=torch.int32).cuda()
            srow = rs_idx.long()[:Mv]
        else:
            srow = crow
        rs = (torch.rand(rows_c // rs_div + 1, generator=torch.Generator().manual_seed(seed + 9)) + 0.5).cuda()
    snap = kc.snapshot(A=A, B=B, a_idx=a_idx, c_idx=c_idx, bias=bias, gpre=gpre, rs=rs, rs_idx=rs_idx, off=off, ts=ts,
                       res=res if epi != "res_inplace" else None)
    gemm_raw(ops, A=A, B=B, C=C, c_dtype=c_dtype, M=M, N=N, K=K, G=G, dtype=dtype, a_row_idx=a_idx,
             a_row_div=a_div or 1, c_row_idx=c_idx, bias=bias.view(-1) if bias is not None else None, pre=pre, gpre=gpre,
             res=res, act=act, offsets=off, tile_starts=ts, row_scale=rs, row_scale_div=rs_div, row_scale_idx=rs_idx)
    torch.cuda.synchronize()
    kc.unchanged(snap)
    # fp64 reference, slot by slot
    A64, B64 = A.to(f64)[arow], B.to(f64)
    g_of = grp[:Mv]
    lin = torch.empty(Mv, N, dtype=f64, device="cuda")
    absacc = torch.empty_like(lin)
    for g in range(G):
        sel = (g_of == g).nonzero().flatten()
        if sel.numel():
            lin[sel] = A64[sel] @ B64[g].t()
            absacc[sel] = A64[sel].abs() @ B64[g].abs().t()
    if bias is not None:
        lin = lin + bias.to(f64)[g_of]
    v, gain = lin, torch.ones_like(lin)
    extra = kc.U32 * lin.abs()
    if act:
        v = gelu64(lin)
        gain = gelu_grad64(lin).abs()
        extra = extra * gain + kc.gelu_eval_extra(lin)
    if gpre is not None:
        gg = gelu_grad64(gpre.to(f64)[crow])
        v = v * gg
        # GELU'(pre) evaluated in fp32: a few ulps of its O(1) terms (Phi(x) + x phi(x) cancels for x < 0)
        gain, extra = gain * gg.abs(), extra * gg.abs() + kc.gelu_eval_extra(gpre.to(f64)[crow]) * lin.abs()
    if rs is not None:
        s = rs.to(f64)[srow // rs_div].unsqueeze(1)
        v = v * s
        gain, extra = gain * s.abs(), extra * s.abs() + kc.U32 * v.abs()
    if res is not None:
        r64 = (res0 if res0 is not None else res).to(f64)[crow]
        extra = extra + kc.U32 * (v.abs() + r64.abs())
        v = v + r64
    bound = kc.gemm_bound(None, None, v, c_dtype, K=K, gain=gain, extra=extra, absacc=absacc)
    keep = None
    if c_rows is not None or Mv < M:
        owned = torch.zeros(rows_c, dtype=torch.bool, device="cuda")
        owned[crow] = True
        keep = (~owned).nonzero().flatten()
    c_check(keep_rows=keep, what="C")
    worst = kc.assert_within(C[crow], v, bound, what="C")
    if pre is not None:
        pre_check(keep_rows=keep, what="pre_out")
        pre_bound = kc.gemm_bound(None, None, lin, dtype, K=K, extra=kc.U32 * lin.abs(), absacc=absacc)
        worst = max(worst, kc.assert_within(pre[crow], lin, pre_bound, what="pre_out"))
    return worst


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("path", list(PATHS))
def test_gemm_paths_by_epilogue(ops, path, epi):
    dtype, M, N, K, apad, ldc, big = PATHS[path]
    if big is not None:
        ops.gemm_set_big(big)
    try:
        w = run_case(ops, dtype, M, N, K, apad, ldc, epi)
    finally:
        if big is not None:
            ops.gemm_set_big(-1)
    WORST[f"{path}/{epi}"] = w
    assert w < 1


# grouped: empty first / middle / last groups, 128- and 129-row groups, slack rows past group_offsets[G]
COUNTS = [0, 128, 0, 129, 37, 0]


@pytest.mark.parametrize("dtype,N,K,ldc,big", [(F16, 256, 128, 264, None), (BF16, 132, 192, 132, None),
                                               (F32, 128, 64, 132, None), (F16, 384, 512, 392, 1)])
@pytest.mark.parametrize("mode", ["bias", "gather_div3", "scatter", "gelu", "rs_idx_divk"])
def test_gemm_grouped(ops, dtype, N, K, ldc, big, mode):
    G = len(COUNTS)
    M = sum(COUNTS) + 45                                       # slack rows [group_offsets[G], M): never written
    kw = dict(G=G, counts=COUNTS)
    epi = {"gather_div3": "plain", "scatter": "bias"}.get(mode, mode)
    if mode == "gather_div3":
        kw["a_div"] = 3
    if mode == "scatter":
        kw.update(scatter=True, c_rows=M + 50)
    if big is not None:
        ops.gemm_set_big(big)
    try:
        w = run_case(ops, dtype, M, N, K, 8 if dtype != F32 else 4, ldc, epi, **kw)
    finally:
        if big is not None:
            ops.gemm_set_big(-1)
    WORST[f"grouped/{dtype}/{mode}"] = w


@pytest.mark.parametrize("G", [65, 96])
@pytest.mark.parametrize("dtype", [F16, F32])
def test_gemm_many_groups(ops, G, dtype):
    """G > 64 takes the scalar tile-owner walk (gemm_dev.h: grouped_tile_owner): m3_gemm_nt accepts it and must be right"""
    g = torch.Generator().manual_seed(G)
    counts = torch.randint(0, 40, (G,), generator=g).tolist()
    counts[0] = counts[G // 2] = counts[-1] = 0
    counts[1] = 129
    M = sum(counts) + 17
    w = run_case(ops, dtype, M, 128, 64, 8 if dtype != F32 else 4, 136, "bias", G=G, counts=counts, a_div=2)
    WORST[f"G{G}/{dtype}"] = w


def test_gemm_m0_writes_nothing(ops):
    A = rnd(4, 64, dtype=F16); B = rnd(128, 64, dtype=F16)
    C, check = kc.guarded(4, 128, F16)
    gemm_raw(ops, A=A, B=B, C=C, c_dtype=F16, M=0, N=128, K=64, dtype=F16)
    torch.cuda.synchronize()
    check(keep_rows=range(4))
