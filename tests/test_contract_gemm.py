"""GPU contract tests of m3_gemm_nt, called through the C ABI with padded leading dimensions: every kernel path (register-
staged 128-row tiles with the generic and the staged epilogue and a K tail, fp32 160-row tiles, the LDS-DMA kernel in both
band orders, the 256 x 256 kernel with partial row and column tiles) crossed with every epilogue kind, dense and grouped
(empty groups, 128 / 129-row groups, slack rows past group_offsets[G], gathers with a non-power-of-two divisor, scatters
whose unmapped rows must stay untouched, G > 64).  Every output is guarded (tests/kernel_contract.py), compared
elementwise against fp64 under gemm_bound, and every input keeps its bits.

Every case also states the path it is meant to run - the kernel and the band of the tile order per PATHS / GROUPED entry,
the epilogue kind per (path, epilogue id) - and asserts it through m3_gemm_plan on the very argument struct it launches, so
a threshold that moves in the dispatch fails the case instead of silently moving it to another kernel.  case_args() builds
the same struct from dummy addresses (no GPU): tests/test_launch_paths_cpu.py pins the paths with it before any GPU run,
and tests/test_engine_launch_census_gpu.py checks that every launch of the engine has a case here (cases())."""
from ctypes import byref

import pytest
import torch

import kernel_contract as kc
import launch_signature as ls

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


class Addr:
    """stands for an operand of a struct that is only planned (case_args): an aligned dummy address and a row stride"""

    def __init__(self, ld, addr=ls.DUMMY):
        self.ld, self.addr = ld, addr

    def data_ptr(self):
        return self.addr

    def stride(self, i):
        return self.ld


def gemm_args(ops, *, A, B, C, c_dtype, M, N, K, G=1, dtype, a_row_idx=None, a_row_div=1, c_row_idx=None, bias=None,
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
    return a


def gemm_raw(ops, expect=None, **kw):
    """m3_gemm_nt through the C ABI.  expect: the signature (launch_signature.gemm_signature) and the band the case states
    for itself - asserted on the struct that is launched, before the launch"""
    a = gemm_args(ops, **kw)
    if expect is not None:
        sig, band = expect
        got = ls.gemm_signature(ops, a)
        assert got == sig, f"the case runs\n  {got}\nand states\n  {sig}"
        assert ops.gemm_plan(a).m_band == band
    ops.check(ops.lib().m3_gemm_nt(byref(a), ops._stream()), "m3_gemm_nt")


# path id: dtype, M, N, K, A row padding (elements), ldc, gemm_set_big mode (None: default), then what the path is meant to
# run: the kernel (m3_gemm_plan's names) and the row tiles per band of the tile order
PATHS = {
    "f32_staged_ldc+4": (F32, 333, 384, 64, 4, 388, None, "staged", 1),
    "f32_tall160": (F32, 11000, 384, 64, 0, 384, None, "staged_tall", 1),
    "f16_staged_n132": (F16, 333, 132, 192, 8, 132, None, "staged", 1),
    "bf16_staged_ldc+4": (BF16, 333, 384, 192, 8, 388, None, "staged", 1),
    "f16_staged_ktail": (F16, 333, 256, 200, 0, 256, None, "staged", 1),
    "f32_staged_ktail": (F32, 333, 256, 72, 0, 256, None, "staged", 1),       # K * 4 B = two whole 128-byte slices + a 32-byte tail
    "bf16_staged_ktail": (BF16, 333, 256, 200, 0, 256, None, "staged", 1),
    "f16_dma_band1_ldc+8": (F16, 1000, 384, 384, 8, 392, None, "dma", 1),
    "bf16_dma_band4": (BF16, 300, 1536, 768, 0, 1536, 0, "dma", 4),
    "f16_big_k512": (F16, 300, 384, 512, 0, 384, 1, "big", 1),
    "bf16_big_k1024_ldc+8": (BF16, 300, 384, 1024, 8, 392, 1, "big", 1),
    # the forms the engine's dense launches take (tests/test_engine_launch_census_gpu.py): every leading dimension a multiple
    # of 8, whole 128-byte K slices, N a multiple of the tile - with a partial last row tile (the ViT-Base token counts) and
    # without one (batch 128 x 197 tokens = 197 whole 128-row tiles)
    "f32_staged_vec8": (F32, 333, 384, 64, 0, 384, None, "staged", 1),
    "f32_staged_vec8_m384": (F32, 384, 384, 64, 0, 384, None, "staged", 1),
    "f16_dma_m256": (F16, 256, 384, 384, 0, 384, None, "dma", 1),
    "bf16_dma_m256": (BF16, 256, 384, 384, 0, 384, None, "dma", 1),
    "f16_big_n512": (F16, 300, 512, 512, 0, 512, 1, "big", 1),
    "bf16_big_n512": (BF16, 300, 512, 512, 0, 512, 1, "big", 1),
}
EPIS = ["plain", "bias", "gelu", "gpre", "res", "res_inplace", "rs_idx_div1_res", "rs_idx_divk", "rs_div3_res", "f32c_gelu",
        "rs_div3_bias_res", "gpre_rs_idx", "f32c_bias"]
# what an epilogue id asks of the call
F32C_EPIS = ("res", "res_inplace", "rs_idx_div1_res", "rs_div3_res", "f32c_gelu", "rs_div3_bias_res", "f32c_bias")   # 16-bit operands, fp32 C
BIAS_EPIS = ("bias", "gelu", "res", "rs_idx_div1_res", "rs_idx_divk", "f32c_gelu", "rs_div3_bias_res", "f32c_bias")
RES_EPIS = ("res", "rs_idx_div1_res", "rs_div3_res", "rs_div3_bias_res")                                    # a separate residual
GPRE_EPIS = ("gpre", "gpre_rs_idx")
RS_DIV = {"rs_idx_div1_res": 1, "rs_idx_divk": 4, "rs_div3_res": 3, "rs_div3_bias_res": 3, "gpre_rs_idx": 1}
# the epilogue kind the two LDS-DMA kernels are instantiated for (gemm_dev.h), per epilogue id; the register-staged
# kernels (every fp32 call among them) have the run-time-flag epilogue only: "any".  The kinds do not look at bias (PLAIN,
# RES) or at row_scale (the factor is always applied); an fp32 C without a residual (GELU in front of it, or the patch
# embedding's bias alone) has no kind of its own
EPI_KIND = {"plain": "plain", "bias": "plain", "gelu": "gelu", "gpre": "gpre", "res": "res", "res_inplace": "res",
            "rs_idx_div1_res": "res", "rs_idx_divk": "plain", "rs_div3_res": "res", "f32c_gelu": "any",
            "rs_div3_bias_res": "res", "gpre_rs_idx": "gpre", "f32c_bias": "any"}


def expected_kind(kernel, epi):
    return EPI_KIND[epi] if kernel in ("dma", "big") else "any"


def case_args(ops, dtype, M, N, K, apad, ldc, epi, *, G=1, counts=None, a_div=None, scatter=False, c_rows=None, seed=0):
    """the argument struct of run_case's call with dummy addresses in place of the operands run_case allocates: the same
    option pattern, the same leading dimensions.  Host only"""
    grouped = counts is not None
    c_dtype = F32 if (dtype == F32 or epi in F32C_EPIS) else dtype
    C = ls.DUMMY * 2
    on = lambda cond, ld=0, addr=ls.DUMMY: Addr(ld, addr) if cond else None       # noqa: E731
    return gemm_args(ops, A=Addr(K + apad), B=Addr(K), C=Addr(ldc, C), c_dtype=c_dtype, M=M, N=N, K=K, G=G, dtype=dtype,
                     a_row_idx=on(a_div is not None), a_row_div=a_div or 1, c_row_idx=on(scatter), bias=on(epi in BIAS_EPIS),
                     pre=on(epi == "gelu", ldc), gpre=on(epi in GPRE_EPIS, ldc),
                     res=on(epi in RES_EPIS, ldc) if epi != "res_inplace" else Addr(ldc, C),
                     act=ops.M3_ACT_GELU if epi in ("gelu", "f32c_gelu") else 0, offsets=on(grouped), tile_starts=on(grouped),
                     row_scale=on(epi in RS_DIV), row_scale_div=RS_DIV.get(epi, 1), row_scale_idx=on(epi in RS_DIV and "idx" in epi))


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


def run_case(ops, dtype, M, N, K, apad, ldc, epi, *, G=1, counts=None, a_div=None, scatter=False, c_rows=None, seed=0,
             kernel=None, band=1):
    """one m3_gemm_nt call with every output guarded; returns the worst err / bound ratio.  kernel / band: the path the
    case states for itself, asserted on the launched struct together with the option pattern case_args gives the case"""
    want = ls.gemm_signature(ops, case_args(ops, dtype, M, N, K, apad, ldc, epi, G=G, counts=counts, a_div=a_div, scatter=scatter,
                                            c_rows=c_rows))
    assert (want.get("kernel"), want.get("epi")) == (kernel, expected_kind(kernel, epi)), f"{want} is not {kernel} / {expected_kind(kernel, epi)}"
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
    c_dtype = F32 if (dtype == F32 or epi in F32C_EPIS) else dtype
    bias = rnd(G, N, scale=0.1, seed=seed + 5) if epi in BIAS_EPIS else None
    act = ops.M3_ACT_GELU if epi in ("gelu", "f32c_gelu") else 0
    C, c_check = kc.guarded(rows_c, N, c_dtype, ld=ldc)
    pre, pre_check = kc.guarded(rows_c, N, dtype, ld=ldc) if epi == "gelu" else (None, None)
    gpre = padded(rows_c, N, ldc, dtype, 1.0, seed + 6) if epi in GPRE_EPIS else None
    res = None
    if epi in RES_EPIS:
        res = padded(rows_c, N, ldc, F32, 1.0, seed + 7)
    res0 = None
    if epi == "res_inplace":
        res0 = rnd(rows_c, N, seed=seed + 7)
        C.copy_(res0)
        res = C
    rs = rs_idx = None
    rs_div = 1
    if epi in RS_DIV:
        rs_div = RS_DIV[epi]
        if "idx" in epi:
            g = torch.Generator().manual_seed(seed + 8)
            rs_idx = torch.randint(0, rows_c, (M,), generator=g, dtype=torch.int32).cuda()
            srow = rs_idx.long()[:Mv]
        else:
            srow = crow
        rs = (torch.rand(rows_c // rs_div + 1, generator=torch.Generator().manual_seed(seed + 9)) + 0.5).cuda()
    snap = kc.snapshot(A=A, B=B, a_idx=a_idx, c_idx=c_idx, bias=bias, gpre=gpre, rs=rs, rs_idx=rs_idx, off=off, ts=ts,
                       res=res if epi != "res_inplace" else None)
    gemm_raw(ops, (want, band), A=A, B=B, C=C, c_dtype=c_dtype, M=M, N=N, K=K, G=G, dtype=dtype, a_row_idx=a_idx,
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
    dtype, M, N, K, apad, ldc, big, kernel, band = PATHS[path]
    if big is not None:
        ops.gemm_set_big(big)
    try:
        w = run_case(ops, dtype, M, N, K, apad, ldc, epi, kernel=kernel, band=band)
    finally:
        if big is not None:
            ops.gemm_set_big(-1)
    WORST[f"{path}/{epi}"] = w
    assert w < 1


# grouped: empty first / middle / last groups, 128- and 129-row groups, slack rows past group_offsets[G]
COUNTS = [0, 128, 0, 129, 37, 0]
# grouped path id: dtype, N, K, ldc, gemm_set_big mode, the kernel it is meant to run (band 1 everywhere)
GROUPED = {
    "f16_dma": (F16, 256, 128, 264, None, "dma"),
    "bf16_staged_n132": (BF16, 132, 192, 132, None, "staged"),
    "f32_staged_ldc+4": (F32, 128, 64, 132, None, "staged"),
    "f16_big": (F16, 384, 512, 392, 1, "big"),
    # the forms of the engine's grouped launches: leading dimensions multiples of 8, N a multiple of the tile
    "f32_staged_vec8": (F32, 128, 64, 136, None, "staged"),
    "bf16_dma": (BF16, 256, 128, 264, None, "dma"),
    "f16_big_n512": (F16, 512, 512, 520, 1, "big"),
    "bf16_big_n512": (BF16, 512, 512, 520, 1, "big"),
}
# grouped mode: epilogue id, run_case options.  The last four are the expert FFN's launches as the engine makes them
# (engine.py: _ffn_fwd / _ffn_bwd): FC1 gathers its rows through the slot map (divisor k = 4) and writes GELU and the
# pre-activations, the FC2 input gradient multiplies by GELU' and by the gate score taken through the slot map while it gathers,
# the FC1 input gradient scatters without a bias
GROUPED_MODES = {
    "bias": ("bias", {}),
    "gather_div3": ("plain", dict(a_div=3)),
    "scatter": ("bias", dict(scatter=True, c_extra=50)),
    "gelu": ("gelu", {}),
    "rs_idx_divk": ("rs_idx_divk", {}),
    "gather4_gelu": ("gelu", dict(a_div=4)),
    "gather4_gpre_rs_idx": ("gpre_rs_idx", dict(a_div=4)),
    "scatter_plain": ("plain", dict(scatter=True, c_extra=50)),
}


def grouped_case(path, mode):
    """(positional arguments, keyword arguments) of run_case / case_args for a grouped case"""
    dtype, N, K, ldc, big, kernel = GROUPED[path]
    epi, opt = GROUPED_MODES[mode]
    opt = dict(opt)
    G = len(COUNTS)
    M = sum(COUNTS) + 45                                       # slack rows [group_offsets[G], M): never written
    kw = dict(G=G, counts=COUNTS)
    extra = opt.pop("c_extra", None)
    if extra is not None:
        kw["c_rows"] = M + extra
    kw.update(opt)
    return (dtype, M, N, K, 8 if dtype != F32 else 4, ldc, epi), kw


def _run_grouped(ops, path, mode):
    big, kernel = GROUPED[path][4:6]
    args, kw = grouped_case(path, mode)
    if big is not None:
        ops.gemm_set_big(big)
    try:
        w = run_case(ops, *args, kernel=kernel, **kw)
    finally:
        if big is not None:
            ops.gemm_set_big(-1)
    WORST[f"grouped/{path}/{mode}"] = w
    assert w < 1


@pytest.mark.parametrize("dtype,N,K,ldc,big", [(F16, 256, 128, 264, None), (BF16, 132, 192, 132, None),
                                               (F32, 128, 64, 132, None), (F16, 384, 512, 392, 1)])
@pytest.mark.parametrize("mode", ["bias", "gather_div3", "scatter", "gelu", "rs_idx_divk"])
def test_gemm_grouped(ops, dtype, N, K, ldc, big, mode):
    (path,) = [p for p, v in GROUPED.items() if v[:5] == (dtype, N, K, ldc, big)]
    _run_grouped(ops, path, mode)


OLD_GROUPED = [(p, m) for p in ("f16_dma", "bf16_staged_n132", "f32_staged_ldc+4", "f16_big")
               for m in ("bias", "gather_div3", "scatter", "gelu", "rs_idx_divk")]                  # test_gemm_grouped's cases


@pytest.mark.parametrize("path,mode", [(p, m) for p in GROUPED for m in GROUPED_MODES if (p, m) not in OLD_GROUPED])
def test_gemm_grouped_as_the_engine_launches(ops, path, mode):
    """the grouped paths and modes test_gemm_grouped does not run: the expert FFN's launches (GROUPED_MODES) on every path,
    and every mode on the paths that have the engine's operand layout"""
    _run_grouped(ops, path, mode)


def many_groups_case(G, dtype):
    g = torch.Generator().manual_seed(G)
    counts = torch.randint(0, 40, (G,), generator=g).tolist()
    counts[0] = counts[G // 2] = counts[-1] = 0
    counts[1] = 129
    M = sum(counts) + 17
    return (dtype, M, 128, 64, 8 if dtype != F32 else 4, 136, "bias"), dict(G=G, counts=counts, a_div=2)


MANY_GROUPS = [(G, dtype) for dtype in (F16, F32) for G in (65, 96)]


@pytest.mark.parametrize("G", [65, 96])
@pytest.mark.parametrize("dtype", [F16, F32])
def test_gemm_many_groups(ops, G, dtype):
    """G > 64 takes the scalar tile-owner walk (gemm_dev.h: grouped_tile_owner): m3_gemm_nt accepts it and must be right.
    K = 64: fp16 rows of 128 bytes go to the LDS-DMA kernel, fp32 to the register-staged one"""
    args, kw = many_groups_case(G, dtype)
    w = run_case(ops, *args, kernel="dma" if dtype == F16 else "staged", **kw)
    WORST[f"G{G}/{dtype}"] = w


def cases():
    """every (case id, gemm_set_big mode, stated kernel, stated band, stated epilogue kind, case_args positional, keyword)
    of this module's tables: what the CPU test pins and the engine census is compared with"""
    for path, (dtype, M, N, K, apad, ldc, big, kernel, band) in PATHS.items():
        for epi in EPIS:
            yield f"{path}/{epi}", big, kernel, band, expected_kind(kernel, epi), (dtype, M, N, K, apad, ldc, epi), {}
    for path in GROUPED:
        for mode in GROUPED_MODES:
            args, kw = grouped_case(path, mode)
            yield f"grouped/{path}/{mode}", GROUPED[path][4], GROUPED[path][5], 1, expected_kind(GROUPED[path][5], args[-1]), args, kw
    for G, dtype in MANY_GROUPS:
        args, kw = many_groups_case(G, dtype)
        kernel = "dma" if dtype == F16 else "staged"
        yield f"G{G}/{dtype}", None, kernel, 1, expected_kind(kernel, "bias"), args, kw


def case_signatures(ops):
    """{case id: (signature, band)} from dummy structs under each case's gemm_set_big mode.  Host only"""
    out = {}
    for cid, big, kernel, band, kind, args, kw in cases():
        if big is not None:
            ops.gemm_set_big(big)
        try:
            a = case_args(ops, *args, **kw)
            out[cid] = (ls.gemm_signature(ops, a), ops.gemm_plan(a).m_band)
        finally:
            if big is not None:
                ops.gemm_set_big(-1)
    return out


def test_gemm_m0_writes_nothing(ops):
    A = rnd(4, 64, dtype=F16); B = rnd(128, 64, dtype=F16)
    C, check = kc.guarded(4, 128, F16)
    gemm_raw(ops, A=A, B=B, C=C, c_dtype=F16, M=0, N=128, K=64, dtype=F16)
    torch.cuda.synchronize()
    check(keep_rows=range(4))
