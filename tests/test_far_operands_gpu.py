"""GPU: m3_gemm_nt, m3_wgrad_tn, m3_wgrad_multi, m3_colsum and m3_conv3x3_fwd on operands that reach past 2 and 4 GiB from their base.

The kernels form addresses in 32 bits wherever the host rules allow it (include/m3vit_hip.h: the reach of m3_gemm_nt, the
step-downs of m3_wgrad_kernel; tests/test_far_operands_cpu.py pins the rules themselves).  Everywhere else in the suite an
operand is a few MB, so a signed offset between 2 and 4 GiB, a 32-bit product where 64 bits are needed or a stride with bit
31 set would pass.  Here an operand is a window of rows megabytes apart inside one unfilled allocation
(kernel_contract.far_rows): a few hundred KB are written, the addresses are real.

Every case
  (a) asserts, through m3_gemm_plan / m3_wgrad_kernel on the struct it launches, the kernel it states for itself;
  (b) runs the call twice on the same values - far operands, then compact ones - and asserts equal plans and BIT-IDENTICAL
      results: an address must not enter the arithmetic;
  (c) holds the far result elementwise to the fp64 reference under the bounds of test_contract_gemm / test_contract_wgrad.
Inputs keep their bits; a far output's whole allocation starts as the sentinel, and everything between its rows must still
be the sentinel afterwards (a store whose offset wrapped at 32 bits lands inside this same allocation).

Each case asserts on the host the row offsets it is about (which rows start above 2^31 / 2^32, that every row tile of a
gathered call reads on both sides of the line).  Memory: at most 8 GiB + small per test (the two-group weight); a test
skips only when the card has less free than it needs plus 2 GiB."""
import ctypes
import gc
from ctypes import byref

import pytest
import torch

import kernel_contract as kc
import launch_signature as ls
import test_contract_gemm as cg
import test_contract_wgrad as cw

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
ES = {F32: 4, F16: 2, BF16: 2}
GIB2, GIB4 = 1 << 31, 1 << 32
MIB = 1 << 20


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _release():
    yield
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def need(nbytes):
    """skip (naming the amount) when the card cannot hold the case's far allocations beside 2 GiB of everything else"""
    assert nbytes <= 10 << 30, "a case may hold 10 GiB at most"
    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + (2 << 30):
        pytest.skip(f"needs {nbytes / 2 ** 30:.2f} GiB + 2 GiB of free device memory, {free / 2 ** 30:.2f} GiB are free")


def span(rows, ld_b, row_bytes):
    return (rows - 1) * ld_b + row_bytes


def note(case, kernel, **top):
    """one line per case for the log: the kernel reached and the highest byte offset touched per far operand"""
    print(f"\nFAR {case}: kernel {kernel}; highest byte offset " + ", ".join(f"{k} {v:,}" for k, v in top.items()))


def sent_rows(rows, cols, dtype, ld):
    """a compact output [rows, cols] with row stride ld, sentinel-filled"""
    buf = torch.empty(rows, ld, dtype=dtype, device="cuda")
    buf.copy_(kc.sentinel_like(buf))
    return buf[:, :cols]


def straddling(M, ld_b, tile, seed, line=GIB2):
    """a permutation of the M rows of a far operand whose every `tile`-row tile holds rows on both sides of `line` and whose
    first tile holds row M - 1 - asserted, not hoped for"""
    g = torch.Generator().manual_seed(seed)
    src = torch.randperm(M, generator=g)
    j = int((src == M - 1).nonzero())
    src[[0, j]] = src[[j, 0]]
    off = src * ld_b
    for t0 in range(0, M, tile):
        o = off[t0:t0 + tile]
        assert bool((o < line).any()) and bool((o >= line).any()), f"tile at row {t0} does not straddle the line"
    assert int(src.max()) == M - 1 and int(src[0]) == M - 1
    return src


# ================================================================================================= m3_gemm_nt
class GemmVals:
    """the values of one GEMM case (compact tensors on the GPU) and its option pattern: every layout of the case is filled
    from them"""

    def __init__(self, path, epi="plain", *, counts=None, a_src=None, a_div=1, c_perm=None, ldc=None, seed=0):
        self.path, self.epi = path, epi
        self.dtype, self.M, self.N, self.K, self.apad, self.ldc, self.big, self.kernel, self.band = cg.PATHS[path]
        if ldc is not None:
            self.ldc = ldc
        dtype, M, N, K = self.dtype, self.M, self.N, self.K
        self.counts = counts
        self.G = len(counts) if counts else 1
        assert counts is None or sum(counts) == M
        self.c_dtype = F32 if (dtype == F32 or epi in cg.F32C_EPIS) else dtype
        self.A = cg.rnd(M, K, dtype=dtype, seed=seed + 1)
        self.B = cg.rnd(self.G * N, K, dtype=dtype, scale=0.06, seed=seed + 2)
        self.bias = cg.rnd(self.G, N, scale=0.1, seed=seed + 5) if epi in cg.BIAS_EPIS else None
        self.gpre = cg.rnd(M, N, dtype=dtype, seed=seed + 6) if epi in cg.GPRE_EPIS else None
        self.res = cg.rnd(M, N, seed=seed + 7) if (epi in cg.RES_EPIS or epi == "res_inplace") else None
        self.act = ops_act(epi)
        self.a_div = a_div
        self.a_idx = None
        if a_src is not None:                                   # slot m reads source row a_src[m] = a_idx[m] // a_div
            self.a_idx = (a_src * a_div + torch.arange(M) % a_div).to(torch.int32).cuda()
            assert torch.equal(self.a_idx.cpu().long() // a_div, a_src) and int(a_src.max()) < M
        self.c_idx = c_perm.to(torch.int32).cuda() if c_perm is not None else None
        self.off = self.ts = None
        self.grp = torch.zeros(M, dtype=torch.long, device="cuda")
        if counts:
            self.off, self.ts, self.grp, Mv = cg._slots(M, self.G, counts)
            assert Mv == M

    def reference(self):
        """(fp64 C, bound, fp64 pre_out, bound) as test_contract_gemm.run_case computes them"""
        f64 = torch.float64
        M, N, K, G = self.M, self.N, self.K, self.G
        arow = self.a_idx.long() // self.a_div if self.a_idx is not None else torch.arange(M, device="cuda")
        A64, B64 = self.A.to(f64)[arow], self.B.to(f64).view(G, N, K)
        lin = torch.empty(M, N, dtype=f64, device="cuda")
        absacc = torch.empty_like(lin)
        for g in range(G):
            sel = (self.grp == g).nonzero().flatten()
            if sel.numel():
                lin[sel] = A64[sel] @ B64[g].t()
                absacc[sel] = A64[sel].abs() @ B64[g].abs().t()
        if self.bias is not None:
            lin = lin + self.bias.to(f64)[self.grp]
        v, gain = lin, torch.ones_like(lin)
        extra = kc.U32 * lin.abs()
        if self.act:
            v = cg.gelu64(lin)
            gain = cg.gelu_grad64(lin).abs()
            extra = extra * gain + kc.gelu_eval_extra(lin)
        if self.gpre is not None:                               # (gelu_grad_pre is read at the DESTINATION row, given in slot order here)
            gg = cg.gelu_grad64(self.gpre.to(f64))
            v = v * gg
            gain, extra = gain * gg.abs(), extra * gg.abs() + kc.gelu_eval_extra(self.gpre.to(f64)) * lin.abs()
        if self.res is not None:
            r64 = self.res.to(f64)
            extra = extra + kc.U32 * (v.abs() + r64.abs())
            v = v + r64
        bound = kc.gemm_bound(None, None, v, self.c_dtype, K=K, gain=gain, extra=extra, absacc=absacc)
        pre_bound = kc.gemm_bound(None, None, lin, self.dtype, K=K, extra=kc.U32 * lin.abs(), absacc=absacc)
        return v, bound, lin, pre_bound


def ops_act(epi):
    from m3vit_amd import ops as _ops
    return _ops.M3_ACT_GELU if epi in ("gelu", "f32c_gelu") else 0


def gemm_launch(ops, v, far_ld=None):
    """one m3_gemm_nt call of the case's values; far_ld {operand: row stride in bytes} names the operands that are far, the
    others take the compact leading dimensions of the path.  Slot order everywhere: with c_row_idx the C-shaped operands
    are written / read through the permutation.  Returns (outputs in slot order, signature, plan fields, far allocations)"""
    far_ld = far_ld or {}
    dtype, M, N, K, G = v.dtype, v.M, v.N, v.K, v.G
    es = ES[dtype]
    fars = {}
    crow = v.c_idx.long() if v.c_idx is not None else None

    def operand(name, rows, cols, dt, ld, values=None, out=False, by_crow=False):
        if name in far_ld:
            view, far = kc.far_rows(rows, cols, far_ld[name], dt)
            fars[name] = far
            if out:
                far.fill(dt)
        else:
            view = sent_rows(rows, cols, dt, ld) if out else torch.empty(rows, ld, dtype=dt, device="cuda")[:, :cols]
        if values is not None:
            if by_crow and crow is not None:
                view[crow] = values
            else:
                view.copy_(values)
        return view

    A = operand("A", M, K, dtype, K + v.apad, v.A)
    B = operand("B", G * N, K, dtype, K, v.B)
    inplace = v.epi == "res_inplace"
    C = operand("C", M, N, v.c_dtype, v.ldc, v.res if inplace else None, out=True, by_crow=True)
    pre = operand("pre", M, N, dtype, v.ldc, out=True) if v.epi == "gelu" else None
    gpre = operand("gpre", M, N, dtype, v.ldc, v.gpre, by_crow=True) if v.gpre is not None else None
    res = C if inplace else (operand("res", M, N, F32, v.ldc, v.res, by_crow=True) if v.res is not None else None)
    snap = kc.snapshot(A=A, B=B, gpre=gpre, res=None if inplace else res, bias=v.bias, a_idx=v.a_idx, c_idx=v.c_idx, off=v.off, ts=v.ts)
    a = cg.gemm_args(ops, A=A, B=B, C=C, c_dtype=v.c_dtype, M=M, N=N, K=K, G=G, dtype=dtype, a_row_idx=v.a_idx, a_row_div=v.a_div,
                     c_row_idx=v.c_idx, bias=v.bias.view(-1) if v.bias is not None else None, pre=pre, gpre=gpre, res=res, act=v.act,
                     offsets=v.off, tile_starts=v.ts)
    for name, far in fars.items():                              # the struct really carries the far strides
        ld = {"A": a.lda, "B": a.ldb, "C": a.ldc, "pre": a.ld_pre, "gpre": a.ld_gpre, "res": a.ld_res}[name]
        assert ld * ES[{"C": v.c_dtype, "res": F32}.get(name, dtype)] == far.ld_bytes
    sig = ls.gemm_signature(ops, a)
    p = ops.gemm_plan(a)
    plan = (p.kernel, p.epilogue, p.tile_m, p.tile_n, p.m_band, p.vec8, p.n_tiles, p.m_tiles_max)
    assert (sig.get("kernel"), sig.get("epi")) == (v.kernel, cg.expected_kind(v.kernel, v.epi)), f"the case runs {sig}"
    if v.counts is None:
        assert p.m_band == v.band
    ops.check(ops.lib().m3_gemm_nt(byref(a), ops._stream()), "m3_gemm_nt")
    torch.cuda.synchronize()
    kc.unchanged(snap)
    for name, dt in (("C", v.c_dtype), ("pre", dtype)):
        if name in fars:
            fars[name].check_outside([(0, N * ES[dt])], dt, what=f"far {name}")
    out = dict(C=(C[crow] if crow is not None else C).contiguous())
    if pre is not None:
        out["pre"] = (pre[crow] if crow is not None else pre).contiguous()
    return out, sig, plan, fars


def gemm_far_and_compact(ops, v, far_ld, case):
    """the three checks of a case; frees the far allocations before the compact twin runs"""
    need(sum(span(v.G * v.N if n == "B" else v.M, ld, 16) for n, ld in far_ld.items()) + (64 << 20))
    if v.big is not None:
        ops.gemm_set_big(v.big)
    try:
        out_f, sig_f, plan_f, fars = gemm_launch(ops, v, far_ld)
        tops = {n: f.nbytes for n, f in fars.items()}
        del fars
        gc.collect()
        torch.cuda.empty_cache()
        out_c, sig_c, plan_c, _ = gemm_launch(ops, v)
    finally:
        if v.big is not None:
            ops.gemm_set_big(-1)
    assert sig_f == sig_c and plan_f == plan_c, f"far and compact calls plan differently:\n  {sig_f} {plan_f}\n  {sig_c} {plan_c}"
    for k in out_f:
        assert kc.same_bits(out_f[k], out_c[k]), f"{case}: {k} of the far call differs in bits from the compact call's"
    ref, bound, lin, pre_bound = v.reference()
    w = kc.assert_within(out_f["C"], ref, bound, what=f"{case}: C")
    if "pre" in out_f:
        w = max(w, kc.assert_within(out_f["pre"], lin, pre_bound, what=f"{case}: pre_out"))
    note(case, sig_f.get("kernel") + "/" + sig_f.get("epi"), **tops)
    assert w < 1


FAR_A_PATHS = ["f32_staged_ldc+4", "f16_staged_ktail", "f32_tall160", "f16_dma_band1_ldc+8", "bf16_dma_band4", "f16_big_k512",
               "bf16_big_k1024_ldc+8"]
TILE_M = {"staged": 128, "staged_tall": 160, "dma": 128, "big": 256}


def a_stride(path):
    """the stride helper's row stride for the path's M, with what makes the case: the 2 GiB line falls inside a row tile
    (neither on a tile boundary nor outside the rows) and the last row ends inside the 4 GiB reach"""
    dtype, M, N, K = cg.PATHS[path][:4]
    kernel = cg.PATHS[path][7]
    ld_b = kc.reach_stride(M)
    first_hi = -(-GIB2 // ld_b)                                  # the first row that starts at or above 2^31
    assert 0 < first_hi < M and first_hi % TILE_M[kernel] != 0
    assert (M + 1) * ld_b < GIB4 <= (M + 1) * (ld_b + 16) and span(M, ld_b, K * ES[dtype]) < GIB4
    return ld_b


@pytest.mark.parametrize("path", FAR_A_PATHS)
def test_gemm_far_a_dense(ops, path):
    v = GemmVals(path, seed=100)
    gemm_far_and_compact(ops, v, {"A": a_stride(path)}, f"gemm far A dense {path}")


@pytest.mark.parametrize("a_div", [1, 3])
@pytest.mark.parametrize("path", ["f16_staged_ktail", "bf16_dma_band4", "bf16_big_k1024_ldc+8"])
def test_gemm_far_a_gathered(ops, path, a_div):
    """a_row_idx over a table of exactly M rows: every row tile gathers rows from both sides of 2^31, the first tile row M - 1"""
    M, kernel = cg.PATHS[path][1], cg.PATHS[path][7]
    ld_b = a_stride(path)
    src = straddling(M, ld_b, TILE_M[kernel], seed=7 + a_div)
    v = GemmVals(path, a_src=src, a_div=a_div, seed=110 + a_div)
    gemm_far_and_compact(ops, v, {"A": ld_b}, f"gemm far A gathered div {a_div} {path}")


@pytest.mark.parametrize("path", ["f32_staged_ldc+4", "f16_dma_band1_ldc+8", "f16_big_k512"])
def test_gemm_far_a_grouped(ops, path):
    """G = 3 with an empty middle group: group 0 ends in a one-row tile at row 128, group 2 in a partial tile whose clamped
    rows read row M - 1, the last one inside the reach"""
    M = cg.PATHS[path][1]
    ld_b = a_stride(path)
    assert (M - 1) * ld_b >= GIB2
    v = GemmVals(path, "bias", counts=[129, 0, M - 129], seed=120)
    gemm_far_and_compact(ops, v, {"A": ld_b}, f"gemm far A grouped {path}")


@pytest.mark.parametrize("path", ["f16_dma_band1_ldc+8", "f16_big_k512"])
def test_gemm_far_b_two_groups(ops, path):
    """the weight of two groups, each just inside the reach: group 1's base is past 4 GiB (the 64-bit g * b_group_b) and its
    upper rows past 2 GiB inside the group - 8 GiB of address space, the largest case"""
    M, N, K = cg.PATHS[path][1:4]
    ldb_b = kc.reach_stride(N - 1)                              # the largest multiple of 16 with N * ldb_b < 2^32
    assert N * ldb_b < GIB4 <= N * (ldb_b + 16) and N * ldb_b > GIB4 - 16 * N
    assert (N - 1) * ldb_b >= GIB2 and span(2 * N, ldb_b, K * 2) > 7 * (1 << 30)
    v = GemmVals(path, "bias", counts=[M // 3, M - M // 3], seed=130)
    gemm_far_and_compact(ops, v, {"B": ldb_b}, f"gemm far B G=2 {path}")


FAR_C_LD = 20 * MIB
FAR_C_PATHS = ["f16_staged_ktail", "bf16_dma_band4", "f16_big_k512"]
# far operand: the epilogue id that has it (test_contract_gemm.EPIS)
FAR_C_CASES = {"C_f32_res_inplace": ("C", "res_inplace"), "C_16bit_scattered": ("C", "plain"), "pre_out": ("pre", "gelu"),
               "gelu_grad_pre": ("gpre", "gpre"), "residual": ("res", "res")}


@pytest.mark.parametrize("what", list(FAR_C_CASES))
@pytest.mark.parametrize("path", FAR_C_PATHS)
def test_gemm_far_c_shaped_operand(ops, path, what):
    """one C-shaped operand with rows 20 MiB apart: rows from 103 start in 2 .. 4 GiB, rows from 205 past 4 GiB.  The
    compact twin's leading dimension is a multiple of 8 like the far one's (the same vec8 class)"""
    M, N = cg.PATHS[path][1:3]
    assert 102 * FAR_C_LD < GIB2 <= 103 * FAR_C_LD and 204 * FAR_C_LD < GIB4 <= 205 * FAR_C_LD and M > 205
    name, epi = FAR_C_CASES[what]
    perm = None
    if what == "C_16bit_scattered":                             # a permutation of the C rows: slots of the first tile write past 4 GiB
        perm = straddling(M, FAR_C_LD, TILE_M[cg.PATHS[path][7]], seed=9, line=GIB4)
    v = GemmVals(path, epi, c_perm=perm, ldc=N + 8, seed=140)
    assert FAR_C_LD % (8 * 4) == 0 and v.ldc % 8 == 0
    gemm_far_and_compact(ops, v, {name: FAR_C_LD}, f"gemm far {what} {path}")


# ================================================================================================= m3_wgrad_tn
class WgradVals:
    def __init__(self, dtype, M, N, K, *, counts=None, c_src=None, c_div=1, scale=False, a_src=None, a_div=1, seed=0):
        self.dtype, self.M, self.N, self.K = dtype, M, N, K
        self.dC = cw.rnd(M, N, dtype=dtype, seed=seed + 1)
        self.A = cw.rnd(M, K, dtype=dtype, seed=seed + 2)
        self.c_div, self.a_div = c_div, a_div
        mk = lambda src, div: None if src is None else (src * div + torch.arange(M) % div).to(torch.int32).cuda()     # noqa: E731
        self.c_idx, self.a_idx = mk(c_src, c_div), mk(a_src, a_div)
        for idx, div in ((self.c_idx, c_div), (self.a_idx, a_div)):
            assert idx is None or int(idx.max()) // div < M
        assert not scale or self.c_idx is not None
        self.c_scale = (torch.rand(M * c_div, generator=torch.Generator().manual_seed(seed + 3)) + 0.5).cuda() if scale else None
        self.counts = counts
        self.G = len(counts) if counts else 1
        self.off, self.grp = None, torch.zeros(M, dtype=torch.long, device="cuda")
        if counts:
            assert sum(counts) == M
            self.off, self.grp, _ = cw.routing(self.G, counts)


def wgrad_launch(ops, v, kernel, *, far=None, mode="slabs", splits=2, want_db=True, chunk=64):
    """one m3_wgrad_tn call through the C ABI and its reduction.  far = the row stride in bytes of the one allocation dC and A are
    windows of, or None for compact operands; mode: "slabs" (m3_wgrad_reduce), "balanced" (chunk_rows = chunk, m3_wgrad_reduce_grouped)
    or "direct".  The option pattern comes from test_contract_wgrad.plan_args, the mode fields are set here.  Returns
    (dW [G, N, K], db [G, N] | None, signature, slab count for the bound, far allocation)"""
    dtype, M, N, K, G = v.dtype, v.M, v.N, v.K, v.G
    es = ES[dtype]
    alloc = None
    if far is not None:                                         # dC and A are windows of the same rows, A behind dC
        assert (N + K) * es <= far
        A, alloc = kc.far_rows(M, K, far, dtype, col_byte=N * es)
        dC = alloc.view(N, dtype)
        assert dC.stride(0) * es == A.stride(0) * es == far and A.data_ptr() - dC.data_ptr() == N * es
    else:
        dC = torch.empty(M, N + 16 // es, dtype=dtype, device="cuda")[:, :N]
        A = torch.empty(M, K + 32 // es, dtype=dtype, device="cuda")[:, :K]
    dC.copy_(v.dC); A.copy_(v.A)
    a = cw.plan_args(ops, dtype, M, N, K, G=G, grouped=v.counts is not None, splits=splits, want_db=want_db, gc=v.c_idx is not None,
                     c_div=v.c_div, sc=v.c_scale is not None, ga=v.a_idx is not None, a_div=v.a_div)
    ptr = lambda t: t.data_ptr() if t is not None else None          # noqa: E731
    a.dC, a.lddc, a.A, a.lda = dC.data_ptr(), dC.stride(0), A.data_ptr(), A.stride(0)
    a.c_row_idx, a.c_row_scale, a.a_row_idx, a.group_offsets = ptr(v.c_idx), ptr(v.c_scale), ptr(v.a_idx), ptr(v.off)
    units = {"slabs": splits * G, "balanced": M // chunk + G, "direct": 0}[mode]
    a.splits, a.chunk_rows, a.units = (splits, 0, 0) if mode != "balanced" else (1, chunk, units)
    ws, wcheck = kc.guarded_ws(max(units, 1) * N * (K + 1))
    dW, dWcheck = kc.guarded(G * N, K, F32)
    db, dbcheck = kc.guarded(G, N, F32) if want_db else (None, None)
    bias_ws = ws[units * N * K:] if want_db and mode != "direct" else None
    a.ws, a.bias_ws = ws.data_ptr(), ptr(bias_ws)
    a.direct_dW = a.direct_db = None
    a.direct_beta = a.direct_beta_db = 0
    if mode == "direct":
        assert splits == 1
        a.direct_dW, a.direct_db = dW.data_ptr(), ptr(db)
    sig = ls.wgrad_signature(ops, a)
    flags = tuple(int(t is not None) for t in (v.c_idx, v.a_idx, v.c_scale))
    assert (sig.get("kernel"), sig.get("mode")) == (kernel, mode) and (sig.get("gc"), sig.get("ga"), sig.get("sc")) == flags, \
        f"the case runs {sig}, not {kernel} / {mode} {flags}"
    snap = kc.snapshot(dC=dC, A=A, c_idx=v.c_idx, a_idx=v.a_idx, c_scale=v.c_scale, off=v.off)
    L = ops.lib()
    ops.check(L.m3_wgrad_tn(byref(a), ops._stream()), "m3_wgrad_tn")
    if mode == "slabs":
        ops.check(L.m3_wgrad_reduce(ops._p(ws), splits, G * N * K, ops._p(dW), 0, ops._p(bias_ws), G * N if want_db else 0, ops._p(db), 0,
                                    ops._stream()), "m3_wgrad_reduce")
    elif mode == "balanced":
        ops.check(L.m3_wgrad_reduce_grouped(ops._p(ws), ops._p(v.off), G, chunk, N * K, ops._p(dW), 0, ops._p(bias_ws), N if want_db else 0,
                                            ops._p(db), 0, ops._stream()), "m3_wgrad_reduce_grouped")
    torch.cuda.synchronize()
    kc.unchanged(snap); wcheck(); dWcheck()
    if want_db:
        dbcheck()
    return dW.contiguous().view(G, N, K), db.contiguous() if want_db else None, sig, max(units, 1), alloc


def wgrad_far_and_compact(ops, v, kernel, case, far, knobs_far, knobs_compact=None, **kw):
    need(span(v.M, far, 4096) + (64 << 20))
    with cw.knobs(ops, *knobs_far):
        dW_f, db_f, sig_f, slabs, alloc = wgrad_launch(ops, v, kernel, far=far, **kw)
    top = alloc.nbytes
    del alloc
    gc.collect()
    torch.cuda.empty_cache()
    with cw.knobs(ops, *(knobs_compact or knobs_far)):
        dW_c, db_c, sig_c, _, _ = wgrad_launch(ops, v, kernel, **kw)
    assert sig_f == sig_c, f"far and compact calls plan differently:\n  {sig_f}\n  {sig_c}"
    assert kc.same_bits(dW_f, dW_c), f"{case}: dW of the far call differs in bits from the compact call's"
    assert db_f is None or kc.same_bits(db_f, db_c), f"{case}: db of the far call differs in bits from the compact call's"
    W, rdb, bW, bdb = cw.reference(v.dC, v.A, v.N, v.K, v.G, v.grp, v.M, slabs, v.dtype, v.c_idx, v.c_div, v.c_scale, v.a_idx, v.a_div)
    w = kc.assert_within(dW_f, W, bW, what=f"{case}: dW")
    if db_f is not None:
        w = max(w, kc.assert_within(db_f, rdb, bdb, what=f"{case}: db"))
    note(case, sig_f.get("kernel") + "/" + sig_f.get("mode"), **{"dC+A": top})
    assert w < 1


UNDER_M = 300
# kernel id: dtype, N, K, (wgrad_set_dma, wgrad_set_big), the kernel
UNDER = {"big_f16": (F16, 256, 256, (None, 1), "big"), "big_bf16": (BF16, 256, 256, (None, 1), "big"),
         "dma_f16": (F16, 384, 128, (2, None), "dma"), "dma_f32": (F32, 384, 128, (2, None), "dma")}
# the per-row factor: fp16 on both kernels (the 256 x 256 kernel has it for fp16 only), fp32 on the 128-wide one
UNDER_CASES = [(k, var) for k in UNDER for var in ("plain", "gathers", "row_scale", "balanced") if var != "row_scale" or k != "big_bf16"]


def under_stride():
    ld_b = kc.reach_stride(UNDER_M)
    assert ld_b == 14_268_992 and 150 * ld_b < GIB2 <= 151 * ld_b and (UNDER_M + 1) * ld_b < GIB4
    return ld_b


@pytest.mark.parametrize("kern,variant", UNDER_CASES)
def test_wgrad_under_the_reach(ops, kern, variant):
    """the two LDS-DMA tile kernels one 16-byte step inside the reach: rows 151 .. 299 start above 2^31, every address a
    whole 32-bit sum.  dC and A are windows of the same rows"""
    dtype, N, K, knobs, kernel = UNDER[kern]
    M, ld_b = UNDER_M, under_stride()
    kw = dict(splits=2)
    if variant == "plain":
        v = WgradVals(dtype, M, N, K, seed=200)
    elif variant in ("gathers", "row_scale"):                 # tables of M rows that straddle 2^31 in every 64-row step
        v = WgradVals(dtype, M, N, K, c_src=straddling(M, ld_b, 64, seed=21), c_div=2, scale=variant == "row_scale",
                      a_src=straddling(M, ld_b, 64, seed=22), a_div=1, seed=210)
    else:                                                       # balanced units, one empty group: r0 != 0 above and below the line
        v = WgradVals(dtype, M, N, K, counts=[130, 0, 170], seed=220)
        kw = dict(mode="balanced", splits=1, chunk=64)
    wgrad_far_and_compact(ops, v, kernel, f"wgrad under the reach {kern} {variant}", ld_b, knobs, **kw)


def test_wgrad_streaming_kernel_under_the_reach(ops):
    M, N, K, ld_b = UNDER_M, 384, 16, under_stride()
    assert ops.wgrad_skinny(N, K)
    v = WgradVals(F16, M, N, K, seed=230)
    wgrad_far_and_compact(ops, v, "skinny", "wgrad under the reach skinny16_f16", ld_b, (None, None), splits=2, want_db=False)


PAST_M, PAST_LD = 100, 48 * MIB
PAST_VARIANTS = ["plain", "gathers_div3", "row_scale", "bias_ws", "direct"]


@pytest.mark.parametrize("variant", PAST_VARIANTS)
def test_wgrad_past_the_reach_steps_down(ops, variant):
    """strides of 48 MiB at M = 100: rows from 43 start in 2 .. 4 GiB, rows from 86 past 4 GiB.  A shape that takes the
    LDS-DMA kernel under m3_wgrad_set_dma(2) must report - and run - the register-staged one; with two parts the first runs
    whole steps on bumped 64-bit pointers, the second starts at row 64 and ends in a clamped 4-row step at the far end.  The
    compact twin is forced onto the same kernel"""
    dtype, M, N, K, ld_b = F16, PAST_M, 384, 128, PAST_LD
    assert 42 * ld_b < GIB2 <= 43 * ld_b and 85 * ld_b < GIB4 <= 86 * ld_b and (M + 1) * ld_b >= GIB4 and M % 32 == 4
    with cw.knobs(ops, 2, None):                                # the premise: inside the reach this call is the LDS-DMA kernel's
        assert ls.wgrad_signature(ops, cw.plan_args(ops, dtype, M, N, K, splits=2)).get("kernel") == "dma"
    src = lambda seed: torch.randperm(M, generator=torch.Generator().manual_seed(seed))      # noqa: E731  (every row, row M - 1 among them)
    kw = dict(splits=2, want_db=variant == "bias_ws")
    if variant in ("plain", "bias_ws"):
        v = WgradVals(dtype, M, N, K, seed=300)
    elif variant == "gathers_div3":
        v = WgradVals(dtype, M, N, K, c_src=src(31), c_div=3, a_src=src(32), a_div=3, seed=310)
    elif variant == "row_scale":
        v = WgradVals(dtype, M, N, K, c_src=src(33), c_div=1, scale=True, seed=320)
    else:
        v = WgradVals(dtype, M, N, K, seed=330)
        kw = dict(mode="direct", splits=1, want_db=True)
    for idx, div in ((v.c_idx, v.c_div), (v.a_idx, v.a_div)):   # gathered tables reach the last row, past 4 GiB
        assert idx is None or int(idx.max()) // div == M - 1
    wgrad_far_and_compact(ops, v, "staged", f"wgrad past the reach {variant}", ld_b, (2, None), (0, 0), **kw)


def test_wgrad_stride_with_bit_31_set(ops):
    """M = 3, ld_b = 2^31 + 16: row 2 starts past 4 GiB, from a two-factor product whose stride does not fit a signed 32-bit
    integer"""
    ld_b = GIB2 + 16
    assert 2 * ld_b > GIB4 and ld_b > 2 ** 31 - 1
    v = WgradVals(F16, 3, 128, 128, seed=400)
    wgrad_far_and_compact(ops, v, "staged", "wgrad stride bit 31", ld_b, (0, 0), splits=1)


# ================================================================================================= m3_wgrad_multi, m3_colsum
MULTI_M, MULTI_LD = 512, 9 * MIB
MULTI_SHAPES = [(384, 128, True), (128, 256, False)]            # (N, K, bias): shapes of the register-staged kernel


def multi_args(ops, views, outs, M, dtype):
    from m3vit_amd import _lib
    a = _lib.WgradMultiArgs()
    for j, ((dC, A), (dW, db)) in enumerate(zip(views, outs)):
        q = a.prob[j]
        q.dC, q.lddc, q.A, q.lda, q.N, q.K = dC.data_ptr(), dC.stride(0), A.data_ptr(), A.stride(0), dC.shape[1], A.shape[1]
        q.dW, q.db, q.beta, q.beta_db = dW.data_ptr(), (db.data_ptr() if db is not None else None), 0, 0
    a.M, a.dtype, a.n, a.parts = M, ops.dt_code(dtype), len(views), 1
    return a


def multi_run(ops, vals, far_ld):
    from m3vit_amd import _lib
    dtype, M = F16, MULTI_M
    widths = [w for (N, K, _) in MULTI_SHAPES for w in (N, K)]
    alloc = None
    if far_ld:
        cb = [sum(widths[:i]) * 2 for i in range(4)]
        last, alloc = kc.far_rows(M, widths[3], far_ld, dtype, col_byte=cb[3])
        wins = [alloc.view(widths[i], dtype, cb[i]) for i in range(3)] + [last]
    else:
        wins = [torch.empty(M, w + 8, dtype=dtype, device="cuda")[:, :w] for w in widths]
    for w, val in zip(wins, vals):
        w.copy_(val)
    views = [(wins[0], wins[1]), (wins[2], wins[3])]
    guards = [(kc.guarded(N, K, F32), kc.guarded(1, N, F32) if b else None) for N, K, b in MULTI_SHAPES]
    outs = [(gw[0], gb[0] if gb else None) for gw, gb in guards]
    p = ops.wgrad_multi_plan(MULTI_SHAPES, M, dtype, 1)
    assert p.allowed and p.parts == 1
    ws, wcheck = kc.guarded_ws(p.ws_elems)
    a = multi_args(ops, views, outs, M, dtype)
    a.ws = ws.data_ptr()
    descs = (_lib.WgradReduceDesc * 2)()
    a.reduce_out = ctypes.cast(descs, ctypes.POINTER(_lib.WgradReduceDesc))
    sig = ls.wgrad_multi_signature(ops, a)
    snap = kc.snapshot(**{f"op{i}": w for i, w in enumerate(wins)})
    ops.check(ops.lib().m3_wgrad_multi(byref(a), ops._stream()), "m3_wgrad_multi")
    ops.check(ops.lib().m3_wgrad_reduce_multi(descs, 2, ops._stream()), "m3_wgrad_reduce_multi")
    torch.cuda.synchronize()
    kc.unchanged(snap); wcheck()
    for gw, gb in guards:
        gw[1]()
        if gb:
            gb[1]()
    res = [(dW.clone(), db.clone() if db is not None else None) for dW, db in outs]          # (copies: the caller reuses the outputs)
    return res, sig, (p.parts, p.tiles, p.workgroups), alloc, (views, outs, guards, a, descs, ws)


def test_wgrad_multi_far_windows_of_one_buffer(ops):
    """two problems whose four operands are windows of the same 512 rows, 9 MiB apart: rows from 456 start past 4 GiB"""
    M, ld_b = MULTI_M, MULTI_LD
    assert 455 * ld_b < GIB4 <= 456 * ld_b and 227 * ld_b < GIB2 <= 228 * ld_b
    need(span(M, ld_b, 4096) + (64 << 20))
    vals = [cw.rnd(M, w, dtype=F16, seed=500 + i) for i, w in enumerate(w for (N, K, _) in MULTI_SHAPES for w in (N, K))]
    res_f, sig_f, plan_f, alloc, keep = multi_run(ops, vals, ld_b)
    # refused before anything is launched: a stride of 2^32 bytes, M = 2^31 - the outputs keep what they hold
    views, outs, guards, a, descs, ws = keep
    for field, bad in (("lddc", GIB4 // 2), ("M", 1 << 31)):
        b = ls.copy_struct(a)
        if field == "M":
            b.M = bad
        else:
            b.prob[1].lddc = bad
        for o in outs:
            o[0].copy_(kc.sentinel_like(o[0]))
        assert ops.lib().m3_wgrad_multi(byref(b), ops._stream()) == -1, field
        assert b"m3_wgrad_multi" in ops.lib().m3_last_error()
        torch.cuda.synchronize()
        assert all(kc.same_bits(o[0].contiguous(), kc.sentinel_like(o[0].contiguous())) for o in outs), f"{field}: a refused call wrote dW"
    top = alloc.nbytes
    del alloc, keep, views, outs, guards, a, descs, ws
    gc.collect(); torch.cuda.empty_cache()
    res_c, sig_c, plan_c, _, _ = multi_run(ops, vals, None)
    assert sig_f == sig_c and plan_f == plan_c
    w = 0.0
    zero = torch.zeros(M, dtype=torch.long, device="cuda")
    for j, (N, K, bias) in enumerate(MULTI_SHAPES):
        assert kc.same_bits(res_f[j][0], res_c[j][0]), f"problem {j}: dW of the far call differs in bits from the compact call's"
        W, rdb, bW, bdb = cw.reference(vals[2 * j], vals[2 * j + 1], N, K, 1, zero, M, 1, F16)
        w = max(w, kc.assert_within(res_f[j][0], W[0], bW[0], what=f"wgrad_multi problem {j}: dW"))
        if bias:
            assert kc.same_bits(res_f[j][1], res_c[j][1])
            w = max(w, kc.assert_within(res_f[j][1].view(N), rdb[0], bdb[0], what=f"wgrad_multi problem {j}: db"))
    note("wgrad_multi", "multi " + str(sig_f), **{"dC0+A0+dC1+A1": top})
    assert w < 1


@pytest.mark.parametrize("grouped", [False, True])
def test_colsum_far_rows(ops, grouped):
    """m3_colsum over the far dC of the past-the-reach cases (64-bit row x stride), through a row map that reaches row M - 1"""
    dtype, M, N, ld_b = F16, PAST_M, 384, PAST_LD
    need(span(M, ld_b, N * 2) + (64 << 20))
    counts = [40, 0, 60] if grouped else None
    G = len(counts) if grouped else 1
    off, grp, _ = cw.routing(G, counts) if grouped else (None, torch.zeros(M, dtype=torch.long, device="cuda"), M)
    c_idx = torch.randperm(M, generator=torch.Generator().manual_seed(6)).to(torch.int32).cuda()
    vals = cw.rnd(M, N, dtype=dtype, seed=600)
    need_ws = int(ops.lib().m3_colsum_ws_elems(M, N, G))

    def run(dC):
        ws, wcheck = kc.guarded_ws(need_ws)
        db, dbc = kc.guarded(G, N, F32)
        snap = kc.snapshot(dC=dC, c_idx=c_idx)
        ops.check(ops.lib().m3_colsum(ops._p(dC), ops.dt_code(dtype), dC.stride(0), ops._p(c_idx), M, N, G, ops._p(off), ops._p(ws),
                                      ops._p(db), 0, ops._stream()), "m3_colsum")
        torch.cuda.synchronize()
        kc.unchanged(snap); wcheck(); dbc()
        return db.contiguous()
    dC, alloc = kc.far_rows(M, N, ld_b, dtype)
    dC.copy_(vals)
    far = run(dC)
    top = alloc.nbytes
    del dC, alloc
    gc.collect(); torch.cuda.empty_cache()
    cdC = torch.empty(M, N + 8, dtype=dtype, device="cuda")[:, :N]
    cdC.copy_(vals)
    assert kc.same_bits(far, run(cdC)), "db of the far call differs in bits from the compact call's"
    L = vals.double()[c_idx.long()]
    ref = torch.stack([L[grp == g].sum(0) for g in range(G)])
    aref = torch.stack([L[grp == g].abs().sum(0) for g in range(G)])
    w = kc.assert_within(far, ref, kc.sum_bound(aref, M + 2, ref, F32), what="colsum db")
    note(f"colsum grouped={grouped}", "colsum", dC=top)
    assert w < 1


# ================================================================================================= m3_conv3x3_fwd
def test_conv3x3_fwd_bordered_operand_past_2_gib(ops):
    """N = 9 images of 1022 x 1022 x 128 channels, fp16: the bordered operand is 2.4 GB and image 8 lies wholly at and above
    2^31 bytes - the kernel multiplies a 32-bit bordered-pixel index by the pixel's 256 bytes.  (m3_conv3x3_dgrad is the same
    launch, the weight gradient is m3_wgrad_tn.)  The fp64 reference is taken for the top 8 and the bottom 8 output rows of
    image 0 and of image 8, from crops of the bordered input; the same crops, run as convolutions of their own, must give
    the same bits (the compact twin)"""
    import conv_common as CC
    import torch.nn.functional as Fn
    from m3vit_amd import conv as MC
    dtype, N, H, W, C, Cout, R = F16, 9, 1022, 1022, 128, 8, 8
    PB = N * (H + 2) * (W + 2)
    assert 8 * (H + 2) * (W + 2) * C * 2 >= GIB2 and PB * C * 2 < GIB4 and (PB - 1) * C * 2 > GIB2
    p = ops.conv3x3_plan(dtype, N, H, W, C, Cout)
    from m3vit_amd import _lib
    assert p.ok and _lib.GEMM_KERNELS[p.kernel] == "big" and p.m_tiles == -(-N * H * W // 256) and p.n_tiles == 1
    need(PB * C * 2 + (1 << 30))
    g = torch.Generator(device="cuda").manual_seed(700)
    xb = torch.empty(N, H + 2, W + 2, C, dtype=dtype, device="cuda").normal_(generator=g)
    xb[:, 0].zero_(); xb[:, -1].zero_(); xb[:, :, 0].zero_(); xb[:, :, -1].zero_()
    gw = torch.Generator().manual_seed(701)
    w = (torch.randn(Cout, C, 3, 3, generator=gw) * 0.05).to(dtype)
    b = torch.randn(Cout, generator=gw)
    w_fwd, bd = MC.weight_operands(w.cuda(), dtype)[0], b.cuda()
    blocks = [(n, y0) for n in (0, N - 1) for y0 in (0, H - R)]          # output rows y0 .. y0 + 7 of image n
    crops = {k: xb[k[0], k[1]:k[1] + R + 2].clone() for k in blocks}      # their bordered rows y0 .. y0 + 9
    snap = kc.snapshot(w=w_fwd, bias=bd, **{f"crop{n}_{y0}": xb[n, y0:y0 + R + 2] for n, y0 in blocks})
    out, check = kc.guarded(N * H * W, Cout, dtype)
    ops.conv3x3_fwd(xb, w_fwd, bd, out=out)
    torch.cuda.synchronize()
    check(what="conv3x3_fwd")
    kc.unchanged(snap)
    idx = ops.conv3x3_index(N, H, W, "cuda")
    B64 = w.permute(0, 2, 3, 1).reshape(Cout, 9 * C).double()
    worst = 0.0
    for (n, y0), crop in crops.items():
        m0 = (n * H + y0) * W
        got = out[m0:m0 + R * W]
        # the pixel table of the block against the host restatement, shifted to the crop's first bordered row
        assert torch.equal(idx[m0:m0 + R * W].cpu().long(), CC.pixel_table(1, R, W) + (n * (H + 2) + y0) * (W + 2))
        twin = ops.conv3x3_fwd(crop.view(1, R + 2, W + 2, C), w_fwd, bd)
        assert kc.same_bits(got.contiguous(), twin), f"image {n}, rows from {y0}: the far block differs in bits from the crop's own run"
        c64 = crop.cpu().double()
        ref = Fn.conv2d(c64.permute(2, 0, 1).unsqueeze(0), w.double(), b.double())          # [1, Cout, R, W]: the crop brings its border
        yr = ref[0].permute(1, 2, 0).reshape(R * W, Cout)
        A = CC.windows(crop.cpu().view(1, R + 2, W + 2, C)).double()
        worst = max(worst, kc.assert_within(got, yr, kc.gemm_bound(A, B64, yr, dtype, K=9 * C, extra=kc.U32 * yr.abs()),
                                            f"conv3x3_fwd image {n}, rows from {y0}"))
    note("conv3x3_fwd 9 x 1022 x 1022 x 128 -> 8", "big/seg", xb=PB * C * 2)
    assert worst < 1
