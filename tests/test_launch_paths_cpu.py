"""CPU: which kernel every contract case runs, pinned before any GPU run.

m3_gemm_plan, m3_wgrad_kernel and m3_attention_plan are host code shared with the launching entry points, so they run on
a machine without a GPU from aligned non-null dummy addresses.  This module walks the case tables of the three contract
modules (test_contract_gemm / _wgrad / _attention) and asserts
  - that each case lands on the path it states (kernel, epilogue kind, band; kernel after the weight gradient's step-downs and
    its instance flags; attention family and instance): a threshold that moves in choose_kernel, gemm_big_eligible,
    wgrad_dma_pays, wgrad_demote or the attention instance rule fails here;
  - completeness: the instances the cases reach are exactly the ones the launchers can instantiate from a legal call."""
from ctypes import byref

import pytest
import torch

import launch_signature as ls
import test_contract_attention as ca
import test_contract_gemm as cg
import test_contract_wgrad as cw

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from m3vit_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------ GEMM
def test_gemm_cases_run_the_path_they_state(ops):
    sigs = cg.case_signatures(ops)
    wrong = []
    for cid, big, kernel, band, kind, args, kw in cg.cases():
        sig, got_band = sigs[cid]
        if (sig.get("kernel"), sig.get("epi"), got_band) != (kernel, kind, band):
            wrong.append(f"{cid}: states {kernel} / {kind} / band {band}, runs {sig.get('kernel')} / {sig.get('epi')} / band {got_band}")
    assert not wrong, "\n".join(wrong)


def test_gemm_cases_reach_every_instance(ops):
    """launch_gemm_staged: the 128-row kernel per dtype and the 160-row one for fp32, with the run-time-flag epilogue;
    launch_gemm_dma / launch_gemm_big: fp16 and bf16, each with the five epilogue kinds (gemm_dev.h: with_epi).  All of
    them can be reached by a legal call: none is listed as unreachable"""
    can = {("staged", "any", d) for d in ("f32", "f16", "bf16")} | {("staged_tall", "any", "f32")}
    can |= {(k, e, d) for k in ("dma", "big") for e in ("any", "gpre", "res", "plain", "gelu") for d in ("f16", "bf16")}
    reached = {(s.get("kernel"), s.get("epi"), s.get("dtype")) for s, _ in cg.case_signatures(ops).values()}
    assert reached == can, (sorted(can - reached), sorted(reached - can))


def _gemm(ops, **kw):
    a = cg.case_args(ops, F16, 1000, 384, 384, 8, 392, "plain")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_gemm_plan_follows_the_mode_and_refuses_what_the_launch_refuses(ops):
    from m3vit_amd import _lib
    name = lambda a: _lib.GEMM_KERNELS[ops.gemm_plan(a).kernel]                   # noqa: E731
    long_k = cg.case_args(ops, *cg.PATHS["f16_big_k512"][:6], "plain")
    assert name(long_k) == "dma"                                    # default mode 2: K = 512 is below the 2048 it asks for
    ops.gemm_set_big(1)
    try:
        assert name(long_k) == "big"
    finally:
        ops.gemm_set_big(-1)
    p = ops.gemm_plan(_gemm(ops))
    assert (p.tile_m, p.tile_n, p.m_band, p.vec8, p.n_tiles, p.m_tiles_max) == (128, 128, 1, 1, 3, 8)
    assert name(_gemm(ops, M=0)) == "none"                           # launches nothing
    for bad in (dict(A=None), dict(C=ls.DUMMY + 8), dict(K=380), dict(ldc=380), dict(G=2), dict(c_dtype=2), dict(dtype=7),
                dict(M=1 << 40)):
        a = _gemm(ops, **bad)
        out = _lib.GemmPlan()
        assert ops.lib().m3_gemm_plan(byref(a), byref(out)) == -1, bad          # M3_ERR_ARG, as m3_gemm_nt returns
        assert b"m3_gemm_plan" in ops.lib().m3_last_error()


# ------------------------------------------------------------------------------------------------ weight gradient
def test_wgrad_cases_run_the_kernel_they_state(ops):
    sigs = cw.case_signatures(ops)
    wrong = []
    for cid, dma, big, kernel, args, kw in cw.cases():
        sig = sigs[cid]
        flags = tuple(int(bool(kw.get(f))) for f in ("gc", "ga", "sc"))
        if (sig.get("kernel"), sig.get("gc"), sig.get("ga"), sig.get("sc")) != (kernel, *flags):
            wrong.append(f"{cid}: states {kernel} {flags}, runs {sig}")
    assert not wrong, "\n".join(wrong)
    # the calls the module's docstrings single out: a per-row factor in bf16 lands on the register-staged kernel from both
    # LDS-DMA kernels; fp16 and fp32 keep the LDS-DMA kernel
    for kern, want in (("dma_bf16", "staged"), ("big_bf16", "staged"), ("dma_f16", "dma"), ("dma_f32", "dma"), ("big_f16", "big")):
        assert sigs[f"grouped/{kern}/None"].get("kernel") == want and sigs[f"grouped/{kern}/None"].get("sc") == 1


def test_wgrad_cases_reach_every_instance(ops):
    """wgrad_staged.hip WgStaged, wgrad_dma.hip WgDma / WgBig (test_contract_wgrad.has_instance states their rule) and the
    streaming kernel's (K, dtype) instances.  All of them can be reached by a legal call: none is listed as unreachable"""
    dts = {F32: "f32", F16: "f16", BF16: "bf16"}
    can = {(k, gc, ga, sc, dts[d]) for k in ("staged", "dma", "big") for d in dts for gc in (0, 1) for ga in (0, 1) for sc in (0, 1)
           if cw.has_instance(k, d, gc, ga, sc)}
    assert len(can) == 18 + 16 + 10
    can |= {("skinny", K, d) for K in (16, 32) for d in dts.values()}
    sigs = cw.case_signatures(ops)
    reached = set()
    for cid, dma, big, kernel, args, kw in cw.cases():
        s = sigs[cid]
        reached.add(("skinny", args[3], s.get("dtype")) if s.get("kernel") == "skinny" else
                    (s.get("kernel"), s.get("gc"), s.get("ga"), s.get("sc"), s.get("dtype")))
    assert reached == can, (sorted(map(str, can - reached)), sorted(map(str, reached - can)))


def test_wgrad_kernel_refuses_what_the_launch_refuses(ops):
    from m3vit_amd import _lib
    for bad in (dict(dC=None), dict(A=ls.DUMMY + 4), dict(splits=0), dict(N=390), dict(c_row_div=2), dict(c_row_scale=ls.DUMMY),
                dict(G=3), dict(chunk_rows=48, group_offsets=ls.DUMMY)):
        a = cw.plan_args(ops, F16, 333, 384, 192, splits=3)
        for k, v in bad.items():
            setattr(a, k, v)
        out = _lib.WgradKernelOut()
        assert ops.lib().m3_wgrad_kernel(byref(a), byref(out)) == -1, bad
        assert b"m3_wgrad_kernel" in ops.lib().m3_last_error()
    k = ops.wgrad_kernel(cw.plan_args(ops, F16, 333, 512, 256, splits=3))
    assert (_lib.WGRAD_KERNELS[k.kernel], k.tile_n, k.tile_k) == ("big", 256, 256)
    k = ops.wgrad_kernel(cw.plan_args(ops, F16, 333, 512, 256, splits=3, ga=True, a_div=3))       # the 256 x 256 kernel shifts
    assert (_lib.WGRAD_KERNELS[k.kernel], k.gather_a, k.tile_n, k.tile_k) == ("staged", 1, 128, 128)


# ------------------------------------------------------------------------------------------------ attention
def test_attention_cases_run_the_instance_they_state(ops):
    wrong = [(dtype, shape, ca.planned(ops, dtype, shape)) for dtype in ca.DTYPES for shape in ca.SHAPES
             if ca.planned(ops, dtype, shape) != ca.stated_plan(dtype, shape)]
    assert not wrong, wrong


def test_attention_cases_reach_every_instance(ops):
    """attention_b16.hip: the resident forward for 4 / 8 / 12 / 16 key tiles, the resident backward for 1..4 (dh 32) and
    1..2 (dh 64) tiles per wave, per 16-bit dtype; the streamed kernels and attention_f32.hip per head dim"""
    fwd, bwd, other = set(), set(), set()
    for dtype in ca.DTYPES:
        for shape in ca.SHAPES:
            ff, nkt, bf, kte = ca.planned(ops, dtype, shape)
            if ff == "resident":
                fwd.add((dtype, shape[3], nkt)); bwd.add((dtype, shape[3], kte))
            else:
                other.add((dtype, shape[3], ff))
    b16 = (F16, BF16)
    assert fwd == {(d, dh, n) for d in b16 for dh in (32, 64) for n in (4, 8, 12, 16)}
    assert bwd == {(d, 32, k) for d in b16 for k in (1, 2, 3, 4)} | {(d, 64, k) for d in b16 for k in (1, 2)}
    assert other == {(d, dh, "streamed") for d in b16 for dh in (32, 64)} | {(F32, dh, "f32") for dh in (32, 64)}
    # wholly masked key tiles of the resident forward: none, one, two and three of the four last tiles are all run
    masked = {ls.attention_signature(ops, "fwd", 1, s[1], s[3]).get("masked_tiles") for s in ca.SHAPES if ca.SHAPES[s]}
    assert masked == {0, 1, 2, 3}
    p = ops.attention_plan(F16, 1201, 64)
    assert (p.bwd_key_blocks, p.fwd_key_tiles, p.bwd_tiles_per_wave) == (5, 0, 0)
    for bad in ((F16, 0, 64), (F16, 100, 48)):
        with pytest.raises(Exception):
            ops.attention_plan(*bad)
