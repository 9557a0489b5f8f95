"""CPU: the reach rules of m3_gemm_nt and m3_wgrad_tn, pinned from both sides on the host code the launches share.

The kernels add 32-bit lane offsets to an operand's base wherever the host rule allows it (include/m3vit_hip.h: m3_gemm_nt's
requirements, m3_wgrad_kernel's step-downs), so the rule is what keeps them inside the operand: a check off by one row, or a
step-down that no longer happens, shows here before anything runs on a GPU (tests/test_far_operands_gpu.py then runs the
kernels on operands that really lie that far out).  m3_gemm_plan and m3_wgrad_kernel read no operand: dummy addresses."""
from ctypes import byref

import pytest
import torch

import launch_signature as ls
import test_contract_gemm as cg
import test_contract_wgrad as cw

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
ES = {F32: 4, F16: 2, BF16: 2}
ERR_ARG = -1


@pytest.fixture(scope="module")
def ops():
    from m3vit_amd import ops as _ops
    return _ops


def gemm_rc(ops, a):
    from m3vit_amd import _lib
    rc = ops.lib().m3_gemm_plan(byref(a), byref(_lib.GemmPlan()))
    if rc:
        assert b"m3_gemm_plan" in ops.lib().m3_last_error()
    return rc


def wgrad_rc(ops, a):
    from m3vit_amd import _lib
    out = _lib.WgradKernelOut()
    rc = ops.lib().m3_wgrad_kernel(byref(a), byref(out))
    if rc:
        assert b"m3_wgrad_kernel" in ops.lib().m3_last_error()
        return rc, None
    return rc, _lib.WGRAD_KERNELS[out.kernel]


# ------------------------------------------------------------------------------------------------ m3_gemm_plan
@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_gemm_reach_of_the_a_panel_and_of_one_weight_group(ops, dtype):
    """(M + 1) * lda * es and N * ldb * es: accepted at 2^32 - 16 * (M + 1) resp. 2^32 - 16 * N, refused one 16-byte step of the
    leading dimension further (exactly 2^32)"""
    es = ES[dtype]
    M, N, K = 255, 256, 64                                     # M + 1 and N divide 2^32
    top = (1 << 32) // 256 // es                               # elements: (M + 1) * top * es == N * top * es == 2^32
    step = 16 // es
    base = lambda: cg.case_args(ops, dtype, M, N, K, 0, N, "plain")                 # noqa: E731
    assert gemm_rc(ops, base()) == 0
    a = ls.copy_struct(base(), lda=top - step)
    assert (M + 1) * a.lda * es == (1 << 32) - 16 * (M + 1) and gemm_rc(ops, a) == 0
    assert gemm_rc(ops, ls.copy_struct(base(), lda=top)) == ERR_ARG
    b = ls.copy_struct(base(), ldb=top - step)
    assert N * b.ldb * es == (1 << 32) - 16 * N and gemm_rc(ops, b) == 0
    assert gemm_rc(ops, ls.copy_struct(base(), ldb=top)) == ERR_ARG
    # both at their last step together; the rule counts M + 1 rows, not M: one row more at the accepted stride is refused
    assert gemm_rc(ops, ls.copy_struct(base(), lda=top - step, ldb=top - step)) == 0
    assert gemm_rc(ops, ls.copy_struct(base(), lda=top - step, M=M + 1)) == ERR_ARG
    # the C-shaped operands are addressed with 64 bits: no reach rule on them
    assert gemm_rc(ops, ls.copy_struct(base(), ldc=1 << 33)) == 0


@pytest.mark.parametrize("dtype", [F32, F16])
def test_gemm_refuses_2_to_the_31_rows(ops, dtype):
    """rows are at least 16 bytes, so the panel rule refuses 2^28 rows and more by itself: the most rows of the shortest row
    are accepted, one more and M = 2^31 are not"""
    es = ES[dtype]
    a = cg.case_args(ops, dtype, 255, 256, 8, 0, 256, "plain")       # lda * es = 16 (fp16) or 32 bytes
    most = (1 << 32) // (a.lda * es) - 2                             # (most + 1) * lda * es == 2^32 - lda * es
    assert gemm_rc(ops, ls.copy_struct(a, M=most)) == 0
    assert gemm_rc(ops, ls.copy_struct(a, M=most + 1)) == ERR_ARG
    assert gemm_rc(ops, ls.copy_struct(a, M=1 << 31)) == ERR_ARG


# ------------------------------------------------------------------------------------------------ m3_wgrad_kernel
@pytest.mark.parametrize("dtype", [F32, F16])
def test_wgrad_refuses_a_4_gib_stride_and_2_to_the_31_rows(ops, dtype):
    es = ES[dtype]
    with cw.knobs(ops, 0, 0):
        base = lambda: cw.plan_args(ops, dtype, 3, 128, 128, splits=1)                # noqa: E731
        for f in ("lddc", "lda"):
            rc, kern = wgrad_rc(ops, ls.copy_struct(base(), **{f: ((1 << 32) - 16) // es}))
            assert (rc, kern) == (0, "staged"), f
            assert wgrad_rc(ops, ls.copy_struct(base(), **{f: (1 << 32) // es}))[0] == ERR_ARG, f
        assert wgrad_rc(ops, ls.copy_struct(base(), M=(1 << 31) - 1))[0] == 0
        assert wgrad_rc(ops, ls.copy_struct(base(), M=1 << 31))[0] == ERR_ARG


# shape id: dtype, N, K, wgrad_set_dma, wgrad_set_big, the kernel inside the reach, the kernel one step past it (the 128-wide
# kernel m3_wgrad_set_dma's rule names for the shape, stepped down once more where that is the LDS-DMA one)
STEP_DOWN = {
    "big_default": (F16, 256, 512, None, None, "big", "staged"),
    "big_default_bf16": (BF16, 512, 256, None, None, "big", "staged"),
    "dma128_f16": (F16, 384, 128, 2, None, "dma", "staged"),
    "dma128_f32": (F32, 384, 128, 2, None, "dma", "staged"),
    "big_over_dma128": (F16, 256, 256, 2, None, "big", "staged"),           # 256 x 256 -> LDS-DMA 128 -> register-staged
    "skinny16_f16": (F16, 384, 16, None, None, "skinny", "staged"),
    "skinny32_f32": (F32, 384, 32, None, None, "skinny", "staged"),        # fp32: the default rule names LDS-DMA, which steps down too
}
GATHERS = {"plain": {}, "gather_c_div2": dict(gc=True, c_div=2), "gather_a_div4": dict(ga=True, a_div=4),
           "gather_both": dict(gc=True, c_div=1, ga=True, a_div=2)}


@pytest.mark.parametrize("gather", list(GATHERS))
@pytest.mark.parametrize("shape", list(STEP_DOWN))
def test_wgrad_step_down_at_the_reach_from_both_sides(ops, shape, gather):
    """(M + 1) * ld_b one 16-byte step under 2^32 keeps the shape's kernel, exactly 2^32 steps down - for the dC stride
    alone, the A stride alone and both.  The streaming kernel takes plain rows only: with gathers it has stepped down
    already, inside the reach too"""
    dtype, N, K, dma, big, inside, outside = STEP_DOWN[shape]
    es = ES[dtype]
    M = 255
    top = (1 << 32) // (M + 1) // es                            # elements: (M + 1) * top * es == 2^32
    step = 16 // es
    kw = GATHERS[gather]
    if inside == "skinny" and kw:
        inside = "dma" if dtype == F32 else "staged"
    with cw.knobs(ops, dma, big):
        if STEP_DOWN[shape][5] == "skinny":
            assert ops.wgrad_skinny(N, K)
        base = lambda: cw.plan_args(ops, dtype, M, N, K, splits=2, want_db=False, **kw)       # noqa: E731
        assert wgrad_rc(ops, base()) == (0, inside)
        under = dict(lddc=top - step, lda=top - step)
        a = ls.copy_struct(base(), **under)
        assert (M + 1) * a.lddc * es == (M + 1) * a.lda * es == (1 << 32) - 16 * (M + 1)
        assert wgrad_rc(ops, a) == (0, inside)
        for over in (dict(lddc=top), dict(lda=top), dict(lddc=top, lda=top)):
            assert wgrad_rc(ops, ls.copy_struct(base(), **{**under, **over})) == (0, outside), over
        # M + 1 rows, not M: one row more at the accepted strides
        assert wgrad_rc(ops, ls.copy_struct(base(), M=M + 1, **under)) == (0, outside)


# ------------------------------------------------------------------------------------------------ the GPU cases' offsets
def test_the_far_layouts_break_every_wrong_address_model():
    """what makes tests/test_far_operands_gpu.py sensitive, as arithmetic on its own constants: under each wrong way of forming
    an address the layouts of its cases give, for rows the cases read or write, an address other than the right one - and
    one inside the same allocation where the test then finds wrong values or a changed sentinel, not a fault"""
    import kernel_contract as kc
    import test_far_operands_gpu as fg
    u32 = lambda x: x & 0xFFFFFFFF                                                   # noqa: E731
    s32 = lambda x: u32(x) - ((x & 0x80000000) << 1)                                 # noqa: E731
    # a signed instead of an unsigned 32-bit offset: every "under the reach" stride puts rows between 2 and 4 GiB
    for M in (300, 333, 1000, 11000):
        ld = kc.reach_stride(M)
        hi = [r for r in range(M) if r * ld >= fg.GIB2]
        assert hi and hi[-1] == M - 1 and all(u32(r * ld) == r * ld and s32(r * ld) < 0 for r in hi)
    # a 32-bit product where 64 bits are needed: the wrapped offset of a row past 4 GiB is another row's neighbourhood, inside
    # the allocation
    for M, ld in ((fg.PAST_M, fg.PAST_LD), (333, fg.FAR_C_LD), (300, fg.FAR_C_LD), (fg.MULTI_M, fg.MULTI_LD), (3, fg.GIB2 + 16)):
        past = [r for r in range(M) if r * ld >= fg.GIB4]
        assert past and all(u32(r * ld) != r * ld and u32(r * ld) < (M - 1) * ld for r in past)
    # the two-group weight: group 1's base as a 32-bit product
    for N in (384,):
        ldb = kc.reach_stride(N - 1)
        assert N * ldb < fg.GIB4 and u32(1 * N * ldb + (N - 1) * ldb) != N * ldb + (N - 1) * ldb
    # a stride whose bit 31 is set: negative as a signed 32-bit integer
    assert s32(fg.GIB2 + 16) < 0
    # the convolution: a bordered pixel index times 256 bytes, signed, goes negative inside image 8
    assert s32(8 * 1024 * 1024 * 256) < 0
