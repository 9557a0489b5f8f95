"""GPU: the heads' 3 x 3 convolutions on the GEMM kernels (csrc/conv.hip) through ops - forward, input gradient, weight and
bias gradient - against float64 F.conv2d and its autograd on the CPU, fed the same 16-bit-rounded operands.

Every output is a guarded allocation (kernel_contract.guarded / guarded_ws), every value is held to gemm_bound at the true
contraction length (9 C forward, 9 Cout input gradient, the pixel count for the weight gradient; sum_bound over the pixels
for the bias gradient), the operands keep their bits and a second run gives the same bits.

Shapes - the smallest at which the path can go wrong.  (N, H, W): (1, 1, 1) every tap but the centre is border; (2, 3, 5)
M = 30, the tile's rows are clamped; (3, 9, 10) M = 270, a second row tile of 14 rows and windows next to image boundaries.
Channels: C = 128 (six K tiles per run), 256 (with Cout = 256 the 256 x 256 weight-gradient kernel), 384; Cout = 40 (a mostly
empty column tile), 256, 264 (two column tiles).  Combinations that run:
  forward + weight / bias gradient  (1,1,1) 128->40 f16 bias | (2,3,5) 256->256 bf16 | (3,9,10) 384->264 f16 bias |
                                    (3,9,10) 128->256 bf16 bias | (2,3,5) 384->40 f16 | (1,1,1) 256->264 bf16 bias
  input gradient (contracts over Cout, which must then be a multiple of 128; writes C columns)
                                    (1,1,1) 40<-128 f16 | (2,3,5) 256<-256 bf16 | (3,9,10) 264<-384 f16 | (3,9,10) 256<-128 bf16
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_common as CC                                          # noqa: E402
from kernel_contract import (U32, assert_within, gemm_bound, guarded, guarded_ws, same_bits, snapshot, sum_bound,   # noqa: E402
                             unchanged)

from m3vit_amd import conv as MC                                  # noqa: E402
from m3vit_amd import ops                                         # noqa: E402

pytestmark = pytest.mark.gpu
F16, BF16 = torch.float16, torch.bfloat16

FWD_CASES = [((1, 1, 1), 128, 40, F16, True), ((2, 3, 5), 256, 256, BF16, False), ((3, 9, 10), 384, 264, F16, True),
             ((3, 9, 10), 128, 256, BF16, True), ((2, 3, 5), 384, 40, F16, False), ((1, 1, 1), 256, 264, BF16, True)]
DGRAD_CASES = [((1, 1, 1), 40, 128, F16), ((2, 3, 5), 256, 256, BF16), ((3, 9, 10), 264, 384, F16), ((3, 9, 10), 256, 128, BF16)]
_id = lambda c: "-".join(str(v).replace("torch.", "").replace(" ", "") for v in c)     # noqa: E731


def _operands(nhw, C, Cout, dtype, bias, seed):
    """16-bit-rounded x, weight and dy (CPU), the fp32 bias"""
    N, H, W = nhw
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g).to(dtype)
    w = (torch.randn(Cout, C, 3, 3, generator=g) * 0.05).to(dtype)
    b = torch.randn(Cout, generator=g) if bias else None
    dy = torch.randn(N, Cout, H, W, generator=g).to(dtype)
    return x, w, b, dy


def _cl(t):
    """CPU [N, C, H, W] -> the GPU channels-last tensor"""
    return t.cuda().contiguous(memory_format=torch.channels_last)


def test_pixel_table_matches_the_host_restatement():
    for N, H, W in ((1, 1, 1), (2, 3, 5), (3, 9, 10)):
        assert torch.equal(ops.conv3x3_index(N, H, W, "cuda").cpu().long(), CC.pixel_table(N, H, W))


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_pad_border_is_bit_exact(dtype):
    N, C, H, W = 3, 40, 9, 10
    x = _cl(torch.randn(N, C, H, W).to(dtype))
    out, check = guarded(N * (H + 2) * (W + 2), C, dtype)
    snap = snapshot(x=x)
    xb = ops.pad_border(x, out=out).view(N, H + 2, W + 2, C)
    check(what="bordered copy")
    unchanged(snap)
    assert same_bits(xb, CC.bordered(x.cpu()).cuda())


@pytest.mark.parametrize("dtype,relu", [(F16, True), (BF16, False)])
def test_bordered_relu_up2x_keeps_the_border_zero(dtype, relu):
    N, C, H, W = 2, 24, 3, 5
    x = _cl(torch.randn(N, C, H, W).to(dtype))
    out, check = guarded(N * (2 * H + 2) * (2 * W + 2), C, dtype)
    out.zero_()
    yb = ops.relu_up2x_fwd_bordered(x, relu=relu, out=out).view(N, 2 * H + 2, 2 * W + 2, C)
    check(what="bordered ReLU + x2")
    dense = ops.relu_up2x_fwd(x, relu=relu)                                     # the existing kernel instance: same arithmetic
    assert same_bits(yb[:, 1:-1, 1:-1, :].contiguous(), dense.permute(0, 2, 3, 1).contiguous())
    border = torch.ones(2 * H + 2, 2 * W + 2, dtype=torch.bool, device="cuda")
    border[1:-1, 1:-1] = False
    assert not bool(yb[:, border].view(torch.int16).any()), "the border of the bordered buffer is no longer all zero"
    # the allocating form zeroes the border itself
    assert same_bits(ops.relu_up2x_fwd_bordered(x, relu=relu), yb)


@pytest.mark.parametrize("case", FWD_CASES, ids=_id)
def test_forward_weight_and_bias_gradient(case):
    nhw, C, Cout, dtype, bias = case
    N, H, W = nhw
    M = N * H * W
    x, w, b, dy = _operands(nhw, C, Cout, dtype, bias, seed=11 + C + Cout)
    y_ref, _, dw_ref, db_ref = CC.conv_reference(x, w, b, dy)
    xb = ops.pad_border(_cl(x))
    w_fwd = MC.weight_operands(w.cuda(), dtype)[0]
    bd = None if b is None else b.cuda()
    dyd = CC.rows(dy).cuda().contiguous()
    snap = snapshot(xb=xb, w=w_fwd, bias=bd, dy=dyd)
    p = ops.conv3x3_plan(dtype, N, H, W, C, Cout)
    assert p.ok and p.n_tiles == -(-Cout // 256) and p.m_tiles == -(-M // 256)

    # ---- forward
    out, check = guarded(M, Cout, dtype)
    ops.conv3x3_fwd(xb, w_fwd, bd, out=out)
    check(what="conv3x3_fwd")
    A = CC.windows(CC.bordered(x)).double()
    B = w.permute(0, 2, 3, 1).reshape(Cout, 9 * C).double()
    yr = CC.rows(y_ref)
    worst = assert_within(out, yr, gemm_bound(A, B, yr, dtype, K=9 * C, extra=U32 * yr.abs() if bias else None), "conv3x3_fwd")
    out2, check2 = guarded(M, Cout, dtype)
    ops.conv3x3_fwd(xb, w_fwd, bd, out=out2)
    check2(what="conv3x3_fwd, second run")
    assert same_bits(out, out2), "two forward runs differ"

    # ---- weight and bias gradient
    def wgrad():
        dw3, c1 = guarded(3 * Cout, 3 * C, torch.float32)
        db, c2 = guarded(1, Cout, torch.float32) if bias else (None, None)
        ws, c3 = guarded_ws(p.wgrad_ws_elems)
        ops.conv3x3_wgrad(xb, dyd, dw3=dw3.view(3, Cout, 3 * C), db=None if db is None else db.view(Cout), ws=ws)
        c1(what="conv3x3_wgrad dw3"); c3(what="conv3x3_wgrad workspace")
        if c2:
            c2(what="conv3x3_wgrad db")
        return dw3.view(3, Cout, 3 * C), db
    dw3, db = wgrad()
    dY = CC.rows(dy).double()
    for r in range(3):
        Ar = CC.windows(CC.bordered(x), run=r).double()
        ref = dw_ref[:, :, r].permute(0, 2, 1).reshape(Cout, 3 * C)              # [co, (dx, c)] of kernel row r
        wr = assert_within(dw3[r], ref, gemm_bound(dY.t(), Ar.t(), ref, torch.float32, K=M), f"conv3x3_wgrad, kernel row {r}")
        worst = max(worst, wr)
    assert torch.equal(MC.assemble_weight_grad(dw3, Cout, C).cpu(),               # the assembly moves values, nothing else
                       torch.stack([dw3[r].cpu().view(Cout, 3, C) for r in range(3)], 1).permute(0, 3, 1, 2))
    if bias:
        worst = max(worst, assert_within(db.view(Cout), db_ref, sum_bound(dY.abs().sum(0), M, db_ref, torch.float32), "bias gradient"))
    dw3b, dbb = wgrad()
    assert same_bits(dw3, dw3b) and (not bias or same_bits(db, dbb)), "two weight-gradient runs differ"
    unchanged(snap)
    print(f"conv3x3 {case}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("case", DGRAD_CASES, ids=_id)
def test_input_gradient(case):
    nhw, C, Cout, dtype = case
    N, H, W = nhw
    M = N * H * W
    x, w, _, dy = _operands(nhw, C, Cout, dtype, False, seed=23 + C + Cout)
    _, dx_ref, _, _ = CC.conv_reference(x, w, None, dy)
    dyb = ops.pad_border(_cl(dy))
    w_flip = MC.weight_operands(w.cuda(), dtype)[1]
    snap = snapshot(dyb=dyb, w_flip=w_flip)
    out, check = guarded(M, C, dtype)
    ops.conv3x3_dgrad(dyb, w_flip, out=out)
    check(what="conv3x3_dgrad")
    A = CC.windows(CC.bordered(dy)).double()
    B = w.flip(2, 3).permute(1, 2, 3, 0).reshape(C, 9 * Cout).double()
    ref = CC.rows(dx_ref)
    worst = assert_within(out, ref, gemm_bound(A, B, ref, dtype, K=9 * Cout), "conv3x3_dgrad")
    out2, check2 = guarded(M, C, dtype)
    ops.conv3x3_dgrad(dyb, w_flip, out=out2)
    check2(what="conv3x3_dgrad, second run")
    assert same_bits(out, out2), "two input-gradient runs differ"
    unchanged(snap)
    print(f"conv3x3 dgrad {case}: worst err / bound {worst:.3f}")


def test_wrappers_validate_before_launching():
    from m3vit_amd._lib import M3Error
    xb = torch.zeros(1, 3, 3, 128, dtype=F16, device="cuda")
    w = torch.zeros(40, 9 * 128, dtype=F16, device="cuda")
    with pytest.raises(M3Error):
        ops.conv3x3_fwd(xb.float(), w.float())                                 # fp32: refused
    with pytest.raises(M3Error):
        ops.conv3x3_fwd(xb, w[:, :-8].contiguous())                            # a weight operand of the wrong size
    with pytest.raises(M3Error):
        ops.conv3x3_fwd(xb, w, out=torch.empty(1, 32, dtype=F16, device="cuda"))   # an undersized output
    with pytest.raises(M3Error):
        ops.conv3x3_fwd(torch.zeros(1, 3, 3, 64, dtype=F16, device="cuda"), torch.zeros(40, 9 * 64, dtype=F16, device="cuda"))
    with pytest.raises(M3Error):
        ops.conv3x3_wgrad(xb, torch.zeros(1, 40, dtype=F16, device="cuda"), ws=torch.empty(8, device="cuda"))
    with pytest.raises(M3Error):
        ops.pad_border(torch.zeros(1, 16, 2, 2, dtype=F16, device="cuda"))      # not channels-last
