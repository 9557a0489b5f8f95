"""CPU: the dispatch of the heads' 3 x 3 convolutions to the GEMM path (m3_conv3x3_plan is host code) and the layout it
rests on - the pixel table, the three-run window addressing with the plan's own K-tile numbers, the K order of the forward
weight operand, the flip of the input-gradient operand and the assembly of the weight gradient - restated in float64 over
bordered arrays and held against F.conv2d and its autograd.  No GPU is touched."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_common as CC                                          # noqa: E402

from m3vit_amd import _lib, ops                                   # noqa: E402
from m3vit_amd import conv as MC                                  # noqa: E402


@pytest.mark.parametrize("C", [128, 256, 384, 768, 1280])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_plan_accepts_the_head_and_tam_widths(C, dtype):
    N, H, W, Cout = 8, 30, 40, 256
    p = ops.conv3x3_plan(dtype, N, H, W, C, Cout)
    assert p.ok == 1 and _lib.CONV_REASONS[p.reason] == "ok" and p.dgrad_ok == 1
    assert _lib.GEMM_KERNELS[p.kernel] == "big" and _lib.GEMM_EPILOGUES[p.epilogue] == "plain"
    assert (p.tile_m, p.tile_n) == (256, 256)
    assert p.M == N * H * W and p.m_tiles == -(-p.M // 256) == 38 and p.n_tiles == 1
    # K = 9 C in 128-byte tiles, three runs of whole, even-numbered tile counts: the kernel's tile-pair loop never straddles a run
    assert p.seg_tiles == 3 * C * 2 // 128 and p.seg_tiles % 2 == 0 and p.k_tiles == 3 * p.seg_tiles == 9 * C * 2 // 128
    assert p.seg_jump_bytes == ((W + 2) * C - 3 * C) * 2
    assert p.bordered_pixels == N * (H + 2) * (W + 2)
    wp = ops.wgrad_launch_plan(p.M, Cout, 3 * C, 1, dtype, grouped=False, bias=True)
    assert p.wgrad_splits == wp.splits and p.wgrad_ws_elems == wp.splits * Cout * (9 * C + 1)
    assert p.wgrad_tile == ops.wgrad_tile(Cout, 3 * C, dtype)[0]


def test_plan_column_tiles_and_input_gradient_rule():
    p = ops.conv3x3_plan(torch.float16, 3, 9, 10, 128, 264)
    assert p.ok and p.n_tiles == 2 and p.m_tiles == 2 and not p.dgrad_ok       # the input gradient contracts over Cout: % 128
    p = ops.conv3x3_plan(torch.float16, 1, 1, 1, 128, 40)
    assert p.ok and (p.M, p.m_tiles, p.n_tiles, p.seg_jump_bytes) == (1, 1, 1, 0) and not p.dgrad_ok
    assert ops.conv3x3_plan(torch.bfloat16, 2, 3, 5, 256, 384).dgrad_ok == 1
    p = ops.conv3x3_plan(torch.float16, 0, 4, 4, 128, 128)
    assert p.ok and _lib.GEMM_KERNELS[p.kernel] == "none" and p.m_tiles == 0


@pytest.mark.parametrize("dtype,C,Cout,why", [(torch.float16, 64, 256, "refuse_cin"), (torch.bfloat16, 192, 256, "refuse_cin"),
                                              (torch.float32, 256, 256, "refuse_dtype"), (torch.float16, 128, 36, "refuse_cout"),
                                              (torch.float16, 1280, 256, "refuse_reach")])
def test_plan_refuses_with_a_reason(dtype, C, Cout, why):
    N, H, W = (8, 30, 40) if why != "refuse_reach" else (64, 256, 256)       # 64 x 258 x 258 x 1280 x 2 bytes > 4 GiB
    p = ops.conv3x3_plan(dtype, N, H, W, C, Cout)
    assert p.ok == 0 and p.dgrad_ok == 0 and _lib.CONV_REASONS[p.reason] == why
    assert _lib.GEMM_KERNELS[p.kernel] == "none" and p.m_tiles == 0 and p.wgrad_ws_elems == 0


def test_plan_rejects_nonsense():
    for bad in ((torch.float16, -1, 4, 4, 128, 128), (torch.float16, 1, 0, 4, 128, 128), (torch.float16, 1, 4, 4, 0, 128),
                (torch.float16, 1 << 19, 1 << 10, 1 << 10, 128, 128)):
        with pytest.raises(_lib.M3Error):
            ops.conv3x3_plan(*bad)


@pytest.mark.parametrize("N,H,W,C", [(1, 1, 1, 128), (2, 3, 5, 256), (3, 9, 10, 384)])
def test_pixel_table_and_window_reach(N, H, W, C):
    t = CC.pixel_table(N, H, W)
    p = ops.conv3x3_plan(torch.float16, N, H, W, C, 256)
    assert t.numel() == p.M == N * H * W and t.unique().numel() == t.numel()
    assert int(t.min()) == 0 and int(t.max()) == ((N - 1) * (H + 2) + H - 1) * (W + 2) + W - 1 < p.bordered_pixels
    # the kernel's addressing with the plan's numbers: K tile kt of row m starts at byte
    # table[m] * C * 2 + kt * 128 + (kt // seg_tiles) * seg_jump_bytes; the last tile of the last pixel ends inside the buffer,
    # and in fact at its very end (the bottom-right tap of the last image is the last bordered pixel)
    kt = p.k_tiles - 1
    end = int(t[-1]) * C * 2 + kt * 128 + (kt // p.seg_tiles) * p.seg_jump_bytes + 128
    assert end == p.bordered_pixels * C * 2
    # every run of every pixel is three whole bordered pixels of its own image: no run crosses into another image
    for r in range(3):
        first = t + r * (W + 2)
        assert bool((first // ((H + 2) * (W + 2)) == (first + 2) // ((H + 2) * (W + 2))).all())
        assert bool(((first + 2) // ((H + 2) * (W + 2)) == t // ((H + 2) * (W + 2))).all())


@pytest.mark.parametrize("N,H,W,C,Cout", [(1, 1, 1, 8, 16), (2, 3, 5, 16, 8), (3, 9, 10, 8, 24)])
def test_weight_operands_reproduce_conv2d_and_its_gradients(N, H, W, C, Cout):
    """the K order (dy, dx, c), the flipped and transposed operand of the input gradient and the assembly of the three
    weight-gradient results, each applied as the plain matrix product the kernels run, in float64"""
    torch.manual_seed(N * 100 + H)
    x, w, b = torch.randn(N, C, H, W).double(), torch.randn(Cout, C, 3, 3).double(), torch.randn(Cout).double()
    dy = torch.randn(N, Cout, H, W).double()
    y_ref, dx_ref, dw_ref, db_ref = CC.conv_reference(x, w, b, dy)
    w_fwd, w_flip = MC.weight_operands(w, torch.float64)
    assert w_fwd.shape == (Cout, 9 * C) and w_flip.shape == (C, 9 * Cout)
    A = CC.windows(CC.bordered(x))
    y = A @ w_fwd.t() + b
    assert torch.allclose(y, CC.rows(y_ref), rtol=1e-12, atol=1e-12)
    dx = CC.windows(CC.bordered(dy)) @ w_flip.t()
    assert torch.allclose(dx, CC.rows(dx_ref), rtol=1e-12, atol=1e-12)
    dw3 = torch.stack([CC.rows(dy).t() @ CC.windows(CC.bordered(x), run=r) for r in range(3)])
    assert torch.allclose(MC.assemble_weight_grad(dw3, Cout, C), dw_ref, rtol=1e-12, atol=1e-12)
    assert torch.allclose(CC.rows(dy).sum(0), db_ref, rtol=1e-12, atol=1e-12)
    # and the reference really is F.conv2d
    assert torch.equal(y_ref, F.conv2d(x, w, b, padding=1))


def test_module_keeps_conv2d_interface_and_falls_back_on_the_cpu():
    torch.manual_seed(0)
    a, b = MC.Conv3x3(128, 128), torch.nn.Conv2d(128, 128, 3, 1, 1)
    assert list(a.state_dict()) == list(b.state_dict()) == ["weight", "bias"]
    b.load_state_dict(a.state_dict())
    x = torch.randn(1, 128, 4, 5)
    assert a.gemm_dtype(x) is None and torch.equal(a(x), b(x))
    from m3vit_amd.heads import TamModule, VisionTransformerUpHead
    for conv in ("miopen", "gemm"):
        h = VisionTransformerUpHead(img_size=(64, 96), embed_dim=128, channels=128, conv=conv)
        assert isinstance(h.conv_0, MC.Conv3x3) == (conv == "gemm") and not isinstance(h.conv_4, MC.Conv3x3)
        t = TamModule(["a", "b"], 128, {"a": 3, "b": 1}, conv=conv)
        assert isinstance(t.layers2[0], MC.Conv3x3) == (conv == "gemm") and not isinstance(t.encoder0[0], MC.Conv3x3)
    keys = [list(VisionTransformerUpHead(img_size=(64, 96), embed_dim=128, channels=128, conv=c).state_dict()) for c in ("miopen", "gemm")]
    assert keys[0] == keys[1]
    with pytest.raises(ValueError):
        VisionTransformerUpHead(conv="auto")
