"""GPU: the module side of the GEMM convolutions - Conv3x3 against nn.Conv2d, and the conv="gemm" option of
VisionTransformerUpHead and TamModule against conv="miopen" and against the fp32 module, in the form of
test_modules_gpu.py::test_head_fused_resize_matches_torch_stages (its rule and constants: the new path must sit as close to
the fp32 module as MIOpen's fp16 path does - e_new < 1.5 e_miopen + 1e-3 for outputs, + 5e-3 for parameter gradients, the
biases in front of a batch norm left out).  Each test also pins that the GEMM path really ran, by counting
Conv3x3Fn.forward calls."""
import contextlib
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_common as CC                                          # noqa: E402
from kernel_contract import U32, assert_within, gemm_bound, same_bits   # noqa: E402

from m3vit_amd import conv as MC                                  # noqa: E402

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = a.detach().double().cpu().flatten(); b = b.detach().double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


@contextlib.contextmanager
def counted():
    """the shapes of the inputs Conv3x3Fn.forward is called with"""
    calls, orig = [], MC.Conv3x3Fn.forward
    MC.Conv3x3Fn.forward = staticmethod(lambda ctx, x, *a: (calls.append(tuple(x.shape)), orig(ctx, x, *a))[1])
    try:
        yield calls
    finally:
        MC.Conv3x3Fn.forward = orig


def test_conv3x3_module_against_conv2d_and_float64():
    torch.manual_seed(1)
    N, C, Cout, H, W = 3, 128, 256, 9, 10
    ours, theirs = MC.Conv3x3(C, Cout).cuda(), nn.Conv2d(C, Cout, 3, 1, 1).cuda()
    assert list(ours.state_dict()) == list(theirs.state_dict())
    theirs.load_state_dict(ours.state_dict())
    x16 = torch.randn(N, C, H, W).half()
    dy = torch.randn(N, Cout, H, W).half()
    w16 = ours.weight.detach().cpu().half()                         # both paths multiply the fp16 copy of the weight
    y_ref, dx_ref, dw_ref, db_ref = CC.conv_reference(x16, w16, ours.bias.detach().cpu(), dy)
    res = {}
    for name, m in (("gemm", ours), ("miopen", theirs)):
        x = x16.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        with counted() as calls, torch.autocast("cuda", dtype=torch.float16):
            y = m(x)
        assert len(calls) == (1 if name == "gemm" else 0), (name, calls)
        assert y.dtype == torch.float16 and y.shape == (N, Cout, H, W) and y.is_contiguous(memory_format=torch.channels_last)
        y.backward(dy.cuda())
        res[name] = (y, x.grad, m.weight.grad, m.bias.grad)
    A = CC.windows(CC.bordered(x16)).double()
    B = w16.permute(0, 2, 3, 1).reshape(Cout, 9 * C).double()
    yr = CC.rows(y_ref)
    assert_within(CC.rows(res["gemm"][0]), yr, gemm_bound(A, B, yr, torch.float16, K=9 * C, extra=U32 * yr.abs()), "Conv3x3 forward")
    for i, (what, ref) in enumerate((("output", y_ref), ("input gradient", dx_ref), ("weight gradient", dw_ref), ("bias gradient", db_ref))):
        e_new, e_old = rel(res["gemm"][i], ref), rel(res["miopen"][i], ref)
        print(f"Conv3x3 {what}: rel err vs float64 {e_new:.2e} (MIOpen {e_old:.2e})")
        assert e_new < 1.5 * e_old + 1e-3, (what, e_new, e_old)
    assert res["gemm"][2].dtype == torch.float32 and res["gemm"][2].shape == ours.weight.shape


def test_conv3x3_module_falls_back_to_miopen_bits():
    """an fp32 input (with or without autocast) or C = 64 goes to nn.Conv2d.forward - pinned by watching _conv_forward - and the
    result has the bits of nn.Conv2d.forward on the same parameters.  MIOpen is asked for its deterministic algorithms for the
    comparison, and both calls read the same parameter tensors: with the default algorithms, an nn.Conv2d module holding a copy
    of the weights gave an fp32 output one ulp (2.4e-7) away from the same nn.Conv2d.forward call made through Conv3x3 on the
    MI355X - a difference inside MIOpen that no comparison of bits survives."""
    torch.manual_seed(2)
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    seen, orig = [], nn.Conv2d._conv_forward
    nn.Conv2d._conv_forward = lambda self, *a: (seen.append(type(self).__name__), orig(self, *a))[1]
    try:
        for C, dtype, auto in ((128, torch.float32, False), (128, torch.float32, True), (64, torch.float16, True)):
            ours = MC.Conv3x3(C, 128).cuda()
            x = torch.randn(2, C, 5, 6, device="cuda").to(dtype).contiguous(memory_format=torch.channels_last)
            del seen[:]
            with counted() as calls, torch.autocast("cuda", dtype=torch.float16, enabled=auto), torch.no_grad():
                nn.Conv2d.forward(ours, x)                          # (MIOpen settles on its algorithm in the first call of a shape)
                yb, ya = nn.Conv2d.forward(ours, x), ours(x)
            assert calls == [] and seen == ["Conv3x3"] * 3, (calls, seen)       # the third is ours(x): nn.Conv2d.forward took it
            assert same_bits(ya, yb), (C, dtype, auto, float((ya.float() - yb.float()).abs().max()))
    finally:
        nn.Conv2d._conv_forward = orig
        torch.backends.cudnn.deterministic = was


def _three_way(make, inputs, run, skip_bias, n_calls):
    """make(conv=, amp=) -> module; run(module, inputs) -> output tensor.  The GEMM module, the MIOpen fp16 module and the
    fp32 module with the same weights: outputs and every parameter gradient by the rule of the module docstring"""
    a, b, ref = make("gemm", True), make("miopen", True), make("miopen", False)
    assert list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict()); ref.load_state_dict(a.state_dict())
    with counted() as calls:
        ya = run(a, inputs, True)
    assert len(calls) == n_calls, calls
    with counted() as calls:
        yb, yr = run(b, inputs, True), run(ref, inputs, False)
    assert calls == []
    assert ya.shape == yr.shape
    ea, eb = rel(ya, yr), rel(yb, yr)
    print(f"outputs vs the fp32 module: gemm {ea:.2e}, miopen {eb:.2e}")
    assert ea < 1.5 * eb + 1e-3, (ea, eb)
    w = torch.randn_like(yr)
    for y in (ya, yb, yr):
        (y.float() * w).sum().backward()
    shown = []
    for (n, p), (_, q), (_, r) in zip(a.named_parameters(), b.named_parameters(), ref.named_parameters()):
        if skip_bias(n):
            continue                      # (a bias in front of a batch norm has a zero gradient: rounding noise only)
        ga, gb = rel(p.grad, r.grad), rel(q.grad, r.grad)
        shown.append((n, f"{ga:.1e}", f"{gb:.1e}"))
        assert ga < 1.5 * gb + 5e-3, (n, ga, gb)
    print("parameter gradients vs the fp32 module (gemm, miopen):", shown)


def test_head_gemm_convolutions_match_miopen_stages():
    """Measured on the MI355X (the statistic is an error against the fp32 head, dominated by ReLU flips and batch-norm
    statistics over 72 pixels, and MIOpen's own part of it moves from run to run): over 12 other seeds and batch sizes 3 and 8
    the worst gemm / miopen ratio of a parameter gradient's error was 1.19 (miopen / gemm: 1.54) and the logits sat at
    1.0-1.1e-3 against MIOpen's 1.3-1.5e-3; this test passed on one box and, on another, missed the rule for one parameter
    (syncbn_fc_0.bias: 0.0591 against 1.5 x 0.0351 + 5e-3 = 0.0576)."""
    from m3vit_amd.heads import VisionTransformerUpHead
    torch.manual_seed(4)
    tok = torch.randn(3, 4 * 6 + 1, 128, device="cuda")

    def make(conv, amp):
        torch.manual_seed(5)
        return VisionTransformerUpHead(img_size=(64, 96), embed_dim=128, channels=128, num_classes=40, amp=amp, conv=conv).cuda().train()
    _three_way(make, tok, lambda m, t, amp: m(t),
               lambda n: n.startswith("conv_") and n.endswith(".bias") and n != "conv_4.bias", n_calls=4)


def test_head_gemm_convolutions_read_the_bordered_stage_output():
    """stages 1-3 of the conv="gemm" head take the previous stage's ReLU + x2 output as a zero-bordered operand (no copy),
    stage 0 a plain channels-last tensor"""
    from m3vit_amd.heads import VisionTransformerUpHead
    torch.manual_seed(6)
    head = VisionTransformerUpHead(img_size=(64, 96), embed_dim=128, channels=128, num_classes=7, amp=True, conv="gemm").cuda().train()
    seen, orig = [], MC.Conv3x3Fn.forward
    MC.Conv3x3Fn.forward = staticmethod(lambda ctx, x, w, b, bordered: (seen.append((tuple(x.shape[2:]), bordered)), orig(ctx, x, w, b, bordered))[1])
    try:
        y = head(torch.randn(2, 25, 128, device="cuda"))
    finally:
        MC.Conv3x3Fn.forward = orig
    assert seen == [((4, 6), False), ((8, 12), True), ((16, 24), True), ((32, 48), True)], seen
    assert y.shape == (2, 7, 64, 96)


def test_tam_gemm_convolutions_match_miopen():
    from m3vit_amd.heads import TamModule
    torch.manual_seed(7)
    feats = {t: torch.randn(2, 128, 8, 12, device="cuda") for t in ("a", "b")}

    def make(conv, amp):
        torch.manual_seed(8)
        return TamModule(["a", "b"], 128, {"a": 5, "b": 1}, conv=conv).cuda().train()

    def run(m, f, amp):
        with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
            out = m(f)
        return torch.cat([out["a"], out["b"]], 1)
    # a convolution's bias in front of a norm layer: layers0-3, encoder, decoder (index 0 of a Sequential that has a norm)
    _three_way(make, feats, run, lambda n: n.endswith(".0.bias") and not n.startswith("layers4"), n_calls=5)
