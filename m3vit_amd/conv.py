"""The decoder heads' 3 x 3, stride-1, padding-1 convolutions on the project's own GEMM kernels (csrc/conv.hip), opt-in.

`Conv3x3` is an `nn.Conv2d` (same parameters, same `state_dict` keys) whose forward takes the GEMM path when the input is a
16-bit channels-last CUDA tensor - or the interior of a zero-bordered buffer, see `relu_up2x_bordered` - and
`m3_conv3x3_plan` accepts the shape for the forward, the input gradient and the weight gradient; anything else is
`nn.Conv2d.forward` (MIOpen), silently.  `Conv3x3Fn` is the autograd Function behind it:

  forward   bordered x [N, H+2, W+2, C]  @  weight.permute(0, 2, 3, 1) as [Cout, 9 C]   -> y [N, Cout, H, W] channels-last
  backward  dx from the bordered dy and the weight flipped in both spatial directions as [C, 9 Cout] (the same kernel),
            d weight / d bias from three weight-gradient problems, one per kernel row, assembled with a permute.

The 16-bit weight operands are made from the fp32 master weight in every forward / backward (a cast and a permute of a
few hundred KB).  A bordered activation travels as an ordinary tensor: the NCHW-shaped view of the buffer's interior, marked
by `relu_up2x_bordered`, which made it; `bordered_buffer` gives the buffer back (or None for any other tensor).
"""
import torch
import torch.nn as nn

_16BIT = (torch.float16, torch.bfloat16)


def bordered_buffer(x, marked=None):
    """the bordered buffer [N, H+2, W+2, C] behind a tensor made by relu_up2x_bordered (checked by its geometry), else None.
    marked: the caller knows the answer to "was it marked" (an autograd Function, whose inputs need not be the caller's objects)"""
    if not (getattr(x, "_m3_zero_border", False) if marked is None else marked) or x.dim() != 4:
        return None
    N, C, H, W = x.shape
    HB, WB = H + 2, W + 2
    if x.stride() != (HB * WB * C, 1, WB * C, C) or x.storage_offset() < (WB + 1) * C:
        return None
    return torch.as_strided(x.detach(), (N, HB, WB, C), (HB * WB * C, WB * C, C, 1), x.storage_offset() - (WB + 1) * C)


def weight_operands(weight, dtype, forward=True, dgrad=True):
    """(forward operand [Cout, 9 C], input-gradient operand [C, 9 Cout]) of a [Cout, C, 3, 3] weight: K order (dy, dx, c),
    the second flipped in both spatial directions and transposed.  None for one that is not asked for"""
    Cout, C = weight.shape[:2]
    w = weight.detach()
    return (w.permute(0, 2, 3, 1).reshape(Cout, 9 * C).to(dtype) if forward else None,
            w.flip(2, 3).permute(1, 2, 3, 0).reshape(C, 9 * Cout).to(dtype) if dgrad else None)


def assemble_weight_grad(dw3, Cout, C):
    """the three [Cout, 3 C] results (row dy: columns (dx, c)) -> d weight [Cout, C, 3, 3]"""
    return dw3.view(3, Cout, 3, C).permute(1, 3, 0, 2).contiguous()


class Conv3x3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, bordered=False):
        from . import ops
        xb = bordered_buffer(x, marked=True) if bordered else ops.pad_border(x.detach())
        N, C, H, W = x.shape
        Cout = weight.shape[0]
        w_fwd = weight_operands(weight, x.dtype, dgrad=False)[0]
        b32 = None if bias is None else bias.detach().float().contiguous()
        y = ops.conv3x3_fwd(xb, w_fwd, b32)
        ctx.save_for_backward(xb, weight)
        ctx.has_bias = bias is not None
        return y.view(N, H, W, Cout).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        from . import ops
        xb, weight = ctx.saved_tensors
        N, HB, WB, C = xb.shape
        H, W, Cout = HB - 2, WB - 2, weight.shape[0]
        g = g.to(xb.dtype).contiguous(memory_format=torch.channels_last)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            w_flip = weight_operands(weight, xb.dtype, forward=False)[1]
            dx = ops.conv3x3_dgrad(ops.pad_border(g), w_flip).view(N, H, W, C).permute(0, 3, 1, 2)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            db = torch.empty(Cout, dtype=torch.float32, device=g.device) if ctx.has_bias else None
            dw3 = ops.conv3x3_wgrad(xb, g.permute(0, 2, 3, 1).reshape(N * H * W, Cout), db=db)
            dw = assemble_weight_grad(dw3, Cout, C).to(weight.dtype)
            if db is not None:
                db = db.to(weight.dtype)
        return dx, dw, db, None


class ReluUp2xBorderedFn(torch.autograd.Function):
    """ReluUp2xFn of heads.py with the output written into the interior of a zero-bordered buffer
    (m3_relu_up2x_fwd_bordered); the backward is the dense one"""

    @staticmethod
    def forward(ctx, x, relu):
        from . import ops
        ctx.save_for_backward(x)
        ctx.relu = bool(relu)
        return ops.relu_up2x_fwd_bordered(x, relu=ctx.relu)[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        from . import ops
        x, = ctx.saved_tensors
        if g.dtype not in (x.dtype, torch.float32):
            g = g.float()
        return ops.relu_up2x_bwd(g.contiguous(memory_format=torch.channels_last), x, relu=ctx.relu), None


def relu_up2x_bordered(x, relu=True):
    """bilinear x2 of relu(x) (channels-last, 16-bit) as the marked interior of a zero-bordered buffer: the next Conv3x3
    reads it in place"""
    y = ReluUp2xBorderedFn.apply(x, relu)
    y._m3_zero_border = True
    return y


class Conv3x3(nn.Conv2d):
    """nn.Conv2d(cin, cout, 3, 1, 1) with the GEMM path where it applies (module docstring); MIOpen everywhere else"""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=True, **kw):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, bias=bias, **kw)

    def gemm_dtype(self, x):
        """the 16-bit dtype the GEMM path would run this input in, or None: MIOpen takes the call"""
        if (self.kernel_size, self.stride, self.padding, self.dilation, self.groups) != ((3, 3), (1, 1), (1, 1), (1, 1), 1):
            return None
        if self.padding_mode != "zeros" or not isinstance(x, torch.Tensor) or x.dim() != 4 or not x.is_cuda or x.dtype not in _16BIT:
            return None
        if torch.is_autocast_enabled():
            auto = torch.get_autocast_dtype("cuda") if hasattr(torch, "get_autocast_dtype") else torch.get_autocast_gpu_dtype()
            if auto != x.dtype:
                return None
        elif self.weight.dtype != x.dtype:
            return None
        if bordered_buffer(x) is None and not x.is_contiguous(memory_format=torch.channels_last):
            return None
        from . import _lib, ops
        N, C, H, W = x.shape
        try:
            p = ops.conv3x3_plan(x.dtype, N, H, W, C, self.out_channels)
        except _lib.M3Error:
            return None
        return x.dtype if (p.ok and p.dgrad_ok and C == self.in_channels) else None

    def forward(self, x):
        if self.gemm_dtype(x) is None:
            return super().forward(x)
        return Conv3x3Fn.apply(x, self.weight, self.bias, bordered_buffer(x) is not None)
