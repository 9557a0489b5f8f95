"""Shared by the 3 x 3 convolution tests (imported, not collected): the host restatement of the bordered layout - the pixel
table, the window of a pixel as the kernels address it - and the float64 references."""
import torch
import torch.nn.functional as F


def pixel_table(N, H, W):
    """what m3_conv3x3_index writes: pixel (n, y, x) -> index of bordered pixel (n, y, x) in [N, H+2, W+2]"""
    n, y, x = torch.meshgrid(torch.arange(N), torch.arange(H), torch.arange(W), indexing="ij")
    return ((n * (H + 2) + y) * (W + 2) + x).reshape(-1)


def bordered(x):
    """[N, C, H, W] -> zero-bordered channels-last [N, H+2, W+2, C]"""
    return F.pad(x.permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1)).contiguous()


def windows(xb, run=None):
    """the A operand as the kernels read it from the flat bordered buffer xb [N, H+2, W+2, C]: row m = the three runs of
    3 C elements that start at element table[m] * C + run * (W + 2) * C -> [M, 9 C] (run = None) or one run's [M, 3 C]"""
    N, HB, WB, C = xb.shape
    flat = xb.reshape(-1)
    start = pixel_table(N, HB - 2, WB - 2) * C
    runs = [flat[(start + r * WB * C).unsqueeze(1) + torch.arange(3 * C).unsqueeze(0)] for r in range(3)]
    return torch.cat(runs, 1) if run is None else runs[run]


def conv_reference(x, w, b, dy):
    """float64 F.conv2d(x, w, b, padding=1) and its autograd gradients for the output gradient dy: (y, dx, dw, db)"""
    x = x.double().requires_grad_(True)
    w = w.double().requires_grad_(True)
    b = None if b is None else b.double().requires_grad_(True)
    y = F.conv2d(x, w, b, padding=1)
    g = torch.autograd.grad(y, [x, w] + ([b] if b is not None else []), dy.double())
    return y.detach(), g[0], g[1], (g[2] if b is not None else None)


def rows(t):
    """[N, C, H, W] -> [N H W, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
