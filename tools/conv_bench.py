#!/usr/bin/env python3
"""The heads' 3 x 3 convolutions on the GEMM path (m3_conv3x3_fwd / _dgrad / _wgrad) against MIOpen (F.conv2d on channels-last
fp16 tensors and aten.convolution_backward) per shape: the four stages of the NYUD head at 8 images (30 x 40 384 -> 256, then
60 x 80, 120 x 160, 240 x 320 at 256 -> 256) and one TAM shape (1280 -> 256 at 256 x 256, --tam-batch images).
Operands STREAMED as in tools/vitb_gemm_bench.py (a ring of activation sets larger than the 256 MiB Infinity Cache: inside
the training step a convolution's input was written launches earlier), HIP events around --iters calls, both paths in one
process, alternating, best of --rounds.  The GEMM path's times are the kernels behind the C ABI entry (the pixel table is
cached, the bordered input is what the previous stage wrote); its dgrad line also shows the dense -> bordered copy of dY it
needs in front.  FLOPs = 2 M Cout 9 C for each of the three.
    python tools/conv_bench.py [--iters 10] [--rounds 3] [--only NAME] [--tam-batch 4]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from m3vit_amd import conv as MC  # noqa: E402
from m3vit_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--only", default="")
ap.add_argument("--tam-batch", type=int, default=4)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("conv_bench: no GPU - nothing is measured without one")
dt, dev = torch.float16, torch.device("cuda:0")


def time_us(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(args.iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / args.iters


def compare(name, flops, variants):
    best = {k: 1e30 for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            best[k] = min(best[k], time_us(fn))
    print(f"  {name:8s} " + "   ".join(f"{k} {v:9.1f} us {flops / v / 1e6:7.1f} TFLOP/s" for k, v in best.items()), flush=True)


def case(name, N, H, W, C, Cout):
    if args.only and args.only not in name:
        return
    M = N * H * W
    p = ops.conv3x3_plan(dt, N, H, W, C, Cout)
    assert p.ok and p.dgrad_ok, name
    ring = int(max(2, min(8, -(-320e6 // (M * (C + Cout) * 2)))))
    print(f"{name}: N={N} {H}x{W} {C}->{Cout}  M={M} row tiles {p.m_tiles} x {p.n_tiles}, K tiles {p.k_tiles}, wgrad tile {p.wgrad_tile} "
          f"parts {p.wgrad_splits}, ring {ring}", flush=True)
    xs = [torch.randn(N, C, H, W, device=dev, dtype=dt).contiguous(memory_format=torch.channels_last) for _ in range(ring)]
    dys = [torch.randn(N, Cout, H, W, device=dev, dtype=dt).contiguous(memory_format=torch.channels_last) for _ in range(ring)]
    w = (torch.randn(Cout, C, 3, 3, device=dev) * 0.05).to(dt).contiguous(memory_format=torch.channels_last)
    b = torch.randn(Cout, device=dev)
    w_fwd, w_flip = MC.weight_operands(w, dt)
    xbs = [ops.pad_border(x) for x in xs]
    dybs = [ops.pad_border(d) for d in dys]
    dyr = [d.permute(0, 2, 3, 1).reshape(M, Cout) for d in dys]
    y = torch.empty(M, Cout, device=dev, dtype=dt)
    dx = torch.empty(M, C, device=dev, dtype=dt)
    dw3 = torch.empty(3, Cout, 3 * C, device=dev)
    db = torch.empty(Cout, device=dev)
    ws = torch.empty(max(p.wgrad_ws_elems, 4), device=dev)
    dyb = torch.empty_like(dybs[0])
    st = [0]

    def nxt():
        st[0] += 1
        return st[0] % ring
    flops = 2.0 * M * Cout * 9 * C
    bh = b.half()
    mask_x, mask_w = (True, False, False), (False, True, True)

    def mi_bwd(mask):
        def f():
            i = nxt()
            torch.ops.aten.convolution_backward(dys[i], xs[i], w, [Cout], [1, 1], [1, 1], [1, 1], False, [0, 0], 1, mask)
        return f
    compare("forward", flops, {"gemm": lambda: ops.conv3x3_fwd(xbs[nxt()], w_fwd, b, out=y),
                               "miopen": lambda: F.conv2d(xs[nxt()], w, bh, padding=1)})
    compare("dgrad", flops, {"gemm": lambda: ops.conv3x3_dgrad(dybs[nxt()], w_flip, out=dx),
                             "gemm+pad": lambda: ops.conv3x3_dgrad(ops.pad_border(dys[nxt()], out=dyb), w_flip, out=dx),
                             "miopen": mi_bwd(mask_x)})

    def our_wgrad():
        i = nxt()
        ops.conv3x3_wgrad(xbs[i], dyr[i], dw3=dw3, db=db, ws=ws)
    compare("wgrad", flops, {"gemm": our_wgrad, "miopen": mi_bwd(mask_w)})
    # same seeded inputs, both paths: the results agree to fp16 rounding (guide: faster and different is not faster)
    ref = F.conv2d(xs[0], w, bh, padding=1)
    got = ops.conv3x3_fwd(xbs[0], w_fwd, b).view(N, H, W, Cout).permute(0, 3, 1, 2)
    err = float((got.float() - ref.float()).norm() / ref.float().norm())
    print(f"  forward vs MIOpen on the same operands: rel {err:.1e}", flush=True)
    assert err < 2e-3, err


print(f"device {torch.cuda.get_device_name(0)}, iters {args.iters}, rounds {args.rounds} (best), fp16, streamed operands")
for nm, (h, w_, c) in zip(("stage0", "stage1", "stage2", "stage3"), ((30, 40, 384), (60, 80, 256), (120, 160, 256), (240, 320, 256))):
    case(nm, 8, h, w_, c, 256)
case("tam", args.tam_batch, 256, 256, 1280, 256)
