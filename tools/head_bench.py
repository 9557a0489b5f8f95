#!/usr/bin/env python3
"""Decoder head (VisionTransformerUpHead, 4 conv + 4 upsample stages) at the NYUD resolution (8 images, 480 x 640, D = 384,
40 classes): forward + backward time of the torch / MIOpen stages, fp32 and under fp16 autocast, per stage.
--conv: instead, the whole head forward + backward under fp16 autocast with its 3 x 3 convolutions on MIOpen (conv="miopen",
the default head) and on the GEMM path (conv="gemm"), alternating in one process, HIP events, best of three rounds."""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from m3vit_amd.heads import VisionTransformerUpHead  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--conv", action="store_true", help='compare conv="miopen" with conv="gemm" on the whole head and stop')
args = ap.parse_args()
dev = torch.device("cuda:0")
B, D = 8, 384
if args.conv:
    torch.manual_seed(0)
    heads = {c: VisionTransformerUpHead(img_size=(480, 640), embed_dim=D, num_classes=40, amp=True, conv=c).to(dev).train()
             for c in ("miopen", "gemm")}
    heads["gemm"].load_state_dict(heads["miopen"].state_dict())
    toks = [torch.randn(B, 30 * 40 + 1, D, device=dev, requires_grad=True) for _ in range(2)]
    best, outs = {c: 1e30 for c in heads}, {}
    for rnd in range(4):                                   # round 0 warms up (MIOpen picks its algorithms there)
        for c, h in heads.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            for i in range(5):
                y = h(toks[i % 2])
                y.float().square().mean().backward()
            e.record()
            torch.cuda.synchronize()
            outs[c] = y.detach()
            if rnd:
                best[c] = min(best[c], s.elapsed_time(e) / 5)
    for c, v in best.items():
        print(f'head 8 x 480 x 640, fp16 autocast, conv="{c}": {v:.2f} ms forward + backward', flush=True)
    d = float((outs["gemm"] - outs["miopen"]).norm() / outs["miopen"].norm())
    print(f"logits of the two heads on the same tokens and weights: rel {d:.1e}")
    sys.exit(0)
FUSED = os.environ.get("M3_HEAD_FUSED", "1") != "0"       # ReLU + x2 resize of a stage as one hand-written kernel each way
head = VisionTransformerUpHead(img_size=(480, 640), embed_dim=D, num_classes=40, fused_resize=FUSED).to(dev).train()
print(f"fused_resize={FUSED}")
tok = torch.randn(B, 30 * 40 + 1, D, device=dev, requires_grad=True)


def run(amp):
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        y = head(tok)
    y.float().square().mean().backward()


for amp in (False, True):
    for _ in range(2):
        run(amp)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 5
    for _ in range(n):
        run(amp)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    fl = 0
    for (h, w, ci) in ((30, 40, 384), (60, 80, 256), (120, 160, 256), (240, 320, 256)):
        fl += 2 * B * h * w * 256 * 9 * ci
    print(f"{'fp16 autocast' if amp else 'fp32'}: {dt * 1e3:.1f} ms fwd+bwd  (3x3 conv FLOPs fwd {fl / 1e9:.0f} G, x3 for fwd+bwd: {3 * fl / dt / 1e12:.0f} TFLOP/s)", flush=True)
# per conv at the largest stage
x = torch.randn(B, 256, 240, 320, device=dev)
conv = head.conv_3
for amp, xx in ((False, x), (True, x.half())):
    cv = conv if not amp else conv.half()
    for _ in range(2):
        cv(xx)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        cv(xx)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 5
    print(f"conv_3 forward alone {'fp16' if amp else 'fp32'} NCHW: {dt * 1e3:.2f} ms = {2 * B * 240 * 320 * 256 * 2304 / dt / 1e12:.0f} TFLOP/s", flush=True)
xh = x.half().to(memory_format=torch.channels_last)
cvh = conv.half().to(memory_format=torch.channels_last)
for _ in range(2):
    cvh(xh)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(5):
    cvh(xh)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / 5
print(f"conv_3 forward alone fp16 channels_last: {dt * 1e3:.2f} ms = {2 * B * 240 * 320 * 256 * 2304 / dt / 1e12:.0f} TFLOP/s", flush=True)
