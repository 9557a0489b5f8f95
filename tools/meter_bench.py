#!/usr/bin/env python3
"""The task meters at the NYUD shapes of BASELINE configs[4]: 8 images of 480 x 640, semseg with 40 fp32 channels-last logits
(the tensor the decoder head hands over), depth with one channel, normals with three.

1. PerformanceMeter.update for (semseg, depth) and for (semseg, depth, normals) through m3vit_amd.meters against a plain-torch
   restatement of what the reference does per step - get_output (the NHWC permute, the int64 argmax map, the normalised copy)
   and the meters' updates with their host reads (three .item() per class, the masked_selects) - in alternating rounds; GPU time
   (device events) and the host-side wall time until the calls have returned, per call.  The buffers are cycled through a ring
   larger than the 256 MB Infinity Cache.
2. m3_meter_iou_update against m3_loss_ce_fwd on the same tensors in the same run: both read pred once (algorithmic bytes: one
   read of pred); the meter does no exp.  The expectation written down beforehand is "no slower than the cross-entropy forward";
   the ratio is reported, nothing is gated on it.
    python tools/meter_bench.py [--iters 20] [--rounds 5] [--out profiles/meter_step.txt]
"""
import argparse
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RING = 3


def timed(fn, iters, warmup=3):
    """(GPU ms per call from device events, host ms per call until the calls returned); fn(i) takes the iteration number"""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    host = (time.perf_counter() - t0) * 1e3 / iters
    b.synchronize()
    return a.elapsed_time(b) / iters, host


class PlainTorchMeters:
    """what the reference runs after every forward, restated in stock torch ops with its host reads"""

    def __init__(self, n_classes):
        self.n_classes = n_classes
        self.reads = 0
        self.tp, self.fp, self.fn = [0] * n_classes, [0] * n_classes, [0] * n_classes
        self.depth = [0.0, 0.0, 0.0]
        self.normals = [0.0] * 6

    def _item(self, t):
        self.reads += 1
        return t.item()

    def semseg(self, out, gt):
        pred = torch.max(out.detach().permute(0, 2, 3, 1), dim=3)[1].squeeze()
        gt = gt.squeeze()
        valid = gt != 255
        for i in range(self.n_classes):
            g, p = gt == i, pred == i
            self.tp[i] += self._item(torch.sum(g & p & valid))
            self.fp[i] += self._item(torch.sum(~g & p & valid))
            self.fn[i] += self._item(torch.sum(g & ~p & valid))

    def depth_(self, out, gt):
        pred, gt = out.detach().permute(0, 2, 3, 1).squeeze(), gt.squeeze()
        mask = gt != 255
        self.depth[0] += self._item(mask.float().sum())
        pred = torch.clamp(pred, min=1e-9)
        self.depth[1] += self._item(torch.masked_select(torch.pow(torch.log(gt) - torch.log(pred), 2), mask).sum())
        self.depth[2] += self._item(torch.masked_select(torch.pow(gt - pred, 2), mask).sum())

    def normals_(self, out, gt):
        pred = (F.normalize(out.detach().permute(0, 2, 3, 1), p=2, dim=3) + 1.0) * 255 / 2.0
        pred = (2 * pred / 255 - 1).permute(0, 3, 1, 2)
        gt = gt.clone()                              # (the reference overwrites the caller's label instead)
        invalid = gt == 255
        pred = pred.masked_fill(invalid, 0.0)
        gt[invalid] = 0.0
        deg = (180 / math.pi) * torch.acos(torch.clamp(torch.sum(pred * gt, 1), min=-1, max=1))
        deg = torch.masked_select(deg, ~invalid[:, 0])
        for k, v in enumerate((torch.sum(deg), torch.sum(torch.pow(deg, 2)), torch.sum((deg < 11.25).float()),
                               torch.sum((deg < 22.5).float()), torch.sum((deg < 30).float()))):
            self.normals[k] += self._item(v)
        self.normals[5] += deg.numel()
        self.reads += 1                              # masked_select sizes its result on the host

    def update(self, out, gt):
        for t in out:
            {"semseg": self.semseg, "depth": self.depth_, "normals": self.normals_}[t](out[t], gt[t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meter_step.txt"))
    args = ap.parse_args()
    from m3vit_amd import _lib, meters, ops
    if not torch.cuda.is_available():
        raise SystemExit("meter_bench needs the GPU: no number here can come from a CPU")
    B, C, H, W = 8, 40, 480, 640
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    outs = [{"semseg": (torch.randn(B, H, W, C, generator=g, device=dev) * 3).permute(0, 3, 1, 2),
             "depth": torch.rand(B, 1, H, W, generator=g, device=dev) * 10,
             "normals": torch.randn(B, H, W, 3, generator=g, device=dev).permute(0, 3, 1, 2)} for _ in range(RING)]
    lab_sem = torch.randint(0, C, (B, 1, H, W), generator=g, device=dev).float()
    lab_sem[torch.rand(B, 1, H, W, generator=g, device=dev) < 0.1] = 255
    lab_dep = torch.rand(B, 1, H, W, generator=g, device=dev) * 10 + 0.1
    lab_dep[torch.rand(B, 1, H, W, generator=g, device=dev) < 0.1] = 255
    lab_nrm = F.normalize(torch.randn(B, 3, H, W, generator=g, device=dev), dim=1)
    lab_nrm[(torch.rand(B, 1, H, W, generator=g, device=dev) < 0.1).expand(B, 3, H, W)] = 255
    gt = {"semseg": lab_sem, "depth": lab_dep, "normals": lab_nrm}
    assert outs[0]["semseg"].is_contiguous(memory_format=torch.channels_last)
    n_sem = outs[0]["semseg"].numel()

    forms, reads = {}, {}
    for tasks in (["semseg", "depth"], ["semseg", "depth", "normals"]):
        ours = meters.PerformanceMeter(tasks, "NYUD")
        plain = PlainTorchMeters(C)
        name = ", ".join(tasks)

        def run_ours(i, ours=ours, tasks=tasks):
            ours.update({t: meters.get_output(outs[i % RING][t], t) for t in tasks}, gt)

        def run_plain(i, plain=plain, tasks=tasks):
            plain.update({t: outs[i % RING][t] for t in tasks}, gt)
        forms[f"plain torch, as the reference ({name})"] = run_plain
        forms[f"m3vit_amd.meters.PerformanceMeter ({name})"] = run_ours
        plain.update({t: outs[0][t] for t in tasks}, gt)
        reads[name] = plain.reads

    lse = torch.empty(B, H, W, device=dev)
    ws_l = torch.empty(ops.loss_ws_elems(n_sem), device=dev)
    rec = torch.zeros(ops.LOSS_REC_WORDS, dtype=torch.int32, device=dev)
    ws_m = torch.empty(ops.meter_ws_elems(_lib.M3_METER_IOU, n_sem, C), dtype=torch.int32, device=dev)
    state = ops.meter_state(_lib.M3_METER_IOU, dev)
    kernels = {
        "m3_loss_ce_fwd (partials + finalize)": lambda i: ops.loss_ce_fwd(outs[i % RING]["semseg"], lab_sem, lse=lse, ws=ws_l, record=rec),
        "m3_meter_iou_update (partials + finalize)": lambda i: ops.meter_iou_update(outs[i % RING]["semseg"], lab_sem, C, ws=ws_m, state=state),
    }
    kt = {k: [] for k in kernels}
    ft = {k: [] for k in forms}
    for _ in range(args.rounds):                 # alternating: a drift of the clocks lands on every variant alike
        for k, fn in kernels.items():
            kt[k].append(timed(fn, args.iters)[0])
        for k, fn in forms.items():
            ft[k].append(timed(fn, args.iters))
    lines = [f"task meters at configs[4]'s NYUD shapes: {B} x {H} x {W}; semseg {C} fp32 channels-last logits ({4 * n_sem / 1e6:.0f} MB), "
             f"depth 1 channel, normals 3 channels; ring of {RING} buffers; {args.rounds} alternating rounds x {args.iters} calls, "
             f"device events", f"device: {torch.cuda.get_device_name(0)}", ""]
    med = {}
    for k, v in kt.items():
        s = sorted(v)
        med[k] = s[len(s) // 2]
        lines.append(f"{k:44s} median {med[k] * 1e3:8.1f} us  range {s[0] * 1e3:8.1f} - {s[-1] * 1e3:8.1f} us   "
                     f"{4 * n_sem / 1e6:6.1f} MB algorithmic -> {4 * n_sem / med[k] / 1e9:6.3f} TB/s")
    ks = list(kernels)
    lines.append(f"IoU update / CE forward, time medians: {med[ks[1]] / med[ks[0]]:.2f}   (expected beforehand: at most 1.00)")
    lines.append("")
    lines.append("one update after a forward, per call:")
    for k, v in ft.items():
        gpu, host = sorted(x[0] for x in v), sorted(x[1] for x in v)
        lines.append(f"  {k:62s} GPU {gpu[0]:7.3f} - {gpu[-1]:7.3f} ms (median {gpu[len(gpu) // 2]:7.3f})   "
                     f"host until the calls returned {host[0]:7.3f} - {host[-1]:7.3f} ms (median {host[len(host) // 2]:7.3f})")
    fk = list(forms)
    mg = lambda k: sorted(x[0] for x in ft[k])[len(ft[k]) // 2]      # noqa: E731
    for j, name in enumerate(reads):
        lines.append(f"  ({name}): plain / ours, GPU time medians: {mg(fk[2 * j]) / mg(fk[2 * j + 1]):.2f}x; blocking host reads per "
                     f"update: {reads[name]} -> 0")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
