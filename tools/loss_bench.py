#!/usr/bin/env python3
"""The criterion at the NYUD shapes of BASELINE configs[4]: 8 images of 480 x 640, semseg with 40 fp32 channels-last logits
(the tensor the decoder head hands over), depth with one channel.

Per kernel, device events around `--iters` calls after a warm-up, the buffers cycled through a ring larger than the 256 MB
Infinity Cache: time and bytes per second over ALGORITHMIC bytes (cross-entropy forward: one read of pred; backward: one read
and one write; the label, lse and record traffic - 1 / C of it - is not counted), beside m3_add_f32 (12 B per element: two
reads, one write) on the same byte count in the same run: the yardstick for a memory-bound kernel done right.

End to end: criterion forward + backward for (semseg, depth) through m3vit_amd.losses.MultiTaskLoss against the same formulas
in stock torch ops (F.cross_entropy(ignore_index=255), the masked_select form of the L1), five alternating rounds, ranges;
GPU time (device events) and the host-side wall time until the calls have returned, per call.
    python tools/loss_bench.py [--iters 20] [--rounds 5] [--out profiles/loss_step.txt]
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_step.txt"))
    args = ap.parse_args()
    from m3vit_amd import losses, ops
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench needs the GPU: no number here can come from a CPU")
    B, C, H, W = 8, 40, 480, 640
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    sem = [(torch.randn(B, H, W, C, generator=g, device=dev) * 3).permute(0, 3, 1, 2) for _ in range(RING)]
    dsem = [torch.empty_like(x) for x in sem]
    dep = [torch.rand(B, 1, H, W, generator=g, device=dev) * 10 for _ in range(RING)]
    ddep = [torch.empty_like(x) for x in dep]
    lab_sem = torch.randint(0, C, (B, 1, H, W), generator=g, device=dev).float()
    lab_sem[torch.rand(B, 1, H, W, generator=g, device=dev) < 0.1] = 255
    lab_dep = torch.rand(B, 1, H, W, generator=g, device=dev) * 10
    lab_dep[torch.rand(B, 1, H, W, generator=g, device=dev) < 0.1] = 255
    assert sem[0].is_contiguous(memory_format=torch.channels_last)
    n_sem, n_dep = sem[0].numel(), dep[0].numel()
    lse = torch.empty(B, H, W, device=dev)
    ws = torch.empty(ops.loss_ws_elems(n_sem), device=dev)
    rec_s = torch.zeros(ops.LOSS_REC_WORDS, dtype=torch.int32, device=dev)
    rec_d = torch.zeros(ops.LOSS_REC_WORDS, dtype=torch.int32, device=dev)
    one = torch.ones((), device=dev)
    ya = [torch.zeros(2 * n_sem // 3, device=dev) for _ in range(RING)]          # 12 B / element: the CE backward's byte count
    yb = [torch.ones(2 * n_sem // 3, device=dev) for _ in range(RING)]
    ops.loss_ce_fwd(sem[0], lab_sem, lse=lse, ws=ws, record=rec_s)
    ops.loss_l1_fwd(dep[0], lab_dep, ws=ws, record=rec_d)

    kernels = {
        "m3_loss_ce_fwd (partials + finalize)": (lambda i: ops.loss_ce_fwd(sem[i % RING], lab_sem, lse=lse, ws=ws, record=rec_s), 4 * n_sem),
        "m3_loss_ce_bwd": (lambda i: ops.loss_ce_bwd(sem[i % RING], lab_sem, lse, rec_s, one, dpred=dsem[i % RING]), 8 * n_sem),
        "m3_loss_l1_fwd (partials + finalize)": (lambda i: ops.loss_l1_fwd(dep[i % RING], lab_dep, ws=ws, record=rec_d), 8 * n_dep),
        "m3_loss_l1_bwd": (lambda i: ops.loss_l1_bwd(dep[i % RING], lab_dep, rec_d, one, dpred=ddep[i % RING]), 12 * n_dep),
        "m3_add_f32 (yardstick, the CE backward's bytes)": (lambda i: ops.add_f32(ya[i % RING], yb[i % RING]), 12 * ya[0].numel()),
    }

    tasks = ["semseg", "depth"]
    weights = {"semseg": 1.0, "depth": 1.0}
    ours = losses.MultiTaskLoss(tasks, torch.nn.ModuleDict({"semseg": losses.SoftMaxwithLoss(), "depth": losses.DepthLoss()}),
                                dict(weights))
    gt = {"semseg": lab_sem, "depth": lab_dep}

    def stock(pred, gt_):
        """the same formulas in stock torch ops, as the reference writes them"""
        s = F.cross_entropy(pred["semseg"], gt_["semseg"][:, 0].long(), ignore_index=255)
        mask = gt_["depth"] != 255
        d = F.l1_loss(torch.masked_select(pred["depth"], mask), torch.masked_select(gt_["depth"], mask))
        return {"semseg": s, "depth": d, "total": torch.sum(torch.stack([weights["semseg"] * s, weights["depth"] * d]))}

    def step(crit):
        def run(i):
            xs = {"semseg": sem[i % RING].detach().requires_grad_(True), "depth": dep[i % RING].detach().requires_grad_(True)}
            crit(xs, gt)["total"].backward()
        return run

    forms = {"stock torch ops (cross_entropy + masked_select L1)": step(stock), "m3vit_amd.losses.MultiTaskLoss": step(ours)}
    kt = {k: [] for k in kernels}
    ft = {k: [] for k in forms}
    for _ in range(args.rounds):                 # alternating: a drift of the clocks lands on every variant alike
        for k, (fn, _) in kernels.items():
            kt[k].append(timed(fn, args.iters)[0])
        for k, fn in forms.items():
            ft[k].append(timed(fn, args.iters))
    lines = [f"criterion at configs[4]'s NYUD shapes: {B} x {H} x {W}; semseg {C} fp32 channels-last logits ({4 * n_sem / 1e6:.0f} MB), "
             f"depth 1 channel ({4 * n_dep / 1e6:.1f} MB); ring of {RING} buffers; {args.rounds} alternating rounds x {args.iters} "
             f"calls, device events", f"device: {torch.cuda.get_device_name(0)}", ""]
    med = {}
    for k, v in kt.items():
        s = sorted(v)
        med[k] = s[len(s) // 2]
        nbytes = kernels[k][1]
        lines.append(f"{k:50s} median {med[k] * 1e3:8.1f} us  range {s[0] * 1e3:8.1f} - {s[-1] * 1e3:8.1f} us   "
                     f"{nbytes / 1e6:7.1f} MB algorithmic -> {nbytes / med[k] / 1e9:6.3f} TB/s")
    rate = lambda k: kernels[k][1] / med[k]      # noqa: E731
    yard = [k for k in kernels if "yardstick" in k][0]
    ks = list(kernels)
    lines.append("")
    lines.append(f"CE forward  / yardstick rate: {rate(ks[0]) / rate(yard):.2f}   (expected: at least 0.50)")
    lines.append(f"CE backward / yardstick rate: {rate(ks[1]) / rate(yard):.2f}   (expected: at least 0.60)")
    lines.append("")
    lines.append("criterion forward + backward, (semseg, depth), per call:")
    for k, v in ft.items():
        gpu, host = sorted(x[0] for x in v), sorted(x[1] for x in v)
        lines.append(f"  {k:52s} GPU {gpu[0]:7.3f} - {gpu[-1]:7.3f} ms (median {gpu[len(gpu) // 2]:7.3f})   "
                     f"host until the calls returned {host[0]:7.3f} - {host[-1]:7.3f} ms (median {host[len(host) // 2]:7.3f})")
    fk = list(forms)
    mg = lambda k: sorted(x[0] for x in ft[k])[len(ft[k]) // 2]      # noqa: E731
    lines.append(f"  stock / ours, GPU time medians: {mg(fk[0]) / mg(fk[1]):.2f}x")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
