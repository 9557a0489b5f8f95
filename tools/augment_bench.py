#!/usr/bin/env python3
"""The device augmentation at the NYUD shapes of BASELINE configs[4]: B = 8 raw samples of 480 x 640 - uint8 image, semseg,
depth, normals, edge (fp32, native size) - warped, flipped, marked and normalised to 480 x 640.

Three things, five alternating rounds of `--iters` calls after a warm-up, device events, every buffer cycled through a ring
larger than the 256 MB Infinity Cache:
  (i)   BatchAugment.__call__ (one m3_augment_batch launch), parameters drawn once per ring slot and reused;
  (ii)  the same pipeline in stock torch ops on the GPU: one grid_sample per map, the post-operations as where / div / sqrt;
  (iii) m3_add_f32 on the call's ALGORITHMIC byte count (every input read once, every output written once) in the same run:
        the yardstick of a memory-bound pass done right; the kernel's rate is given as a fraction of it.
Also: the host time until the call has returned (with and without the draw), and the host-to-device bytes of a batch against
the reference's fp32 CHW tensors.  The reference's own CPU pipeline (cv2) cannot be timed here: cv2 is not available.

Expectation, written before the first measurement: a memory-bound pass whose cubic taps (16 per pixel for image and normals)
come from L1 / L2; the uint8 image is read byte by byte.  The byte loads and the 16 taps cost issue slots, not HBM bytes:
expected 0.3 to 0.6 of the yardstick's rate, and several times faster than the stock torch pipeline, which makes about ten
passes over the maps.
    python tools/augment_bench.py [--iters 20] [--rounds 5] [--out profiles/augment_step.txt]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_step.txt"))
    args = ap.parse_args()
    from m3vit_amd import ops
    from m3vit_amd.augment import IMAGENET_MEAN, IMAGENET_STD, BatchAugment
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs the GPU: no number here can come from a CPU")
    B, H, W = 8, 480, 640
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    tasks = ["semseg", "depth", "normals", "edge"]

    def raw():
        n = torch.randn(B, H, W, 3, generator=g, device=dev)
        d = torch.rand(B, H, W, generator=g, device=dev) * 9 + 0.5
        d[torch.rand(B, H, W, generator=g, device=dev) < 0.05] = 0
        return {"image": torch.randint(0, 256, (B, H, W, 3), generator=g, device=dev, dtype=torch.uint8),
                "semseg": torch.randint(0, 40, (B, H, W), generator=g, device=dev).float(), "depth": d,
                "normals": n / n.norm(dim=-1, keepdim=True),
                "edge": (torch.rand(B, H, W, generator=g, device=dev) < 0.1).float()}

    ring = [raw() for _ in range(RING)]
    augs = [BatchAugment.from_config("NYUD", tasks) for _ in range(RING)]          # one per slot: its own output buffers
    pars = [a.draw(B, (H, W), dev) for a in augs]
    in_bytes = sum(t.numel() * t.element_size() for t in ring[0].values())
    out0 = augs[0](ring[0], pars[0])
    out_bytes = sum(t.numel() * t.element_size() for t in out0.values())
    nbytes = in_bytes + out_bytes
    n_y = nbytes // 12                                                              # m3_add_f32: 12 B per element
    ya = [torch.zeros(n_y, device=dev) for _ in range(RING)]
    yb = [torch.ones(n_y, device=dev) for _ in range(RING)]

    mean = torch.tensor(IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=dev).view(1, 3, 1, 1)
    xs = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
    ys = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)

    def stock(batch, p):
        """the same pipeline in stock torch ops: the grid from the same matrices, grid_sample per map, the post-operations"""
        A, aux = p.mats.float(), p.aux
        a = [A[:, k].view(B, 1, 1) for k in range(6)]
        u, v = a[0] * xs + a[1] * ys + a[2], a[3] * xs + a[4] * ys + a[5]
        grid = torch.stack([2 * u / (W - 1) - 1, 2 * v / (H - 1) - 1], -1)
        sc, cs, sn, fl = (aux[:, k].view(B, 1, 1) for k in range(4))
        samp = lambda t, mode: F.grid_sample(t, grid, mode=mode, padding_mode="zeros", align_corners=True)   # noqa: E731
        img = samp(batch["image"].permute(0, 3, 1, 2).float(), "bicubic")
        img = (torch.trunc(img.clamp(0, 255)) / 255 - mean) / std
        sem = samp(batch["semseg"].unsqueeze(1), "nearest")
        edge = samp(batch["edge"].unsqueeze(1), "nearest")
        dep = samp(batch["depth"].unsqueeze(1), "nearest") / sc.unsqueeze(1)
        dep = torch.where(dep == 0, 255.0, dep)
        nrm = samp(batch["normals"].permute(0, 3, 1, 2), "bicubic")
        n0 = torch.where(fl != 0, -nrm[:, 0], nrm[:, 0])
        r0, r1 = n0 * cs + nrm[:, 1] * sn, nrm[:, 1] * cs - n0 * sn
        r = torch.stack([r0, r1, nrm[:, 2]], 1)
        nn = r.norm(dim=1, keepdim=True)
        nrm = torch.where(nn == 0, 255.0, r / (nn + 1.1920929e-07))
        return {"image": img, "semseg": sem, "depth": dep, "normals": nrm, "edge": edge}

    forms = {
        "(i)   BatchAugment.__call__ (m3_augment_batch)": lambda i: augs[i % RING](ring[i % RING], pars[i % RING]),
        "(ii)  stock torch ops (grid_sample per map)": lambda i: stock(ring[i % RING], pars[i % RING]),
        "(iii) m3_add_f32 (yardstick, the call's bytes)": lambda i: ops.add_f32(ya[i % RING], yb[i % RING]),
    }
    drawn = lambda i: augs[i % RING](ring[i % RING])                              # noqa: E731  with a fresh draw per call
    ft = {k: [] for k in forms}
    dt = []
    for _ in range(args.rounds):                 # alternating: a drift of the clocks lands on every variant alike
        for k, fn in forms.items():
            ft[k].append(timed(fn, args.iters))
        dt.append(timed(drawn, args.iters))
    px = B * H * W
    lines = [f"dense-prediction augmentation at configs[4]'s NYUD shapes: {B} x {H} x {W} -> {H} x {W}; uint8 image + semseg + "
             f"depth + normals + edge (fp32); rots [0], scales [1.0, 1.2, 1.5], flips; ring of {RING} buffer sets "
             f"({RING * nbytes / 1e6:.0f} MB); {args.rounds} alternating rounds x {args.iters} calls, device events",
             f"device: {torch.cuda.get_device_name(0)}",
             f"algorithmic bytes per call: {in_bytes / 1e6:.1f} MB in + {out_bytes / 1e6:.1f} MB out = {nbytes / 1e6:.1f} MB",
             "expectation (written before measuring): memory-bound, cubic taps from cache; (i) at 0.3 - 0.6 of the yardstick's "
             "rate and several times faster than (ii)", ""]
    med = {}
    for k, v in ft.items():
        gpu, host = sorted(x[0] for x in v), sorted(x[1] for x in v)
        med[k] = gpu[len(gpu) // 2]
        lines.append(f"{k:50s} GPU median {med[k] * 1e3:8.1f} us  range {gpu[0] * 1e3:8.1f} - {gpu[-1] * 1e3:8.1f} us   "
                     f"{nbytes / med[k] / 1e9:6.3f} TB/s   host until returned {host[0] * 1e3:7.1f} - {host[-1] * 1e3:7.1f} us")
    ks = list(forms)
    lines.append("")
    lines.append(f"(i) rate / yardstick rate: {med[ks[2]] / med[ks[0]]:.2f}     (ii) / (i), GPU time medians: {med[ks[1]] / med[ks[0]]:.2f}x")
    gpu, host = sorted(x[0] for x in dt), sorted(x[1] for x in dt)
    lines.append(f"(i) with a fresh draw per call (host random numbers, one pinned buffer, one non-blocking copy): GPU "
                 f"{gpu[0] * 1e3:.1f} - {gpu[-1] * 1e3:.1f} us, host until returned {host[0] * 1e3:.1f} - {host[-1] * 1e3:.1f} us")
    ours_h2d = in_bytes + 64 * B
    ref_h2d = px * 4 * (3 + 1 + 1 + 3 + 1)
    lines.append(f"host-to-device bytes per batch: raw maps + parameters {ours_h2d / 1e6:.1f} MB ({ours_h2d / px:.1f} B / pixel; "
                 f"{(ours_h2d - px * 6) / 1e6:.1f} MB with semseg and edge as uint8) against the reference's fp32 CHW tensors "
                 f"{ref_h2d / 1e6:.1f} MB ({ref_h2d / px:.0f} B / pixel)")
    lines.append("the reference's CPU pipeline (cv2.warpAffine per map on the loader's workers) is unmeasured: cv2 is not available here")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
