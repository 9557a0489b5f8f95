#!/usr/bin/env python3
"""The token sharing stage (m3vit_amd.sharing.SharingStage: predictor + transition + broadcast) at T = 2 tasks, B = 128,
N = 197, D = 384, Dg = 64, fp16 - the token backbone's ViT-Small shape - in three forms, alternating rounds, device events
around `--iters` iterations after a warm-up:
  (i)   SharingStage forward, and forward + backward (two launches forward, two backward)
  (ii)  the same arithmetic in stock torch ops: the float restatement of tests/sharing_cases.py (stage(), dense form, the
        statistics' host reads left out) run on the GPU in float32 on the fp16 inputs, forward and forward + backward
  (iii) m3_add_f32 on a buffer of the forward's algorithmic bytes (12 B per element): the streaming rate this project
        measures its row kernels against
and the row pass and the compaction launch by themselves.  Bytes are algorithmic, per position: the forward reads the T rows
and the T Gumbel pairs and writes the T rows, shared_x, T scores and the bits; the backward reads x_t, d y_t, d shared_x,
shared_x, d g, G, bits and writes d x_t.
    python tools/sharing_bench.py [--iters 200] [--rounds 5] [--out profiles/sharing_stage.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters            # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharing_stage.txt"))
    args = ap.parse_args()
    import sharing_cases as SC
    from m3vit_amd import ops
    from m3vit_amd.sharing import ShareabilityPredictor, SharingStage
    T, B, N, D, Dg, dt = 2, 128, 197, 384, 64, torch.float16
    P = B * N
    c = SC.case(T, (B, N), D, Dg, "f16", hard=False, prev=True)
    I = SC.make_inputs(c)
    pred = ShareabilityPredictor(D, Dg).cuda().train()
    with torch.no_grad():
        pred.w_gate.copy_(I["w_gate"].cuda())
    stage = SharingStage(pred, T)
    xs = [I["xs"][t].cuda().view(B, N, D).requires_grad_(True) for t in range(T)]
    emb = I["task_emb"].cuda().requires_grad_(True)
    noise, prev = I["noise"].cuda(), I["prev"].cuda().view(B, N)
    dys = [torch.randn(B, N, D, device="cuda", dtype=dt) for _ in range(T)]
    dsx, dg = torch.randn(P, D, device="cuda", dtype=dt), torch.randn(T, B, N, device="cuda")
    leaves = xs + [pred.w_gate, emb]

    def ours_fwd():
        with torch.no_grad():
            return stage({t: xs[t] for t in range(T)}, prev, emb, noise=noise)

    def ours_fwd_bwd():
        outs, sh = stage({t: xs[t] for t in range(T)}, prev, emb, noise=noise)
        return torch.autograd.grad([outs[t] for t in range(T)] + [sh.x, sh.g], leaves, dys + [dsx, dg])

    def torch_stage():
        r = SC.stage(torch.stack([x.view(P, D) for x in xs]).float(), pred.w_gate, emb, noise, 1.0, False, prev_bits=prev.view(-1),
                     with_stats=False)
        return [r["y"].to(dt), r["shared_x"].to(dt), r["G"]]

    def torch_fwd():
        with torch.no_grad():
            return torch_stage()

    def torch_fwd_bwd():
        y, sx, G = torch_stage()
        return torch.autograd.grad([y, sx, G], leaves, [torch.stack([d.view(P, D) for d in dys]), dsx, dg.view(T, P)])

    # the two forward launches by themselves, on detached buffers
    xd = [x.detach().view(P, D) for x in xs]
    w, e = pred.w_gate.detach(), emb.detach()
    bits = ops.share_stage_fwd(xd, w, e, noise, 1.0, False)[2]
    fwd_bytes = P * (2 * T * D * 2 + D * 2 + T * 8 + T * 4 + 8)
    bwd_bytes = P * (3 * T * D * 2 + 2 * D * 2 + 2 * T * 4 + 8)
    n_add = fwd_bytes // 12
    buf_a, buf_b = torch.zeros(n_add, device="cuda"), torch.ones(n_add, device="cuda")
    forms = {"(i) SharingStage forward": ours_fwd, "(i) SharingStage forward + backward": ours_fwd_bwd,
             "(ii) torch restatement forward": torch_fwd, "(ii) torch restatement forward + backward": torch_fwd_bwd,
             "m3_share_stage_fwd (row pass)": lambda: ops.share_stage_fwd(xd, w, e, noise, 1.0, False),
             "m3_share_compact (index + statistics)": lambda: ops.share_compact(bits, T, prev.view(-1)),
             "(iii) m3_add_f32 (yardstick)": lambda: ops.add_f32(buf_a, buf_b)}
    # faster and different is not faster: the two forms agree on the routing before anything is timed
    ours, ref = ours_fwd(), torch_fwd()
    assert torch.equal(ours[1].bits.view(-1).cpu(), I["ref"]["bits"]), "the kernel's bits differ from the float64 restatement's"
    torch.testing.assert_close(ours[1].x.float(), ref[1].float(), rtol=2e-3, atol=2e-3)
    times = {k: [] for k in forms}
    for _ in range(args.rounds):                 # alternating: a drift of the clocks lands on every form alike
        for k, fn in forms.items():
            times[k].append(timed(fn, args.iters))
    shared = int(ours[1].count.item())
    lines = [f"token sharing stage: T = {T}, B = {B}, N = {N}, D = {D}, Dg = {Dg}, fp16; {P} positions, {shared} shared; "
             f"{args.rounds} alternating rounds x {args.iters} iterations, device events",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    med = {}
    for k, v in times.items():
        s = sorted(v)
        med[k] = s[len(s) // 2]
        lines.append(f"{k:48s} median {med[k]:8.4f} ms   rounds " + " ".join(f"{x:.4f}" for x in v))
    lines.append("")
    rate = {"fwd": fwd_bytes / med["m3_share_stage_fwd (row pass)"] / 1e9, "add": 12 * n_add / med["(iii) m3_add_f32 (yardstick)"] / 1e9}
    lines.append(f"forward row pass: {fwd_bytes // P} B/position, {fwd_bytes / 1e6:.1f} MB -> {rate['fwd']:.3f} TB/s")
    lines.append(f"m3_add_f32 on {12 * n_add / 1e6:.1f} MB -> {rate['add']:.3f} TB/s")
    lines.append(f"m3_share_stage_fwd / m3_add_f32 streaming rate: {rate['fwd'] / rate['add']:.2f}")
    bwd_ms = med["(i) SharingStage forward + backward"] - med["(i) SharingStage forward"]
    lines.append(f"backward (forward + backward minus forward): {bwd_ms:.4f} ms for {bwd_bytes // P} B/position -> "
                 f"{bwd_bytes / bwd_ms / 1e9:.3f} TB/s")
    lines.append(f"SharingStage against the torch restatement: forward {med['(ii) torch restatement forward'] / med['(i) SharingStage forward']:.2f}x, "
                 f"forward + backward {med['(ii) torch restatement forward + backward'] / med['(i) SharingStage forward + backward']:.2f}x")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
