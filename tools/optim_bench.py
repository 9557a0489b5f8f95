#!/usr/bin/env python3
"""The optimizer tail of a training step at BASELINE configs[1]'s real parameter set: "gradients ready -> operand copies fresh"
in three forms, five alternating rounds each, device events around `--iters` iterations after a warm-up:
  (i)   torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(foreach=True) + engine.prepare_weights()
  (ii)  the same with AdamW(fused=True)
  (iii) m3vit_amd.optim.FusedAdamW(max_grad_norm=..) through for_engine (its step() ends with prepare_weights())
and, in the same run, the kernels of (iii) by themselves (m3_optim_prepare, m3_optim_step, m3_cast_batch) beside the
streaming rate of m3_add_f32 on a buffer of the same element count (12 B per element): the yardstick for a memory-bound
kernel done right.  Bytes are algorithmic: the norm pass reads g (4 B per element), the AdamW step reads p, g, m, v and writes
p, m, v (28 B per element).
    python tools/optim_bench.py [--iters 50] [--rounds 5] [--out profiles/optim_step.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warmup=5):
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step.txt"))
    args = ap.parse_args()
    from m3vit_amd import ops
    from m3vit_amd.config import VIT_SMALL_MOE, BackboneConfig, init_params
    from m3vit_amd.engine import BackboneEngine
    from m3vit_amd.optim import FusedAdamW
    cfg = BackboneConfig(**VIT_SMALL_MOE)
    eng = BackboneEngine(cfg, init_params(cfg, seed=1), batch=1, dtype=torch.float16)      # batch 1: no activations to speak of
    n = eng.flat_grads.numel()
    g = torch.Generator(device="cuda").manual_seed(1)
    eng.flat_grads.copy_(torch.randn(n, generator=g, device="cuda") * 1e-3)
    params = list(eng.params.values())
    for name, p in eng.params.items():
        p.grad = eng.grads[name]
    hyper = dict(lr=1e-3, weight_decay=0.05)
    clip = 1.0
    opts = {"foreach": torch.optim.AdamW(params, foreach=True, **hyper), "fused": torch.optim.AdamW(params, fused=True, **hyper)}
    ours = FusedAdamW.for_engine(eng, max_grad_norm=clip, **hyper)

    def torch_form(key):
        def run():
            torch.nn.utils.clip_grad_norm_(params, clip)
            opts[key].step()
            eng.prepare_weights()
        return run

    forms = {"(i) clip_grad_norm_ + AdamW(foreach=True) + prepare_weights": torch_form("foreach"),
             "(ii) clip_grad_norm_ + AdamW(fused=True) + prepare_weights": torch_form("fused"),
             "(iii) FusedAdamW(max_grad_norm).for_engine step": ours.step}
    ours.step()                                  # builds the tables
    plan = ours._plan
    buf_a, buf_b = torch.zeros(n, device="cuda"), torch.ones(n, device="cuda")
    parts = {"m3_optim_prepare (norm + finalize)": (lambda: plan.prepare(max_norm=clip), 4),
             "m3_optim_step (AdamW)": (plan.step, 28),
             "m3_cast_batch (prepare_weights)": (eng.prepare_weights, None),
             "m3_add_f32 (yardstick)": (lambda: ops.add_f32(buf_a, buf_b), 12)}
    times = {k: [] for k in list(forms) + list(parts)}
    for _ in range(args.rounds):                 # alternating: a drift of the clocks lands on every variant alike
        for k, fn in forms.items():
            times[k].append(timed(fn, args.iters))
        for k, (fn, _) in parts.items():
            times[k].append(timed(fn, args.iters))
    lines = [f"optimizer tail at configs[1]: {len(params)} parameter tensors, {n} elements ({4 * n / 1e6:.1f} MB of fp32 "
             f"gradients), {plan.total} chunks; {args.rounds} alternating rounds x {args.iters} iterations, device events",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    med = {}
    for k, v in times.items():
        s = sorted(v)
        med[k] = s[len(s) // 2]
        lines.append(f"{k:68s} median {med[k]:8.3f} ms   rounds " + " ".join(f"{x:.3f}" for x in v))
    lines.append("")
    for k, (_, bpe) in parts.items():
        if bpe is not None:
            lines.append(f"{k:68s} {bpe:2d} B/element -> {bpe * n / med[k] / 1e9:7.3f} TB/s")
    rate = lambda k: parts[k][1] * n / med[k]          # noqa: E731
    lines.append(f"m3_optim_step / m3_add_f32 streaming rate: {rate('m3_optim_step (AdamW)') / rate('m3_add_f32 (yardstick)'):.2f}")
    keys = list(forms)
    lines.append(f"(iii) against (i): {med[keys[0]] / med[keys[2]]:.2f}x, against (ii): {med[keys[1]] / med[keys[2]]:.2f}x")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
