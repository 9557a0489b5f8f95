#!/usr/bin/env python3
"""What the opt-in routing statistics (BackboneEngine moe_stats=True: one m3_moe_stats launch per MoE block and task pass,
inside the captured step) cost on the bench workload - configs[1], fp16, batch 128, two task passes on two streams
(m3vit_amd.step.MultiTaskStep, hipGraph replay).  Prints ms/step with the statistics off and on, and the statistics the
last step left (read once, after the timing).
    python tools/moe_stats_bench.py [--steps 20] [--only on|off]
For the time per launch: rocprofv3 --kernel-trace --stats -- python tools/moe_stats_bench.py --only on
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from m3vit_amd.config import BackboneConfig, init_params  # noqa: E402
from m3vit_amd.step import MultiTaskStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--only", choices=("on", "off"), default=None)
args = ap.parse_args()

B = 128
cfg = BackboneConfig(img_size=(224, 224), embed_dim=384, depth=12, num_heads=12, mlp_ratio=4.0, moe_mlp_ratio=1.0,
                     moe_experts=16, moe_top_k=4, gate_dim=386, multi_gate=True)
params = init_params(cfg, seed=1)
g = torch.Generator().manual_seed(1000)
images = torch.randn(B, 3, *cfg.img_size, generator=g).cuda()
dtok = (torch.randn(B, cfg.num_tokens, cfg.embed_dim, generator=g) * 0.05).cuda()
for flag in ((False, True) if args.only is None else (args.only == "on",)):
    run = MultiTaskStep(cfg, params, batch=B, dtype=torch.float16, tasks=[0, 1], moe_stats=flag)
    run.bind(images, dtok)
    run.step()
    torch.cuda.synchronize()
    run.capture()
    for _ in range(args.warmup):
        run.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run.step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    print(f"moe_stats={'on ' if flag else 'off'}: {dt * 1e3:8.3f} ms/step  ({run.launch}, {len(run.engs)} stream(s), "
          f"{args.steps} steps)", flush=True)
    if flag:
        for task, eng in zip(run.tasks, run.engs):
            blocks, total = eng.moe_stats()
            an = total["analysis"]
            print(f"  task {task}: gate_entropy {an['gate_entropy']:.4f}  top1_prob_mean {an['top1_prob_mean']:.4f}  "
                  f"dead_expert_ratio {an['dead_expert_ratio']:.3f}  expert_load_cv {an['expert_load_cv']:.4f}  "
                  f"moe_out_norm_ratio {an['moe_out_norm_ratio']:.4f}  ({total['moe_blocks']} MoE blocks)", flush=True)
    del run
    torch.cuda.empty_cache()
