"""expert load of bench.py's synthetic step (random-init router on random images): rows per expert per MoE layer and task
pass, max / mean - what the grouped kernels' balance provisions see.   python tools/route_counts_probe.py --config 3|4|1"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=3)
ap.add_argument("--units", action="store_true", help="all counts of every MoE launch of every task pass and the longest "
                "work unit of the balanced weight gradient under both ways to cut a group")
args = ap.parse_args()
import bench
from m3vit_amd.config import BackboneConfig, init_params
from m3vit_amd.step import MultiTaskStep
wl = bench.WORKLOADS[args.config]
cfg = BackboneConfig(**wl["cfg"])
dev = torch.device("cuda", 0)
run = MultiTaskStep(cfg, init_params(cfg, seed=1), batch=wl["batch"], dtype=torch.float16, device=str(dev), cv_weight=0.01,
                    parallel_tasks=False, graph=False)
g = torch.Generator().manual_seed(1000)
images = torch.randn(wl["batch"], 3, *cfg.img_size, generator=g).to(dev)
dtok = (torch.randn(wl["batch"], cfg.num_tokens, cfg.embed_dim, generator=g) * 0.05).to(dev)
run.bind(images, dtok)
eng = run.eng
if args.units:
    # every task pass of the step (the engine's context keeps the last pass only): all counts per MoE launch and the
    # longest work unit of the balanced weight gradient - the map the kernels use (equal shares, m3_wgrad_unit_of's rule)
    # against units of chunk_rows rows with the remainder on a group's last one
    from m3vit_amd import ops
    R = wl["batch"] * cfg.num_tokens * cfg.moe_top_k
    chunk = ops.wgrad_launch_plan(R, cfg.embed_dim, cfg.embed_dim, cfg.moe_experts, torch.float16, grouped=True).chunk_rows
    print(f"# config {args.config}: routed rows {R}, chunk_rows {chunk}")
    eng.prepare_weights()
    eng.zero_grad()
    ratios = []
    for t in run.tasks:
        run._full(eng, t)
        torch.cuda.synchronize()
        for i, a in enumerate(eng.act):
            r = a.get("route") if isinstance(a, dict) else None
            if r is None:
                continue
            c = r.counts.cpu().int().tolist()
            n = [-(-x // chunk) for x in c]
            cut = max(min(x, chunk) for x in c)
            eq = max((-(-(-(-x // k)) // 64) * 64 if k > 1 else x) for x, k in zip(c, n) if k)
            ratios.append(eq / cut)
            print(f"task {t} block {i}: units {sum(n)} longest unit chunk-cut {cut} equal-shares {eq} ratio {eq / cut:.3f} counts {c}")
    print(f"# mean ratio {sum(ratios) / len(ratios):.3f} over {len(ratios)} launches")
    sys.exit(0)
run.serial_step()
torch.cuda.synchronize()
for i, a in enumerate(eng.act):
    r = a.get("route") if isinstance(a, dict) else None
    if r is None:
        continue
    c = r.counts.cpu().float()
    print(f"block {i}: experts {c.numel()} rows {int(c.sum())} mean {c.mean():.0f} max {int(c.max())} min {int(c.min())} max/mean {float(c.max() / c.mean()):.2f} "
          f"top4 {sorted(c.int().tolist(), reverse=True)[:4]}")
