#!/usr/bin/env python3
"""Step time of the module path under torch DistributedDataParallel at BASELINE configs[1] (batch 128, two tasks, the joint
step: backbone(x, task_id) per task inside ONE forward, one backward - models/models.py:299-320, train/train_utils.py:423-457;
f16 activations), four legs:

  views        the plain module path (fused executor, .grad-view gradient delivery) - bench.py's `module_path`
  ddp_fused    the same model inside a ONE-rank DistributedDataParallel(device_ids=[0], find_unused_parameters=True) on the
               nccl (RCCL) backend, as train_fastmoe.py wraps it with --moe_data_distributed: autograd delivery
  autograd     fused_grads="autograd" without DDP: what the autograd delivery itself costs
  ddp_per_op   fused=False under the same one-rank DDP: the per-op autograd Functions

Each leg runs in a child process of its own under `timeout`; the parent prints one JSON line with the four legs and the
ratios ddp_fused / ddp_per_op and ddp_fused / views.
    python tools/ddp_module_bench.py [--steps 20] [--warmup 5] [--batch 128] [--legs views,ddp_fused,autograd,ddp_per_op]
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("views", "ddp_fused", "autograd", "ddp_per_op")


def run_leg(leg, steps, warmup, batch):
    import torch
    import torch.nn as nn
    sys.path.insert(0, ROOT)
    import m3vit_amd
    m3vit_amd.install_fmoe_shim()
    from m3vit_amd.config import VIT_SMALL_MOE, BackboneConfig, init_params
    from m3vit_amd.vit import VisionTransformerMoE
    kw = dict(VIT_SMALL_MOE)
    cfg = BackboneConfig(**kw)
    fused = False if leg == "ddp_per_op" else "auto"
    grads = "autograd" if leg == "autograd" else "auto"
    model = VisionTransformerMoE(vmoe_noisy_std=0.0, act_dtype=torch.float16, fused=fused, fused_grads=grads, **kw).cuda()
    model.load_state_dict(init_params(cfg, seed=1))
    model.train()
    tasks = list(range(cfg.num_tasks))

    class Joint(nn.Module):                            # the backbone once per task inside one forward (heads.MultiTaskModel)
        def __init__(self, backbone):
            super().__init__()
            self.backbone = backbone

        def forward(self, x):
            return [self.backbone(x, task_id=t) for t in tasks]

    net = Joint(model)
    ddp = leg.startswith("ddp")
    if ddp:
        import torch.distributed as dist
        from torch.nn.parallel import DistributedDataParallel
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("nccl", rank=0, world_size=1)
        net = DistributedDataParallel(net, device_ids=[0], find_unused_parameters=True)
    g = torch.Generator().manual_seed(1000)
    images = torch.randn(batch, 3, *cfg.img_size, generator=g).cuda()
    dtok = (torch.randn(batch, cfg.num_tokens, cfg.embed_dim, generator=g) * 0.05).cuda()
    params = list(model.parameters())

    def step():
        for p in params:                               # optimizer.zero_grad(set_to_none=True)
            p.grad = None
        loss = sum((tok * dtok).sum() + 0.01 * cv for tok, cv in net(images))
        loss.backward()
        with torch.no_grad():                          # stands for optimizer.step(): every parameter written in place
            torch._foreach_mul_(params, 1.0)

    for _ in range(max(warmup, 3)):                    # first use eager, second use captures the hipGraphs
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    dt_s = (time.perf_counter() - t0) / steps
    out = {"leg": leg, "ms_per_step": round(1e3 * dt_s, 3), "host_ms_per_step": round(1e3 * t_host / steps, 3),
           "images_per_s": round(batch / dt_s, 1), "fused_fallback_reason": model.fused_fallback_reason,
           "fused_grads_used": model.fused_grads_used}
    if ddp:
        import torch.distributed as dist
        dist.destroy_process_group()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per leg")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)        # (child process)
    a = ap.parse_args()
    if a.leg is not None:
        print(json.dumps(run_leg(a.leg, a.steps, a.warmup, a.batch)), flush=True)
        return 0
    res = {}
    for leg in a.legs.split(","):
        assert leg in LEGS, leg
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--leg", leg,
               "--steps", str(a.steps), "--warmup", str(a.warmup), "--batch", str(a.batch)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not lines:
            res[leg] = {"error": f"exit status {p.returncode}"}
            print(f"{leg}: exit status {p.returncode}; the remaining legs are not run", file=sys.stderr, flush=True)
            break
        res[leg] = json.loads(lines[-1])
        print(f"{leg}: {res[leg]['ms_per_step']} ms/step", file=sys.stderr, flush=True)
    ms = {k: v.get("ms_per_step") for k, v in res.items()}
    if ms.get("ddp_fused") and ms.get("ddp_per_op"):
        res["ddp_fused_over_ddp_per_op"] = round(ms["ddp_fused"] / ms["ddp_per_op"], 3)
    if ms.get("ddp_fused") and ms.get("views"):
        res["ddp_fused_over_views"] = round(ms["ddp_fused"] / ms["views"], 3)
    print(json.dumps(res))
    return 0 if all("error" not in v for v in res.values() if isinstance(v, dict)) else 1


if __name__ == "__main__":
    sys.exit(main())
