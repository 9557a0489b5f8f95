#!/usr/bin/env python3
"""The pretraining recipe (csrc/pretrain.hip, m3vit_amd/pretrain.py) at BASELINE configs[1]'s shapes - batch 128, 3 x 224 x 224
images, 1000 classes, the ViT-S MoE classification model's parameter set - each piece beside its stock-torch form on the same
device in the same run: five alternating rounds, device events around `--iters` iterations after a warm-up (GPU time) and the
wall clock until the calls have returned (host time, no synchronisation inside).  Inputs that are larger than a few MB rotate
through a ring that exceeds the 256 MB Infinity Cache (image batches, parameter sets); the logits (0.5 MB) fit any cache in
both forms.
  mix         m3_mix_batch in place              | Mixup: x.mul_(lam).add_(x.flip(0).mul_(1 - lam)); CutMix: the slice assignment
  loss        SoftTargetCrossEntropy fwd + bwd   | torch.sum(-t * log_softmax(x, -1), -1).mean() fwd + bwd
  evaluation  ClsEvalMeter.update                | cross_entropy + topk(5) + three .item()
  EMA         ModelEma.update (one launch)       | a loop over state_dict(): ema.mul_(d).add_(p, alpha=1 - d)
m3_mix_batch and m3_ema_update are also given as a streaming rate beside m3_add_f32 on the same byte count (bytes are
algorithmic: mix reads and writes every image once, 8 B per element; EMA reads two and writes one, 12 B; add the same 12 B).
Last, the whole pretrain_step with the recipe (Mixup + SoftTargetCrossEntropy + ModelEma) and without it (hard labels through
torch's nn.CrossEntropyLoss, no mixing, no EMA).
    python tools/pretrain_bench.py [--iters 20] [--rounds 5] [--batch 128] [--out profiles/pretrain_step.txt]
--distill runs another leg INSTEAD (the default output is unchanged): the distillation criterion (m3_loss_distill_fwd / _bwd
through pretrain.DistillLossFn, soft at tau 3 and hard, fp32 student logits under fp16 teacher logits) beside the reference's
formula in stock torch ops (pretrain/models/losses.py:53-64), forward + backward; and the whole pretrain_step of a distilled
model (N = 198, hard distillation against a mean-pool + Linear teacher) beside the non-distilled one (N = 197) and the
distilled model without the teacher term (criterion 'none': what the second token and head cost by themselves), all with
Mixup + SoftTargetCrossEntropy + ModelEma.
    python tools/pretrain_bench.py --distill [--out profiles/distill_step.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warmup=3):
    """(GPU ms per call from device events, host ms per call until the calls returned)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    host = (time.perf_counter() - t0) * 1e3 / iters
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters, host


def ring(make, count):
    items, k = [make() for _ in range(count)], [0]

    def nxt():
        k[0] = (k[0] + 1) % count
        return items[k[0]]
    return nxt


def report(times, header):
    """median GPU / host ms per row and the rounds' GPU times; returns {name: (GPU ms, host ms)}"""
    med, lines = {}, header + ["", f"{'':62s} {'GPU ms':>9s} {'host ms':>9s}   GPU ms by round"]
    for name, v in times.items():
        gs, hs = sorted(x[0] for x in v), sorted(x[1] for x in v)
        med[name] = (gs[len(gs) // 2], hs[len(hs) // 2])
        lines.append(f"{name:62s} {med[name][0]:9.3f} {med[name][1]:9.3f}   " + " ".join(f"{x[0]:.3f}" for x in v))
    return med, lines


def distill_leg(args):
    from types import SimpleNamespace as NS
    from m3vit_amd import pretrain
    from m3vit_amd.cls import MoEViTConfig, MoEViTForImageNet
    from m3vit_amd.functional import DistillLossFn
    from m3vit_amd.optim import FusedAdamW
    dev = torch.device("cuda")
    B, C, tau = args.batch, 1000, 3.0
    g = torch.Generator(device="cuda").manual_seed(1)
    logits = torch.randn(B, C, device=dev, generator=g) * 3
    teacher_logits = (torch.randn(B, C, device=dev, generator=g) * 3).half()

    def ours(kind):
        def run():
            x = logits.detach().requires_grad_(True)
            DistillLossFn.apply(x, teacher_logits, kind, tau)[0].backward()
        return run

    def torch_soft():
        x = logits.detach().requires_grad_(True)
        (F.kl_div(F.log_softmax(x / tau, dim=1), F.log_softmax(teacher_logits / tau, dim=1), reduction="sum", log_target=True)
         * (tau * tau) / x.numel()).backward()

    def torch_hard():
        x = logits.detach().requires_grad_(True)
        F.cross_entropy(x, teacher_logits.argmax(dim=1)).backward()

    pieces = {"distill soft: m3_loss_distill fwd + bwd": ours("soft"), "distill soft: torch kl_div(log_softmax, log_softmax)": torch_soft,
              "distill hard: m3_loss_distill fwd + bwd": ours("hard"), "distill hard: torch cross_entropy(x, t.argmax(1))": torch_hard}

    class Teacher(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(3, C)

        def forward(self, x):
            return self.fc(x.mean((2, 3))).half()

    if not args.no_step:
        img_bytes = B * 3 * 224 * 224 * 4
        images = ring(lambda: torch.randn(B, 3, 224, 224, device=dev, generator=g), max(2, -(-320 * 2 ** 20 // img_bytes)))
        labels = torch.randint(0, C, (B,), device=dev, generator=g)
        base = dict(mixup=0.8, cutmix=1.0, smoothing=0.1, cutmix_minmax=None, distillation_alpha=0.5, distillation_tau=1.0)
        np.random.seed(0)
        mix = pretrain.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=C)

        def step_of(distilled, kind):
            model = MoEViTForImageNet(MoEViTConfig(distilled=distilled), act_dtype=torch.float16).to(dev).train()
            opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.05, max_grad_norm=1.0)
            scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
            crit = pretrain.build_criterion(NS(distillation_type=kind, **base),
                                            teacher_model=Teacher().to(dev).eval() if kind != "none" else None)
            ema = pretrain.ModelEma(model, decay=0.9999)
            return lambda: pretrain.pretrain_step(model, crit, opt, scaler, images(), labels, mixup_fn=mix, model_ema=ema,
                                                  clip_grad=1.0)
        pieces["step: distilled (N = 198), hard distillation + recipe"] = step_of(True, "hard")
        pieces["step: not distilled (N = 197), recipe"] = step_of(False, "none")
        pieces["step: distilled (N = 198), recipe, no teacher term"] = step_of(True, "none")

    times = {name: [] for name in pieces}
    for _ in range(args.rounds):
        for name, fn in pieces.items():
            times[name].append(timed(fn, max(3, args.iters // 4) if name.startswith("step") else args.iters))
    med, lines = report(times, [f"distillation at configs[1]: batch {B}, {C} classes, fp32 student logits, fp16 teacher logits, tau {tau:g}; "
                                f"{args.rounds} alternating rounds x {args.iters} iterations (whole step: {max(3, args.iters // 4)})",
                                f"device: {torch.cuda.get_device_name(0)}"])
    lines.append("")
    names = list(pieces)
    for o, t in ((names[0], names[1]), (names[2], names[3])):
        lines.append(f"{o:62s} GPU {med[t][0] / med[o][0]:6.2f}x, host {med[t][1] / med[o][1]:6.2f}x against the stock form")
    if not args.no_step:
        a, b = med[names[4]], med[names[5]]
        c = med[names[6]]
        lines.append(f"whole step: {a[0]:.3f} ms distilled, {b[0]:.3f} ms not distilled: {a[0] - b[0]:+.3f} ms GPU "
                     f"({100 * (a[0] / b[0] - 1):+.2f} %), {a[1] - b[1]:+.3f} ms host; of that the second token and head alone "
                     f"(distilled model, criterion 'none'): {c[0] - b[0]:+.3f} ms GPU ({100 * (c[0] / b[0] - 1):+.2f} %)")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--no-step", action="store_true", help="leave out the whole-step rows")
    ap.add_argument("--distill", action="store_true", help="the distillation leg instead (criterion and distilled step)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "distill_step.txt" if args.distill else "pretrain_step.txt")
    if args.distill:
        return distill_leg(args)
    from m3vit_amd import ops, pretrain
    from m3vit_amd.cls import MoEViTConfig, MoEViTForImageNet
    from m3vit_amd.optim import FusedAdamW
    dev = torch.device("cuda")
    B, C = args.batch, 1000
    g = torch.Generator(device="cuda").manual_seed(1)
    model = MoEViTForImageNet(MoEViTConfig(), act_dtype=torch.float16).to(dev).train()
    n_param = sum(v.numel() for v in model.state_dict().values() if v.dtype == torch.float32)

    # ---- mix: a ring of image batches past the Infinity Cache
    img_bytes = B * 3 * 224 * 224 * 4
    n_ring = max(2, -(-320 * 2 ** 20 // img_bytes))
    images = ring(lambda: torch.randn(B, 3, 224, 224, device=dev, generator=g), n_ring)
    lam_mix = torch.full((B,), 0.3, device=dev)
    box0 = torch.zeros(B, 4, dtype=torch.int32, device=dev)
    yl, yh, xl, xh = 40, 180, 30, 170
    lam_cut = torch.full((B,), 1 - (yh - yl) * (xh - xl) / (224 * 224), device=dev)
    box1 = torch.tensor([[yl, yh, xl, xh]] * B, dtype=torch.int32, device=dev)

    def torch_mixup():
        x = images()
        x.mul_(0.3).add_(x.flip(0).mul_(0.7))

    def torch_cutmix():
        x = images()
        x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]

    n_img = B * 3 * 224 * 224
    add_a, add_b = ring(lambda: torch.zeros(n_img, device=dev), 3), ring(lambda: torch.ones(n_img, device=dev), 3)

    # ---- loss and evaluation at [B, 1000]
    logits = torch.randn(B, C, device=dev, generator=g) * 3
    labels = torch.randint(0, C, (B,), device=dev, generator=g)
    soft, _ = ops.mix_target(labels, lam_mix, C, 0.1)
    ours_loss = pretrain.SoftTargetCrossEntropy()

    def loss_ours():
        x = logits.detach().requires_grad_(True)
        ours_loss(x, soft).backward()

    def loss_torch():
        x = logits.detach().requires_grad_(True)
        torch.sum(-soft * F.log_softmax(x, dim=-1), dim=-1).mean().backward()

    meter = pretrain.ClsEvalMeter()
    sums = [0.0, 0.0, 0.0]

    def eval_torch():
        loss = F.cross_entropy(logits, labels)
        top = logits.topk(5, 1)[1].t().eq(labels.view(1, -1))
        sums[0] += loss.item() * B
        sums[1] += top[:1].reshape(-1).float().sum().item()
        sums[2] += top[:5].reshape(-1).float().sum().item()

    # ---- EMA over the model's parameter set, a ring of shadows and sources past the cache
    n_sets = max(2, -(-320 * 2 ** 20 // (8 * n_param)))
    emas = [pretrain.ModelEma(model, decay=0.9999) for _ in range(n_sets)]
    k = [0]

    def ema_ours():
        k[0] = (k[0] + 1) % n_sets
        emas[k[0]].update(model)

    def ema_torch():
        k[0] = (k[0] + 1) % n_sets
        with torch.no_grad():
            for e, p in zip(emas[k[0]].shadow.values(), model.state_dict().values()):
                if e.dtype == torch.float32:
                    e.mul_(0.9999).add_(p, alpha=1 - 0.9999)
                else:
                    e.copy_(p)

    pa, pb = ring(lambda: torch.zeros(n_param, device=dev), 3), ring(lambda: torch.ones(n_param, device=dev), 3)

    pieces = {
        "mix: m3_mix_batch, Mixup (in place)": lambda: ops.mix_batch(images(), lam_mix, box0),
        "mix: torch flip / mul_ / add_": torch_mixup,
        "mix: m3_mix_batch, CutMix (in place)": lambda: ops.mix_batch(images(), lam_cut, box1),
        "mix: torch slice assignment": torch_cutmix,
        "yardstick: m3_add_f32, image-batch elements": lambda: ops.add_f32(add_a(), add_b()),
        "loss: SoftTargetCrossEntropy fwd + bwd": loss_ours,
        "loss: torch sum(-t * log_softmax) fwd + bwd": loss_torch,
        "evaluation: ClsEvalMeter.update": lambda: meter.update(logits, labels),
        "evaluation: cross_entropy + topk + 3 .item()": eval_torch,
        "EMA: ModelEma.update (m3_ema_update)": ema_ours,
        "EMA: torch loop over state_dict()": ema_torch,
        "yardstick: m3_add_f32, parameter-set elements": lambda: ops.add_f32(pa(), pb()),
    }

    # ---- the whole step
    if not args.no_step:
        opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.05, max_grad_norm=1.0)
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
        from types import SimpleNamespace as NS
        base = dict(cutmix_minmax=None, distillation_type="none", distillation_alpha=0.5, distillation_tau=1.0)
        crit = pretrain.build_criterion(NS(mixup=0.8, cutmix=1.0, smoothing=0.1, **base))
        stock = torch.nn.CrossEntropyLoss()
        np.random.seed(0)
        mix = pretrain.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=C)
        ema = emas[0]
        pieces["step: pretrain_step with Mixup + SoftTargetCE + ModelEma"] = lambda: pretrain.pretrain_step(
            model, crit, opt, scaler, images(), labels, mixup_fn=mix, model_ema=ema, clip_grad=1.0)
        pieces["step: pretrain_step, nn.CrossEntropyLoss, no mixing, no EMA"] = lambda: pretrain.pretrain_step(
            model, lambda s, o, t: stock(o, t), opt, scaler, images(), labels, clip_grad=1.0)

    times = {name: [] for name in pieces}
    for _ in range(args.rounds):                 # alternating: a drift of the clocks lands on every variant alike
        for name, fn in pieces.items():
            times[name].append(timed(fn, max(3, args.iters // 4) if name.startswith("step") else args.iters))
    med = {}
    lines = [f"pretraining recipe at configs[1]: batch {B}, 3 x 224 x 224 fp32 images ({img_bytes / 1e6:.1f} MB, ring of {n_ring}), "
             f"{C} classes, {n_param} fp32 parameter elements ({4 * n_param / 1e6:.1f} MB, ring of {n_sets} shadow sets); "
             f"{args.rounds} alternating rounds x {args.iters} iterations (whole step: {max(3, args.iters // 4)})",
             f"device: {torch.cuda.get_device_name(0)}", "",
             f"{'':62s} {'GPU ms':>9s} {'host ms':>9s}   GPU ms by round"]
    for name, v in times.items():
        gs, hs = sorted(x[0] for x in v), sorted(x[1] for x in v)
        med[name] = (gs[len(gs) // 2], hs[len(hs) // 2])
        lines.append(f"{name:62s} {med[name][0]:9.3f} {med[name][1]:9.3f}   " + " ".join(f"{x[0]:.3f}" for x in v))
    lines.append("")

    def rate(name, bytes_):
        return bytes_ / med[name][0] / 1e9       # TB/s

    y_img = rate("yardstick: m3_add_f32, image-batch elements", 12 * n_img)
    y_par = rate("yardstick: m3_add_f32, parameter-set elements", 12 * n_param)
    for name, bytes_, y in (("mix: m3_mix_batch, Mixup (in place)", 8 * n_img, y_img),
                            ("mix: m3_mix_batch, CutMix (in place)", 8 * n_img, y_img),
                            ("EMA: ModelEma.update (m3_ema_update)", 12 * n_param, y_par)):
        lines.append(f"{name:62s} {rate(name, bytes_):6.2f} TB/s, {rate(name, bytes_) / y:.2f} of m3_add_f32's {y:.2f} TB/s")
    pairs = [("mix: torch flip / mul_ / add_", "mix: m3_mix_batch, Mixup (in place)"),
             ("mix: torch slice assignment", "mix: m3_mix_batch, CutMix (in place)"),
             ("loss: torch sum(-t * log_softmax) fwd + bwd", "loss: SoftTargetCrossEntropy fwd + bwd"),
             ("evaluation: cross_entropy + topk + 3 .item()", "evaluation: ClsEvalMeter.update"),
             ("EMA: torch loop over state_dict()", "EMA: ModelEma.update (m3_ema_update)")]
    lines.append("")
    for stock_name, ours_name in pairs:
        lines.append(f"{ours_name:62s} GPU {med[stock_name][0] / med[ours_name][0]:6.2f}x, host "
                     f"{med[stock_name][1] / med[ours_name][1]:6.2f}x against the stock form")
    if not args.no_step:
        a, b = (med[n] for n in list(pieces)[-2:])
        lines.append(f"whole step: {a[0]:.3f} ms with the recipe, {b[0]:.3f} ms without: the recipe adds {a[0] - b[0]:.3f} ms GPU, "
                     f"{a[1] - b[1]:.3f} ms host")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
