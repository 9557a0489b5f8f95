"""GPU: the backbone with a distillation token (distilled=True: cls, dist in front of the patches, N = patches + 2) - the fused
executor against the float64 oracle, the module path fused against per-op, the classification wrapper's two heads and one
distilled pretraining step, and the attention kernels at N = 198.

The oracle is unchanged: oracle.ref_torch.patch_embed concatenates cls_token.expand(B, -1, -1) in front of the patches and adds
pos_embed, so a cls_token of shape [1, 2, D] = cat(cls, dist) with a [1, patches + 2, D] pos_embed IS the distilled backbone;
that parameter's gradient splits into cls_token's and dist_token's."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_contract as kc                                       # noqa: E402
import pretrain_cases as PC                                        # noqa: E402
from test_engine import F16_TOL, GRAD_FACTOR, rel                  # noqa: E402
from test_pretrain_gpu import no_host_sync                         # noqa: E402

pytestmark = pytest.mark.gpu


def _tn(shape, gen):
    t = torch.empty(shape)
    torch.nn.init.trunc_normal_(t, std=.02, generator=gen)
    return t


def distilled_params(cfg, seed):
    """the oracle's random parameters with a dist_token and the wider pos_embed"""
    from oracle import ref_torch as R
    P = R.init_backbone_params(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 1000)
    P["pos_embed"] = _tn((1, cfg.num_tokens + 1, cfg.embed_dim), g)
    P["dist_token"] = _tn((1, 1, cfg.embed_dim), g)
    return P


def oracle_leaves(P):
    """float64 leaves for the oracle: dist_token folded into a [1, 2, D] cls_token"""
    Pr = {k: v.detach().clone().double().cpu() for k, v in P.items() if k != "dist_token"}
    Pr["cls_token"] = torch.cat((Pr["cls_token"], P["dist_token"].detach().double().cpu()), 1)
    return {k: v.requires_grad_() for k, v in Pr.items()}


def oracle_grad(Pr, name):
    if name == "cls_token":
        return None if Pr[name].grad is None else Pr[name].grad[:, :1]
    if name == "dist_token":
        return None if Pr["cls_token"].grad is None else Pr["cls_token"].grad[:, 1:2]
    return Pr[name].grad


def check_distilled_engine(cfg, dtype, tol, tasks, B=3, seed=5, noisy=False, follow_routing=False):
    """tests/test_engine.py's _check_backbone for a distilled parameter set (its tolerances: tol on the tokens, GRAD_FACTOR
    tol per parameter tensor, exact routing agreement in every MoE block)"""
    from m3vit_amd.engine import BackboneEngine
    from oracle import ref_torch as R
    D, N = cfg.embed_dim, cfg.num_tokens + 1
    P = distilled_params(cfg, seed)
    torch.manual_seed(0)
    img = torch.randn(B, 3, *cfg.img_size)
    dtok = torch.randn(B, N, D) * 0.1
    cvw = 0.01
    eng = BackboneEngine(cfg, P, batch=B, dtype=dtype)
    assert eng.distilled and eng.N == N and eng.T == B * N
    eng.zero_grad()
    Pr = oracle_leaves(P)
    tot = 0.0
    moe_blocks = [i for i in range(cfg.depth) if cfg.is_moe(i)]
    for task in tasks:
        noises = None
        if noisy:                                                  # B (np + 2) rows: the distillation token is routed too
            gen = torch.Generator().manual_seed(100 + task)
            noises = {i: torch.randn(B * N, cfg.moe_experts, generator=gen) for i in moe_blocks}
        tok, cv = eng.forward(img.cuda(), task, noises=None if noises is None else {i: n.cuda() for i, n in noises.items()})
        assert tuple(tok.shape) == (B, N, D)
        nz64 = None if noises is None else {i: n.double() for i, n in noises.items()}
        if follow_routing:
            ovr = {i: eng.act[i]["gate"]["idx"].cpu() for i in moe_blocks}
            tok_ref, cv_ref, aux = R.backbone_forward(Pr, cfg, img.double(), task, route_override=ovr, noises=nz64)
            with torch.no_grad():
                free = R.backbone_forward(Pr, cfg, img.double(), task, noises=nz64)[2]
            for i in moe_blocks:
                h2 = eng.act[i]["h2"].double().cpu()
                gx = torch.cat((h2, aux[i]["gate_x"][:, D:].detach()), 1)
                (own, _), *_ = R.gate_vmoe(gx, aux[i]["w_gate"].detach(), cfg.moe_top_k)
                assert torch.equal(ovr[i], own), f"block {i}: indices are not the top-k of the engine's own gate input"
                flipped = (ovr[i] != free[i]["idx"]).any(1).float().mean()
                assert float(flipped) < 0.2, f"block {i}: {float(flipped):.2%} of the tokens routed differently"
        else:
            tok_ref, cv_ref, aux = R.backbone_forward(Pr, cfg, img.double(), task, noises=nz64)
            for i in moe_blocks:
                assert torch.equal(eng.act[i]["gate"]["idx"].cpu(), aux[i]["idx"]), f"routing differs in block {i}"
        tok_err = rel(tok, tok_ref)
        assert tok_err < tol, tok_err
        assert abs(float(cv) - float(cv_ref.detach())) < 1e-3 * max(1.0, abs(float(cv_ref.detach())))
        eng.backward(dtok.cuda(), cv_weight=cvw)
        tot = tot + (tok_ref * dtok.double()).sum() + cvw * cv_ref
    tot.backward()
    bad, worst = [], ("", 0.0)
    for name, g in eng.grads.items():
        ref = oracle_grad(Pr, name)
        if ref is None:
            assert float(g.abs().max()) == 0.0, name
            continue
        e = rel(g, ref)
        if e > worst[1]:
            worst = (name, e)
        if e > tol * GRAD_FACTOR:
            bad.append((name, e))
    e_dist = rel(eng.grads["dist_token"], oracle_grad(Pr, "dist_token"))
    print(f"[{dtype}] tokens rel {tok_err:.2e} (bound {tol:.0e}); worst gradient {worst[0]} {worst[1]:.2e}, dist_token {e_dist:.2e} "
          f"(bound {tol * GRAD_FACTOR:.0e})")
    assert not bad, bad
    assert float(eng.grads["dist_token"].abs().max()) > 0.0 and e_dist <= tol * GRAD_FACTOR, ("dist_token", e_dist)
    return eng


def _small_cfg(**over):
    from oracle import ref_torch as R
    kw = dict(img_size=(32, 48), embed_dim=64, depth=4, num_heads=2, mlp_ratio=4.0, moe_mlp_ratio=1.0, moe_experts=4,
              moe_top_k=2, gate_dim=66, multi_gate=True)
    kw.update(over)
    return R.BackboneCfg(**kw)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-4), (torch.float16, F16_TOL)])
def test_distilled_engine_fwd_bwd_matches_oracle(dtype, tol):
    """img 32 x 48: 6 patches, N = 8.  fp32: the routing of every MoE block equals the float64 run's.  fp16: one of the 24
    tokens of block 3 has two experts whose logits lie closer than the fp16 rounding of the gate input moves them (measured: one
    flipped token, task 0), so the routing is held to tests/test_engine.py's fp16 form - the engine's indices are EXACTLY the
    oracle gate's top-k on the engine's own gate input, and the values are compared with the oracle following them."""
    eng = check_distilled_engine(_small_cfg(), dtype, tol, tasks=(0, 1), follow_routing=dtype == torch.float16)
    st = eng.moe_stats()
    assert st is None                                              # built without moe_stats


def test_distilled_engine_noisy_gate_takes_noise_for_every_token():
    check_distilled_engine(_small_cfg(moe_experts=8, vmoe_noisy_std=1.0), torch.float32, 2e-4, tasks=(0, 1), noisy=True)


def test_distilled_engine_moe_stats_count_positions_without_one_prefix():
    """total_positions stays B (N - 1) per MoE block (vision_transformer_moe.py:820 counts x.shape[1] - 1, distilled or not)"""
    from m3vit_amd.engine import BackboneEngine
    cfg = _small_cfg()
    B = 3
    eng = BackboneEngine(cfg, distilled_params(cfg, 5), batch=B, dtype=torch.float32, moe_stats=True)
    eng.forward(torch.randn(B, 3, 32, 48).cuda(), 0)
    blocks, agg = eng.moe_stats()
    assert agg["moe_blocks"] == 2 and agg["total_positions"] == 2 * B * 7
    assert all(b["gate_token_count"] == B * 8 for b in blocks.values())


def test_distilled_engine_checkpoint_mode_gives_the_same_bits():
    from m3vit_amd.engine import BackboneEngine
    cfg = _small_cfg()
    P = distilled_params(cfg, 5)
    B = 3
    img, dtok = torch.randn(B, 3, 32, 48).cuda(), (torch.randn(B, 8, 64) * 0.1).cuda()
    out = []
    for ckpt in (False, True):
        eng = BackboneEngine(cfg, P, batch=B, dtype=torch.float16, checkpoint=ckpt)
        eng.zero_grad()
        tok, cv = eng.forward(img, 1)
        tok = tok.clone()
        eng.backward(dtok, cv_weight=0.01)
        out.append((tok, {n: g.clone() for n, g in eng.grads.items()}))
    assert kc.same_bits(out[0][0], out[1][0])
    bad = [(n, rel(out[1][1][n], g)) for n, g in out[0][1].items() if rel(out[1][1][n], g) > 1e-5]
    assert not bad, bad


def test_distilled_engine_at_the_real_sequence_length():
    """224 x 224, D 384: N = 198, the first even N the short-sequence attention kernels meet; fp16, depth 2, B 2"""
    from oracle import ref_torch as R
    cfg = R.BackboneCfg(img_size=(224, 224), embed_dim=384, depth=2, num_heads=12, mlp_ratio=4.0, moe_mlp_ratio=1.0,
                        moe_experts=16, moe_top_k=4, gate_dim=386, multi_gate=True)
    eng = check_distilled_engine(cfg, torch.float16, F16_TOL, tasks=(0,), B=2, seed=7, follow_routing=True)
    assert eng.N == 198


# -------------------------------------------------------------------------------------------------------- module path
KW = dict(img_size=(32, 48), embed_dim=64, depth=4, num_heads=2, moe_top_k=2, gate_dim=66, multi_gate=True, moe_experts=4)


def _module(fused, fused_grads="auto", seed=9):
    from m3vit_amd.vit import VisionTransformerMoE
    cfg = _small_cfg()
    m = VisionTransformerMoE(mlp_ratio=4.0, moe_mlp_ratio=1, vmoe_noisy_std=0.0, fused=fused, fused_grads=fused_grads,
                             distilled=True, **KW).cuda()
    m.load_state_dict(distilled_params(cfg, seed))
    return m.train()


@pytest.mark.parametrize("grads", ["views", "autograd"])
def test_distilled_module_fused_matches_per_op(grads):
    """tests/test_fused_module_gpu.py::test_fused_module_matches_per_op_module_path's tolerances: tokens and balance loss 1e-5,
    every parameter gradient 2e-4 (fp32: summation order only)"""
    a, b = _module("auto", grads), _module(False)
    assert tuple(a.pos_embed.shape) == (1, 8, 64) and a.num_token == 2
    img = torch.randn(4, 3, 32, 48).cuda()
    dtok = (torch.randn(4, 8, 64) * 0.1).cuda()
    for rep in range(3):                                           # eager, capture, replay
        for m in (a, b):
            m.zero_grad(set_to_none=True)
            loss = 0.0
            for task in (0, 1):
                tok, cv = m(img, task_id=task)
                loss = loss + (tok * dtok).sum() + 0.01 * cv
            loss.backward()
            m.last = (tok.detach(), cv.detach())
        assert a.fused_fallback_reason is None and a.fused_grads_used == grads and b._fused is None
        assert a._fused.slots[0].eng.distilled and a._fused.slots[0].eng.N == 8
        assert rel(a.last[0], b.last[0]) < 1e-5 and abs(float(a.last[1]) - float(b.last[1])) < 1e-5
        bad = [(n, rel(p.grad, q.grad)) for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters())
               if rel(p.grad, q.grad) > 2e-4]
        assert not bad, (rep, bad)
        assert float(a.dist_token.grad.abs().max()) > 0.0


# ------------------------------------------------------------------------------------------- classification wrapper
NUM_CLASSES = 16                                                   # (tests/test_pretrain_gpu.py: the head's GEMM shapes)


def _cls_model(seed=7, act=torch.float16):
    from m3vit_amd.cls import MoEViTConfig, MoEViTForImageNet
    cfg = MoEViTConfig(img_size=32, patch_size=16, embed_dim=64, depth=2, num_heads=2, num_classes=NUM_CLASSES, moe_experts=4,
                       moe_top_k=2, gate_dim=64, vmoe_noisy_std=0.0, distilled=True)
    torch.manual_seed(seed)
    return MoEViTForImageNet(cfg, act_dtype=act).cuda().train()


def test_distilled_classifier_heads_training_pair_and_evaluation_mean():
    model = _cls_model(act=torch.float32)
    x = torch.randn(4, 3, 32, 32, generator=PC._gen(3)).cuda()
    out = model(x)
    assert model.encoder.fused_fallback_reason is None
    logits = out["logits"]
    assert isinstance(logits, tuple) and len(logits) == 2
    assert all(tuple(v.shape) == (4, NUM_CLASSES) and v.dtype == torch.float32 for v in logits)
    assert not kc.same_bits(logits[0], logits[1])
    # the two heads against torch on the encoder's own tokens: LayerNorm of rows 0 and 1, then the two Linears
    with torch.no_grad():
        tokens, _ = model.encoder(x)
        pre = torch.nn.functional.layer_norm(tokens[:, :2].double(), (64,), model.norm.weight.double(), model.norm.bias.double(),
                                             model.norm.eps)
        ref_cls = pre[:, 0] @ model.head.weight.double().t() + model.head.bias.double()
        ref_dist = pre[:, 1] @ model.head_dist.weight.double().t() + model.head_dist.bias.double()
    assert rel(logits[0], ref_cls) < 2e-4 and rel(logits[1], ref_dist) < 2e-4
    model.eval()
    with torch.no_grad():
        ev = model(x)["logits"]
    assert torch.is_tensor(ev) and tuple(ev.shape) == (4, NUM_CLASSES)
    assert rel(ev, (ref_cls + ref_dist) / 2) < 2e-4
    # the evaluation meter takes that mean as it is
    from m3vit_amd.pretrain import ClsEvalMeter
    meter = ClsEvalMeter()
    meter.update(ev, torch.randint(0, NUM_CLASSES, (4,), generator=PC._gen(4)).cuda())
    assert float(meter.state[3]) == 4.0


class _Teacher(torch.nn.Module):
    def __init__(self, classes):
        super().__init__()
        self.fc = torch.nn.Linear(3, classes)

    def forward(self, x):
        return (self.fc(x.float().mean((2, 3))) * 4).half()           # a teacher under autocast returns 16 bits


def test_distilled_pretrain_step_with_hard_distillation():
    from types import SimpleNamespace as NS
    from m3vit_amd.optim import FusedAdamW
    from m3vit_amd.pretrain import Mixup, ModelEma, build_criterion, pretrain_step
    model = _cls_model()
    teacher = _Teacher(NUM_CLASSES).cuda().eval()
    opt = FusedAdamW(model.parameters(), lr=1e-2, weight_decay=0.05, max_grad_norm=1.0)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    crit = build_criterion(NS(mixup=0.8, cutmix=1.0, cutmix_minmax=None, smoothing=0.1, distillation_type="hard",
                              distillation_alpha=0.5, distillation_tau=1.0), teacher_model=teacher)
    assert crit.distillation_type == "hard" and crit.teacher_model is teacher
    ema = ModelEma(model, decay=0.9)
    assert {"encoder.dist_token", "head_dist.weight", "head_dist.bias"} <= set(ema.state_dict())
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=NUM_CLASSES, mode="elem")
    lam = np.array([0.3, 1.0, 0.75, 0.6], dtype=np.float32)
    box = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [8, 24, 8, 24], [0, 0, 0, 0]], dtype=np.int32)
    mix.draw = lambda B, H, W: (lam, box)
    g = PC._gen(21)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    teacher_before = [p.detach().clone() for p in teacher.parameters()]
    for step in range(2):
        x = torch.randn(4, 3, 32, 32, generator=g).cuda()
        y = torch.randint(0, NUM_CLASSES, (4,), generator=g).cuda()
        loss, cv = pretrain_step(model, crit, opt, scaler, x, y, mixup_fn=mix, model_ema=ema, moe_cv_weight=0.01, clip_grad=1.0)
        assert model.encoder.fused_fallback_reason is None
        assert loss.is_cuda and cv.is_cuda and math.isfinite(float(loss)) and math.isfinite(float(cv))
    now = model.state_dict()
    for k in ("encoder.dist_token", "head_dist.weight", "encoder.cls_token", "head.weight", "encoder.pos_embed"):
        assert not kc.same_bits(before[k], now[k]), f"two steps left {k} unchanged"
    assert not kc.same_bits(ema.state_dict()["encoder.dist_token"], before["encoder.dist_token"])
    assert all(p.grad is None for p in teacher.parameters())
    assert all(kc.same_bits(a, p.detach()) for a, p in zip(teacher_before, teacher.parameters()))
    st = crit.last_stats
    assert all(v.is_cuda and v.dim() == 0 and math.isfinite(float(v)) for v in st.values()) and float(st["loss_distill"]) > 0.0

    # the criterion on the model's pair, the mix and the EMA read nothing back (all warmed up above)
    x = torch.randn(4, 3, 32, 32, generator=g).cuda()
    y = torch.randint(0, NUM_CLASSES, (4,), generator=g).cuda()
    pair = tuple(torch.randn(4, NUM_CLASSES, generator=g).cuda().requires_grad_(True) for _ in range(2))
    torch.cuda.synchronize()
    with no_host_sync():
        xm, soft = mix(x, y)
        crit(xm, pair, soft).backward()
        ema.update(model)
    torch.cuda.synchronize()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in pair)


# ---------------------------------------------------------------------------------------------------- attention, N = 198
@pytest.mark.parametrize("dh", [32, 64])
def test_attention_at_n198_fp16(dh):
    """the sequence length a distilled ViT-S brings (196 patches + 2): forward and backward against float64 within
    kernel_contract's attention bounds"""
    from m3vit_amd import ops
    B, N, H = 2, 198, 3
    D = H * dh
    g = torch.Generator().manual_seed(31 + dh)
    qkv = (torch.randn(B * N, 3 * D, generator=g)).half().cuda()
    d_o = (torch.randn(B * N, D, generator=g) * 0.5).half().cuda()
    o, ocheck = kc.guarded(B * N, D, torch.float16)
    lse, lcheck = kc.guarded(B * H, N, torch.float32)
    dqkv, dcheck = kc.guarded(B * N, 3 * D, torch.float16)
    ops.attention_fwd(qkv, B, N, H, dh, o, lse.view(B, H, N))
    need = int(ops.lib().m3_attention_bwd_ws_elems(B, N, H, dh))
    ws = torch.empty(max(need, 1), dtype=torch.float32, device="cuda")
    ops.attention_bwd(qkv, o, d_o, lse.view(B, H, N), B, N, H, dh, dqkv, dq_ws=ws if need else None)
    torch.cuda.synchronize()
    ocheck(what="o"); lcheck(what="lse"); dcheck(what="dqkv")
    q, k, v = (t.permute(0, 2, 1, 3) for t in qkv.double().cpu().view(B, N, 3, H, dh).unbind(2))       # [B, H, N, dh]
    q, k, v = (t.contiguous().requires_grad_() for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * dh ** -0.5
    lse_ref = torch.logsumexp(s, -1)
    o_ref = torch.softmax(s, -1) @ v
    do64 = d_o.double().cpu().view(B, N, H, dh).permute(0, 2, 1, 3)
    dq_ref, dk_ref, dv_ref = torch.autograd.grad(o_ref, (q, k, v), do64)
    ob, lb = kc.attention_fwd_bounds(q.detach(), k.detach(), v.detach(), o_ref.detach(), lse_ref.detach(), torch.float16)
    o4 = o.view(B, N, H, dh).permute(0, 2, 1, 3)
    kc.assert_within(o4, o_ref.detach(), ob, "o")
    kc.assert_within(lse.view(B, H, N), lse_ref.detach(), lb, "lse")
    # the backward reads the kernel's own (rounded) o
    bq, bk, bv = kc.attention_bwd_bounds(q.detach(), k.detach(), v.detach(), o4.double().cpu(), do64, dq_ref, dk_ref, dv_ref,
                                         torch.float16)
    d5 = dqkv.view(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    kc.assert_within(d5[0], dq_ref, bq, "dq")
    kc.assert_within(d5[1], dk_ref, bk, "dk")
    kc.assert_within(d5[2], dv_ref, bv, "dv")
