"""CPU: the distillation closed forms of tests/distill_cases.py against torch's own functions written as
pretrain/models/losses.py:55-64 writes them, their float32 evaluation against the bounds the kernels are held to, and the
distilled model's construction (key set, pos_embed, config, checkpoint resize, DistillationLoss constructor rules)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distill_cases as DC                                         # noqa: E402
import pretrain_cases as PC                                        # noqa: E402
from kernel_contract import assert_within                          # noqa: E402


def _inputs(B, C, dtypes=(torch.float32, torch.float32)):
    """(student, teacher) float64 logits holding values of the pair's dtypes"""
    x = PC.make_logits(B, C).to(dtypes[0]).double()
    t = DC.make_teacher(B, C).to(dtypes[1]).double()
    return x, t


@pytest.mark.parametrize("kind", DC.KINDS, ids=DC.kind_id)
@pytest.mark.parametrize("B,C", DC.SHAPES, ids=lambda v: str(v))
def test_closed_forms_agree_with_torch_in_float64(B, C, kind):
    """value and gradient of distill_ref against kl_div(...) * t * t / numel and cross_entropy(x, teacher.argmax(1))"""
    x, t = _inputs(B, C)
    r = DC.distill_ref(x, t, *kind)
    xr = x.clone().requires_grad_()
    if kind[0] == "soft":
        tau = kind[1]
        ref = F.kl_div(F.log_softmax(xr / tau, dim=1), F.log_softmax(t / tau, dim=1), reduction="sum",
                       log_target=True) * (tau * tau) / xr.numel()
    else:
        ref = F.cross_entropy(xr, t.argmax(dim=1))
    ref.backward()
    assert abs(float(r["loss"]) - float(ref.detach())) <= 1e-12 * max(1.0, abs(float(ref.detach())))
    assert float((r["grad"] - xr.grad).abs().max()) <= 1e-14


@pytest.mark.parametrize("pair", DC.DTYPE_PAIRS, ids=DC.pair_id)
@pytest.mark.parametrize("kind", DC.KINDS, ids=DC.kind_id)
@pytest.mark.parametrize("B,C", DC.SHAPES, ids=lambda v: str(v))
def test_float32_evaluation_stays_within_the_kernel_bounds(B, C, kind, pair):
    x, t = _inputs(B, C, pair)
    r = DC.distill_ref(x, t, *kind)
    r32 = DC.distill_ref(x.float(), t.float(), *kind)
    loss_b, grad_b, lse_b = DC.distill_bounds(r, torch.float32)
    assert_within(r32["loss"].reshape(1), r["loss"].reshape(1), loss_b, "loss")
    assert_within(r32["grad"], r["grad"], grad_b, "gradient")
    assert_within(r32["lse"], r["lse"], lse_b, "lse")


def test_argmax_ties_go_to_the_lowest_index():
    t = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, -1.0, 5.0, 5.0]], dtype=torch.float64)
    assert DC.argmax_low(t).tolist() == [1, 0, 2]


# ------------------------------------------------------------------------------------------------------- the model
def _cfg(**kw):
    from m3vit_amd.cls import MoEViTConfig
    base = dict(img_size=32, patch_size=16, embed_dim=64, depth=2, num_heads=2, num_classes=10, moe_experts=4, moe_top_k=2,
                gate_dim=64)
    base.update(kw)
    return MoEViTConfig(**base)


def test_distilled_model_constructs_with_the_reference_key_set():
    from m3vit_amd.cls import MoEViTForImageNet
    plain = MoEViTForImageNet(_cfg())
    m = MoEViTForImageNet(_cfg(distilled=True))
    keys, base = set(m.state_dict()), set(plain.state_dict())
    assert keys - base == {"encoder.dist_token", "head_dist.weight", "head_dist.bias"} and base <= keys
    npatch = (32 // 16) ** 2
    assert tuple(m.encoder.pos_embed.shape) == (1, npatch + 2, 64) and tuple(plain.encoder.pos_embed.shape) == (1, npatch + 1, 64)
    assert tuple(m.encoder.dist_token.shape) == (1, 1, 64) and m.encoder.num_token == 2 and plain.encoder.num_token == 1
    assert plain.encoder.dist_token is None and plain.head_dist is None
    assert tuple(m.head_dist.weight.shape) == (10, 64) and float(m.head_dist.bias.detach().abs().max()) == 0.0
    assert 0.0 < float(m.head_dist.weight.detach().std()) < 0.04 and 0.0 < float(m.encoder.dist_token.detach().std()) < 0.04
    assert m.no_weight_decay() == {"encoder.pos_embed", "encoder.cls_token", "encoder.dist_token"}
    assert plain.no_weight_decay() == {"encoder.pos_embed", "encoder.cls_token"}
    assert m.encoder.no_weight_decay() == {"pos_embed", "cls_token", "dist_token"}
    assert m.encoder._cfg_kwargs["distilled"] is True and plain.encoder._cfg_kwargs["distilled"] is False


def test_backbone_config_counts_the_distillation_token():
    from m3vit_amd.config import BackboneConfig, init_params
    assert BackboneConfig().num_tokens == 197 and BackboneConfig(distilled=True).num_tokens == 198
    kw = dict(img_size=(32, 48), embed_dim=64, depth=2, num_heads=2, moe_experts=4, moe_top_k=2, gate_dim=66)
    P, P2 = init_params(BackboneConfig(**kw)), init_params(BackboneConfig(distilled=True, **kw))
    assert "dist_token" not in P and tuple(P["pos_embed"].shape) == (1, 7, 64)
    assert tuple(P2["dist_token"].shape) == (1, 1, 64) and tuple(P2["pos_embed"].shape) == (1, 8, 64)
    assert set(P2) - set(P) == {"dist_token"}


def test_resize_pos_embed_keeps_the_prefix_rows():
    from m3vit_amd.checkpoint import resize_pos_embed, to_backbone_state
    pe = torch.randn(1, 2 + 16, 8, generator=torch.Generator().manual_seed(3))
    out = resize_pos_embed(pe, (6, 5), num_prefix=2)
    assert tuple(out.shape) == (1, 2 + 30, 8) and torch.equal(out[:, :2], pe[:, :2])
    one = pe[:, 1:]
    assert torch.equal(resize_pos_embed(one, (6, 5)), resize_pos_embed(one, (6, 5), num_prefix=1))
    assert torch.equal(out[:, 2:], resize_pos_embed(one, (6, 5))[:, 1:])
    with pytest.raises(ValueError):
        resize_pos_embed(pe, (6, 5))                               # 17 patch positions are no square grid
    state, _ = to_backbone_state({"pos_embed": pe, "dist_token": torch.zeros(1, 1, 8), "cls_token": torch.zeros(1, 1, 8)},
                                 grid_hw=(6, 5))
    assert torch.equal(state["pos_embed"], out)


def test_distillation_loss_constructor_rules():
    from m3vit_amd.pretrain import CrossEntropy, DistillationLoss
    teacher = torch.nn.Linear(4, 3)
    for kind in ("soft", "hard"):
        with pytest.raises(NotImplementedError):
            DistillationLoss(CrossEntropy(), None, kind, 0.5, 1.0)
    with pytest.raises(ValueError):
        DistillationLoss(CrossEntropy(), teacher, "medium", 0.5, 1.0)
    crit = DistillationLoss(CrossEntropy(), teacher, "hard", 0.5, 1.0)
    assert crit.distillation_type == "hard" and crit.teacher_model is teacher
    assert DistillationLoss(CrossEntropy(), None, "none", 0.5, 1.0).distillation_type == "none"
