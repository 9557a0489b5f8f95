"""Routing statistics, host side (no GPU): the public attributes of VisionTransformerMoE / Block with moe_stats on and off,
the record parser, and the fold of block dicts into `latest_moe_stats` against a float64 restatement of the definitions
(written here from the specification, key by key):

  per block   gate_entropy_sum, top1_prob_sum, gate_token_count, expert_load_hist [E], expert_load_cv, clean_logit_std,
              moe_out_norm_ratio, expert_hidden_dim, active_vs_dense_flops_ratio
  backbone    moe_blocks, total_positions = sum_blocks B * max(N - 1, 0), analysis:
              gate_entropy = sum entropy sums / sum token counts, top1_prob_mean likewise (0.0 for no tokens),
              expert_load_hist = element-wise sum, dead_expert_ratio = share of its zero entries,
              the other five keys = plain means over the MoE blocks."""
import struct

import pytest
import torch

from m3vit_amd import moe_stats as ms
from m3vit_amd.vit import VisionTransformerMoE

CFG = dict(img_size=32, patch_size=16, embed_dim=64, depth=4, num_heads=2, num_classes=3, mlp_ratio=4.0, moe_mlp_ratio=1.5,
           moe_experts=8, moe_top_k=2)


def test_attributes_with_the_flag_on():
    model = VisionTransformerMoE(moe_stats=True, **CFG)
    assert model.latest_moe_stats is None                       # before any forward
    assert model.wandb_logger is None
    for i, blk in enumerate(model.blocks):
        assert blk.last_moe_analysis is None
        if blk.moe:
            assert blk.expert_hidden_dim == int(64 * 1.5) and isinstance(blk.expert_hidden_dim, int)
            assert blk.active_vs_dense_flops_ratio == pytest.approx(2 * 96 / 256, abs=0.0)
            assert isinstance(blk.active_vs_dense_flops_ratio, float)
        else:
            assert blk.expert_hidden_dim is None and blk.active_vs_dense_flops_ratio is None
    assert [blk.moe for blk in model.blocks] == [False, True, False, True]


def test_flag_off_is_none_and_does_not_raise():
    model = VisionTransformerMoE(**CFG)
    assert model.moe_stats is False
    assert model.latest_moe_stats is None
    assert all(blk.last_moe_analysis is None for blk in model.blocks)
    # the static fields do not depend on the flag (the reference sets them in the constructor)
    assert model.blocks[1].expert_hidden_dim == 96


def test_moe_mlp_ratio_defaults_to_mlp_ratio():
    cfg = dict(CFG)
    cfg.pop("moe_mlp_ratio")
    model = VisionTransformerMoE(moe_stats=True, **cfg)
    assert model.blocks[1].expert_hidden_dim == 256
    assert model.blocks[1].active_vs_dense_flops_ratio == 2.0


def test_origin_convention_is_refused_loudly():
    with pytest.raises(NotImplementedError):
        VisionTransformerMoE(moe_stats=True, convention="origin", **CFG)


def _words(entropy, top1, std, ratio, cv, tokens, hist):
    f = [entropy, top1, std, ratio, cv, 0.0, 0.0]
    w = list(struct.unpack("<7i", struct.pack("<7f", *f)))
    return w + [tokens] + list(hist)


def test_parse_record_types_and_values():
    hist = [3, 0, 7, 1]
    d = ms.parse_record(_words(1.5, 2.25, 0.5, 0.125, 0.75, 11, hist), 4, 96, 0.75)
    assert d == {"gate_entropy_sum": 1.5, "top1_prob_sum": 2.25, "gate_token_count": 11, "expert_load_hist": hist,
                 "expert_load_cv": 0.75, "clean_logit_std": 0.5, "moe_out_norm_ratio": 0.125, "expert_hidden_dim": 96,
                 "active_vs_dense_flops_ratio": 0.75}
    assert type(d["gate_token_count"]) is int and type(d["expert_hidden_dim"]) is int
    assert all(type(v) is int for v in d["expert_load_hist"])
    for key in ("gate_entropy_sum", "top1_prob_sum", "expert_load_cv", "clean_logit_std", "moe_out_norm_ratio",
                "active_vs_dense_flops_ratio"):
        assert type(d[key]) is float
    assert ms.record_words(4) == len(_words(0, 0, 0, 0, 0, 0, hist))


def _block(seed, E, tokens):
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(6, generator=g, dtype=torch.float64).tolist()
    hist = torch.randint(0, 4, (E,), generator=g).tolist()
    hist[0] = 0                                                  # expert 0 dead in every block, others maybe
    return {"gate_entropy_sum": 100 * r[0], "top1_prob_sum": 50 * r[1], "gate_token_count": tokens, "expert_load_hist": hist,
            "expert_load_cv": r[2], "clean_logit_std": r[3], "moe_out_norm_ratio": r[4], "expert_hidden_dim": 96 + seed,
            "active_vs_dense_flops_ratio": r[5]}


def test_aggregate_against_the_float64_restatement():
    E, B, N = 8, 3, 5
    blocks = [_block(s, E, B * N) for s in range(3)]
    got = ms.aggregate(blocks, B * max(N - 1, 0))
    assert set(got) == {"moe_blocks", "total_positions", "analysis"}
    assert got["moe_blocks"] == 3 and type(got["moe_blocks"]) is int
    assert got["total_positions"] == 3 * B * (N - 1) and type(got["total_positions"]) is int
    an = got["analysis"]
    assert set(an) == {"gate_entropy", "top1_prob_mean", "expert_load_hist", "dead_expert_ratio", "expert_load_cv",
                       "clean_logit_std", "moe_out_norm_ratio", "expert_hidden_dim", "active_vs_dense_flops_ratio"}
    tokens = float(sum(b["gate_token_count"] for b in blocks))
    assert an["gate_entropy"] == pytest.approx(sum(b["gate_entropy_sum"] for b in blocks) / tokens, rel=1e-15)
    assert an["top1_prob_mean"] == pytest.approx(sum(b["top1_prob_sum"] for b in blocks) / tokens, rel=1e-15)
    hist = [sum(b["expert_load_hist"][e] for b in blocks) for e in range(E)]
    assert an["expert_load_hist"] == hist and all(type(v) is int for v in an["expert_load_hist"])
    dead = sum(1 for v in hist if v == 0)
    assert dead >= 1
    assert an["dead_expert_ratio"] == dead / E
    for key in ("expert_load_cv", "clean_logit_std", "moe_out_norm_ratio", "expert_hidden_dim", "active_vs_dense_flops_ratio"):
        assert an[key] == pytest.approx(sum(float(b[key]) for b in blocks) / 3.0, rel=1e-15)
        assert type(an[key]) is float
    for key in ("gate_entropy", "top1_prob_mean", "dead_expert_ratio"):
        assert type(an[key]) is float


def test_aggregate_zero_tokens_and_no_blocks():
    z = _block(1, 4, 0)
    z["gate_entropy_sum"] = z["top1_prob_sum"] = 0.0
    an = ms.aggregate([z], 0)["analysis"]
    assert an["gate_entropy"] == 0.0 and an["top1_prob_mean"] == 0.0
    empty = ms.aggregate([], 7)
    assert empty["moe_blocks"] == 0 and empty["total_positions"] == 0
    assert empty["analysis"]["expert_load_hist"] == [] and empty["analysis"]["dead_expert_ratio"] == 0.0
    assert empty["analysis"]["expert_load_cv"] == 0.0


def test_cls_only_images_have_zero_positions():
    """total_positions counts patches: N - 1 per image, never negative"""
    assert ms.aggregate([_block(0, 4, 2)], 2 * max(1 - 1, 0))["total_positions"] == 0
