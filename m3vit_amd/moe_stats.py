"""Host side of the routing statistics: the record m3_moe_stats writes (layout in include/m3vit_hip.h) as the reference's
per-block `last_moe_analysis` dict (models/moe/ckpt/vision_transformer_moe.py:552-562), and the backbone-level fold into
`latest_moe_stats` (:799-873).  Pure Python on numbers the caller already holds - nothing here touches the device except
`read_records`, the ONE device-to-host copy of a pass's records."""
from __future__ import annotations

import struct

# the record's word indices, from include/m3vit_hip.h; HDR: four-byte words before the histogram
from ._lib import (M3_MOE_STATS_CLEAN_STD as CLEAN_STD, M3_MOE_STATS_ENTROPY_SUM as ENTROPY_SUM,  # noqa: F401
                   M3_MOE_STATS_H_SUMSQ as H_SUMSQ, M3_MOE_STATS_HIST as HDR, M3_MOE_STATS_LOAD_CV as LOAD_CV,
                   M3_MOE_STATS_M_SUMSQ as M_SUMSQ, M3_MOE_STATS_NORM_RATIO as NORM_RATIO, M3_MOE_STATS_TOKENS as TOKENS,
                   M3_MOE_STATS_TOP1_SUM as TOP1_SUM)


def record_words(E: int) -> int:
    return HDR + int(E)


def static_fields(dim, mlp_ratio, moe_mlp_ratio, top_k):
    """(expert_hidden_dim, active_vs_dense_flops_ratio) of a MoE block: the expert hidden width and
    top_k * expert_hidden_dim / max(int(dim * mlp_ratio), 1) (the dense MLP's width; vision_transformer_moe.py:400-419)"""
    hidden = int(dim * moe_mlp_ratio)
    dense = int(dim * mlp_ratio)
    return hidden, float(top_k * hidden) / float(max(dense, 1))


def parse_record(words, E: int, expert_hidden_dim: int = 0, flops_ratio: float = 0.0) -> dict:
    """words: the record's HDR + E int32 words as a sequence of Python ints -> the block dict, with the reference's key
    names and Python types"""
    w = [int(v) for v in words[:HDR + E]]
    f = struct.unpack(f"<{HDR}f", struct.pack(f"<{HDR}i", *w[:HDR]))
    return {
        "gate_entropy_sum": float(f[ENTROPY_SUM]),
        "top1_prob_sum": float(f[TOP1_SUM]),
        "gate_token_count": int(w[TOKENS]),
        "expert_load_hist": [int(v) for v in w[HDR:HDR + E]],
        "expert_load_cv": float(f[LOAD_CV]),
        "clean_logit_std": float(f[CLEAN_STD]),
        "moe_out_norm_ratio": float(f[NORM_RATIO]),
        "expert_hidden_dim": int(expert_hidden_dim),
        "active_vs_dense_flops_ratio": float(flops_ratio),
    }


def read_records(records, E: int, static=(0, 0.0)):
    """records: int32 device tensor [n_blocks, HDR + E] -> list of block dicts (one copy, one synchronisation)"""
    rows = records.cpu().tolist()
    return [parse_record(r, E, *static) for r in rows]


def aggregate(blocks, positions_per_block: int) -> dict:
    """The backbone dict from the MoE blocks' dicts, in block order (vision_transformer_moe.py:799-873):
    gate_entropy / top1_prob_mean are the summed sums over the summed token count (0.0 for no tokens), the histogram is
    summed element-wise, dead_expert_ratio is the share of its zero entries, the other five keys are means over the blocks.
    positions_per_block = B * max(N - 1, 0)."""
    blocks = [b for b in blocks if isinstance(b, dict)]
    n = len(blocks)
    tokens = sum(int(b["gate_token_count"]) for b in blocks)
    hist = None
    for b in blocks:
        h = b.get("expert_load_hist")
        if h is None:
            continue
        if hist is None:
            hist = [0] * len(h)
        if len(hist) == len(h):
            hist = [a + int(v) for a, v in zip(hist, h)]
    hist = hist or []
    mean = lambda key: sum(float(b[key]) for b in blocks) / float(max(n, 1))           # noqa: E731
    return {
        "moe_blocks": n,
        "total_positions": n * int(positions_per_block),
        "analysis": {
            "gate_entropy": (sum(float(b["gate_entropy_sum"]) for b in blocks) / float(tokens)) if tokens > 0 else 0.0,
            "top1_prob_mean": (sum(float(b["top1_prob_sum"]) for b in blocks) / float(tokens)) if tokens > 0 else 0.0,
            "expert_load_hist": hist,
            "dead_expert_ratio": (float(sum(1 for v in hist if v == 0)) / float(len(hist))) if hist else 0.0,
            "expert_load_cv": mean("expert_load_cv"),
            "clean_logit_std": mean("clean_logit_std"),
            "moe_out_norm_ratio": mean("moe_out_norm_ratio"),
            "expert_hidden_dim": mean("expert_hidden_dim"),
            "active_vs_dense_flops_ratio": mean("active_vs_dense_flops_ratio"),
        },
    }
