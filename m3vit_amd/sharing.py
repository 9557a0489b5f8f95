"""The persistent-sharing stage of the reference's token backbone (models/moe/token/) over the HIP kernels of
csrc/share.hip, with the reference's names, constructor arguments, parameter names and call signatures:

  ShareabilityPredictor, Aggregation            token/shareability.py:14-121
  AggregationStage                              models/moe/aggregation_stages.py
  SharingRegularizationLoss                     token/sharing_loss.py
  transition_stage, apply_shared_broadcast      TokenBlock's methods, token/vision_transformer_moe.py:519-671, as functions
  SharingStage                                  predictor + transition + broadcast of TokenBlock.forward (:873-959) fused: one
                                                row pass, one autograd node, no host read, graph-capturable
  TokenFFNStage                                 step 5 of TokenBlock.forward for the blocks that need no router: the dense
                                                block's dense_mlp_stage + shared_dense_forward + apply_shared_broadcast
                                                (:443-515, :966-984), or the shared_ffn branch of an MoE block (:1002-1014),
                                                over private and shared rows only (csrc/token_ffn.hip)

Differences from the reference, all on purpose:
  * no host read in SharingStage, Aggregation, AggregationStage or SharingRegularizationLoss: no nonzero(), .any() or
    .item().  Where the reference returns early because nothing is shared or nothing needs aggregating, the kernels run
    and write the same values; Aggregation.forward always returns the dense tensor (zero rows where nothing is aggregated)
    and never None; SharingRegularizationLoss returns a float32 zero where the reference returns an int64 one;
  * transition_stage / apply_shared_broadcast return exactly what the methods return - the compact [K, C] shared_x, the [K]
    int64 index, the Nones when nothing is shared, Python integers in trans_aux - which costs ONE host read of the
    statistics words (K among them) in transition_stage; apply_shared_broadcast reads nothing;
  * ShareabilityPredictor.forward takes noise= (the Gumbel draws, [.., 2]); absent, they are drawn on the device as
    F.gumbel_softmax draws them;
  * 2 <= num_tasks <= 8, d_model a multiple of 8 up to 1024; CPU tensors raise M3Error: there is no eager fallback.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import _lib, ops
from .functional import ShareAggregateFn, SharePredictFn, ShareStageFn, TokenFFNFn

__all__ = ["ShareabilityPredictor", "Aggregation", "AggregationStage", "SharingRegularizationLoss", "SharingStage",
           "SharedTokens", "TokenFFNStage", "transition_stage", "apply_shared_broadcast"]

_STAT = {k[len("M3_SHARE_STAT_"):].lower(): v for k, v in _lib.CONSTANTS.items() if k.startswith("M3_SHARE_STAT_")}


def _gpu(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.M3Error(f"{name} must be a GPU tensor (no CPU path)")
    return t


def _tasks(outs, num_tasks, what):
    """the task tensors of a {task_id: tensor} dictionary (or a list) in task order"""
    T = len(outs) if num_tasks is None else num_tasks
    if not 2 <= T <= ops.SHARE_MAX_T:
        raise _lib.M3Error(f"{what}: num_tasks={T}; the sharing kernels take 2 to {ops.SHARE_MAX_T} tasks")
    xs = [_gpu(outs[t], f"{what}: outs[{t}]") for t in range(T)]
    for t, x in enumerate(xs):
        if x.shape != xs[0].shape or x.dtype != xs[0].dtype or x.dim() != 3:
            raise _lib.M3Error(f"{what}: outs[{t}] is {x.dtype} {tuple(x.shape)}, outs[0] {xs[0].dtype} {tuple(xs[0].shape)}; "
                               "every task tensor must be [B, N, C] of one dtype")
    return xs


def gumbel_noise(shape, device):
    """the draws of F.gumbel_softmax: -log of a unit exponential, float32, on the device"""
    return -torch.empty(shape, dtype=torch.float32, device=device).exponential_().log()


class ShareabilityPredictor(nn.Module):
    """Gumbel-softmax shareability predictor: the shared probability of every token from [token | task embedding] @ w_gate."""

    def __init__(self, d_model, d_task_emb=0, temperature=1.0, hard=False):
        super().__init__()
        self.d_model = d_model
        self.d_task_emb = d_task_emb
        d_input = d_model + d_task_emb if d_task_emb > 0 else d_model
        self.w_gate = nn.Parameter(torch.zeros(d_input, 2), requires_grad=True)
        self.temperature = temperature
        self.hard = hard
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.kaiming_uniform_(self.w_gate, a=math.sqrt(5))

    def _hard(self):
        return self.hard if self.training else True

    def forward(self, inp, task_emb=None, noise=None):
        """inp [B, N, D] or [B*N, D]; task_emb [E], [B, E] or [B, N, E]; returns the shared probability [B, N] or [B*N]
        (float32).  The [E] form - the one a TokenBlock passes - runs wholly in the kernel; the other two compute their
        share of the logits with one torch product first."""
        _gpu(inp, "inp")
        assert not (self.d_task_emb > 0 and task_emb is None), (
            "ShareabilityPredictor requires task_emb when d_task_emb > 0 (check task_emb_T_E wiring).")
        lead = inp.shape[:-1]
        D = inp.shape[-1]
        P = inp.numel() // D
        if noise is None:
            noise = gumbel_noise((P, 2), inp.device)
        else:
            noise = _gpu(noise, "noise").reshape(P, 2)
        w, emb, offset = self.w_gate, None, None
        if task_emb is not None and task_emb.dim() == 1:
            emb = _gpu(task_emb, "task_emb")
        elif task_emb is not None:
            if task_emb.dim() == 2:
                B = lead[0] if len(lead) > 1 else 1
                flat = task_emb.unsqueeze(1).expand(B, P // B, -1).reshape(P, -1)
            else:
                flat = task_emb.reshape(P, -1)
            offset = flat.to(torch.float32) @ self.w_gate[D:]
            w = self.w_gate[:D]
        g = SharePredictFn.apply(inp, w, emb, noise, offset, float(self.temperature), self._hard())
        return g.reshape(*lead) if len(lead) > 1 else g


def _pack_masks(masks):
    """int64 bits of a list of [B, N] bool masks (bit t = masks[t]), torch ops on the device"""
    bits = torch.zeros(masks[0].shape, dtype=torch.int64, device=masks[0].device)
    for t, m in enumerate(masks):
        bits |= m.to(torch.int64) << t
    return bits.reshape(-1)


class Aggregation(nn.Module):
    """The mean over the tasks whose mask is set, at the positions aggregation_mask names.  Returns the dense [B, N, D]
    tensor (valid where aggregation_mask is set, zero elsewhere); never None."""

    def __init__(self, eps=1e-6):
        super().__init__()
        self.eps = eps

    def _run(self, task_outputs, curr_shared_masks, aggregation_mask):
        xs = _tasks(task_outputs, len(curr_shared_masks), "Aggregation")
        need = _gpu(aggregation_mask, "aggregation_mask").reshape(-1).to(torch.bool).contiguous()
        *ys, agg = ShareAggregateFn.apply(_pack_masks(curr_shared_masks), need, float(self.eps), *xs)
        return ys, agg.view(xs[0].shape)

    def forward(self, task_outputs, curr_shared_masks, aggregation_mask):
        return self._run(task_outputs, curr_shared_masks, aggregation_mask)[1]


class AggregationStage(nn.Module):
    """Writes the aggregate back to the tasks that took part: outs[t] = aggregated where agg_needed & shared_masks[t]."""

    def __init__(self, aggregation_module, num_tasks: int):
        super().__init__()
        self.agg = aggregation_module
        self.num_tasks = num_tasks

    def forward(self, outs: dict, shared_masks: list, agg_needed_mask: torch.Tensor):
        if agg_needed_mask is None:
            return outs
        ys, _ = self.agg._run(outs, list(shared_masks)[:self.num_tasks], agg_needed_mask)
        for t, y in enumerate(ys):
            outs[t] = y
        return outs


class SharingRegularizationLoss(nn.Module):
    """L_share = lambda * max(0, S^2 - sum_t S_t^2), S the shared positions and S_t those task t takes part in, counted by
    m3_share_compact and combined in float32 in the reference's order.  No host read."""

    def __init__(self, lambda_share: float = 0.01):
        super().__init__()
        self.lambda_share = lambda_share

    def forward(self, shared_bits: torch.Tensor, num_tasks: int) -> torch.Tensor:
        _gpu(shared_bits, "shared_bits")
        if self.lambda_share <= 0.0:
            return torch.zeros((), dtype=torch.float32, device=shared_bits.device)
        _, _, stats = ops.share_compact(shared_bits.contiguous().reshape(-1), num_tasks, want_idx=False)
        return _share_loss_from_stats(stats, num_tasks, self.lambda_share)


def _share_loss_from_stats(stats, num_tasks, lambda_share):
    f = stats.to(torch.float32)
    S = f[_STAT["s"]]
    sq = f[_STAT["s_t"]:_STAT["s_t"] + num_tasks]
    acc = torch.zeros((), dtype=torch.float32, device=stats.device)
    for t in range(num_tasks):                      # the reference's order of additions
        acc = acc + sq[t] * sq[t]
    return lambda_share * torch.clamp(S * S - acc, min=0.0)


def _aux_from_words(w, device, dtype):
    """the trans_aux dictionary of TokenBlock.transition_stage from the statistics words (a list of Python integers)"""
    return {
        "cv_loss": torch.zeros((), dtype=dtype, device=device),
        "stats": {"shared_positions": w[_STAT["positions"]], "shared_tasktoken_count": w[_STAT["tasktokens"]]},
        "analysis": {"shared_bits_flip_count": w[_STAT["flips"]], "shared_bits_flip_total": w[_STAT["flip_total"]],
                     "partial_split_count": w[_STAT["partial"]], "partial_split_total": w[_STAT["partial_total"]]},
    }


class SharedTokens:
    """What SharingStage.forward leaves for the rest of the block, all device-resident:
      bits      int64 [B, N]      bit t: task t uses the shared path at the position
      x         [B*N, C]          the representative token, dense (zero rows where bits == 0); carries gradient
      flat_idx  int32 [B*N]       the flat positions with bits != 0, ascending, then -1
      count     int32 [1]         how many
      g         float32 [T, B, N] the predictor's scores
      stats     int64 words       m3_share_compact's statistics (aux() reads them)"""

    def __init__(self, bits, x, flat_idx, count, g, stats, num_tasks):
        self.bits, self.x, self.flat_idx, self.count, self.g, self.stats, self.num_tasks = bits, x, flat_idx, count, g, stats, num_tasks
        self._aux = None

    def aux(self):
        """the reference's trans_aux dictionary; the first call copies the statistics words to the host (one read)"""
        if self._aux is None:
            self._aux = _aux_from_words(self.stats.tolist(), self.x.device, self.x.dtype)
        return self._aux

    def compact(self):
        """(shared_x [K, C], shared_flat_idx int64 [K]) as TokenBlock.transition_stage returns them, or (None, None) when
        nothing is shared: one host read (of K)"""
        K = int(self.count.item())
        if K == 0:
            return None, None
        idx = self.flat_idx[:K].to(torch.int64)
        return self.x.index_select(0, idx), idx

    def regularization(self, lambda_share=0.01):
        """SharingRegularizationLoss of these bits from the statistics already counted: no launch of its own"""
        return _share_loss_from_stats(self.stats, self.num_tasks, lambda_share)


class SharingStage(nn.Module):
    """TokenBlock.forward's steps 2 - 4 in one: g_shared[t] = share_pred(outs[t], task_emb_T_E[t]), transition_stage,
    apply_shared_broadcast.  Two launches (the row pass; compaction + statistics), no host read, fixed shapes, the caller's
    stream; one autograd node whose backward is m3_share_stage_bwd."""

    def __init__(self, share_pred: ShareabilityPredictor, num_tasks: int, eps: float = 1e-6):
        super().__init__()
        if not 2 <= num_tasks <= ops.SHARE_MAX_T:
            raise _lib.M3Error(f"SharingStage: num_tasks={num_tasks}; the sharing kernels take 2 to {ops.SHARE_MAX_T} tasks")
        self.share_pred = share_pred
        self.num_tasks = num_tasks
        self.eps = eps

    def forward(self, outs, prev_shared_bits=None, task_emb_T_E=None, gamma=0.5, noise=None):
        """outs {t: [B, N, C]}; prev_shared_bits int64 [B, N] or None; task_emb_T_E [T, E] (or None when the predictor has
        no task embedding); noise float32 [T, B, N, 2] (drawn on the device when absent).  Returns (outs, SharedTokens):
        a new dictionary with the broadcast applied."""
        T, sp = self.num_tasks, self.share_pred
        xs = _tasks(outs, T, "SharingStage")
        B, N, C = xs[0].shape
        assert not (sp.d_task_emb > 0 and task_emb_T_E is None), (
            "ShareabilityPredictor requires task_emb when d_task_emb > 0 (check task_emb_T_E wiring).")
        emb = None
        if sp.d_task_emb > 0:
            emb = _gpu(task_emb_T_E, "task_emb_T_E")[:T]
        if noise is None:
            noise = gumbel_noise((T, B * N, 2), xs[0].device)
        else:
            noise = _gpu(noise, "noise").to(torch.float32).reshape(T, B * N, 2).contiguous()
        *ys, sx, bits, g = ShareStageFn.apply(sp.w_gate, emb, noise, float(sp.temperature), sp._hard(), float(gamma),
                                              float(self.eps), *xs)
        prev = None
        if prev_shared_bits is not None and prev_shared_bits.shape == (B, N):
            prev = _gpu(prev_shared_bits, "prev_shared_bits").contiguous().reshape(-1)
        idx, count, stats = ops.share_compact(bits, T, prev)
        out = dict(outs) if isinstance(outs, dict) else list(outs)
        for t, y in enumerate(ys):
            out[t] = y
        return out, SharedTokens(bits.view(B, N), sx, idx, count, g.view(T, B, N), stats, T)


class TokenFFNStage(nn.Module):
    """TokenBlock.forward's step 5 where no router is needed, as one autograd node over the rows that differ:
      mode "all"     the dense block: outs = dense_mlp_stage(outs, shared_bits); shared_out = shared_dense_forward(shared_x);
                     outs = apply_shared_broadcast(outs, shared_bits, shared_out) - private rows and one row per shared
                     position through ONE norm2 / mlp, one FC1 and one FC2 launch for all of them
      mode "shared"  the MoE block's shared branch: shared_out = shared_x + drop_path(shared_ffn(norm2(shared_x))), then the
                     broadcast; private rows pass through (they are the router's)
    Holds the caller's nn.LayerNorm and Mlp (a TokenBlock's norm2 and mlp / shared_ffn), as SharingStage holds its predictor:
    its state-dict keys are the block's own: norm2.*, mlp.fc1.*, mlp.fc2.* (mode "shared": norm2.*, shared_ffn.fc1.*, shared_ffn.fc2.*).  A position shared by s
    tasks costs one FFN row, not s; the row count stays on the device: no host read, fixed shapes, the caller's stream,
    graph-capturable.  Refused (M3Error): Mlp.drop.p > 0 in training, an activation other than the erf GELU, num_tasks outside
    2 .. 8, C or H no multiple of 8, C > 1024, CPU tensors, and whatever the GEMM's own reach rule refuses."""

    def __init__(self, norm2: nn.LayerNorm, mlp: nn.Module, num_tasks: int, mode: str = "all", drop_path: float = 0.0):
        super().__init__()
        if not 2 <= num_tasks <= ops.SHARE_MAX_T:
            raise _lib.M3Error(f"TokenFFNStage: num_tasks={num_tasks}; the token kernels take 2 to {ops.SHARE_MAX_T} tasks")
        if mode not in ops.TOKEN_FFN_MODES:
            raise _lib.M3Error(f"TokenFFNStage: mode {mode!r} is neither 'all' nor 'shared'")
        if not isinstance(norm2, nn.LayerNorm) or len(norm2.normalized_shape) != 1 or norm2.weight is None or norm2.bias is None:
            raise _lib.M3Error("TokenFFNStage: norm2 must be an nn.LayerNorm over the last dimension with weight and bias")
        act = getattr(mlp, "act", None)
        if not isinstance(act, nn.GELU) or getattr(act, "approximate", "none") != "none":
            raise _lib.M3Error(f"TokenFFNStage: the activation is {type(act).__name__}; the FC1 epilogue computes the erf GELU only")
        C, H = mlp.fc1.in_features, mlp.fc1.out_features
        if norm2.normalized_shape[0] != C or mlp.fc2.in_features != H or mlp.fc2.out_features != C:
            raise _lib.M3Error(f"TokenFFNStage: norm2 {tuple(norm2.normalized_shape)}, fc1 {C} -> {H}, fc2 {mlp.fc2.in_features} -> "
                               f"{mlp.fc2.out_features} do not make a residual FFN")
        if mlp.fc1.bias is None or mlp.fc2.bias is None:
            raise _lib.M3Error("TokenFFNStage: fc1 and fc2 must have a bias, as the reference's Mlp")
        if C % 8 or H % 8 or not 8 <= C <= ops.SHARE_MAX_D:
            raise _lib.M3Error(f"TokenFFNStage: C={C} and H={H} must be multiples of 8 and C at most {ops.SHARE_MAX_D}")
        if not 0.0 <= float(drop_path) < 1.0:
            raise _lib.M3Error(f"TokenFFNStage: drop_path={drop_path} outside [0, 1)")
        self.norm2 = norm2
        self.add_module(self._ffn_name(mode), mlp)       # the TokenBlock's name for it: mlp, or shared_ffn in an MoE block
        self.num_tasks, self.mode, self.drop_path = num_tasks, mode, float(drop_path)

    @staticmethod
    def _ffn_name(mode):
        return "mlp" if mode == "all" else "shared_ffn"

    @property
    def ffn(self):
        return getattr(self, self._ffn_name(self.mode))

    def _drop_p(self):
        d = getattr(self.ffn, "drop", None)
        return float(getattr(d, "p", 0.0) or 0.0)

    def forward(self, outs, shared: "SharedTokens | None" = None, path_scale=None, shared_path_scale=None):
        """outs {t: [B, N, C]} (SharingStage's, the broadcast already applied); shared: its SharedTokens, or None = nothing
        is shared (the reference's shared_bits=None); path_scale f32 [B] / shared_path_scale f32 [B, N] or [B*N]: the DropPath
        factors of the private rows (one per sample and block) and of the shared rows (one per shared row), None = 1 - or, in
        training with drop_path > 0, drawn on the device.  Returns a new dictionary (or list)."""
        T = self.num_tasks
        if self.training and self._drop_p() > 0.0:
            raise _lib.M3Error(f"TokenFFNStage: Mlp.drop.p={self._drop_p()} in training; element-wise dropout is not built on this path")
        xs = _tasks(outs, T, "TokenFFNStage")
        B, N, C = xs[0].shape
        if C != self.ffn.fc1.in_features:
            raise _lib.M3Error(f"TokenFFNStage: tokens of width {C}, the Mlp takes {self.ffn.fc1.in_features}")
        dev = xs[0].device
        if shared is None:
            bits = torch.zeros(B * N, dtype=torch.int64, device=dev)
            sx = torch.zeros((B * N, C), dtype=xs[0].dtype, device=dev)
        else:
            bits = _gpu(shared.bits, "shared.bits").contiguous().reshape(-1)
            sx = _gpu(shared.x, "shared.x")
            if bits.dtype != torch.int64 or bits.numel() != B * N or sx.shape != (B * N, C) or sx.dtype != xs[0].dtype:
                raise _lib.M3Error(f"TokenFFNStage: shared.bits {bits.dtype} {tuple(shared.bits.shape)} / shared.x {sx.dtype} "
                                   f"{tuple(sx.shape)} do not go with outs {xs[0].dtype} {(B, N, C)}")
        if self.training and self.drop_path > 0.0:
            keep = 1.0 - self.drop_path
            if path_scale is None and self.mode == "all":
                path_scale = torch.floor(keep + torch.rand(B, dtype=torch.float32, device=dev)) / keep
            if shared_path_scale is None:
                shared_path_scale = torch.floor(keep + torch.rand(B * N, dtype=torch.float32, device=dev)) / keep
        if path_scale is not None:
            path_scale = _gpu(path_scale, "path_scale").to(torch.float32).reshape(-1).contiguous()
        if shared_path_scale is not None:
            shared_path_scale = _gpu(shared_path_scale, "shared_path_scale").to(torch.float32).reshape(-1).contiguous()
        ys = TokenFFNFn.apply(bits, self.norm2.weight, self.norm2.bias, float(self.norm2.eps), self.ffn.fc1.weight,
                              self.ffn.fc1.bias, self.ffn.fc2.weight, self.ffn.fc2.bias, path_scale, shared_path_scale,
                              self.mode, N, sx, *xs)
        out = dict(outs) if isinstance(outs, dict) else list(outs)
        for t, y in enumerate(ys):
            out[t] = y
        return out


def transition_stage(outs, prev_shared_bits, g_shared, gamma=0.5, eps=1e-6, num_tasks=None):
    """TokenBlock.transition_stage as a function: (shared_bits int64 [B, N], shared_x [K, C] or None, shared_flat_idx
    int64 [K] or None, trans_aux).  The scores are the caller's: the stage kernel is not involved, the mixing is torch's
    index arithmetic on the K positions m3_share_compact lists.  ONE host read: the statistics words (K among them)."""
    xs = _tasks(outs, num_tasks, "transition_stage")
    T = len(xs)
    B, N, C = xs[0].shape
    G = torch.stack([_gpu(g_shared[t], f"g_shared[{t}]") for t in range(T)], dim=0)
    M = G >= gamma
    M = M & (M.sum(dim=0) >= 2).unsqueeze(0)
    bits = _pack_masks(list(M.reshape(T, B * N)))
    prev = None
    if prev_shared_bits is not None and prev_shared_bits.shape == (B, N):
        prev = _gpu(prev_shared_bits, "prev_shared_bits").contiguous().reshape(-1)
    idx, _, stats = ops.share_compact(bits, T, prev)
    words = stats.tolist()                                              # the one host read
    aux = _aux_from_words(words, xs[0].device, xs[0].dtype)
    K = words[_STAT["positions"]]
    if K == 0:
        return bits.view(B, N), None, None, aux
    flat = idx[:K].to(torch.int64)
    GM = (G * M.to(G.dtype)).reshape(T, B * N)[:, flat]
    W = GM / (GM.sum(dim=0, keepdim=True) + eps)
    shared_x = xs[0].new_zeros((K, C))
    for t in range(T):
        shared_x = shared_x + W[t].unsqueeze(-1) * xs[t].reshape(B * N, C)[flat]
    return bits.view(B, N), shared_x, flat, aux


def apply_shared_broadcast(outs, shared_bits, shared_x, shared_flat_idx=None, *, num_tasks=None):
    """TokenBlock.apply_shared_broadcast as a function: outs[t][b, n] = shared_x[row of (b, n)] where bit t of shared_bits
    is set; outs itself when shared_x is None.  The compact rows are scattered to the dense layout, then one torch.where per
    task; no host read (a missing shared_flat_idx is recomputed by m3_share_compact)."""
    if shared_x is None:
        return outs
    xs = _tasks(outs, num_tasks, "apply_shared_broadcast")
    B, N, C = xs[0].shape
    assert shared_bits.shape == (B, N), f"shared_bits shape {shared_bits.shape} != {(B, N)}"
    if shared_flat_idx is None:
        shared_flat_idx, _, _ = ops.share_compact(shared_bits.contiguous().reshape(-1), len(xs))
        shared_flat_idx = shared_flat_idx[:shared_x.shape[0]]
    if shared_flat_idx.numel() == 0:
        return outs
    dense = shared_x.new_zeros((B * N, C)).index_copy(0, shared_flat_idx.to(torch.int64), shared_x)
    for t, x in enumerate(xs):
        m = ((shared_bits.reshape(-1) >> t) & 1).bool().unsqueeze(-1)
        outs[t] = torch.where(m, dense, x.reshape(B * N, C)).view(B, N, C)
    return outs
