"""Fused forward/backward executor for the MoE-ViT backbone hot path on one MI355X.

Host-side mirror of VisionTransformerMoE.forward_features / Block / Attention /
FMoETransformerMLP (models/moe/ckpt/vision_transformer_moe.py:283-313,438-487,780-880,
models/moe/ckpt/custom_moe_layer.py:161-322) as a straight-line sequence of HIP kernel
launches on one stream, with no host synchronisation anywhere (the reference has ~9
`.item()` syncs per MoE block plus fastmoe's count `.cpu()`):

  * fp32 master parameters (reference state_dict names/shapes), fp32 residual stream,
    activations feeding MFMA stored in the activation dtype (fp16 or fp32);
  * every Linear is the hand-written NT GEMM; dgrads use transposed operand copies of
    the weights that are refreshed once per step by `prepare_weights()`;
  * the MoE MLP is gate -> route_build -> grouped FC1 (+bias+GELU, row gather fused into
    the A load) -> grouped FC2 (+bias, scatter to token-major fused into the store) ->
    combine (+residual);
  * activations needed by the backward are kept resident (288 GB HBM: a whole ViT-S pass
    at batch 128 is ~5 GB), nothing is recomputed (the reference's
    --use_checkpointing False mode, run_exps.sh:17).

torch is used for buffer ownership and for the O(E) cv-loss arithmetic only.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch

from . import moe_stats as _ms
from . import ops
from .engine_ep import ExpertParallelMixin
from .ops import M3_ACT_GELU


def _cut(t, es):
    return t if es is None else t[es]


class BackboneEngine(ExpertParallelMixin):
    def __init__(self, cfg, params: Dict[str, torch.Tensor], batch: int, dtype=torch.float16,
                 device="cuda:0", ep_group=None, ep_world: int = 1, ep_rank: int = 0, share: "BackboneEngine" = None,
                 wgrad_stream: bool = False, checkpoint: bool = False, ep_capacity: float = 0.0,
                 experts_are_local: bool = False, ep_chunks: int = 1, ep_native: bool = False, moe_stats: bool = False):
        """params: GLOBAL parameters (all E experts).  With ep_world > 1 this rank keeps experts
        [ep_rank*E/W, (ep_rank+1)*E/W) (utils/common_config.py:179-185) and exchanges routed rows with
        the other ranks over torch.distributed (RCCL) - see engine_ep._experts_fwd_ep.
        share: another engine of the same configuration whose parameters and operand copies this one
        uses (params is ignored); it gets its own activations, scratch and gradient buffer, so the two
        can run different task passes concurrently on different HIP streams.
        wgrad_stream: launch the weight-gradient GEMMs of backward() on a second HIP stream - they hang off
        the dgrad chain (nothing downstream reads them), so they can fill the chain's memory-bound phases.
        checkpoint: the reference's default memory mode (`use_checkpointing`, train_fastmoe.py:178 ->
        torch.utils.checkpoint around every block, vision_transformer_moe.py:495-524): forward keeps only each block's
        input; backward re-runs a block's forward (same kernels, same inputs: bit-identical activations) right before
        its backward.  All blocks then share ONE set of activation buffers.  With sharded experts (ep_world > 1, the
        reference's default combination) the recompute repeats NO collective: what crossed the wire in the forward - the
        exchange plan, the rows received for the local experts and the expert outputs that came back - is kept per MoE
        block, and only the local work (gate, FC1 of the local experts) is re-run.
        ep_capacity (with ep_world > 1; 0 = off): exchange the routed rows with a FIXED capacity of
        ceil(ep_capacity * R / W) rows per (source, destination) pair (R = T * k rows routed by a rank; 1.25 leaves a
        quarter of head room over a uniform routing) instead of the exact a2a-v: equal splits, the plan stays on the device
        (m3_ep_plan_fixed), NOTHING of the exchange is read by the host - one host read per STEP (ep_overflowed()) instead
        of one per MoE layer and pass, and a step that a collective library can capture.  A pair that routes more rows than
        the capacity raises the flag; the step's results are then incomplete and the caller repeats it on the exact path
        (MultiTaskStep does).
        ep_chunks (with ep_world > 1, exact exchange; 1 = one all-to-all-v each way): cut every exchange into this many
        chunks of E_loc / ep_chunks local experts (on every destination) and overlap them with the experts' GEMMs inside ONE
        pass - see engine_ep._experts_fwd_ep_chunked.  Same results bit for bit.
        ep_native (with ep_world > 1; opt-in, never run on more than one rank on this build box): the count and row exchanges
        go through the library's own RCCL entry points (m3vit_amd/ep_native.py: m3_ep_exchange_counts / m3_ep_dispatch /
        m3_ep_return) instead of torch.distributed's all_to_all_single.
        experts_are_local (with ep_world > 1): the expert tensors in `params` are already this rank's slice [E / W, ..] (a
        module built the way utils/common_config.py:179-185 builds it: moe_experts // world_size experts per rank) and are
        taken as they are - in place - instead of being cut out of global tensors.
        moe_stats (off by default: no buffer, no launch): every forward also leaves each MoE block's routing statistics -
        the reference's `last_moe_analysis` (vision_transformer_moe.py:461-478,546-562) - in a device-resident record
        (m3_moe_stats, launched behind the block's combine on the pass's stream, also inside a captured pass); nothing is
        read by the host until moe_stats() is called.  Under expert parallelism a rank reports its own tokens (every exchange
        variant brings the expert outputs home token-major, which is what the kernel reads)."""
        self.moe_stats_on = bool(moe_stats)
        assert not (checkpoint and wgrad_stream), "checkpoint mode re-uses the activation buffers a wgrad stream may still read"
        self.checkpoint = bool(checkpoint)
        assert dtype in (torch.float16, torch.bfloat16, torch.float32), "activation dtype: float16, bfloat16 or float32"
        self.cfg = cfg
        self.dev = torch.device(device)
        self.dt = dtype
        self.B = batch
        self.ep_group, self.ep_world, self.ep_rank = ep_group, int(ep_world), int(ep_rank)
        self.ep_capacity = float(ep_capacity) if int(ep_world) > 1 else 0.0
        assert not (self.ep_capacity and checkpoint), "fixed-capacity exchange: not with activation checkpointing"
        self.ep_fixed = self.ep_capacity > 0.0                 # switched off by the step runner for the exact repeat of a step
        self.D = cfg.embed_dim
        self.heads = cfg.num_heads
        self.dh = self.D // self.heads
        self.P = cfg.patch_size
        self.hp, self.wp = cfg.img_size[0] // self.P, cfg.img_size[1] // self.P
        self.np_ = self.hp * self.wp
        # a distilled model (vision_transformer_moe.py:602,627-629) carries a distillation token behind cls: told by the
        # parameters, not by cfg (the oracle's BackboneCfg has no such field)
        self.distilled = "dist_token" in (share.params if share is not None else params)
        self.N = self.np_ + (2 if self.distilled else 1)
        self.T = self.B * self.N
        self.E = cfg.moe_experts
        self.k = cfg.moe_top_k
        self.Hd = int(self.D * cfg.mlp_ratio)
        self.Hm = int(self.D * cfg.moe_mlp_ratio)
        self.R = self.T * self.k
        self.depth = cfg.depth
        assert self.E % self.ep_world == 0, "experts must divide evenly over the EP ranks"
        self.E_loc = self.E // self.ep_world
        self.ep_chunks = int(ep_chunks) if (self.ep_world > 1 and int(ep_chunks) > 1) else 1
        self.ep_native = None
        if ep_native and self.ep_world > 1:
            assert not ep_capacity, "ep_native carries the exact exchange only (the fixed-capacity form is one equal-split all-to-all)"
            if share is not None and getattr(share, "ep_native", None) is not None:
                self.ep_native = share.ep_native                   # one communicator per expert-parallel group and process
            else:
                from .ep_native import NativeExchange
                self.ep_native = NativeExchange(self.ep_rank, self.ep_world, group=ep_group, device=device)
        assert self.E_loc % self.ep_chunks == 0, "ep_chunks must divide the experts per rank"
        is_exp = lambda n: ".mlp.experts." in n                                  # noqa: E731
        lo, hi = self.ep_rank * self.E_loc, (self.ep_rank + 1) * self.E_loc
        if share is not None:
            self.params = share.params
        else:
            if self.ep_world > 1:
                names = [n for n in params if not is_exp(n)] + [n for n in params if is_exp(n)]     # experts last
            else:
                # replicated experts: everything is all-reduced, so order the flat buffer by WHEN a gradient is
                # final in backward() - blocks from the top down, then the embeddings: after
                # backward_blocks(.., b) the prefix flat_grads[:grad_prefix(b)] is final and can be all-reduced
                # while the blocks below still run
                names = sorted(params, key=lambda n: -self._block_of(n))
            cut = self.ep_world > 1 and not experts_are_local
            self.params = {n: (params[n][lo:hi] if (is_exp(n) and cut) else params[n])
                           .to(self.dev, torch.float32).contiguous() for n in names}
            for n, p in self.params.items():
                if is_exp(n):
                    assert p.shape[0] == self.E_loc, f"{n}: {p.shape[0]} experts on this rank, expected {self.E_loc}"
        self.n_dense = sum(p.numel() for n, p in self.params.items() if not is_exp(n))
        self.n_upper = self.grad_prefix(self.split_block)
        # one flat fp32 gradient buffer (views per parameter): zeroing is one memset and the data-parallel
        # sync is one RCCL all-reduce (xGMI is point-to-point: few large collectives)
        total = sum(p.numel() for p in self.params.values())
        self.flat_grads = torch.zeros(total, dtype=torch.float32, device=self.dev)
        self.grads, o = {}, 0
        for n, p in self.params.items():
            self.grads[n] = self.flat_grads[o:o + p.numel()].view_as(p)
            o += p.numel()
        dense_only = bool(getattr(cfg, "dense_only", False))
        self.is_moe = [(i % 2 == 1) and not dense_only for i in range(self.depth)]
        self.wg_stream = torch.cuda.Stream(device=self.dev) if (wgrad_stream and self.ep_world == 1) else None
        self._readers, self._ev_pool, self._ev_i = {}, [], 0
        self._alloc()
        if share is not None:
            self.wc, self.wt, self.wgate_c, self.cast_plan = share.wc, share.wt, share.wgate_c, None
        else:
            self.prepare_weights()

    @property
    def split_block(self):
        """first block of the 'upper half' (its gradients occupy flat_grads[:n_upper])"""
        return self.cfg.depth // 2

    @property
    def stem_blocks(self):
        """number of leading blocks before the first MoE block: together with the patch embedding they see neither the
        task id nor the gate, so every task pass of a step computes the same values there (MultiTaskStep share_stem)"""
        return next((i for i in range(self.depth) if self.is_moe[i]), self.depth)

    @staticmethod
    def _block_of(name: str) -> int:
        return int(name.split(".")[1]) if name.startswith("blocks.") else -1

    def grad_prefix(self, block: int) -> int:
        """number of leading elements of flat_grads that belong to blocks >= `block` (0 under expert parallelism,
        where the buffer is ordered dense-first instead)"""
        if self.ep_world > 1:
            return 0
        return sum(p.numel() for n, p in self.params.items() if self._block_of(n) >= block)

    # ------------------------------------------------------------------ buffers
    def _e(self, *shape, dtype=None):
        return torch.empty(*shape, dtype=dtype or self.dt, device=self.dev)

    def _alloc(self):
        T, D, R = self.T, self.D, self.R
        f32 = torch.float32
        self.act = []
        shared = {}                                            # checkpoint mode: one buffer per (block kind, name)

        keep = ("x2", "y") if self.ep_world > 1 else ("x2",)     # expert parallel: the returned expert outputs stay per block

        def buf(a, key, *shape, dtype=None):
            if self.checkpoint and key not in keep:
                k_ = (a["_moe"], key)
                if k_ not in shared:
                    shared[k_] = self._e(*shape, dtype=dtype)
                a[key] = shared[k_]
            else:
                a[key] = self._e(*shape, dtype=dtype)

        for i in range(self.depth):
            a = {"_moe": bool(self.is_moe[i])}
            a["x_in"] = None                                   # alias of previous block's output
            buf(a, "mean1", T, dtype=f32); buf(a, "rstd1", T, dtype=f32)
            buf(a, "h1", T, D)
            buf(a, "qkv", T, 3 * D)
            buf(a, "o", T, D)
            buf(a, "lse", self.B, self.heads, self.N, dtype=f32)
            buf(a, "x1", T, D, dtype=f32)
            buf(a, "mean2", T, dtype=f32); buf(a, "rstd2", T, dtype=f32)
            buf(a, "h2", T, D)
            if self.is_moe[i]:
                buf(a, "hid_pre", R, self.Hm)
                buf(a, "hid", R, self.Hm)
                buf(a, "y", R, D)
            else:
                buf(a, "pre", T, self.Hd)
                buf(a, "u", T, self.Hd)
            buf(a, "x2", T, D, dtype=f32)
            self.act.append(a)
        Kp = self.cfg.in_chans * self.P * self.P
        self.rows = self._e(self.B * self.np_, Kp)
        self.patch = self._e(self.B * self.np_, D, dtype=f32)
        self.x0 = self._e(T, D, dtype=f32)
        # backward scratch (reused by every block)
        Hmax = max(self.Hd, self.Hm)
        self.s_dxa = self._e(T, D, dtype=f32)
        self.s_dxb = self._e(T, D, dtype=f32)
        self.s_dx_t = self._e(T, D)
        self._plan_wgrad_batch()
        # batched weight gradients: the copy the norm2 backward emits (proj's dC) gets a buffer of its own, because the block-entry
        # copy in s_dx_t (fc2's dC) is read again by the block's one weight-gradient launch
        self.s_dx_tb = self._e(T, D) if self.wgrad_batched else None
        self.s_dpre = self._e(max(T * self.Hd, R * self.Hm))
        self.s_dh = self._e(T, D)
        self.s_dh32 = self._e(T, D, dtype=f32)
        self.s_do = self._e(T, D)
        self.s_dqkv = self._e(T, 3 * D)
        self.s_dy = self._e(R, D) if self.ep_world > 1 else None       # local experts read score * d x straight from d x
        self.s_dxe = self._e(R, D)
        self.s_dscore = self._e(T, self.k, dtype=f32)
        self.s_dpatch = self._e(self.B * self.np_, D)
        self.ones_k = torch.ones(T, self.k, dtype=f32, device=self.dev)
        # shared workspaces
        wg = 0
        shapes = [(T, self.Hd, D, 1), (T, D, self.Hd, 1), (T, 3 * D, D, 1), (T, D, D, 1),
                  (R, self.Hm, D, self.E), (R, D, self.Hm, self.E), (self.B * self.np_, D, Kp, 1), (T, D, self.E, 1)]
        if self.ep_capacity:                                   # the padded exchange contracts over the capacity bound
            W = self.ep_world
            self.ep_cap = (-(-int(self.ep_capacity * R + W - 1) // W) + 7) // 8 * 8        # rows per (source, destination) pair
            shapes += [(W * self.ep_cap, self.Hm, D, self.E_loc), (W * self.ep_cap, D, self.Hm, self.E_loc)]
        for (M, N, K, G) in shapes:
            wg = max(wg, ops.wgrad_ws_elems(M, N, K, G, grouped=G > 1, dtype=self.dt))
        # weight-gradient slab reductions ride in front of the NEXT weight-gradient launch of the pass (ops.WgradQueue: two
        # slab workspaces used in turn); with a wgrad side stream every call reduces for itself (its launches are not in
        # one stream order with flush())
        self.wq = ops.WgradQueue(wg, self.dev) if self.wg_stream is None else None
        self.ws_wgrad = self._e(wg, dtype=f32) if self.wq is None else None
        # the batched launches' slabs: two buffers of their own, used in turn (a batch's reductions are pending until the next
        # weight-gradient launch of the pass; the queue's buffers stay as large as the largest single call needs)
        wgm = max(ops.wgrad_multi_ws_elems(b, T, self.dt) for b in self._wgrad_batch_shapes().values()) if self.wgrad_batched else 0
        self.ws_wgrad_multi = [self._e(wgm, dtype=f32) for _ in range(2)] if self.wgrad_batched else None
        self._wgm_i = 0
        cs = max(int(ops.lib().m3_colsum_ws_elems(T, 3 * D, 1)), int(ops.lib().m3_colsum_ws_elems(T, self.Hd, 1)),
                 int(ops.lib().m3_colsum_ws_elems(R, max(self.Hm, D), self.E)))
        self.ws_colsum = self._e(cs, dtype=f32)
        # LayerNorm parameter-gradient partials: one slot per LayerNorm (2 * block + {0: norm1, 1: norm2}), reduced by ONE
        # launch per backward_blocks() call instead of one 24-workgroup launch behind every LayerNorm backward
        self.ln_nblk = int(ops.lib().m3_ln_bwd_blocks(T, D))
        self.ws_ln = self._e(2 * self.depth, 2, self.ln_nblk, D, dtype=f32)
        self.ln_table = ops.LnGradTable([(self.grads[f"blocks.{i}.{n}.weight"], self.grads[f"blocks.{i}.{n}.bias"])
                                         for i in range(self.depth) for n in ("norm1", "norm2")], self.dev)
        need_dq = int(ops.lib().m3_attention_bwd_ws_elems(self.B, self.N, self.heads, self.dh))
        self.ws_dq = self._e(need_dq, dtype=f32) if need_dq else None
        self.ws_gate_dw = self._e(ops.lib().m3_gate_dw_blocks(T) * self.cfg_d_gate() * self.E, dtype=f32)
        # gate backward through the MFMA GEMMs when E rows are 16-byte multiples
        es = 2 if self.dt in (torch.float16, torch.bfloat16) else 4
        self.gate_via_gemm = (self.E * es) % 16 == 0
        # ... and the gate's share of d h2 folded into the gather-sum of the routed rows' gradients (m3_combine_gate_bwd)
        # when w_gate^T fits its LDS image
        self.fused_gate_dx = self.E * (D + 4) * 4 <= 64 * 1024
        # task-conditioned gate (custom_moe_layer.py:161-181): one shared w_gate [D + gtsd, E] per MoE block
        self.task_cond = self.cfg.gate_task_specific_dim >= 0 and not self.cfg.multi_gate
        self.s_dl_t = self._e(T, self.E)
        self.s_dl = self._e(T, self.E, dtype=f32)
        self.cv_acc = torch.zeros(1, dtype=f32, device=self.dev)
        # routing statistics (opt-in): one record per MoE block + the partials workspace of m3_moe_stats
        self.stats_rec = self.ws_stats = None
        self.stats_row = {i: j for j, i in enumerate(i for i in range(self.depth) if self.is_moe[i])}
        if self.moe_stats_on and self.stats_row:
            self.stats_rec = torch.zeros(len(self.stats_row), _ms.record_words(self.E), dtype=torch.int32, device=self.dev)
            self.ws_stats = self._e(ops.moe_stats_ws_elems(T, self.E), dtype=f32)
        if self.ep_world > 1:
            self._alloc_ep()

    def cfg_d_gate(self):
        g = self.cfg.gate_task_specific_dim
        return self.D if g < 0 else self.D + g

    # ------------------------------------------------------------- weight copies
    def _linear_names(self):
        names = ["patch_embed.proj"]
        for i in range(self.depth):
            b = f"blocks.{i}."
            names += [b + "attn.qkv", b + "attn.proj"]
            if self.is_moe[i]:
                names += [b + "mlp.experts.htoh4", b + "mlp.experts.h4toh"]
            else:
                names += [b + "mlp.fc1", b + "mlp.fc2"]
        return names

    def prepare_weights(self):
        """Refresh the activation-dtype operand copies W [.., N, K] and W^T [.., K, N] of every
        Linear / FMoELinear weight (and the w_gate copies) from the fp32 masters: one batched launch
        per optimizer step."""
        if not hasattr(self, "wc"):
            self.wc, self.wt, self.wgate_c = {}, {}, {}
            jobs = []
            for n in self._linear_names():
                w = self.params[n + ".weight"]
                w2 = w.reshape(w.shape[0], -1) if n == "patch_embed.proj" else w
                self.wc[n] = w2 if self.dt == torch.float32 else torch.empty_like(w2, dtype=self.dt)
                if n != "patch_embed.proj":
                    self.wt[n] = torch.empty(*w2.shape[:-2], w2.shape[-1], w2.shape[-2], dtype=self.dt, device=self.dev)
                plain = None if self.dt == torch.float32 else self.wc[n]
                if plain is not None or n in self.wt:
                    jobs.append((w2, plain, self.wt.get(n)))          # both copies from one read of the master
            if self.dt != torch.float32:
                for n, p in self.params.items():
                    if n.endswith("w_gate"):
                        self.wgate_c[n] = torch.empty_like(p, dtype=self.dt)
                        jobs.append((p, self.wgate_c[n], None))
            self.cast_plan = ops.CastPlan(jobs, self.dt) if jobs else None
        if self.cast_plan is not None:
            self.cast_plan.run()

    def zero_grad(self):
        self.flat_grads.zero_()
        if self.wq is not None:
            # a step that aborted between a queued weight-gradient call and flush() leaves a slab-reduction descriptor behind
            # whose slabs were never (fully) written; it must not ride in front of THIS step's first launch
            self.wq.reset()

    # ------------------------------------------------------------- checkpoints
    def state_dict(self):
        """This rank's parameters as CPU tensors under the reference's key names (experts: the LOCAL slice under
        expert parallelism, as train_fastmoe's rank shards hold them - m3vit_amd/checkpoint.py)."""
        from collections import OrderedDict
        return OrderedDict((n, p.detach().cpu().clone()) for n, p in self.params.items())

    def load_state(self, state, strict: bool = True):
        """Copy a state_dict (local expert slices, e.g. from checkpoint.to_backbone_state) into the fp32 masters
        and refresh the operand copies.  Returns the keys of `state` that were not used."""
        missing = [n for n in self.params if n not in state]
        if strict and missing:
            raise KeyError(f"state_dict lacks {missing[:5]}{'...' if len(missing) > 5 else ''}")
        for n, p in self.params.items():
            if n in state:
                src = state[n]
                if tuple(src.shape) != tuple(p.shape):
                    raise ValueError(f"{n}: checkpoint shape {tuple(src.shape)} != parameter shape {tuple(p.shape)}")
                p.copy_(src.to(p.device, torch.float32))
        self.prepare_weights()
        return [k for k in state if k not in self.params]

    # ------------------------------------------------------------------ forward
    def _gate_weight(self, i, task_id):
        b = f"blocks.{i}.mlp.gate."
        if self.cfg.multi_gate:
            return b + f"{task_id}.w_gate"           # custom_moe_layer.py:213-214
        return b + "w_gate"

    def _task_feature(self, task_id):
        """tsf = gate_task_represent(one_hot(task_id)) (vision_transformer_moe.py:793-797; new_Mlp :263-281:
        fc1 -> GELU -> fc2 -> LayerNorm) and the per-block logit bias tsf @ w_gate[D:], which is what
        cat(inp, tsf.repeat(T, 1)) @ w_gate (custom_moe_layer.py:176-179) adds to every token's logits.
        A [num_tasks] -> [gtsd] vector MLP: kept as a torch autograd graph over leaf copies of its six
        parameters; backward() finishes it from the d(logit bias) the gate kernels produce."""
        import torch.nn.functional as F
        p, D = self.params, self.D
        names = [f"gate_task_represent.{n}" for n in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias",
                                                      "norm.weight", "norm.bias")]
        leaves = [p[n].detach().requires_grad_() for n in names]
        with torch.enable_grad():
            h = F.gelu(leaves[0][:, task_id] + leaves[1])          # fc1(one_hot(task)) = column task of fc1.weight
            h = F.linear(h, leaves[2], leaves[3])
            tsf = F.layer_norm(h, (h.shape[-1],), leaves[4], leaves[5], 1e-6)
        self._tsf = dict(names=names, leaves=leaves, tsf=tsf)
        tv = tsf.detach()
        return {i: tv @ p[self._gate_weight(i, task_id)][D:] for i in range(self.depth) if self.is_moe[i]}

    def _task_feature_block_bwd(self, a, dl, st):
        """One MoE block's share of the task-conditioned gate backward, written straight after the block's d logits
        exist: w_gate[D:] += outer(tsf, colsum(d logits)) and d tsf += w_gate[D:] @ colsum(d logits).  It must be part of
        backward_blocks(): a data-parallel step all-reduces a block's gradient slice as soon as backward_blocks() has
        passed the block (step.py), so nothing may be added to it later."""
        p, gr, D = self.params, self.grads, self.D
        tv = self._tsf["tsf"].detach()
        dlb = ops.colsum(dl, torch.empty(self.E, device=self.dev), ws=self.ws_colsum)
        gr[a["wname"]][D:].addr_(tv, dlb)
        if st.get("d_tsf") is None:
            st["d_tsf"] = torch.zeros_like(tv)
        st["d_tsf"] += p[a["wname"]][D:] @ dlb

    def _task_feature_bwd(self, d_tsf):
        """d tsf -> the gate_task_represent parameters (block -1: the last gradient slice)."""
        t = self._tsf
        if d_tsf is not None:
            for n, g in zip(t["names"], torch.autograd.grad(t["tsf"], t["leaves"], d_tsf)):
                self.grads[n] += g
        self._tsf = None

    # The expert FFN of MoE block i - the ONE place its launches are stated.  Slot m of M (expert-major; `offsets` / `tiles`:
    # the group offsets and tile prefix) stands for row idx[m] // div of x / d y and row idx[m] of y / d x: local experts pass
    # (row_of_slot, k), the expert-parallel exchanges (engine_ep.py) their regroup index with div 1.  es: the experts the
    # GEMMs run on (the chunked exchange: one chunk of the local experts).
    def _ffn_fwd(self, i, x, hid_pre, hid, y, M, idx, div, offsets, tiles, es=None):
        """grouped FC1 (+bias+GELU, rows of x gathered through idx) -> hid_pre, hid; grouped FC2 (+bias, rows scattered
        through idx) -> y.  y None: FC1 only (the checkpoint recompute under expert parallelism)."""
        fc1, fc2, p = f"blocks.{i}.mlp.experts.htoh4", f"blocks.{i}.mlp.experts.h4toh", self.params
        ops.gemm_nt(x, _cut(self.wc[fc1], es), hid, M=M, bias=_cut(p[fc1 + ".bias"], es), act=M3_ACT_GELU, pre_out=hid_pre,
                    a_row_idx=idx, a_row_div=div, group_offsets=offsets, tile_starts=tiles)
        if y is not None:
            ops.gemm_nt(hid, _cut(self.wc[fc2], es), y, M=M, bias=_cut(p[fc2 + ".bias"], es), c_row_idx=idx,
                        group_offsets=offsets, tile_starts=tiles)

    def _ffn_bwd(self, i, dy, x, hid_pre, hid, dhp, dx, M, idx, div, offsets, tiles, es=None, score=None,
                 dgrad=True, wgrad=True):
        """mirror of _ffn_fwd: FC2 weight gradient, FC2 input gradient (d y -> dhp), FC1 weight gradient, FC1 input gradient
        (dhp -> dx, rows scattered through idx), in this order.  score (local experts): slot m's row of d y is score[idx[m]]
        times the row read - the combine's backward folded in (see backward_blocks).  dgrad / wgrad False leave that half out
        (the chunked exchange: input gradients per chunk, weight gradients once over all local experts, es not applied).
        The reads= tags and _before_write order the weight-gradient side stream (no-ops without one)."""
        fc1, fc2 = f"blocks.{i}.mlp.experts.htoh4", f"blocks.{i}.mlp.experts.h4toh"
        assert es is None or not wgrad
        if wgrad:
            self._wgrad(dy, hid, fc2 + ".weight", M=M, c_row_idx=idx, c_row_div=div, c_row_scale=score,
                        group_offsets=offsets, bias=fc2 + ".bias", reads=("dx_t",))
        if dgrad:
            self._before_write("dpre")
            ops.gemm_nt(dy, _cut(self.wt[fc2], es), dhp, M=M, gelu_grad_pre=hid_pre, a_row_idx=idx, a_row_div=div,
                        row_scale=score, row_scale_idx=idx if score is not None else None, group_offsets=offsets,
                        tile_starts=tiles)
        if wgrad:
            self._wgrad(dhp, x, fc1 + ".weight", M=M, a_row_idx=idx, a_row_div=div, group_offsets=offsets,
                        bias=fc1 + ".bias", reads=("dpre",))
        if dgrad:
            ops.gemm_nt(dhp, _cut(self.wt[fc1], es), dx, M=M, c_row_idx=idx, group_offsets=offsets, tile_starts=tiles)

    def _block_forward(self, i, x, loss_acc):
        """block i on residual stream x -> its output buffer (vision_transformer_moe.py:438-562: pre-LN attention +
        MLP / MoE branch).  Called by forward() and, in checkpoint mode, again by backward_blocks() right before the
        block's backward (loss_acc None there: the balance loss was already counted)."""
        task_id, tsf_bias, noises, path_scales = self._fwd_ctx
        P_, p = self.P, self.params
        B, T, D = self.B, self.T, self.D
        N = self.N
        a = self.act[i]
        b = f"blocks.{i}."
        a["x_in"] = x
        ops.layernorm_fwd(x, p[b + "norm1.weight"], p[b + "norm1.bias"], a["h1"], a["mean1"], a["rstd1"])
        ops.gemm_nt(a["h1"], self.wc[b + "attn.qkv"], a["qkv"], bias=p[b + "attn.qkv.bias"])
        ops.attention_fwd(a["qkv"], B, self.N, self.heads, self.dh, a["o"], a["lse"])
        ps = None if path_scales is None else path_scales.get(i)
        a["ps"] = ps
        sa, sm = (None, None) if ps is None else ps
        ops.gemm_nt(a["o"], self.wc[b + "attn.proj"], a["x1"], bias=p[b + "attn.proj.bias"], residual=x,
                    row_scale=sa, row_scale_div=N)
        ops.layernorm_fwd(a["x1"], p[b + "norm2.weight"], p[b + "norm2.bias"], a["h2"], a["mean2"], a["rstd2"])
        if not self.is_moe[i]:
            ops.gemm_nt(a["h2"], self.wc[b + "mlp.fc1"], a["u"], bias=p[b + "mlp.fc1.bias"], act=M3_ACT_GELU,
                        pre_out=a["pre"])
            ops.gemm_nt(a["u"], self.wc[b + "mlp.fc2"], a["x2"], bias=p[b + "mlp.fc2.bias"], residual=a["x1"],
                        row_scale=sm, row_scale_div=N)
        else:
            wname = self._gate_weight(i, task_id)
            a["wname"] = wname
            wg = p[wname]
            wg_tok = wg if wg.shape[0] == D else wg[:D]
            noise = None if noises is None else noises.get(i)
            std = (self.cfg.vmoe_noisy_std / self.E) if noise is not None else 0.0
            # gate + balance loss (importance, load, cv^2 and its gradient) + dispatch metadata: three launches (the routing
            # histogram comes out of the gate kernel, its scan rides in the balance launch)
            g = ops.gate_fwd(a["h2"], wg_tok, self.k, logit_bias=None if tsf_bias is None else tsf_bias[i],
                             noise=noise, noise_std=std, dense=True, loss_acc=loss_acc, route=self.ep_world == 1)
            a["gate"] = g
            if self.ep_world > 1:
                self._experts_fwd_ep(i, a, g, recompute=loss_acc is None)
            else:
                r = g["route"] if g["route"] is not None else ops.route_build(g["idx32"], self.E)     # (None when 16 % k != 0)
                a["route"] = r
                self._ffn_fwd(i, a["h2"], a["hid_pre"], a["hid"], a["y"], self.R, r.row_of_slot, self.k, r.offsets, r.tile_starts)
            if sm is not None:                          # out = x1 + scale[sample] * sum_j score_j y_j
                a["sm_tok"] = sm.view(B, 1).expand(B, N).reshape(T, 1).contiguous()
                a["score_s"] = g["score"] * a["sm_tok"]
            ops.combine_fwd(a["y"], a["score_s"] if sm is not None else g["score"], a["x1"], a["x2"])
            if self.stats_rec is not None and loss_acc is not None:      # (not in the checkpoint recompute: counted once)
                # the UNSCALED score: m is the layer output before DropPath, a dropped sample still reports its experts
                ops.moe_stats(g["score"], g["clean"], g["gates"], a["h2"], a["y"],
                              g["load_prob"] if g["load_prob"] is not None else g["load"],
                              self.stats_rec[self.stats_row[i]], ws=self.ws_stats)
        return a["x2"]

    def moe_stats(self):
        """The routing statistics of the last forward: ({block index: the block's dict}, the backbone dict), in the
        reference's key names and Python types (m3vit_amd.moe_stats).  ONE device-to-host copy of the records, made here
        and only here; None when the engine was built without moe_stats or has no MoE block."""
        if self.stats_rec is None:
            return None
        static = _ms.static_fields(self.D, self.cfg.mlp_ratio, self.cfg.moe_mlp_ratio, self.k)
        rows = _ms.read_records(self.stats_rec, self.E, static)
        blocks = {i: rows[j] for i, j in self.stats_row.items()}
        return blocks, _ms.aggregate([blocks[i] for i in sorted(blocks)], self.B * max(self.N - 1, 0))

    def forward(self, images: torch.Tensor, task_id: Optional[int], tsf_bias=None, noises=None, path_scales=None,
                stem_of: "BackboneEngine" = None):
        """Returns (tokens fp32 [B,N,D], total_cv_loss).  noises: {block: [T,E]} caller-supplied N(0,1).
        Task-conditioned configs compute the per-block logit bias tsf @ w_gate[D:] here (tsf_bias overrides
        it with a caller-supplied {block: [E]} and then no gradient flows to the task embedding).
        path_scales: {block: (attn [B], mlp [B])} fp32 per-sample DropPath factors of the block's two residual
        branches (stochastic depth, vision_transformer_moe.py:167-185: floor(keep + U) / keep, drawn by the caller -
        pretrain/configs/deit_moe_small.yaml:51 trains with drop_path > 0); the factor rides on the epilogue of the
        GEMM that closes the branch (proj, fc2) or on the combine scores (MoE), and on the gradient entering the
        branch in backward.
        stem_of: an engine (this one or another of the same step) whose forward_stem() already holds the patch embedding
        and the blocks below the first MoE block for THESE images; this pass starts at the first MoE block from that
        output and its backward stops there (backward_blocks(depth - 1, stem_blocks); the caller adds the passes'
        d x and runs the stem's backward once - MultiTaskStep)."""
        x = self.forward_begin(images, task_id, tsf_bias=tsf_bias, noises=noises, path_scales=path_scales, stem_of=stem_of)
        for i in range(self.stem_blocks if stem_of is not None else 0, self.depth):
            x = self._block_forward(i, x, self.cv_acc)
        return self.forward_end(x)

    def forward_stem(self, images: torch.Tensor):
        """patch embedding, cls / pos and the blocks below the first MoE block (task-independent: no gate, no task id;
        the reference's DropPath schedule gives block 0 rate 0, vision_transformer_moe.py:761).  Returns their output."""
        self._fwd_ctx = (None, None, None, None)
        x = self._embed(images)
        for i in range(self.stem_blocks):
            x = self._block_forward(i, x, None)
        return x

    def _embed(self, images):
        ops.im2row(images, self.P, self.rows)
        ops.gemm_nt(self.rows, self.wc["patch_embed.proj"], self.patch, bias=self.params["patch_embed.proj.bias"])
        p = self.params
        if self.distilled:
            ops.assemble_tokens2(self.patch, p["cls_token"], p["dist_token"], p["pos_embed"], self.B, self.np_, self.D, self.x0)
        else:
            ops.assemble_tokens(self.patch, p["cls_token"], p["pos_embed"], self.B, self.np_, self.D, self.x0)
        return self.x0

    # The forward in resumable pieces (patch embedding / one block at a time / result), so that a step runner can
    # interleave the blocks of several task passes on the host (expert parallelism: while one pass waits for its
    # exchange's split sizes, the other pass's queued kernels keep the GPU busy).
    def forward_begin(self, images: torch.Tensor, task_id: Optional[int], tsf_bias=None, noises=None, path_scales=None,
                      stem_of: "BackboneEngine" = None):
        self._tsf = None
        if self.task_cond and tsf_bias is None and task_id is not None:
            tsf_bias = self._task_feature(task_id)
        self.cv_acc.zero_()
        self.task_id = task_id
        self._fwd_ctx = (task_id, tsf_bias, noises, path_scales)
        if stem_of is None:
            return self._embed(images)
        s = self.stem_blocks
        assert path_scales is None or all(path_scales.get(i) is None for i in range(s)), "a shared stem takes no DropPath draw"
        return stem_of.act[s - 1]["x2"] if s > 0 else stem_of.x0

    def forward_end(self, x):
        # total cv_loss = sum over MoE blocks of cv^2(importance) + cv^2(load)  (vision_transformer_moe.py:453-459,540)
        return x.view(self.B, self.N, self.D), self.cv_acc[0].clone()

    def sync_grads(self, group=None, world: int = 1):
        """Data-parallel gradient sync (mean): everything when experts are replicated, only the non-expert
        slice of the flat buffer under expert parallelism (expert params have dp_comm == "none",
        custom_moe_layer.py:159)."""
        if world <= 1:
            return
        import torch.distributed as dist
        buf = self.flat_grads[: self.n_dense] if self.ep_world > 1 else self.flat_grads
        dist.all_reduce(buf, group=group)
        buf.div_(world)

    # ----------------------------------------------------------------- backward
    def _fork(self, reads, fn):
        """Run fn() - weight-gradient launches - on the wgrad stream, ordered after everything queued so far
        on the current stream; `reads` names the scratch buffers it reads, which the main chain may only
        overwrite after _before_write(name)."""
        if self.wg_stream is None:
            fn()
            return
        ready = self._event()
        ready.record(torch.cuda.current_stream())
        self.wg_stream.wait_event(ready)
        with torch.cuda.stream(self.wg_stream):
            fn()
            done = self._event()
            done.record(self.wg_stream)
        for r in reads:
            self._readers[r] = done

    def _event(self):
        # events come from a pool that lives as long as the engine (none is destroyed while a hipGraph
        # capture that recorded it is open) and is walked in the same order every backward()
        if self._ev_i == len(self._ev_pool):
            self._ev_pool.append(torch.cuda.Event())
        self._ev_i += 1
        return self._ev_pool[self._ev_i - 1]

    def _before_write(self, *names):
        for n in names:
            ev = self._readers.pop(n, None)
            if ev is not None:
                torch.cuda.current_stream().wait_event(ev)

    def _join_wgrad(self):
        if self.wg_stream is not None:
            torch.cuda.current_stream().wait_stream(self.wg_stream)
            self._readers.clear()

    def _wgrad_batch_shapes(self):
        """(N, K, has bias) of the dense-row weight gradients of a dense / an MoE block, in the order the backward produces them"""
        D, Hd = self.D, self.Hd
        attn = [(D, D, True), (3 * D, D, True)]
        return {"dense": [(D, Hd, True), (Hd, D, True)] + attn, "moe": attn}

    def _plan_wgrad_batch(self):
        """Batched weight gradients: the dense-row weight gradients of a block's backward - fc2, fc1, proj, qkv of a dense block,
        proj, qkv of an MoE block - go out as ONE launch (ops.wgrad_multi) behind the block's attention backward instead of
        one launch each where their dC appears; the experts' and the router's stay where they are.  M3_WGRAD_BATCH=0 / 1
        forces the per-weight / the batched path (default: batched).  The per-weight path stays where the batch cannot
        run: with a weight-gradient side stream (its launches are ordered by events per operand), under activation
        checkpointing and expert parallelism (not wired), and where the library refuses the batch (fp32, the ViT-Base
        widths: ops.wgrad_multi_plan).  self.wgrad_batched says which path runs, self.wgrad_batch_why why not."""
        why = None
        if os.environ.get("M3_WGRAD_BATCH", "1") == "0":
            why = "M3_WGRAD_BATCH=0"
        elif self.wg_stream is not None:
            why = "weight-gradient side stream"
        elif self.checkpoint:
            why = "activation checkpointing"
        elif self.ep_world > 1:
            why = "expert parallelism"
        elif not all(ops.wgrad_multi_plan(b, self.T, self.dt).allowed for b in self._wgrad_batch_shapes().values()):
            why = "refused by m3_wgrad_multi_plan"
        self.wgrad_batched, self.wgrad_batch_why = why is None, why
        self.wgrad_multi_calls = 0

    def _wgrad_or_batch(self, batch, dC, A, name, bias, reads):
        """a dense-row weight gradient: launched now (batch is None), or put on the block's list for _wgrad_batch"""
        if batch is None:
            self._wgrad(dC, A, name, bias=bias, reads=reads)
        else:
            batch.append((dC, A, self.grads[name], self.grads[bias], 1))

    def _wgrad_batch(self, batch):
        ops.wgrad_multi(batch, self.T, ws=self.ws_wgrad_multi[self._wgm_i], queue=self.wq)
        self._wgm_i ^= 1
        self.wgrad_multi_calls += 1

    def _wgrad(self, dC, A, name, M=None, bias=None, reads=(), **kw):
        """weight grad (+ fused bias grad) accumulated into self.grads"""
        self._fork(reads, lambda: ops.wgrad_tn(dC, A, self.grads[name], M=M, beta=1, ws=self.ws_wgrad, queue=self.wq,
                                               db=self.grads[bias] if bias is not None else None, **kw))

    def backward(self, d_tokens: torch.Tensor, cv_weight=0.0):
        """Accumulates parameter gradients of  <tokens, d_tokens> + cv_weight * total_cv_loss
        into self.grads (beta = 1: the joint multi-task backward, train/train_utils.py:437-457).
        cv_weight: a python float, or a 1-element fp32 device tensor (the upstream gradient of cv_loss handed over by
        torch.autograd - read by the gate's backward kernel, so a captured backward follows its value)."""
        self.backward_begin(d_tokens, cv_weight)
        self.backward_blocks(self.depth - 1, 0)
        return self.backward_end()

    # The backward in three resumable pieces, so that a data-parallel trainer can all-reduce the gradients
    # of the upper blocks (complete after backward_blocks(depth-1, s)) while the lower blocks still run.
    def backward_begin(self, d_tokens: torch.Tensor, cv_weight=0.0):
        self._ev_i = 0
        dx = self.s_dxa
        dx.copy_(d_tokens.reshape(self.T, self.D))
        self._bw = dict(dx=dx, other=self.s_dxb, have_dx_t=False, cv_weight=cv_weight, d_tsf=None)

    def backward_blocks(self, hi: int, lo: int):
        """blocks hi, hi-1, ..., lo (inclusive); after it the gradients of every parameter of those blocks
        are final on the wgrad stream (backward_sync_wgrad) / current stream."""
        p, gr = self.params, self.grads
        B, T, D, R, k = self.B, self.T, self.D, self.R, self.k
        st = self._bw
        dx, other, have_dx_t, cv_weight = st["dx"], st["other"], st["have_dx_t"], st["cv_weight"]
        for i in range(hi, lo - 1, -1):
            a = self.act[i]
            b = f"blocks.{i}."
            if self.checkpoint:                             # the shared activation buffers hold another block's values
                self._block_forward(i, a["x_in"], None)
            sa, sm = (None, None) if a.get("ps") is None else a["ps"]
            # batched weight gradients: the block's dense-row calls are collected and launched once, behind the attention
            # backward; until then s_dx_t keeps fc2's dC, so the norm2 backward's copy (proj's dC) goes to s_dx_tb
            batch = [] if self.wgrad_batched else None
            dx_t1 = self.s_dx_tb if self.wgrad_batched else self.s_dx_t
            if not self.is_moe[i]:
                if sm is not None:                          # DropPath: the gradient entering the branch is scale * d x
                    self._before_write("dx_t")
                    ops.scale_rows_cast(dx, sm, self.N, self.s_dx_t)
                elif not have_dx_t:
                    self._before_write("dx_t")
                    ops.cast_f32(dx, self.s_dx_t)
                dpre = self.s_dpre[: T * self.Hd].view(T, self.Hd)
                self._wgrad_or_batch(batch, self.s_dx_t, a["u"], b + "mlp.fc2.weight", b + "mlp.fc2.bias", ("dx_t",))
                self._before_write("dpre")
                ops.gemm_nt(self.s_dx_t, self.wt[b + "mlp.fc2"], dpre, gelu_grad_pre=a["pre"])
                self._wgrad_or_batch(batch, dpre, a["h2"], b + "mlp.fc1.weight", b + "mlp.fc1.bias", ("dpre",))
                ops.gemm_nt(dpre, self.wt[b + "mlp.fc1"], self.s_dh)
                dh2 = self.s_dh
            else:
                g, r = a["gate"], a["route"]
                score = a["score_s"] if sm is not None else g["score"]
                if self.ep_world > 1:
                    self._before_write("dy")
                    ops.combine_bwd(dx, a["y"], score, self.s_dy, self.s_dscore)
                    if sm is not None:
                        self.s_dscore.mul_(a["sm_tok"])         # d score = scale * d(scale * score)
                    self._experts_bwd_ep(i, a)
                else:
                    # The combine's backward d y[t*k+j] = score[t,j] * d x[t] is a row scaling, and a row scaling commutes
                    # with the expert GEMMs behind it: FC2's input-gradient GEMM gathers its rows from d x (activation
                    # dtype copy, [T, D]) through row_of_slot / k and applies the score in its epilogue; FC2's weight
                    # gradient takes the same rows and multiplies by the score where they enter LDS.  The [T*k, D] copy
                    # d y is never written (one 2*R*D-byte store and two such reads less per MoE block); the combine
                    # backward only produces d score.
                    if not have_dx_t:
                        self._before_write("dx_t")
                        ops.cast_f32(dx, self.s_dx_t)
                    ops.combine_bwd(dx, a["y"], score, None, self.s_dscore)
                    if sm is not None:
                        self.s_dscore.mul_(a["sm_tok"])         # d score = scale * d(scale * score)
                    self._ffn_bwd(i, self.s_dx_t, a["h2"], a["hid_pre"], a["hid"], self.s_dpre[: R * self.Hm].view(R, self.Hm),
                                  self.s_dxe, R, r.row_of_slot, k, r.offsets, r.tile_starts, score=score)
                # gate: d score from the combine, d importance / d load from the cv loss
                cvw_dev = cv_weight if isinstance(cv_weight, torch.Tensor) else None
                bal = cvw_dev is not None or cv_weight != 0.0
                self._before_write("dl")
                dl = ops.gate_bwd_logits(g["noisy"], g["idx"], self.s_dscore, g["d_importance"] if bal else None, k,
                                         balance_scale=1.0 if cvw_dev is not None else cv_weight, balance_scale_dev=cvw_dev,
                                         idx_next=g["idx_next"],
                                         d_load_prob=g["d_load_prob"] if bal else None, clean=g["clean"],
                                         top_logits=g["top_logits"], noise_std=g["noise_std"], out=self.s_dl,
                                         out_act=self.s_dl_t if (self.gate_via_gemm and self.dt != torch.float32) else None)
                # token rows of w_gate ([:D]; the task-conditioned rows [D:]: _task_feature_block_bwd below)
                wg, dwg = p[a["wname"]][:D], gr[a["wname"]][:D]
                dh2_moe = self.s_dh32
                if self.gate_via_gemm:
                    # (a dedicated VALU kernel for d w_gate - m3_gate_bwd_params, 4 columns x E accumulators per thread - was
                    # measured in round 3: 24 us + 6 us partial reduce against 17.5 us for the padded TN GEMM whose reduce rides
                    # along: the GEMM stays)
                    # d w_gate += h2^T dl (TN GEMM) ; dh2 = sum_j dxe[t,j] + dl w_gate^T
                    dl_t = dl if self.dt == torch.float32 else self.s_dl_t      # (written by the gate's backward kernel itself)
                    self._fork(("dl",), lambda: ops.wgrad_tn(a["h2"], dl_t, dwg, beta=1, ws=self.ws_wgrad, queue=self.wq))
                    if self.fused_gate_dx:
                        # one pass over the [T, D] result, stored in the activation dtype like a dense block's d h2 (the sum
                        # itself is formed in fp32): the LayerNorm backward below reads half the bytes
                        ops.combine_gate_bwd(self.s_dxe, k, dl, wg, self.s_dh)
                        dh2_moe = self.s_dh
                    else:
                        ops.combine_fwd(self.s_dxe, self.ones_k, None, self.s_dh32)
                        wg_t = wg if self.dt == torch.float32 else self.wgate_c[a["wname"]][:D]
                        ops.gemm_nt(dl_t, wg_t, self.s_dh32, residual=self.s_dh32)
                else:
                    ops.combine_fwd(self.s_dxe, self.ones_k, None, self.s_dh32)       # dh2 = sum_j dxe[t,j]
                    ops.gate_bwd_params(a["h2"], wg, dl, d_w_gate=dwg, beta_dw=1, dx=self.s_dh32,
                                        beta_dx=1, part_dw=self.ws_gate_dw)
                if self._tsf is not None:
                    self._task_feature_block_bwd(a, dl, st)
                dh2 = dh2_moe
            self._before_write("dx_t")
            ops.layernorm_bwd(dh2, a["x1"], a["mean2"], a["rstd2"], p[b + "norm2.weight"], dx, other, None, None,
                              ws=self.ws_ln[2 * i + 1],
                              dx_act=dx_t1 if sa is None else None)           # also emits the activation-dtype copy
            dx, other = other, dx                                        # dx = d x1
            if sa is not None:
                ops.scale_rows_cast(dx, sa, self.N, dx_t1)               # DropPath of the attention branch
            self._wgrad_or_batch(batch, dx_t1, a["o"], b + "attn.proj.weight", b + "attn.proj.bias", ("dx_t",))
            ops.gemm_nt(dx_t1, self.wt[b + "attn.proj"], self.s_do)
            self._before_write("dqkv")
            ops.attention_bwd(a["qkv"], a["o"], self.s_do, a["lse"], B, self.N, self.heads, self.dh, self.s_dqkv,
                              dq_ws=self.ws_dq)
            self._wgrad_or_batch(batch, self.s_dqkv, a["h1"], b + "attn.qkv.weight", b + "attn.qkv.bias", ("dqkv",))
            if batch is not None:                                        # before the norm1 backward overwrites s_dx_t
                self._wgrad_batch(batch)
            ops.gemm_nt(self.s_dqkv, self.wt[b + "attn.qkv"], self.s_dh)
            # does the block below consume the activation-dtype copy of d x directly?  (a dense block without DropPath: fc2's
            # backward GEMMs; an MoE block with local experts: FC2's backward GEMMs, which apply the gate score themselves)
            nxt_dx_t = i > 0 and ((self.is_moe[i - 1] and self.ep_world == 1) or
                                  (not self.is_moe[i - 1] and self.act[i - 1].get("ps") is None))
            if nxt_dx_t:
                self._before_write("dx_t")
            ops.layernorm_bwd(self.s_dh, a["x_in"], a["mean1"], a["rstd1"], p[b + "norm1.weight"], dx, other, None, None,
                              ws=self.ws_ln[2 * i],
                              dx_act=self.s_dx_t if nxt_dx_t else None)
            dx, other = other, dx
            have_dx_t = nxt_dx_t
        # the last weight-gradient call's slabs (a data-parallel step all-reduces these blocks' slice next); on the stream
        # the weight-gradient launches went to
        if self.wq is not None:
            self._fork((), self.wq.flush)
        # norm weight / bias gradients of the blocks just done, all in one launch (their partial slots are contiguous)
        if hi >= lo:
            ops.layernorm_bwd_reduce(self.ws_ln, self.ln_nblk, self.D, self.ln_table, 2 * lo, 2 * (hi - lo + 1), beta=1)
        st.update(dx=dx, other=other, have_dx_t=have_dx_t)

    def backward_sync_wgrad(self):
        """make the current stream wait for the weight-gradient launches issued so far (no-op without a wgrad stream)"""
        self._join_wgrad()

    def accept_dx(self, others):
        """shared stem: add the other task passes' gradient at the stem's output to this pass's; the stem's backward
        then runs once on the sum (it is linear in d x)."""
        st = self._bw
        for o in others:
            ops.add_f32(st["dx"].view(-1), o._bw["dx"].view(-1))
        st["have_dx_t"] = False                       # the activation-dtype copy was this pass's d x alone

    def backward_end(self, stem: bool = True):
        """stem=False: a pass that started from another engine's stem - nothing below its first block is its own"""
        p, gr = self.params, self.grads
        B, D = self.B, self.D
        dx = self._bw["dx"]
        if stem:
            # patch embedding / cls / pos
            if self.distilled:
                ops.tokens_bwd2(dx, B, self.np_, D, self.s_dpatch, gr["pos_embed"].view(self.N, D), gr["cls_token"].view(D),
                                gr["dist_token"].view(D), beta=1)
            else:
                ops.tokens_bwd(dx, B, self.np_, D, self.s_dpatch, gr["pos_embed"].view(self.N, D), gr["cls_token"].view(D), beta=1)
            gw = gr["patch_embed.proj.weight"].view(D, -1)
            self._fork((), lambda: ops.wgrad_tn(self.s_dpatch, self.rows, gw, beta=1, ws=self.ws_wgrad, queue=self.wq,
                                                db=gr["patch_embed.proj.bias"]))
        if self.wq is not None:
            self._fork((), self.wq.flush)
        self._join_wgrad()
        if self._tsf is not None:
            self._task_feature_bwd(self._bw.get("d_tsf"))
        return dx
