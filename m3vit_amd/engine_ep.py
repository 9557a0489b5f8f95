"""Expert parallelism of the fused executor: the routed rows' exchange around BackboneEngine's expert FFN
(engine._ffn_fwd / _ffn_bwd) in its three variants - exact all-to-all-v, the same cut into chunks that overlap the
experts' GEMMs, and fixed capacity - forward and backward, with their buffers.

A mixin of BackboneEngine, not a member object: every buffer here is an attribute of the engine itself.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from . import ops


class ExpertParallelMixin:
    def _alloc_ep(self):
        D, R, W = self.D, self.R, self.ep_world
        moe = [i for i in range(self.depth) if self.is_moe[i]]
        # expert-parallel exchange plans: one regroup index per MoE block (kept for the backward; a rank can
        # receive at most what all ranks route) and the pinned landing buffer of the split sizes
        self.ep_regroup = {i: torch.empty(W * R, dtype=torch.int32, device=self.dev) for i in moe}
        self.ep_splits_host = torch.empty(2 * W, dtype=torch.int64, pin_memory=True)
        if self.ep_chunks > 1:
            # chunked exchange: rows are routed by a CHUNK-MAJOR key - (chunk of the local expert, destination rank,
            # expert inside the chunk) - so that what goes to every rank for one chunk of its experts is one
            # contiguous run of the send buffer, in destination order (one all_to_all_single per chunk)
            C, Ec = self.ep_chunks, self.E_loc // self.ep_chunks
            e = torch.arange(self.E)
            d_, rest = e // self.E_loc, e % self.E_loc
            self.ep_key = ((rest // Ec) * (W * Ec) + d_ * Ec + rest % Ec).to(torch.int32).to(self.dev)
            self.ep_regroup_c = {i: torch.empty(C, W * R, dtype=torch.int32, device=self.dev) for i in moe}
            self.ep_splits_host_c = torch.empty(C, 2 * W, dtype=torch.int64, pin_memory=True)
        if self.ep_capacity:
            self.ep_overflow = torch.zeros(1, dtype=torch.int32, device=self.dev)
            n = W * self.ep_cap
            # static buffers of the padded exchange, per MoE block (a captured step replays on fixed addresses)
            # (zeroed once: the rows of a pair's share that no routed row fills travel over the wire as they are - never read
            # back, unpad_idx does not select them, but they should not be whatever the allocator left there)
            z = lambda *shape: torch.zeros(*shape, dtype=self.dt, device=self.dev)                   # noqa: E731
            self.ep_fx = {i: dict(x_send=z(n, D), x_recv=z(n, D), hid_pre=z(n, self.Hm),
                                  hid=z(n, self.Hm), y_recv=z(n, D), y_back=z(n, D),
                                  recv_counts=torch.zeros(self.E, dtype=torch.int64, device=self.dev), plan=None)
                          for i in moe}
            self.ep_fx_bwd = dict(dy_send=z(n, D), dy_recv=z(n, D), dhp=z(n, self.Hm),
                                  dx_recv=z(n, D), dx_back=z(n, D))

    def _a2a(self, x, in_splits, out_splits):
        out = torch.empty((sum(out_splits),) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
        if self.ep_native is not None:
            self.ep_native.dispatch_async(out, x.contiguous(), out_splits, in_splits).wait()
            return out
        dist.all_to_all_single(out, x.contiguous(), output_split_sizes=out_splits, input_split_sizes=in_splits,
                               group=self.ep_group)
        return out

    def _a2a_async(self, out, x, out_splits, in_splits):
        if self.ep_native is not None:
            return self.ep_native.dispatch_async(out, x, out_splits, in_splits)
        return dist.all_to_all_single(out, x, output_split_sizes=out_splits, input_split_sizes=in_splits, group=self.ep_group,
                                      async_op=True)

    def _exchange_counts(self, send):
        if self.ep_native is not None:
            return self.ep_native.exchange_counts(send)
        recv = torch.empty_like(send)
        dist.all_to_all_single(recv, send, group=self.ep_group)
        return recv

    def _experts_fwd_ep(self, i, a, g, recompute=False):
        """EP forward of one MoE layer: ONE count exchange + ONE row exchange each way (m3vit_amd/ep.py has
        the same logic for the module API).  Rows are routed by GLOBAL expert id, so the expert-major send
        buffer is already grouped by destination rank; received rows are regrouped from (src, expert) to
        (expert, src) order for the local grouped GEMMs.
        recompute (checkpoint mode, called from backward_blocks): the gate has just been re-run on the same input, so the
        routing is the forward's; the plan, the received rows and the returned outputs a["y"] were kept - only FC1 of the
        local experts is run again (its hidden activations are what the backward needs), no collective."""
        if self.ep_fixed:
            return self._experts_fwd_ep_fixed(i, a, g)
        if self.ep_chunks > 1 and not recompute:
            return self._experts_fwd_ep_chunked(i, a, g)
        if recompute:
            ep = a["ep"]
            n = ep["n"]
            if n > 0:
                ep["hid_pre"], ep["hid"] = self._e(n, self.Hm), self._e(n, self.Hm)
                self._ffn_fwd(i, ep["x_recv"], ep["hid_pre"], ep["hid"], None, n, ep["rg"], 1, ep["offsets"], ep["tile_starts"])
            return
        r = ops.route_build(g["idx32"], self.E, want_counts64=True)
        a["route"] = r
        x_send = self._e(self.R, self.D)
        ops.gather_rows(a["h2"], r.row_of_slot, x_send, div=self.k)
        recv = self._exchange_counts(r.counts64)
        # the plan (regroup index, expert-major offsets, tile prefix) is built on the device; the host reads the
        # 2 W split sizes the a2a-v API needs and nothing else
        plan = ops.ep_plan(r.counts64, recv, self.ep_world, self.E_loc, self.ep_regroup[i], splits_host=self.ep_splits_host)
        n = plan.n_recv
        x_recv = self._a2a(x_send, plan.in_splits, plan.out_splits)
        ep = dict(plan=plan, n=n, rg=plan.regroup, offsets=plan.offsets, tile_starts=plan.tile_starts)
        y_recv = self._e(n, self.D)
        ep["x_recv"] = x_recv
        if n > 0:
            # the (src, expert) -> (expert, src) regroup is the A-row gather of FC1 and the C-row scatter of FC2:
            # expert-major slot i reads x_recv[rg[i]] and writes y_recv[rg[i]] - no regrouped copies
            ep["hid_pre"], ep["hid"] = self._e(n, self.Hm), self._e(n, self.Hm)
            self._ffn_fwd(i, x_recv, ep["hid_pre"], ep["hid"], y_recv, n, ep["rg"], 1, ep["offsets"], ep["tile_starts"])
        y_send = self._a2a(y_recv, plan.out_splits, plan.in_splits)
        ops.gather_rows(y_send, r.pos, a["y"])                       # back to token-major [T*k, D]
        if self.checkpoint:                                          # local hidden activations: recomputed in backward
            ep["hid_pre"] = ep["hid"] = None
        a["ep"] = ep

    def _experts_bwd_ep(self, i, a):
        """mirror of _experts_fwd_ep: self.s_dy (token-major d y) -> expert grads (local experts only) and
        self.s_dxe (token-major d of the routed input copies)."""
        if a["ep"].get("fixed"):
            return self._experts_bwd_ep_fixed(i, a)
        if a["ep"].get("chunked"):
            return self._experts_bwd_ep_chunked(i, a)
        r, ep = a["route"], a["ep"]
        plan, n = ep["plan"], ep["n"]
        dy_send = ops.gather_rows(self.s_dy, r.row_of_slot, self._e(self.R, self.D))
        dy_recv = self._a2a(dy_send, plan.in_splits, plan.out_splits)
        dx_recv = self._e(n, self.D)
        if n > 0:
            self._ffn_bwd(i, dy_recv, ep["x_recv"], ep["hid_pre"], ep["hid"], self._e(n, self.Hm), dx_recv,
                          n, ep["rg"], 1, ep["offsets"], ep["tile_starts"])
        dx_send = self._a2a(dx_recv, plan.out_splits, plan.in_splits)
        ops.gather_rows(dx_send, r.pos, self.s_dxe)

    # ------------------------------------------------------------------ exchange overlapped inside ONE pass
    def _experts_fwd_ep_chunked(self, i, a, g):
        """_experts_fwd_ep with every exchange cut into ep_chunks all-to-all-v's, chunk c = the rows for local experts
        [c E_loc / C, (c + 1) E_loc / C) of EVERY rank (custom_moe_layer.py:263-265): all chunks' row
        exchanges are queued on the collective library's stream at once; the grouped FC1 / FC2 of chunk c start when ITS rows
        have arrived - the later chunks are still in flight - and its outputs start their way home under the next chunk's GEMMs.
        Exposed per direction: one chunk's exchange instead of the whole.  The count exchange and the plans (C m3_ep_plan
        launches, ONE host read of the C * 2 W split sizes) are as before.  What the backward and a checkpoint recompute need
        is kept in the unchunked form - one received buffer (the chunks side by side), one regroup index, offsets and tile
        prefix over all local experts - so every row keeps its expert-major position and the results are bit-identical to the
        one-exchange path."""
        D, dev = self.D, self.dev
        C, W = self.ep_chunks, self.ep_world
        Ec = self.E_loc // C
        key = self.ep_key[g["idx32"].reshape(-1).long()].view(-1, self.k).contiguous()     # chunk-major routing keys
        r = ops.route_build(key, self.E, want_counts64=True)
        a["route"] = r
        x_send = self._e(self.R, D)
        ops.gather_rows(a["h2"], r.row_of_slot, x_send, div=self.k)
        send = r.counts64.view(C, W, Ec)
        snd_dm = send.permute(1, 0, 2).contiguous()                                         # destination-major for the count exchange
        rcv_dm = self._exchange_counts(snd_dm.view(-1)).view_as(snd_dm)
        recv = rcv_dm.permute(1, 0, 2).contiguous()                                         # [C][source][expert of the chunk]
        plans = ops.ep_plan_chunks(send.contiguous(), recv, W, Ec, self.ep_regroup_c[i], self.ep_splits_host_c)
        ns = [sum(pl.in_splits) for pl in plans]
        nr = [pl.n_recv for pl in plans]
        sb = [sum(ns[:c]) for c in range(C + 1)]
        rb = [sum(nr[:c]) for c in range(C + 1)]
        n = rb[C]
        x_recv, y_recv = self._e(n, D), self._e(n, D)
        hid_pre, hid = self._e(n, self.Hm), self._e(n, self.Hm)
        y_send = self._e(self.R, D)
        works = [self._a2a_async(x_recv[rb[c]:rb[c + 1]], x_send[sb[c]:sb[c + 1]], plans[c].out_splits, plans[c].in_splits)
                 for c in range(C)]
        back = []
        for c in range(C):
            works[c].wait()
            pl, rows = plans[c], slice(rb[c], rb[c + 1])
            if nr[c] > 0:
                self._ffn_fwd(i, x_recv[rows], hid_pre[rows], hid[rows], y_recv[rows], nr[c], pl.regroup, 1, pl.offsets,
                              pl.tile_starts, es=slice(c * Ec, (c + 1) * Ec))
            back.append(self._a2a_async(y_send[sb[c]:sb[c + 1]], y_recv[rows], pl.in_splits, pl.out_splits))
        # the unchunked view of the plan for the backward / a checkpoint recompute: chunk c's rows sit at rb[c] of the received
        # buffer and its experts at c * Ec of the local experts
        rg = torch.cat([plans[c].regroup + rb[c] for c in range(C)]) if n else self.ep_regroup_c[i][0, :0]
        offs = torch.cat([plans[c].offsets[:-1] + rb[c] for c in range(C)] +
                         [torch.full((1,), n, dtype=torch.int32, device=dev)])
        ts_all, base_t = [], torch.zeros((), dtype=torch.int32, device=dev)
        for pl in plans:
            ts_all.append(pl.tile_starts[:-1] + base_t)
            base_t = base_t + pl.tile_starts[-1]
        ts_all.append(base_t.reshape(1))
        ep = dict(plan=None, chunked=True, plans=plans, sb=sb, rb=rb, n=n, rg=rg.contiguous(), offsets=offs.contiguous(),
                  tile_starts=torch.cat(ts_all).contiguous(), x_recv=x_recv, hid_pre=hid_pre, hid=hid)
        for w_ in back:
            w_.wait()
        ops.gather_rows(y_send, r.pos, a["y"])                       # back to token-major [T*k, D]
        if self.checkpoint:                                          # local hidden activations: recomputed in backward
            ep["hid_pre"] = ep["hid"] = None
        a["ep"] = ep

    def _experts_bwd_ep_chunked(self, i, a):
        """mirror of _experts_fwd_ep_chunked: the d y rows travel in the same chunks; chunk c's input-gradient GEMMs run while the
        later chunks are in flight and its d x rows go home under the next chunk's GEMMs; the weight gradients (all local
        experts at once, on the side-by-side buffers - the same launches as the one-exchange path) run last, under the
        returning exchanges."""
        D, r, ep = self.D, a["route"], a["ep"]
        C, Ec = self.ep_chunks, self.E_loc // self.ep_chunks
        plans, sb, rb, n = ep["plans"], ep["sb"], ep["rb"], ep["n"]
        dy_send = ops.gather_rows(self.s_dy, r.row_of_slot, self._e(self.R, D))
        dy_recv, dx_recv, dhp = self._e(n, D), self._e(n, D), self._e(n, self.Hm)
        dx_send = self._e(self.R, D)
        works = [self._a2a_async(dy_recv[rb[c]:rb[c + 1]], dy_send[sb[c]:sb[c + 1]], plans[c].out_splits, plans[c].in_splits)
                 for c in range(C)]
        back = []
        for c in range(C):
            works[c].wait()
            pl, rows = plans[c], slice(rb[c], rb[c + 1])
            if rb[c + 1] > rb[c]:
                self._ffn_bwd(i, dy_recv[rows], None, ep["hid_pre"][rows], None, dhp[rows], dx_recv[rows], rb[c + 1] - rb[c],
                              pl.regroup, 1, pl.offsets, pl.tile_starts, es=slice(c * Ec, (c + 1) * Ec), wgrad=False)
            back.append(self._a2a_async(dx_send[sb[c]:sb[c + 1]], dx_recv[rows], pl.in_splits, pl.out_splits))
        if n > 0:
            self._ffn_bwd(i, dy_recv, ep["x_recv"], None, ep["hid"], dhp, None, n, ep["rg"], 1, ep["offsets"], None, dgrad=False)
        for w_ in back:
            w_.wait()
        ops.gather_rows(dx_send, r.pos, self.s_dxe)

    # ------------------------------------------------------------------ fixed capacity
    def _experts_fwd_ep_fixed(self, i, a, g):
        """_experts_fwd_ep with ep_cap rows per (source, destination) pair: the send buffer is the padded [W * cap, D]
        image gathered straight from h2 through pad_idx, rows arrive at source * cap + ..., the grouped GEMMs take the
        device-resident regroup / offsets / tile prefix with M = the capacity bound (surplus workgroups retire on the
        device-side tile prefix), and the outputs come home through unpad_idx.  Every exchange is an all-to-all with equal
        splits: no sizes, nothing for the host to read."""
        fx = self.ep_fx[i]
        W, cap = self.ep_world, self.ep_cap
        r = ops.route_build(g["idx32"], self.E, want_counts64=True)
        a["route"] = r
        dist.all_to_all_single(fx["recv_counts"], r.counts64, group=self.ep_group)
        plan = fx["plan"] = ops.ep_plan_fixed(r.counts64, fx["recv_counts"], W, self.E_loc, cap, r, self.ep_overflow,
                                              bufs=fx["plan"])
        ops.gather_rows(a["h2"], plan.pad_idx, fx["x_send"], div=self.k)
        dist.all_to_all_single(fx["x_recv"], fx["x_send"], group=self.ep_group)
        self._ffn_fwd(i, fx["x_recv"], fx["hid_pre"], fx["hid"], fx["y_recv"], W * cap, plan.regroup, 1, plan.offsets,
                      plan.tile_starts)
        dist.all_to_all_single(fx["y_back"], fx["y_recv"], group=self.ep_group)
        ops.gather_rows(fx["y_back"], plan.unpad_idx, a["y"])            # back to token-major [T*k, D]
        a["ep"] = dict(fixed=True)

    def _experts_bwd_ep_fixed(self, i, a):
        fx, fb = self.ep_fx[i], self.ep_fx_bwd
        plan = fx["plan"]
        ops.gather_rows(self.s_dy, plan.pad_idx, fb["dy_send"])
        dist.all_to_all_single(fb["dy_recv"], fb["dy_send"], group=self.ep_group)
        self._ffn_bwd(i, fb["dy_recv"], fx["x_recv"], fx["hid_pre"], fx["hid"], fb["dhp"], fb["dx_recv"],
                      self.ep_world * self.ep_cap, plan.regroup, 1, plan.offsets, plan.tile_starts)
        dist.all_to_all_single(fb["dx_back"], fb["dx_recv"], group=self.ep_group)
        ops.gather_rows(fb["dx_back"], plan.unpad_idx, self.s_dxe)

    def ep_overflowed(self) -> bool:
        """fixed-capacity exchange: did any (source, destination) pair of any layer since the last call route more rows
        than the capacity?  ONE host read; clears the flag."""
        if not self.ep_capacity:
            return False
        over = bool(int(self.ep_overflow.item()))
        if over:
            self.ep_overflow.zero_()
        return over
