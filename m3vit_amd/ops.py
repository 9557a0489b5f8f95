"""Tensor-level wrappers over the C ABI (include/m3vit_hip.h).

torch is used here only as the owner of device memory and streams: every function
hands raw device pointers + sizes to libm3vit_hip.so and launches on torch's current
HIP stream.  No function in this module computes anything with torch ops.
"""
from __future__ import annotations

import contextlib
import ctypes
import gc
import math
import os
from ctypes import byref, c_void_p
from typing import Optional

import torch

from . import _lib
from ._lib import (M3_ACT_GELU, M3_ACT_NONE, M3_BF16, M3_F16, M3_F32, GemmArgs, WgradArgs, WgradMultiArgs, WgradMultiPlan,
                   WgradMultiShape, WgradPlan, WgradReduceDesc, WgradShape, check, lib)

_DT = {torch.float32: M3_F32, torch.float16: M3_F16, torch.bfloat16: M3_BF16}      # bf16: every entry point


def dt_code(dtype: torch.dtype) -> int:
    try:
        return _DT[dtype]
    except KeyError:
        raise _lib.M3Error(f"unsupported activation dtype {dtype}; use float32, float16 or bfloat16")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else c_void_p(t.data_ptr())


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


@contextlib.contextmanager
def graph_capture(g: "torch.cuda.CUDAGraph"):
    """`torch.cuda.graph(g, capture_error_mode="thread_local")` with Python's cyclic garbage collector held off until the
    capture has ended.  torch no longer collects before a capture (only under torch.compiler.config.force_cudagraph_gc), so
    an automatic collection can start INSIDE one - any allocation of the captured Python code may trigger it - and run the
    finalizers of dead objects of earlier work (captured graphs, events, streams' work) on the capturing thread, where
    their HIP calls are not allowed: the process aborts in the middle of the collection.  The garbage is collected after
    the capture instead.  (thread_local: other threads of the process, such as the RCCL watchdog polling its events, may
    keep making HIP calls while this thread captures.)"""
    enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            yield
    finally:
        if enabled:
            gc.enable()


def _req(t: torch.Tensor, dtype=None, name="tensor", numel=None, min_numel=None):
    """device, dtype, contiguity and size of a tensor handed to the C ABI, checked before anything is launched: the kernels
    read and write raw pointers, so a wrong dtype is reinterpreted and an undersized buffer is written past its end.
    numel: the exact element count the call reads / writes; min_numel: a lower bound (workspaces, index vectors)."""
    if not isinstance(t, torch.Tensor):
        raise _lib.M3Error(f"{name} must be a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise _lib.M3Error(f"{name} must live on the GPU (no CPU path)")
    if dtype is not None and t.dtype != dtype:
        raise _lib.M3Error(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.M3Error(f"{name} must be contiguous")
    if numel is not None and t.numel() != numel:
        raise _lib.M3Error(f"{name} must hold {numel} elements, got {t.numel()} (shape {tuple(t.shape)})")
    if min_numel is not None and t.numel() < min_numel:
        raise _lib.M3Error(f"{name} must hold at least {min_numel} elements, got {t.numel()}")
    return t


def _act(t: torch.Tensor, name="tensor", numel=None):
    """an activation-dtype tensor (fp32 / fp16 / bf16)"""
    _req(t, name=name, numel=numel)
    dt_code(t.dtype)
    return t


def _dims(t: torch.Tensor, n: int, name="tensor"):
    if not isinstance(t, torch.Tensor):
        raise _lib.M3Error(f"{name} must be a tensor, got {type(t).__name__}")
    if t.dim() != n:
        raise _lib.M3Error(f"{name} must be {n}-d, got shape {tuple(t.shape)}")
    return t.shape


# ----------------------------------------------------------------------------- gate
def gate_fwd(x, w_gate, k, logit_bias=None, noise=None, noise_std=0.0, dense=True, want_idx32=True,
             loss_acc=None, route=False, want_counts64=False):
    """x [T,D] f32/f16, w_gate [D,E] f32 (rows beyond D are ignored: pass w_gate[:D] + bias for
    task conditioning).  Returns dict with idx i64 [T,k], idx32, idx_next i32 [T], score, top_logits,
    clean, noisy, gates (dense only), importance f32 [E], load i64 [E], and the block's balance loss
    cv_loss = cv^2(importance) + cv^2(load) (0-dim) with its gradients d_importance / d_load_prob [E].
    For noisy training (noise given, noise_std != 0, k < E; needs dense) load is the Normal-CDF form
    load_prob f32 [E] (vision_transformer_moe.py:456-457), otherwise the count and d_load_prob is None.
    loss_acc: optional 1-element f32 tensor the loss is also added to.
    route: also build the dispatch metadata (result["route"]: a Route as route_build(idx32, E) returns it) from the gate
    kernel's own per-block counts - the histogram pass is not launched and the scan rides in the balance launch
    (m3_balance_route); needs k | 16."""
    _req(x, name="x")
    T, D = _dims(x, 2, "x")
    E = _dims(w_gate, 2, "w_gate")[1]
    _req(w_gate, torch.float32, "w_gate", D * E)
    dev = x.device
    kp = min(k + 1, E)
    f32 = torch.float32
    idx = torch.empty((T, k), dtype=torch.int64, device=dev)
    idx32 = torch.empty((T, k), dtype=torch.int32, device=dev) if want_idx32 else None
    idx_next = torch.empty((T,), dtype=torch.int32, device=dev) if kp > k else None
    score = torch.empty((T, k), dtype=f32, device=dev)
    top = torch.empty((T, kp), dtype=f32, device=dev)
    clean = torch.empty((T, E), dtype=f32, device=dev) if dense else None
    noisy = torch.empty((T, E), dtype=f32, device=dev) if dense else None
    gates = torch.empty((T, E), dtype=f32, device=dev) if dense else None
    nblk = lib().m3_gate_num_blocks(T)
    # one allocation for the partials and the [E]-sized results
    prob = noise is not None and float(noise_std) != 0.0 and k < E and dense
    pi = torch.empty((max(nblk, 1), E), dtype=f32, device=dev)
    pl = torch.empty((max(nblk, 1), E), dtype=torch.int32, device=dev)
    pp = torch.empty((max(nblk, 1), E), dtype=f32, device=dev) if prob else None
    small = torch.empty((4, E), dtype=f32, device=dev)
    imp, load_prob, d_imp, d_lp = small[0], (small[1] if prob else None), small[2], (small[3] if prob else None)
    load = torch.empty(E, dtype=torch.int64, device=dev)
    loss = torch.empty((), dtype=f32, device=dev)
    if logit_bias is not None:
        _req(logit_bias, f32, "logit_bias", E)
    if noise is not None:
        _req(noise, f32, "noise", T * E)
    if loss_acc is not None:
        _req(loss_acc, f32, "loss_acc", 1)
    route = bool(route) and T > 0 and 16 % k == 0 and want_idx32
    pc = torch.empty((2, max(nblk, 1), E), dtype=torch.int32, device=dev) if route else None     # counts, then their prefix
    a = _lib.GateFwdArgs(_p(x), dt_code(x.dtype), T, D, x.stride(0), _p(w_gate), E, _p(logit_bias), _p(noise),
                         float(noise_std), k, _p(idx), _p(idx32), _p(idx_next), _p(score), _p(top), _p(clean), _p(noisy),
                         _p(gates), _p(pi), _p(pl), _p(pp), _p(pc))
    check(lib().m3_gate_fwd(byref(a), _stream()), "m3_gate_fwd")
    r = None
    if route:
        n = T * k
        r = Route()
        r.n, r.E, r.k = n, E, k
        meta = torch.empty(3 * E + 2, dtype=torch.int32, device=dev)
        r.counts, r.offsets, r.tile_starts = meta[:E], meta[E:2 * E + 1], meta[2 * E + 1:]
        r.pos = torch.empty(n, dtype=torch.int32, device=dev)
        r.row_of_slot = torch.empty(n, dtype=torch.int32, device=dev)
        r.counts64 = torch.empty(E, dtype=torch.int64, device=dev) if want_counts64 else None
        check(lib().m3_balance_route(_p(pi), _p(pl), _p(pp), nblk, E, _p(imp), _p(load), _p(load_prob), _p(loss),
                                     _p(loss_acc), _p(d_imp), _p(d_lp), _p(pc[0]), _p(pc[1]), _p(r.counts), _p(r.offsets),
                                     _p(r.tile_starts), _p(r.counts64), _stream()), "m3_balance_route")
        check(lib().m3_route_assign(_p(idx32), n, E, k, _p(pc[1]), _p(r.offsets), _p(r.pos), _p(r.row_of_slot), _stream()),
              "m3_route_assign")
    else:
        check(lib().m3_balance_loss(_p(pi), _p(pl), _p(pp), nblk, E, _p(imp), _p(load),
                                    _p(load_prob), _p(loss), _p(loss_acc), _p(d_imp), _p(d_lp), _stream()),
              "m3_balance_loss")
    return dict(route=r, idx=idx, idx32=idx32, idx_next=idx_next, score=score, top_logits=top, clean=clean, noisy=noisy,
                gates=gates, importance=imp, load=load, load_prob=load_prob, cv_loss=loss, d_importance=d_imp,
                d_load_prob=d_lp, noise_std=float(noise_std) if prob else 0.0)


def gate_bwd_logits(noisy, idx, d_score, d_importance, k, *, balance_scale=1.0, d_top=None, idx_next=None,
                    d_load_prob=None, clean=None, top_logits=None, noise_std=0.0, out=None, balance_scale_dev=None,
                    out_act=None):
    """d_logits [T,E] from d_score [T,k], d_top [T,k+1], balance_scale * (d_importance, d_load_prob) [E].
    balance_scale_dev: optional 1-element f32 device tensor multiplied onto balance_scale inside the kernel.
    out_act: optional [T,E] tensor (activation dtype) that receives a second copy of the result."""
    T, E = _dims(noisy, 2, "noisy")
    kp = min(k + 1, E)
    f32 = torch.float32
    _req(noisy, f32, "noisy")
    _req(idx, torch.int64, "idx", T * k)
    for t_, name, n in ((clean, "clean", T * E), (out, "out", T * E), (d_score, "d_score", T * k),
                        (d_top, "d_top", T * kp), (top_logits, "top_logits", T * kp), (d_importance, "d_importance", E),
                        (d_load_prob, "d_load_prob", E), (balance_scale_dev, "balance_scale_dev", 1)):
        if t_ is not None:
            _req(t_, f32, name, n)
    if idx_next is not None:
        _req(idx_next, torch.int32, "idx_next", T)
    if out_act is not None:
        _act(out_act, "out_act", T * E)
    dl = torch.empty_like(noisy) if out is None else out
    a = _lib.GateBwdArgs(_p(noisy), _p(clean), _p(top_logits), _p(idx), _p(idx_next), _p(d_score), _p(d_top),
                         _p(d_importance), _p(d_load_prob), float(balance_scale), float(noise_std), T, E, k, _p(dl),
                         _p(balance_scale_dev), _p(out_act), dt_code(out_act.dtype) if out_act is not None else M3_F32)
    check(lib().m3_gate_bwd_logits(byref(a), _stream()), "m3_gate_bwd_logits")
    return dl


def gate_bwd_params(x, w_gate, d_logits, d_w_gate=None, beta_dw=0, dx=None, beta_dx=0, part_dw=None):
    T, D = _dims(x, 2, "x")
    E = _dims(w_gate, 2, "w_gate")[1]
    _act(x, "x"); _req(w_gate, torch.float32, "w_gate", min_numel=D * E); _req(d_logits, torch.float32, "d_logits", T * E)
    if d_w_gate is not None:
        _req(d_w_gate, torch.float32, "d_w_gate", D * E)
    if dx is not None:
        _req(dx, torch.float32, "dx", T * D)
    if d_w_gate is not None and part_dw is None:
        part_dw = torch.empty((lib().m3_gate_dw_blocks(T), D, E), dtype=torch.float32, device=x.device)
    if d_w_gate is not None:
        _req(part_dw, torch.float32, "part_dw", min_numel=lib().m3_gate_dw_blocks(T) * D * E)
    check(lib().m3_gate_bwd_params(_p(x), dt_code(x.dtype), T, D, x.stride(0), _p(w_gate), E, _p(d_logits),
                                   _p(part_dw) if d_w_gate is not None else None, _p(d_w_gate), beta_dw,
                                   _p(dx), dx.stride(0) if dx is not None else 0, beta_dx, _stream()),
          "m3_gate_bwd_params")


# ---------------------------------------------------------------------------- route
class Route:
    """Device-resident dispatch metadata (no host sync).  Expert ids outside [0, E) are a caller error: such entries
    get no slot (their token-major output rows are never written) while pos / row_of_slot stay in range; check()
    - a host sync, for tests and debugging - raises when any entry was dropped."""
    __slots__ = ("counts", "offsets", "pos", "row_of_slot", "tile_starts", "counts64", "n", "E", "k")

    def check(self):
        routed = int(self.offsets[-1])
        if routed != self.n:
            raise _lib.M3Error(f"route_build: {self.n - routed} of {self.n} expert ids lie outside [0, {self.E})")
        return self


def route_build(idx32: torch.Tensor, E: int, want_counts64=False) -> Route:
    _req(idx32, torch.int32, "idx32")
    n = idx32.numel()
    dev = idx32.device
    r = Route()
    r.n, r.E, r.k = n, E, idx32.shape[-1] if idx32.dim() > 1 else 1
    r.counts = torch.empty(E, dtype=torch.int32, device=dev)
    r.offsets = torch.empty(E + 1, dtype=torch.int32, device=dev)
    r.pos = torch.empty(n, dtype=torch.int32, device=dev)
    r.row_of_slot = torch.empty(n, dtype=torch.int32, device=dev)
    r.tile_starts = torch.empty(E + 1, dtype=torch.int32, device=dev)
    r.counts64 = torch.empty(E, dtype=torch.int64, device=dev) if want_counts64 else None
    ws = torch.empty(int(lib().m3_route_ws_elems(n, E)), dtype=torch.int32, device=dev)
    if n == 0:                                   # nothing routed: all-zero metadata, no launch
        for t_ in (r.counts, r.offsets, r.tile_starts):
            t_.zero_()
        if r.counts64 is not None:
            r.counts64.zero_()
        return r
    check(lib().m3_route_build(_p(idx32), n, E, _p(r.counts), _p(r.offsets), _p(r.pos), _p(r.row_of_slot),
                               _p(r.tile_starts), _p(r.counts64), _p(ws), _stream()), "m3_route_build")
    return r


class EpPlan:
    """Device-resident expert-parallel exchange plan (m3_ep_plan) + the two split lists the a2a-v API needs."""
    __slots__ = ("splits", "regroup", "offsets", "tile_starts", "in_splits", "out_splits", "n_recv")


def ep_plan(send_counts64, recv_counts64, world: int, e_loc: int, regroup_buf: torch.Tensor, splits_host=None) -> EpPlan:
    """Plan of one expert-parallel exchange from the two count vectors, computed on the device; the host reads only the
    2 * world split sizes (one small copy into pinned memory; torch.distributed's a2a-v takes python lists)."""
    _req(send_counts64, torch.int64, "send_counts", world * e_loc)
    _req(recv_counts64, torch.int64, "recv_counts", world * e_loc)
    _req(regroup_buf, torch.int32, "regroup_buf")
    dev = send_counts64.device
    p = EpPlan()
    p.splits = torch.empty(2 * world, dtype=torch.int64, device=dev)
    p.offsets = torch.empty(e_loc + 1, dtype=torch.int32, device=dev)
    p.tile_starts = torch.empty(e_loc + 1, dtype=torch.int32, device=dev)
    check(lib().m3_ep_plan(_p(send_counts64), _p(recv_counts64), world, e_loc, _p(p.splits), _p(regroup_buf),
                           regroup_buf.numel(), _p(p.offsets), _p(p.tile_starts), _stream()), "m3_ep_plan")
    if splits_host is None:
        splits_host = torch.empty(2 * world, dtype=torch.int64, pin_memory=True)
    splits_host.copy_(p.splits, non_blocking=True)
    torch.cuda.current_stream().synchronize()          # the one host read of the exchange: 2 * world integers
    sp = splits_host.tolist()
    p.in_splits, p.out_splits = sp[:world], sp[world:]
    p.n_recv = sum(p.out_splits)
    if p.n_recv > regroup_buf.numel():
        raise _lib.M3Error(f"ep_plan: {p.n_recv} received rows exceed the regroup buffer ({regroup_buf.numel()})")
    p.regroup = regroup_buf[: p.n_recv]
    return p


def ep_plan_chunks(send_counts64, recv_counts64, world: int, e_chunk: int, regroup_bufs: torch.Tensor, splits_host=None):
    """The plans of an exchange cut into C chunks of e_chunk local experts each (send / recv counts laid out
    [C][world][e_chunk]: the routing keys are chunk-major, BackboneEngine ep_chunks): C m3_ep_plan launches, then ONE host read
    of all C * 2 * world split sizes.  regroup_bufs: i32 [C, capacity].  Returns a list of EpPlan."""
    _req(send_counts64, torch.int64, "send_counts"); _req(recv_counts64, torch.int64, "recv_counts")
    _req(regroup_bufs, torch.int32, "regroup_bufs")
    C = regroup_bufs.shape[0]
    assert send_counts64.numel() == C * world * e_chunk == recv_counts64.numel()
    dev = send_counts64.device
    send, recv = send_counts64.view(C, world * e_chunk), recv_counts64.view(C, world * e_chunk)
    splits = torch.empty(C, 2 * world, dtype=torch.int64, device=dev)
    plans = []
    for c in range(C):
        p = EpPlan()
        p.splits = splits[c]
        p.offsets = torch.empty(e_chunk + 1, dtype=torch.int32, device=dev)
        p.tile_starts = torch.empty(e_chunk + 1, dtype=torch.int32, device=dev)
        check(lib().m3_ep_plan(_p(send[c]), _p(recv[c]), world, e_chunk, _p(p.splits), _p(regroup_bufs[c]),
                               regroup_bufs.shape[1], _p(p.offsets), _p(p.tile_starts), _stream()), "m3_ep_plan")
        plans.append(p)
    if splits_host is None:
        splits_host = torch.empty(C, 2 * world, dtype=torch.int64, pin_memory=True)
    splits_host.copy_(splits, non_blocking=True)
    torch.cuda.current_stream().synchronize()          # the one host read of the exchange: C * 2 * world integers
    sp = splits_host.tolist()
    for c, p in enumerate(plans):
        p.in_splits, p.out_splits = sp[c][:world], sp[c][world:]
        p.n_recv = sum(p.out_splits)
        if p.n_recv > regroup_bufs.shape[1]:
            raise _lib.M3Error(f"ep_plan_chunks: {p.n_recv} received rows exceed the regroup buffer ({regroup_bufs.shape[1]})")
        p.regroup = regroup_bufs[c, : p.n_recv]
    return plans


class EpPlanFixed:
    """Device-resident plan of a fixed-capacity exchange (m3_ep_plan_fixed): nothing of it is read by the host."""
    __slots__ = ("cap", "world", "regroup", "offsets", "tile_starts", "pad_idx", "unpad_idx", "splits")


def ep_plan_fixed(send_counts64, recv_counts64, world: int, e_loc: int, cap: int, route: "Route", overflow: torch.Tensor,
                  bufs: Optional[EpPlanFixed] = None) -> EpPlanFixed:
    """Plan of one expert-parallel exchange with `cap` rows per (source, destination) pair, entirely on the device.
    overflow: i32 [1] flag the kernel raises (and never clears) when a pair routes more than cap rows.
    bufs: a previous plan whose index buffers are overwritten (static addresses for a captured step)."""
    _req(send_counts64, torch.int64, "send_counts"); _req(recv_counts64, torch.int64, "recv_counts")
    _req(overflow, torch.int32, "overflow")
    dev = send_counts64.device
    p = bufs
    if p is None:
        p = EpPlanFixed()
        p.cap, p.world = int(cap), int(world)
        p.regroup = torch.empty(world * cap, dtype=torch.int32, device=dev)
        p.pad_idx = torch.empty(world * cap, dtype=torch.int32, device=dev)
        p.unpad_idx = torch.empty(max(route.n, 1), dtype=torch.int32, device=dev)
        p.offsets = torch.empty(e_loc + 1, dtype=torch.int32, device=dev)
        p.tile_starts = torch.empty(e_loc + 1, dtype=torch.int32, device=dev)
        p.splits = torch.empty(2 * world, dtype=torch.int64, device=dev)
    assert p.cap == cap and p.world == world and p.unpad_idx.numel() >= route.n
    check(lib().m3_ep_plan_fixed(_p(send_counts64), _p(recv_counts64), world, e_loc, cap, _p(route.row_of_slot), _p(route.pos),
                                 route.n, _p(p.splits), _p(p.regroup), _p(p.offsets), _p(p.tile_starts), _p(p.pad_idx),
                                 _p(p.unpad_idx), _p(overflow), _stream()), "m3_ep_plan_fixed")
    return p


# ----------------------------------------------------------------------------- GEMM
def gemm_nt(A, B, C, *, M=None, bias=None, act=M3_ACT_NONE, pre_out=None, gelu_grad_pre=None, residual=None,
            a_row_idx=None, a_row_div=1, c_row_idx=None, group_offsets=None, tile_starts=None, row_scale=None,
            row_scale_div=1, row_scale_idx=None):
    """C[m,n] = epi(sum_k A[arow(m),k] B[g][n,k]).  A [rows,K]; B [N,K] or [G,N,K]; C [rows,N] (f32 or A.dtype)."""
    _req(A, name="A"); _req(B, A.dtype, "B"); _req(C, name="C")
    G = 1 if B.dim() == 2 else B.shape[0]
    N, K = B.shape[-2], B.shape[-1]
    a = GemmArgs()
    a.A = A.data_ptr(); a.lda = A.stride(0)
    a.a_row_idx = _p(a_row_idx)
    a.a_row_div = a_row_div
    a.B = B.data_ptr(); a.ldb = B.stride(-2)
    a.C = C.data_ptr(); a.ldc = C.stride(0); a.c_dtype = dt_code(C.dtype)
    a.c_row_idx = _p(c_row_idx)
    a.bias = _p(bias)
    a.pre_out = _p(pre_out)
    a.ld_pre = pre_out.stride(0) if pre_out is not None else 0
    a.gelu_grad_pre = _p(gelu_grad_pre)
    a.ld_gpre = gelu_grad_pre.stride(0) if gelu_grad_pre is not None else 0
    a.residual = _p(residual)
    a.ld_res = residual.stride(0) if residual is not None else 0
    a.act = act
    if row_scale is not None:
        _req(row_scale, torch.float32, "row_scale")
    a.row_scale = _p(row_scale)
    a.row_scale_div = row_scale_div
    if row_scale_idx is not None:
        _req(row_scale_idx, torch.int32, "row_scale_idx")
        assert row_scale is not None
    a.row_scale_idx = _p(row_scale_idx)
    if M is None:
        M = a_row_idx.numel() if a_row_idx is not None else A.shape[0]
    a.M = M; a.N = N; a.K = K; a.G = G
    a.group_offsets = _p(group_offsets)
    a.tile_starts = _p(tile_starts)
    a.dtype = dt_code(A.dtype)
    if bias is not None:
        _req(bias, torch.float32, "bias")
    if residual is not None:
        _req(residual, torch.float32, "residual")
    if M == 0:
        return C
    check(lib().m3_gemm_nt(byref(a), _stream()), "m3_gemm_nt")
    return C


def gemm_plan(a: GemmArgs) -> _lib.GemmPlan:
    """What m3_gemm_nt would do with the argument struct `a` (m3_gemm_plan in include/m3vit_hip.h): .kernel / .epilogue
    (names: _lib.GEMM_KERNELS / _lib.GEMM_EPILOGUES), the tile and the tile order.  Host code: launches nothing, reads no
    operand."""
    p = _lib.GemmPlan()
    check(lib().m3_gemm_plan(byref(a), byref(p)), "m3_gemm_plan")
    return p


def gemm_set_big(mode: int):
    """which gemm_nt calls take the 256 x 256-tile kernel for long contractions (include/m3vit_hip.h: m3_gemm_set_big):
    0 never, 1 every call it can run, 2 (default) those with enough tiles to fill the chip, -1 re-read M3_GEMM_BIG"""
    check(lib().m3_gemm_set_big(int(mode)), "m3_gemm_set_big")


def set_cache_hints(mask: int):
    """which kernel families run their non-temporal instances (include/m3vit_hip.h: m3_set_cache_hints): an OR of the
    M3_HINT_* bits, -1 re-reads M3_CACHE_HINTS (unset: M3_HINT_DEFAULT).  Results are bit-identical under every mask."""
    check(lib().m3_set_cache_hints(int(mask)), "m3_set_cache_hints")


_WGRAD_DIRECT = os.environ.get("M3_WGRAD_DIRECT", "1") != "0"      # one part per group: the kernel accumulates into dW itself (no slabs)


def _wgrad_reduce(d: WgradReduceDesc):
    """launch the slab reduction a descriptor names"""
    if d.chunk_rows:
        check(lib().m3_wgrad_reduce_grouped(d.ws, d.group_offsets, d.G, d.chunk_rows, d.elems, d.dW, d.beta, d.bias_ws,
                                            d.bias_elems, d.db, d.beta_db, _stream()), "m3_wgrad_reduce_grouped")
    else:
        check(lib().m3_wgrad_reduce(d.ws, d.splits, d.elems, d.dW, d.beta, d.bias_ws, d.bias_elems, d.db, d.beta_db,
                                    _stream()), "m3_wgrad_reduce")


class WgradQueue:
    """Weight-gradient calls of ONE stream whose slab reductions ride in front of the next call's launch
    (m3_wgrad_args.prev) instead of being launched by themselves: two slab workspaces used in turn, the reduction of the
    latest call pending until the next wgrad_tn(.., queue=self) or flush().  Whoever reads the gradients (an all-reduce,
    the optimizer, a test) calls flush() first."""

    def __init__(self, ws_elems: int, device):
        self.ws = [torch.empty(ws_elems, dtype=torch.float32, device=device) for _ in range(2)]
        self.i = 0
        self.pending = None          # (ctypes array of WgradReduceDesc - one, or those of a wgrad_multi call -, tensors they point at)

    def reset(self):
        """drop a pending reduction without running it (step boundaries: see BackboneEngine.zero_grad)"""
        self.pending = None
        self.i = 0

    def flush(self):
        if self.pending is None:
            return
        descs, _keep = self.pending
        self.pending = None
        if len(descs) > 1:
            check(lib().m3_wgrad_reduce_multi(descs, len(descs), _stream()), "m3_wgrad_reduce_multi")
        elif descs[0].elems:
            _wgrad_reduce(descs[0])

    def take_prev(self, a, writes=()):
        """the pending reduction into a.prev / a.n_prev of the next call's arguments; one that writes a tensor the call
        itself writes (data pointers in `writes`) cannot ride in front of it and runs now"""
        if self.pending is None:
            return
        if any(d.dW in writes or (d.db is not None and d.db in writes) for d in self.pending[0]):
            self.flush()
            return
        a.prev = ctypes.cast(self.pending[0], ctypes.POINTER(WgradReduceDesc))
        a.n_prev = len(self.pending[0])


def wgrad_launch_plan(M, N, K, G, dtype, *, grouped, bias=True, splits=0, direct_ok=False) -> WgradPlan:
    """How m3_wgrad_tn cuts this call up (m3_wgrad_plan in include/m3vit_hip.h): .splits / .chunk_rows / .units for
    m3_wgrad_args, .direct, .ws_elems fp32 elements of slab workspace.  splits = 0: the library's rule."""
    s = WgradShape(M, N, K, G, dt_code(dtype), bool(grouped), bool(bias), splits, bool(direct_ok))
    p = WgradPlan()
    check(lib().m3_wgrad_plan(byref(s), byref(p)), "m3_wgrad_plan")
    return p


def wgrad_plan(M, G, splits, grouped):
    """(chunk_rows, slab slots) of a call cut into the caller's `splits` row parts (N, K and the dtype do not enter then)"""
    p = wgrad_launch_plan(M, 1, 1, G, torch.float32, grouped=grouped, bias=False, splits=splits)
    return p.chunk_rows, p.units


def wgrad_ws_elems(M, N, K, G, grouped, bias=True, *, dtype):
    """fp32 elements of workspace wgrad_tn needs for this shape with the default splits"""
    return wgrad_launch_plan(M, N, K, G, dtype, grouped=grouped, bias=bias).ws_elems


def default_wgrad_splits(M, N, K, G, dtype):
    """row parts wgrad_tn cuts this shape into when the caller names none"""
    return wgrad_launch_plan(M, N, K, G, dtype, grouped=G > 1).splits


def wgrad_tn(dC, A, dW, *, M=None, beta=0, splits=None, ws=None, c_row_idx=None, a_row_idx=None, a_row_div=1,
             group_offsets=None, db=None, beta_db=None, c_row_div=1, c_row_scale=None, queue: Optional[WgradQueue] = None):
    """dW[g][n,k] (+)= sum_m dC[crow(m),n] A[arow(m),k].  dW f32 [N,K] or [G,N,K].
    db (optional, f32 [N] / [G,N]): bias gradient = column sums of dC, fused into the same pass.
    c_row_div / c_row_scale (with c_row_idx): slot m reads c_row_scale[c_row_idx[m]] * dC[c_row_idx[m] // c_row_div].
    queue: this call's slab reduction is left pending in the queue (dW is complete only after the queue's next call or
    flush()) and the queue's previous pending reduction runs in front of this launch."""
    _req(dC, name="dC"); _req(A, dC.dtype, "A"); _req(dW, torch.float32, "dW")
    G = 1 if dW.dim() == 2 else dW.shape[0]
    N, K = dW.shape[-2], dW.shape[-1]
    if M is None:
        M = c_row_idx.numel() if c_row_idx is not None else dC.shape[0]
    bdb = beta if beta_db is None else beta_db
    if M == 0:                                   # nothing to contract over: no launch (an empty tensor has no address)
        if not beta:
            dW.zero_()
        if db is not None and not bdb:
            db.zero_()
        return dW
    # direct mode (include/m3vit_hip.h: m3_wgrad_args.direct_dW) where the plan has one part per group: no slabs, no reduction
    p = wgrad_launch_plan(M, N, K, G, dC.dtype, grouped=group_offsets is not None, bias=db is not None, splits=splits or 0,
                   direct_ok=_WGRAD_DIRECT and dW.data_ptr() % 16 == 0)
    if queue is not None:
        ws = queue.ws[queue.i]
        assert ws.numel() >= p.ws_elems, "WgradQueue workspace too small for this shape"
    elif ws is None or ws.numel() < p.ws_elems:
        ws = torch.empty(max(p.ws_elems, 4), dtype=torch.float32, device=dW.device)
    a = WgradArgs()
    a.dC = dC.data_ptr(); a.lddc = dC.stride(0)
    a.c_row_idx = _p(c_row_idx)
    a.c_row_div = c_row_div
    if c_row_scale is not None:
        _req(c_row_scale, torch.float32, "c_row_scale")
        assert c_row_idx is not None
    a.c_row_scale = _p(c_row_scale)
    a.A = A.data_ptr(); a.lda = A.stride(0)
    a.a_row_idx = _p(a_row_idx)
    a.a_row_div = a_row_div
    a.M = M; a.N = N; a.K = K; a.G = G
    a.group_offsets = _p(group_offsets)
    a.splits = p.splits; a.chunk_rows = p.chunk_rows; a.units = p.units
    a.ws = ws.data_ptr()
    a.dtype = dt_code(dC.dtype)
    if db is not None:
        _req(db, torch.float32, "db")
    if p.direct:
        a.direct_dW = dW.data_ptr(); a.direct_beta = 1 if beta else 0
        a.direct_db = _p(db)
        a.direct_beta_db = 1 if bdb else 0
    else:
        # the reduction of this call's slabs; both slab kinds in one launch where db and the bias slabs are 16-byte aligned
        bias_ws = ws[p.units * N * K:] if db is not None else None
        a.bias_ws = _p(bias_ws)
        fuse = db is not None and db.data_ptr() % 16 == 0 and bias_ws.data_ptr() % 16 == 0
        assert db is None or fuse or queue is None, "queued wgrad: db and the bias slabs must be 16-byte aligned"
        assert db is None or fuse or not p.chunk_rows, "balanced grouped wgrad: db and the bias slabs must be 16-byte aligned"
        per = 1 if p.chunk_rows else G                              # balanced: elements per group, else of all groups
        descs = (WgradReduceDesc * 1)()
        d = descs[0]
        d.ws = ws.data_ptr(); d.splits = p.splits; d.elems = per * N * K
        d.group_offsets = a.group_offsets if p.chunk_rows else None
        d.G = G; d.chunk_rows = p.chunk_rows
        d.dW = dW.data_ptr(); d.beta = beta
        d.bias_ws = bias_ws.data_ptr() if fuse else None
        d.bias_elems = per * N if fuse else 0
        d.db = db.data_ptr() if fuse else None
        d.beta_db = bdb
    if queue is not None:                                          # the previous call's reduction rides in front; in direct mode
        queue.take_prev(a, (a.direct_dW, a.direct_db) if p.direct else ())    # not one into the tensor this launch read-add-writes
    check(lib().m3_wgrad_tn(byref(a), _stream()), "m3_wgrad_tn")
    if p.direct:                                                   # nothing to reduce (and the queue's slab buffer was not used)
        if queue is not None:
            queue.pending = None
    elif queue is not None:
        queue.pending = (descs, (ws, dW, db, group_offsets))
        queue.i ^= 1
    else:
        _wgrad_reduce(d)
        if db is not None and not fuse:
            check(lib().m3_wgrad_bias_reduce(_p(bias_ws), p.splits, G * N, _p(db), bdb, _stream()), "m3_wgrad_bias_reduce")
    return dW


def _wgrad_multi_shape(problems, M, dtype, parts):
    s = WgradMultiShape()
    s.M = M; s.dtype = dt_code(dtype); s.n = len(problems); s.parts = parts
    for j, (N, K, bias) in enumerate(problems):
        s.N[j] = N; s.K[j] = K; s.bias[j] = 1 if bias else 0
    return s


def wgrad_multi_plan(shapes, M, dtype, parts=0) -> WgradMultiPlan:
    """How m3_wgrad_multi runs the batch of dense weight gradients `shapes` = [(N, K, has bias), ..] over M rows
    (m3_wgrad_multi_plan in include/m3vit_hip.h): .allowed (0: keep a call per weight), .parts, .tiles, .workgroups,
    .ws_elems fp32 elements of slab workspace.  parts = 0: the library's rule."""
    assert 1 <= len(shapes) <= _lib.WGRAD_MULTI_MAX, f"1 .. {_lib.WGRAD_MULTI_MAX} problems"
    p = WgradMultiPlan()
    check(lib().m3_wgrad_multi_plan(byref(_wgrad_multi_shape(shapes, M, dtype, parts)), byref(p)), "m3_wgrad_multi_plan")
    return p


def wgrad_multi_ws_elems(shapes, M, dtype, parts=0) -> int:
    """fp32 elements of workspace wgrad_multi needs for this batch"""
    return wgrad_multi_plan(shapes, M, dtype, parts).ws_elems


def wgrad_multi(problems, M, *, parts=0, ws=None, queue: Optional[WgradQueue] = None):
    """dW_j (+)= dC_j^T A_j, db_j (+)= column sums of dC_j for every problem (dC, A, dW, db or None, beta[, beta_db]) in ONE
    launch (m3_wgrad_multi): plain rows 0 .. M-1 of 16-bit operands, shapes wgrad_multi_plan allows.  queue: the slab
    reductions are left pending in it and the queue's previous reduction runs in front of this launch; else they run
    as one launch behind it.  With a queue, ws (optional) is the caller's slab buffer in place of the queue's next one: it
    must stay untouched until the pending reduction has run, and must not be the buffer of the call before."""
    n = len(problems)
    assert 1 <= n <= _lib.WGRAD_MULTI_MAX, f"1 .. {_lib.WGRAD_MULTI_MAX} problems"
    a = WgradMultiArgs()
    dt = problems[0][0].dtype
    shapes = []
    for j, pr in enumerate(problems):
        dC, A, dW, db, beta = pr[:5]
        _req(dC, dt, "dC"); _req(A, dt, "A"); _req(dW, torch.float32, "dW")
        N, K = dW.shape
        assert dC.shape[0] >= M and A.shape[0] >= M and dC.shape[1] == N and A.shape[1] == K, "wgrad_multi: operand shapes"
        q = a.prob[j]
        q.dC = dC.data_ptr(); q.lddc = dC.stride(0); q.A = A.data_ptr(); q.lda = A.stride(0); q.N = N; q.K = K
        q.dW = dW.data_ptr(); q.beta = 1 if beta else 0
        if db is not None:
            _req(db, torch.float32, "db", numel=N)
            q.db = db.data_ptr(); q.beta_db = 1 if (beta if len(pr) < 6 else pr[5]) else 0
        shapes.append((N, K, db is not None))
    p = wgrad_multi_plan(shapes, M, dt, parts)
    own_ws = ws is not None
    if queue is not None:
        ws = ws if own_ws else queue.ws[queue.i]
        assert ws.numel() >= p.ws_elems, "wgrad_multi: slab workspace too small for this batch"
    elif ws is None or ws.numel() < p.ws_elems:
        ws = torch.empty(max(p.ws_elems, 4), dtype=torch.float32, device=problems[0][2].device)
    a.M = M; a.dtype = dt_code(dt); a.n = n; a.parts = p.parts; a.ws = ws.data_ptr()
    descs = (WgradReduceDesc * n)()
    a.reduce_out = ctypes.cast(descs, ctypes.POINTER(WgradReduceDesc))
    if queue is not None:
        queue.take_prev(a, [t.data_ptr() for pr in problems for t in (pr[2], pr[3]) if t is not None])
    check(lib().m3_wgrad_multi(byref(a), _stream()), "m3_wgrad_multi")
    if queue is not None:
        queue.pending = (descs, (ws, problems))
        if not own_ws:
            queue.i ^= 1
    else:
        check(lib().m3_wgrad_reduce_multi(descs, n, _stream()), "m3_wgrad_reduce_multi")


def wgrad_set_big(on: int):
    """256 x 256 weight-gradient tiles for the 16-bit ViT-Base shapes: 1 on (default) / 0 off / -1 from M3_WGRAD_BIG
    (include/m3vit_hip.h: m3_wgrad_set_big); switch before sizing workspaces"""
    check(lib().m3_wgrad_set_big(int(on)), "m3_wgrad_set_big")


def wgrad_set_dma(on: int):
    """LDS-DMA weight-gradient kernel: 0 never / 1 where it pays (default) / 2 wherever it can run / -1 from M3_WGRAD_DMA
    (include/m3vit_hip.h: m3_wgrad_set_dma);
    switch before sizing workspaces (the default row splits follow the kernel's workgroups per CU)"""
    check(lib().m3_wgrad_set_dma(int(on)), "m3_wgrad_set_dma")


def wgrad_tile(N, K, dtype=None):
    """(tn, tk): the output tile m3_wgrad_tn uses for this shape (m3_wgrad_tile in include/m3vit_hip.h)"""
    if dtype is None:
        return 128, 128
    tn, tk = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().m3_wgrad_tile(N, K, dt_code(dtype), byref(tn), byref(tk)), "m3_wgrad_tile")
    return tn.value, tk.value


def wgrad_skinny(N, K, G=1) -> bool:
    """m3_wgrad_tn takes plain calls of this shape (K = 16 / 32, one group) with the streaming kernel (m3_wgrad_skinny)"""
    return bool(lib().m3_wgrad_skinny(int(N), int(K), int(G)))


def wgrad_kernel(a: WgradArgs) -> _lib.WgradKernelOut:
    """The kernel m3_wgrad_tn would launch for the argument struct `a`, after its step-downs, and the instance flags
    (m3_wgrad_kernel in include/m3vit_hip.h; names: _lib.WGRAD_KERNELS).  Host code: launches nothing, reads no operand."""
    out = _lib.WgradKernelOut()
    check(lib().m3_wgrad_kernel(byref(a), byref(out)), "m3_wgrad_kernel")
    return out


def colsum(dC, db, *, M=None, beta=0, c_row_idx=None, group_offsets=None, ws=None):
    _req(dC, name="dC"); _req(db, torch.float32, "db")
    G = 1 if db.dim() == 1 else db.shape[0]
    N = db.shape[-1]
    if dC.dim() != 2 or dC.shape[1] != N:
        raise _lib.M3Error(f"dC must be [M, {N}] like db's columns, got shape {tuple(dC.shape)}")
    if M is None:
        M = dC.shape[0]
    need = int(lib().m3_colsum_ws_elems(M, N, G))
    if ws is None:
        ws = torch.empty(need, dtype=torch.float32, device=dC.device)
    _req(ws, torch.float32, "ws", min_numel=need)
    check(lib().m3_colsum(_p(dC), dt_code(dC.dtype), dC.stride(0), _p(c_row_idx), M, N, G, _p(group_offsets),
                          _p(ws), _p(db), beta, _stream()), "m3_colsum")
    return db


# -------------------------------------------------------------------- combine / LN
def combine_fwd(y, score, residual, out):
    T, k = _dims(score, 2, "score")
    D = y.shape[-1]
    _req(score, torch.float32, "score"); _act(y, "y", T * k * D); _req(out, torch.float32, "out", T * D)
    if residual is not None:
        _req(residual, torch.float32, "residual", T * D)
    check(lib().m3_combine_fwd(_p(y), dt_code(y.dtype), _p(score), _p(residual), T, k, D, _p(out), _stream()),
          "m3_combine_fwd")
    return out


def combine_bwd(dout, y, score, dy, dscore):
    """dy (may be None: d score only) [T*k, D] = score * dout ; dscore [T, k] = <dout, y>"""
    T, k = _dims(score, 2, "score")
    D = y.shape[-1]
    _req(score, torch.float32, "score"); _act(y, "y", T * k * D); _req(dout, torch.float32, "dout", T * D)
    _req(dscore, torch.float32, "dscore", T * k)
    if dy is not None:
        _req(dy, y.dtype, "dy", T * k * D)
    check(lib().m3_combine_bwd(_p(dout), _p(y), dt_code(y.dtype), _p(score), T, k, D, _p(dy), _p(dscore), _stream()),
          "m3_combine_bwd")


def combine_gate_bwd(dxe, k, d_logits, w_gate, dh):
    """dh [T, D] (fp32 or dxe's dtype) = sum_j dxe[t*k+j] + d_logits [T, E] @ w_gate[:D] [D, E]^T  (one pass; m3_combine_gate_bwd)"""
    T, E = _dims(d_logits, 2, "d_logits")
    D = dxe.shape[-1]
    _req(d_logits, torch.float32, "d_logits"); _req(w_gate, torch.float32, "w_gate", D * E); _act(dxe, "dxe", T * k * D)
    _act(dh, "dh", T * D)
    if tuple(w_gate.shape) != (D, E):
        raise _lib.M3Error(f"w_gate must be [{D}, {E}], got {tuple(w_gate.shape)}")
    if dh.dtype not in (torch.float32, dxe.dtype):
        raise _lib.M3Error(f"dh must be float32 or {dxe.dtype}, got {dh.dtype}")
    check(lib().m3_combine_gate_bwd(_p(dxe), dt_code(dxe.dtype), T, k, D, _p(d_logits), _p(w_gate), E, _p(dh), dt_code(dh.dtype),
                                    _stream()), "m3_combine_gate_bwd")
    return dh


def moe_stats_ws_elems(T, E) -> int:
    return int(lib().m3_moe_stats_ws_elems(T, E))


def moe_stats(score, clean, gates, h, y, load, record, ws=None):
    """One MoE block's routing statistics (m3_moe_stats) into `record`, an int32 tensor of moe_stats.record_words(E) words
    (layout: include/m3vit_hip.h; m3vit_amd.moe_stats.parse_record reads it).  score [T,k], clean / gates [T,E] f32;
    h [T,D] and y [T*k,D] in one activation dtype, rows may be strided; load [E] float32 or int64.  Nothing is read back."""
    T, k = _dims(score, 2, "score")
    E = _dims(gates, 2, "gates")[1]
    D = h.shape[-1]
    _req(score, torch.float32, "score"); _req(gates, torch.float32, "gates", T * E); _req(clean, torch.float32, "clean", T * E)
    for t_, name, rows in ((h, "h", T), (y, "y", T * k)):
        if not t_.is_cuda or t_.dtype not in _DT or t_.dtype != h.dtype or t_.dim() != 2 or tuple(t_.shape) != (rows, D) or \
                (rows > 1 and t_.stride(0) < D) or (D > 1 and t_.stride(1) != 1):
            raise _lib.M3Error(f"{name} must be [{rows}, {D}] {h.dtype} with unit column stride, got {tuple(t_.shape)} "
                               f"{t_.dtype} strides {tuple(t_.stride())}")
    if load.dtype not in (torch.float32, torch.int64):
        raise _lib.M3Error(f"load must be float32 or int64, got {load.dtype}")
    _req(load, load.dtype, "load", E)
    _req(record, torch.int32, "record", min_numel=8 + E)
    need = moe_stats_ws_elems(T, E)
    if ws is None:
        ws = torch.empty(need, dtype=torch.float32, device=score.device)
    _req(ws, torch.float32, "ws", min_numel=need)
    lf, li = (load, None) if load.dtype == torch.float32 else (None, load)
    check(lib().m3_moe_stats(_p(score), _p(clean), _p(gates), _p(h), h.stride(0) if T > 1 else D, _p(y),
                             y.stride(0) if T * k > 1 else D, dt_code(h.dtype), _p(lf), _p(li), T, E, k, D, _p(ws),
                             _p(record), _stream()), "m3_moe_stats")
    return record


def gather_rows(src, idx, dst, div=1, k=1):
    """dst[i] = sum_{j<k} src[idx[i*k+j] // div]."""
    nout, D = _dims(dst, 2, "dst")
    _act(dst, "dst"); _req(src, dst.dtype, "src"); _req(idx, torch.int32, "idx", min_numel=nout * k)
    if src.numel() % max(D, 1) or (src.dim() > 0 and src.shape[-1] != D):
        raise _lib.M3Error(f"src rows must be {D} wide like dst, got shape {tuple(src.shape)}")
    check(lib().m3_gather_rows(_p(src), dt_code(src.dtype), _p(idx), div, nout, k, D, _p(dst), _stream()), "m3_gather_rows")
    return dst


def layernorm_fwd(x, gamma, beta, y, mean, rstd, eps=1e-6):
    T, D = _dims(x, 2, "x")
    _req(x, torch.float32, "x"); _req(gamma, torch.float32, "gamma", D); _req(beta, torch.float32, "beta", D)
    _act(y, "y", T * D); _req(mean, torch.float32, "mean", T); _req(rstd, torch.float32, "rstd", T)
    check(lib().m3_layernorm_fwd(_p(x), T, D, _p(gamma), _p(beta), float(eps), _p(y), dt_code(y.dtype), _p(mean),
                                 _p(rstd), _stream()), "m3_layernorm_fwd")


def layernorm_bwd(dy, x, mean, rstd, gamma, dx_res, dx, dgamma, dbeta, beta=0, ws=None, dx_act=None):
    """dgamma = dbeta = None: the parameter-gradient partials stay in ws (fp32 [2, ln_bwd_blocks(T), D]) for a later
    batched layernorm_bwd_reduce."""
    T, D = _dims(x, 2, "x")
    nblk = lib().m3_ln_bwd_blocks(T, D)
    _req(x, torch.float32, "x"); _act(dy, "dy", T * D); _req(mean, torch.float32, "mean", T)
    _req(rstd, torch.float32, "rstd", T); _req(gamma, torch.float32, "gamma", D); _req(dx, torch.float32, "dx", T * D)
    if dx_res is not None:
        _req(dx_res, torch.float32, "dx_res", T * D)
    for t_, n_ in ((dgamma, "dgamma"), (dbeta, "dbeta")):
        if t_ is not None:
            _req(t_, torch.float32, n_, D)
    if (dgamma is None) != (dbeta is None):
        raise _lib.M3Error("layernorm_bwd: dgamma and dbeta go together (both None: the partials stay in ws)")
    if dx_act is not None:
        _act(dx_act, "dx_act", T * D)
    if ws is None:
        ws = torch.empty(2 * nblk * D, dtype=torch.float32, device=x.device)
    _req(ws, torch.float32, "ws", min_numel=2 * nblk * D)
    check(lib().m3_layernorm_bwd(_p(dy), dt_code(dy.dtype), _p(x), _p(mean), _p(rstd), _p(gamma), _p(dx_res), T, D,
                                 _p(dx), _p(ws), _p(dgamma), _p(dbeta), beta, _p(dx_act),
                                 dt_code(dx_act.dtype) if dx_act is not None else M3_F32, _stream()), "m3_layernorm_bwd")


class LnGradTable:
    """device-resident (dgamma, dbeta) pointer pairs of a model's LayerNorms, in workspace-slot order"""

    def __init__(self, pairs, device):
        self.keep = pairs
        arr = (_lib.LnParamGrads * len(pairs))()
        for d, (g, b) in zip(arr, pairs):
            _req(g, torch.float32, "dgamma"); _req(b, torch.float32, "dbeta")
            d.dgamma, d.dbeta = g.data_ptr(), b.data_ptr()
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
        self.n = len(pairs)


def layernorm_bwd_reduce(ws, nblk, D, table: LnGradTable, first, count, beta=1):
    """dgamma / dbeta of LayerNorms first .. first+count-1 from their partial slots ws[j] (fp32 [n, 2, nblk, D])"""
    _req(ws, torch.float32, "ws")
    if ws.dim() != 4 or tuple(ws.shape[1:]) != (2, nblk, D):
        raise _lib.M3Error(f"ws must be [n, 2, {nblk}, {D}], got {tuple(ws.shape)}")
    if first < 0 or count < 0 or first + count > min(table.n, ws.shape[0]):
        raise _lib.M3Error(f"layers [{first}, {first + count}) exceed the table ({table.n}) or the workspace ({ws.shape[0]})")
    check(lib().m3_layernorm_bwd_reduce(_p(ws), ws.stride(0), nblk, D, _p(table.table), first, count, beta, _stream()),
          "m3_layernorm_bwd_reduce")


# ------------------------------------------------------------------------ attention
def attention_plan(dtype, N, dh) -> _lib.AttentionPlan:
    """kernel family and instance of attention_fwd / attention_bwd for (dtype, N, dh) (m3_attention_plan in
    include/m3vit_hip.h; names: _lib.ATTN_FAMILIES).  Host code."""
    p = _lib.AttentionPlan()
    check(lib().m3_attention_plan(dt_code(dtype), int(N), int(dh), byref(p)), "m3_attention_plan")
    return p


def attention_fwd(qkv, B, N, heads, dh, o, lse):
    _act(qkv, "qkv", B * N * 3 * heads * dh); _req(o, qkv.dtype, "o", B * N * heads * dh)
    _req(lse, torch.float32, "lse", B * heads * N)
    check(lib().m3_attention_fwd(_p(qkv), dt_code(qkv.dtype), B, N, heads, dh, _p(o), _p(lse), _stream()),
          "m3_attention_fwd")


def attention_bwd(qkv, o, d_o, lse, B, N, heads, dh, dqkv, dq_ws=None):
    need = int(lib().m3_attention_bwd_ws_elems(B, N, heads, dh))
    C = heads * dh
    _act(qkv, "qkv", B * N * 3 * C); _req(o, qkv.dtype, "o", B * N * C); _req(d_o, qkv.dtype, "d_o", B * N * C)
    _req(lse, torch.float32, "lse", B * heads * N); _req(dqkv, qkv.dtype, "dqkv", B * N * 3 * C)
    if need and dq_ws is None:
        dq_ws = torch.empty(need, dtype=torch.float32, device=qkv.device)
    if need:
        _req(dq_ws, torch.float32, "dq_ws", min_numel=need)
    check(lib().m3_attention_bwd(_p(qkv), _p(o), _p(d_o), _p(lse), dt_code(qkv.dtype), B, N, heads, dh, _p(dqkv),
                                 _p(dq_ws) if need else None, _stream()), "m3_attention_bwd")


# ---------------------------------------------------------------------- elementwise
def cast_matrix(src, dst, transpose=False):
    """src f32 [G,R,C] or [R,C] -> dst (act dtype) same shape, or [G,C,R] when transpose."""
    if src.dim() not in (2, 3):
        raise _lib.M3Error(f"src must be [G,R,C] or [R,C], got shape {tuple(src.shape)}")
    G = 1 if src.dim() == 2 else src.shape[0]
    R, C = src.shape[-2], src.shape[-1]
    _req(src, torch.float32, "src"); _act(dst, "dst", G * R * C)
    check(lib().m3_cast_matrix(_p(src), G, R, C, 1 if transpose else 0, _p(dst), dt_code(dst.dtype), _stream()),
          "m3_cast_matrix")
    return dst


class CastPlan:
    """Device-resident descriptor table for m3_cast_batch: every (fp32 master -> operand copies) job of a
    model, converted by ONE launch per optimizer step."""

    def __init__(self, jobs, dst_dtype):
        # jobs: list of (src fp32 [.., rows, cols], dst [.., rows, cols] or None, dst_t [.., cols, rows] or None):
        # the plain and / or the transposed copy, both written from one read of src
        arr = (_lib.CastDesc * len(jobs))()
        t0 = 0
        self.keep = []
        for d, job in zip(arr, jobs):
            src, dst, dst_t = job
            _req(src, torch.float32, "src")
            rows, cols = src.shape[-2], src.shape[-1]
            G = src.numel() // (rows * cols)
            for o in (dst, dst_t):
                if o is not None:
                    _req(o, dst_dtype, "dst")
                    assert o.numel() == src.numel()
            assert dst is not None or dst_t is not None
            d.src, d.G, d.rows, d.cols, d.tile_start = src.data_ptr(), G, rows, cols, t0
            d.dst = _p(dst)
            d.dst_t = _p(dst_t)
            t0 += G * ((rows + 31) // 32) * ((cols + 31) // 32)
            self.keep += [src, dst, dst_t]
        self.n, self.total, self.dtype = len(jobs), t0, dst_dtype
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(jobs[0][0].device)

    def run(self):
        check(lib().m3_cast_batch(_p(self.table), self.n, self.total, dt_code(self.dtype), _stream()), "m3_cast_batch")


def add_f32(dst, src):
    """dst += src (flat fp32 buffers)."""
    _req(dst, torch.float32, "dst"); _req(src, torch.float32, "src", dst.numel())
    check(lib().m3_add_f32(_p(dst), _p(src), dst.numel(), _stream()), "m3_add_f32")
    return dst


# ------------------------------------------------------------------------ optimizer
OPTIM_KINDS = {"adamw": _lib.M3_OPTIM_ADAMW, "adam": _lib.M3_OPTIM_ADAM, "sgd": _lib.M3_OPTIM_SGD}


def optim_table(rows):
    """host half of the descriptor table of m3_optim_prepare / m3_optim_step: rows = [(p_ptr, g_ptr, m_ptr, v_ptr or 0, n,
    group)] -> (ctypes array of m3_optim_desc, total_chunks).  chunk_start is the running sum of ceil(n / 4096); vec_ok is
    set when every pointer of the row is 16-byte aligned (the 16-byte path), else the row takes the scalar path."""
    arr = (_lib.OptimDesc * len(rows))()
    c0 = 0
    for d, (pp, pg, pm, pv, n, group) in zip(arr, rows):
        if n < 1:
            raise _lib.M3Error("an optimizer descriptor needs at least one element")
        d.p, d.g, d.m, d.v, d.n, d.group, d.chunk_start = pp, pg, pm, pv or None, n, group, c0
        d.vec_ok = int(all(q % 16 == 0 for q in (pp, pg, pm, pv or 0)))
        c0 += -(-n // _lib.M3_OPTIM_CHUNK)
    if c0 >= 2 ** 31:
        raise _lib.M3Error("too many optimizer chunks for one launch")
    return arr, c0


def optim_hyper_row(lr, beta1=0.0, beta2=0.0, eps=0.0, weight_decay=0.0, decoupled=False, nesterov=False):
    """one row of the fp32 [groups][8] hyper-parameter table: lr, beta1 (SGD: momentum), beta2, eps, weight_decay, flags,
    and the low halves of beta1 / beta2 (beta = fp32 hi + fp32 lo carries the Python double to the device)"""
    import struct
    f32 = lambda x: struct.unpack("f", struct.pack("f", x))[0]                 # noqa: E731
    b1, b2 = float(beta1), float(beta2)
    flags = (_lib.M3_OPTIM_DECOUPLED if decoupled else 0) | (_lib.M3_OPTIM_NESTEROV if nesterov else 0)
    return (float(lr), f32(b1), f32(b2), float(eps), float(weight_decay), float(flags), b1 - f32(b1), b2 - f32(b2))


class OptimPlan:
    """Device-resident tables of the fused optimizer step (m3_optim_prepare, m3_optim_step), analogous to CastPlan: one
    descriptor per parameter tensor, one hyper-parameter row per group, plus the norm partials and the `state` block
    (skip flag, step counter, total_norm, clip_coef, inv_scale and the per-group coefficients) the two calls share.

    entries: [(p, g, m, v or None, group)] fp32 contiguous GPU tensors of equal element counts (v None for SGD);
    state: the state block of an earlier plan over the same groups (keeps the step counter), else a zeroed one is made."""

    def __init__(self, entries, n_groups, kind, state=None):
        if kind not in OPTIM_KINDS:
            raise _lib.M3Error(f"unknown optimizer kind {kind!r}; one of {sorted(OPTIM_KINDS)}")
        if not entries:
            raise _lib.M3Error("OptimPlan needs at least one parameter tensor")
        self.kind, self.n_groups = OPTIM_KINDS[kind], int(n_groups)
        rows, self.keep = [], []
        for p, g, m, v, group in entries:
            n = _req(p, torch.float32, "parameter").numel()
            _req(g, torch.float32, "gradient", n); _req(m, torch.float32, "first-moment / momentum state", n)
            if (v is None) != (kind == "sgd"):
                raise _lib.M3Error("the second-moment state is given for Adam / AdamW and only for them")
            if v is not None:
                _req(v, torch.float32, "second-moment state", n)
            if not 0 <= group < self.n_groups:
                raise _lib.M3Error(f"group {group} outside 0 .. {self.n_groups - 1}")
            rows.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr() if v is not None else 0, n, group))
            self.keep += [p, g, m, v]
        dev = entries[0][0].device
        arr, self.total = optim_table(rows)
        self.n = len(rows)
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        self.hyper = torch.zeros(self.n_groups, _lib.M3_OPTIM_HYPER, dtype=torch.float32, device=dev)
        self.hyper_rows = None
        self.partials = torch.empty(2 * self.total, dtype=torch.float32, device=dev)
        elems = lib().m3_optim_state_elems(self.n_groups)
        if state is not None:
            _req(state, torch.float32, "state", elems)
        self.state = state if state is not None else torch.zeros(elems, dtype=torch.float32, device=dev)

    def set_hyper(self, rows):
        """rows: one optim_hyper_row per group.  Copied to the device (one non-blocking copy from a pinned buffer) only when
        a value differs from what the device table holds."""
        rows = [tuple(r) for r in rows]
        if rows == self.hyper_rows:
            return
        if len(rows) != self.n_groups or any(len(r) != _lib.M3_OPTIM_HYPER for r in rows):
            raise _lib.M3Error(f"the hyper-parameter table is [{self.n_groups}][{_lib.M3_OPTIM_HYPER}]")
        # a fresh pinned buffer per change (torch's host allocator keeps it alive until the copy has run): the previous
        # copy may still be in flight and nothing here waits for the device
        host = torch.tensor(rows, dtype=torch.float64).to(torch.float32).pin_memory()
        self.hyper.copy_(host, non_blocking=True)
        self.hyper_rows = rows

    def prepare(self, grad_scale=None, found_inf=None, max_norm=0.0, want_norm=False):
        """the norm / skip / coefficient half of a step, on the current stream.  grad_scale, found_inf: 1-element fp32 GPU
        tensors or None (what torch.amp.GradScaler.step hands to an optimizer that supports AMP scaling)."""
        if self.hyper_rows is None:
            raise _lib.M3Error("OptimPlan.set_hyper() has not been called")
        for t, name in ((grad_scale, "grad_scale"), (found_inf, "found_inf")):
            if t is not None:
                _req(t, torch.float32, name, 1)
        want = bool(want_norm) or max_norm > 0
        check(lib().m3_optim_prepare(_p(self.table), self.n, self.total, _p(self.hyper), self.n_groups, self.kind,
                                     _p(grad_scale), _p(found_inf), float(max_norm), int(want), _p(self.partials),
                                     _p(self.state), _stream()), "m3_optim_prepare")

    def step(self):
        check(lib().m3_optim_step(_p(self.table), self.n, self.total, _p(self.hyper), _p(self.state), self.kind, _stream()),
              "m3_optim_step")

    # views of the state block (device tensors; reading one is the caller's synchronisation)
    @property
    def skipped(self):
        return self.state[0:1].view(torch.int32)[0]

    @property
    def step_count(self):
        return self.state[1:2].view(torch.int32)[0]

    @property
    def total_norm(self):
        return self.state[2]

    @property
    def clip_coef(self):
        return self.state[3]


# ---------------------------------------------------------------------------- dense-prediction losses (csrc/loss.hip)
LOSS_REC_WORDS = _lib.M3_LOSS_REC_WORDS
_LABEL_DT = {torch.float32: _lib.M3_LABEL_F32, torch.int64: _lib.M3_LABEL_I64, torch.uint8: _lib.M3_LABEL_U8}


def loss_ws_elems(n: int) -> int:
    """fp32 elements of the partials workspace of a loss forward over a pred of n elements (m3_loss_ws_elems)"""
    return int(lib().m3_loss_ws_elems(n))


def loss_layout(pred, name="pred"):
    """(pred as the kernels read it, layout code).  A 4-d CUDA tensor of an activation dtype; NCHW-contiguous and
    channels-last storage are read in place, a pred in neither layout is made NCHW-contiguous (one copy) - the gradient then
    comes back contiguous."""
    if not isinstance(pred, torch.Tensor):
        raise _lib.M3Error(f"{name} must be a tensor, got {type(pred).__name__}")
    if not pred.is_cuda:
        raise _lib.M3Error(f"{name} must live on the GPU (no CPU path)")
    if pred.dim() != 4 or pred.numel() == 0:
        raise _lib.M3Error(f"{name} must be a non-empty [B, C, H, W] tensor, got shape {tuple(pred.shape)}")
    dt_code(pred.dtype)
    if pred.is_contiguous():
        return pred, _lib.M3_LAYOUT_NCHW
    if pred.is_contiguous(memory_format=torch.channels_last):
        return pred, _lib.M3_LAYOUT_NHWC
    return pred.contiguous(), _lib.M3_LAYOUT_NCHW


def _loss_bufs(pred, ws, record):
    need = loss_ws_elems(pred.numel())
    if ws is None:
        ws = torch.empty(need, dtype=torch.float32, device=pred.device)
    _req(ws, torch.float32, "ws", min_numel=need)
    if record is None:
        record = torch.empty(LOSS_REC_WORDS, dtype=torch.int32, device=pred.device)
    _req(record, torch.int32, "record", numel=LOSS_REC_WORDS)
    return ws, record


def _loss_bwd_bufs(pred, layout, record, grad_out, dpred):
    _req(record, torch.int32, "record", numel=LOSS_REC_WORDS)
    _req(grad_out, torch.float32, "grad_out", numel=1)
    fmt = torch.channels_last if layout == _lib.M3_LAYOUT_NHWC else torch.contiguous_format
    if dpred is None:
        dpred = torch.empty_like(pred, memory_format=fmt)
    if not dpred.is_cuda or dpred.dtype != pred.dtype or dpred.shape != pred.shape or not dpred.is_contiguous(memory_format=fmt):
        raise _lib.M3Error(f"dpred must have pred's dtype, shape and layout ({pred.dtype}, {tuple(pred.shape)}), got "
                           f"{dpred.dtype}, {tuple(dpred.shape)}, strides {tuple(dpred.stride())}")
    return dpred


def _class_label(label, pred, name="label"):
    B, C, H, W = pred.shape
    if not isinstance(label, torch.Tensor) or label.dtype not in _LABEL_DT:
        raise _lib.M3Error(f"{name} must be a float32, int64 or uint8 tensor")
    if tuple(label.shape) not in ((B, 1, H, W), (B, H, W)):
        raise _lib.M3Error(f"{name} must be [{B}, 1, {H}, {W}] or [{B}, {H}, {W}], got {tuple(label.shape)}")
    _req(label, name=name, numel=B * H * W)
    if not 2 <= C <= 255:
        raise _lib.M3Error(f"cross-entropy takes 2 <= C <= 255 classes, got {C}")
    return label


def loss_label_like(label, pred, layout, name="label"):
    """an fp32 label of pred's shape, in pred's layout (L1 / BCE read both as one flat span): a label in the other layout is
    copied once - only possible for C > 1, which none of the reference's depth / edge / saliency heads has"""
    if not isinstance(label, torch.Tensor) or not label.is_cuda:
        raise _lib.M3Error(f"{name} must be a GPU tensor (no CPU path)")
    if label.dtype != torch.float32 or label.shape != pred.shape:
        raise _lib.M3Error(f"{name} must be float32 of pred's shape {tuple(pred.shape)}, got {label.dtype} {tuple(label.shape)}")
    fmt = torch.channels_last if layout == _lib.M3_LAYOUT_NHWC else torch.contiguous_format
    return label if label.is_contiguous(memory_format=fmt) else label.contiguous(memory_format=fmt)


def loss_ce_fwd(pred, label, *, lse=None, ws=None, record=None):
    """Pixel-wise softmax cross-entropy (m3_loss_ce_fwd).  pred [B,C,H,W] fp32 / fp16 / bf16, NCHW or channels-last (see
    loss_layout); label [B,1,H,W] or [B,H,W] float32 / int64 / uint8, 255 = ignored.  Returns (record, lse): the int32 record
    (layout: include/m3vit_hip.h) and the per-pixel log-sum-exp [B,H,W] the backward reads.  Nothing is read back."""
    pred, layout = loss_layout(pred)
    B, C, H, W = pred.shape
    _class_label(label, pred)
    ws, record = _loss_bufs(pred, ws, record)
    if lse is None:
        lse = torch.empty(B, H, W, dtype=torch.float32, device=pred.device)
    _req(lse, torch.float32, "lse", numel=B * H * W)
    check(lib().m3_loss_ce_fwd(_p(pred), dt_code(pred.dtype), _p(label), _LABEL_DT[label.dtype], B, C, H, W, layout, _p(lse),
                               _p(ws), _p(record), _stream()), "m3_loss_ce_fwd")
    return record, lse


def loss_ce_bwd(pred, label, lse, record, grad_out, *, dpred=None):
    """d pred of loss_ce_fwd, scaled by the 0-dim float32 GPU tensor grad_out (read on the device); in pred's dtype and layout"""
    pred, layout = loss_layout(pred)
    B, C, H, W = pred.shape
    _class_label(label, pred)
    _req(lse, torch.float32, "lse", numel=B * H * W)
    dpred = _loss_bwd_bufs(pred, layout, record, grad_out, dpred)
    check(lib().m3_loss_ce_bwd(_p(pred), dt_code(pred.dtype), _p(label), _LABEL_DT[label.dtype], _p(lse), _p(record),
                               _p(grad_out), B, C, H, W, layout, _p(dpred), _stream()), "m3_loss_ce_bwd")
    return dpred


def loss_l1_fwd(pred, label, *, ws=None, record=None):
    """Masked L1 (m3_loss_l1_fwd): mean |pred - label| over label != 255.  label: float32 of pred's shape.  Returns record."""
    pred, layout = loss_layout(pred)
    B, C, H, W = pred.shape
    label = loss_label_like(label, pred, layout)
    ws, record = _loss_bufs(pred, ws, record)
    check(lib().m3_loss_l1_fwd(_p(pred), dt_code(pred.dtype), _p(label), B, C, H, W, layout, _p(ws), _p(record), _stream()),
          "m3_loss_l1_fwd")
    return record


def loss_l1_bwd(pred, label, record, grad_out, *, dpred=None):
    pred, layout = loss_layout(pred)
    B, C, H, W = pred.shape
    label = loss_label_like(label, pred, layout)
    dpred = _loss_bwd_bufs(pred, layout, record, grad_out, dpred)
    check(lib().m3_loss_l1_bwd(_p(pred), dt_code(pred.dtype), _p(label), _p(record), _p(grad_out), B, C, H, W, layout,
                               _p(dpred), _stream()), "m3_loss_l1_bwd")
    return dpred


def _normals_label(label, pred):
    if not isinstance(label, torch.Tensor) or not label.is_cuda:
        raise _lib.M3Error("label must be a GPU tensor (no CPU path)")
    if label.dtype != torch.float32 or label.shape != pred.shape:
        raise _lib.M3Error(f"label must be float32 of pred's shape {tuple(pred.shape)}, got {label.dtype} {tuple(label.shape)}")
    if not 1 <= pred.shape[1] <= _lib.M3_LOSS_NORMALS_MAX_C:
        raise _lib.M3Error(f"the normals loss takes 1 <= C <= {_lib.M3_LOSS_NORMALS_MAX_C}, got {pred.shape[1]}")
    if label.is_contiguous():
        return label, _lib.M3_LAYOUT_NCHW
    if label.is_contiguous(memory_format=torch.channels_last):
        return label, _lib.M3_LAYOUT_NHWC
    return label.contiguous(), _lib.M3_LAYOUT_NCHW


def loss_normals_fwd(pred, label, norm=1, *, ws=None, record=None):
    """Normalised normals loss (m3_loss_normals_fwd): t = pred / (|pred|_2 + 1e-12) over C, sum of |t - label| (norm 1) or
    (t - label)^2 (norm 2) over label != 255, / max(n_valid, 1e-6).  pred and label each in either layout.  Returns record."""
    if norm not in (1, 2):
        raise _lib.M3Error(f"norm must be 1 or 2, got {norm}")
    pred, layout = loss_layout(pred)
    B, C, H, W = pred.shape
    label, ll = _normals_label(label, pred)
    ws, record = _loss_bufs(pred, ws, record)
    check(lib().m3_loss_normals_fwd(_p(pred), dt_code(pred.dtype), _p(label), B, C, H, W, layout, ll, norm, _p(ws), _p(record),
                                    _stream()), "m3_loss_normals_fwd")
    return record


def loss_normals_bwd(pred, label, record, grad_out, norm=1, *, dpred=None):
    if norm not in (1, 2):
        raise _lib.M3Error(f"norm must be 1 or 2, got {norm}")
    pred, layout = loss_layout(pred)
    B, C, H, W = pred.shape
    label, ll = _normals_label(label, pred)
    dpred = _loss_bwd_bufs(pred, layout, record, grad_out, dpred)
    check(lib().m3_loss_normals_bwd(_p(pred), dt_code(pred.dtype), _p(label), _p(record), _p(grad_out), B, C, H, W, layout, ll,
                                    norm, _p(dpred), _stream()), "m3_loss_normals_bwd")
    return dpred


def loss_bce_fwd(pred, label, pos_weight=None, *, ws=None, record=None):
    """Balanced binary cross-entropy (m3_loss_bce_fwd), size_average: labels = label >= 0.5, w = pos_weight or, for None,
    n_neg / (n_pos + n_neg) formed on the device.  label: float32 of pred's shape.  Returns record."""
    pred, layout = loss_layout(pred)
    B, C, H, W = pred.shape
    label = loss_label_like(label, pred, layout)
    ws, record = _loss_bufs(pred, ws, record)
    check(lib().m3_loss_bce_fwd(_p(pred), dt_code(pred.dtype), _p(label), B, C, H, W, layout, 0 if pos_weight is None else 1,
                                0.0 if pos_weight is None else float(pos_weight), _p(ws), _p(record), _stream()),
          "m3_loss_bce_fwd")
    return record


def loss_bce_bwd(pred, label, record, grad_out, *, dpred=None):
    pred, layout = loss_layout(pred)
    B, C, H, W = pred.shape
    label = loss_label_like(label, pred, layout)
    dpred = _loss_bwd_bufs(pred, layout, record, grad_out, dpred)
    check(lib().m3_loss_bce_bwd(_p(pred), dt_code(pred.dtype), _p(label), _p(record), _p(grad_out), B, C, H, W, layout,
                                _p(dpred), _stream()), "m3_loss_bce_bwd")
    return dpred


# --------------------------------------------------------------------------------------- task metrics (csrc/meter.hip)
METER_WORDS = {_lib.M3_METER_IOU: _lib.M3_METER_IOU_WORDS, _lib.M3_METER_DEPTH: _lib.M3_METER_DEPTH_WORDS,
               _lib.M3_METER_NORMALS: _lib.M3_METER_NORMALS_WORDS, _lib.M3_METER_SAL: _lib.M3_METER_SAL_WORDS}


def meter_ws_elems(kind: int, n: int, aux: int = 0) -> int:
    """four-byte words of the partials workspace of a meter update over a pred of n elements (m3_meter_ws_elems); aux:
    n_classes for the IoU meter, B for saliency"""
    return int(lib().m3_meter_ws_elems(kind, n, aux))


def meter_state(kind: int, device) -> torch.Tensor:
    """a zeroed accumulator state: int64 words, the double sums among them read through .view(torch.float64)
    (layout: include/m3vit_hip.h, M3_METER_*)"""
    return torch.zeros(METER_WORDS[kind], dtype=torch.int64, device=device)


def _meter_bufs(kind, pred, aux, ws, state):
    need = meter_ws_elems(kind, pred.numel(), aux)
    if need <= 0:
        raise _lib.M3Error(f"no meter of kind {kind} takes a pred of shape {tuple(pred.shape)} (aux {aux})")
    if ws is None:
        ws = torch.empty(need, dtype=torch.int32, device=pred.device)
    _req(ws, torch.int32, "ws", min_numel=need)
    if state is None:
        state = meter_state(kind, pred.device)
    _req(state, torch.int64, "state", numel=METER_WORDS[kind])
    return ws, state


def meter_iou_update(pred, label, n_classes, *, ws=None, state=None):
    """Class-IoU counts (m3_meter_iou_update) ADDED to state: pred [B,C,H,W] raw logits (argmax fused in), label [B,1,H,W] or
    [B,H,W] float32 / int64 / uint8, 255 = ignored.  Returns state.  Nothing is read back."""
    pred, layout = loss_layout(pred)
    B, C, H, W = pred.shape
    _class_label(label, pred)
    if not 1 <= int(n_classes) <= _lib.M3_METER_IOU_BINS:
        raise _lib.M3Error(f"n_classes must be in [1, {_lib.M3_METER_IOU_BINS}], got {n_classes}")
    ws, state = _meter_bufs(_lib.M3_METER_IOU, pred, int(n_classes), ws, state)
    check(lib().m3_meter_iou_update(_p(pred), dt_code(pred.dtype), _p(label), _LABEL_DT[label.dtype], B, C, H, W, layout,
                                    int(n_classes), _p(ws), _p(state), _stream()), "m3_meter_iou_update")
    return state


def meter_depth_update(pred, label, *, ws=None, state=None):
    """Depth sums (m3_meter_depth_update) ADDED to state: over label != 255, (label - p)^2 and (log label - log p)^2 with
    p = max(pred, 1e-9).  label: float32 of pred's shape.  Returns state."""
    pred, layout = loss_layout(pred)
    B, C, H, W = pred.shape
    label = loss_label_like(label, pred, layout)
    ws, state = _meter_bufs(_lib.M3_METER_DEPTH, pred, 0, ws, state)
    check(lib().m3_meter_depth_update(_p(pred), dt_code(pred.dtype), _p(label), B, C, H, W, layout, _p(ws), _p(state), _stream()),
          "m3_meter_depth_update")
    return state


def meter_normals_update(pred, label, *, ws=None, state=None):
    """Angular-error sums and counts (m3_meter_normals_update) ADDED to state: pred [B,3,H,W] raw (normalised in the kernel),
    label float32 [B,3,H,W], each in either layout.  Returns state."""
    pred, layout = loss_layout(pred)
    B, C, H, W = pred.shape
    if C != 3:
        raise _lib.M3Error(f"the normals meter takes C = 3, got {C}")
    label, ll = _normals_label(label, pred)
    ws, state = _meter_bufs(_lib.M3_METER_NORMALS, pred, 0, ws, state)
    check(lib().m3_meter_normals_update(_p(pred), dt_code(pred.dtype), _p(label), B, H, W, layout, ll, _p(ws), _p(state),
                                        _stream()), "m3_meter_normals_update")
    return state


def meter_sal_update(pred, label, *, ws=None, state=None):
    """Saliency (m3_meter_sal_update): per image and threshold jaccard / precision / recall of sigmoid(pred) > t against
    label != 0, ADDED to state's running sums.  pred [B,1,H,W] raw logits, label float32 of pred's shape.  Returns state."""
    pred, layout = loss_layout(pred)
    B, C, H, W = pred.shape
    if C != 1:
        raise _lib.M3Error(f"the saliency meter takes C = 1, got {C}")
    if B > _lib.M3_LOSS_MAX_BLOCKS:
        raise _lib.M3Error(f"the saliency meter takes at most {_lib.M3_LOSS_MAX_BLOCKS} images per update, got {B}")
    label = loss_label_like(label, pred, layout)
    ws, state = _meter_bufs(_lib.M3_METER_SAL, pred, B, ws, state)
    check(lib().m3_meter_sal_update(_p(pred), dt_code(pred.dtype), _p(label), B, H, W, _p(ws), _p(state), _stream()),
          "m3_meter_sal_update")
    return state


# ------------------------------------------------------------------------------- pretraining recipe (csrc/pretrain.hip)
CLS_EVAL_WORDS = _lib.M3_CLS_EVAL_WORDS


def _mix_lam(lam, B):
    if B < 2 or B % 2:
        raise _lib.M3Error(f"mixing pairs sample i with B-1-i: the batch must be even and non-empty, got B = {B}")
    _req(lam, torch.float32, "lam", numel=B)


def mix_batch(x, lam, box, *, out=None, out_dtype=None):
    """Mixup / CutMix of x [B,C,H,W] (float32, contiguous) with its batch-reversed self (m3_mix_batch): lam float32 [B], box
    int32 [B,4] = yl, yh, xl, xh per sample, both on the device; an empty box means Mixup for that sample.  out=None: in place
    (returns x), or with out_dtype a new tensor of that activation dtype; out=x is in place too.  Nothing is read back."""
    B, C, H, W = _dims(x, 4, "x")
    _req(x, torch.float32, "x")
    _mix_lam(lam, B)
    _req(box, torch.int32, "box", numel=4 * B)
    if out is None:
        out = x if out_dtype in (None, torch.float32) else torch.empty_like(x, dtype=out_dtype)
    _act(out, "out", numel=x.numel())
    if out.shape != x.shape:
        raise _lib.M3Error(f"out must have x's shape {tuple(x.shape)}, got {tuple(out.shape)}")
    if out.data_ptr() == x.data_ptr() and out.dtype != torch.float32:
        raise _lib.M3Error("in place only with a float32 output")
    check(lib().m3_mix_batch(_p(x), B, C, H, W, _p(lam), _p(box), _p(out), dt_code(out.dtype), _stream()), "m3_mix_batch")
    return out


def mix_target(label, lam, num_classes, smoothing=0.0, *, out=None, n_bad=None):
    """The dense soft target float32 [B, num_classes] of mix_batch's pairing (m3_mix_target): label int64 [B], lam float32 [B].
    Returns (target, n_bad): n_bad a 1-element int32 device tensor, the labels outside [0, num_classes)."""
    if not isinstance(label, torch.Tensor) or label.dim() != 1:
        raise _lib.M3Error("label must be a 1-d int64 tensor")
    B, C = label.numel(), int(num_classes)
    _req(label, torch.int64, "label")
    _mix_lam(lam, B)
    if C < 1 or B * C >= 2 ** 31 - 2 ** 20:
        raise _lib.M3Error(f"num_classes = {C} with B = {B}: need C >= 1 and B * C < 2^31 - 2^20")
    if not 0.0 <= float(smoothing) <= 1.0:
        raise _lib.M3Error(f"smoothing must be in [0, 1], got {smoothing}")
    if out is None:
        out = torch.empty(B, C, dtype=torch.float32, device=label.device)
    _req(out, torch.float32, "out", numel=B * C)
    if n_bad is None:
        n_bad = torch.empty(1, dtype=torch.int32, device=label.device)
    _req(n_bad, torch.int32, "n_bad", numel=1)
    check(lib().m3_mix_target(_p(label), _p(lam), B, C, float(smoothing), _p(out), _p(n_bad), _stream()), "m3_mix_target")
    return out, n_bad


def softce_ws_elems(B: int) -> int:
    return int(lib().m3_softce_ws_elems(B))


def _softce_args(logits, target, smoothing):
    """(B, C, dense target or None, labels or None) of a soft-target / label-smoothing cross-entropy call"""
    B, C = _dims(logits, 2, "logits")
    _act(logits, "logits")
    if B < 1 or not 1 <= C <= _lib.M3_SOFTCE_MAX_C:
        raise _lib.M3Error(f"logits must be [B >= 1, 1 <= C <= {_lib.M3_SOFTCE_MAX_C}], got {tuple(logits.shape)}")
    if B * C >= 2 ** 31 - 2 ** 20:
        raise _lib.M3Error(f"{B * C} logits: the kernels index with 32 bits")
    if not isinstance(target, torch.Tensor):
        raise _lib.M3Error(f"target must be a tensor, got {type(target).__name__}")
    if not 0.0 <= float(smoothing) <= 1.0:
        raise _lib.M3Error(f"smoothing must be in [0, 1], got {smoothing}")
    if target.dtype == torch.int64:
        if target.dim() != 1:
            raise _lib.M3Error(f"hard labels must be int64 [B], got shape {tuple(target.shape)}")
        _req(target, torch.int64, "target", numel=B)
        return B, C, None, target
    if tuple(target.shape) != (B, C):
        raise _lib.M3Error(f"a dense target must be float32 of the logits' shape {(B, C)}, got {target.dtype} {tuple(target.shape)}")
    _req(target, torch.float32, "target", numel=B * C)
    return B, C, target, None


def loss_softce_fwd(logits, target, smoothing=0.0, *, lse=None, tsum=None, ws=None, record=None):
    """Cross-entropy of logits [B, C] (fp32 / fp16 / bf16) against a dense float32 target [B, C] or int64 labels [B] with a
    smoothing scalar (m3_loss_softce_fwd).  Returns (record, lse, tsum): the int32 record of the dense-prediction losses
    (loss value, 1 / B, bad labels), the rows' log-sum-exp and - for a dense target - their target sums, both for the
    backward.  Nothing is read back."""
    B, C, dense, lab = _softce_args(logits, target, smoothing)
    dev = logits.device
    need = softce_ws_elems(B)
    if ws is None:
        ws = torch.empty(need, dtype=torch.float32, device=dev)
    _req(ws, torch.float32, "ws", min_numel=need)
    if record is None:
        record = torch.empty(LOSS_REC_WORDS, dtype=torch.int32, device=dev)
    _req(record, torch.int32, "record", numel=LOSS_REC_WORDS)
    if lse is None:
        lse = torch.empty(B, dtype=torch.float32, device=dev)
    _req(lse, torch.float32, "lse", numel=B)
    if dense is not None and tsum is None:
        tsum = torch.empty(B, dtype=torch.float32, device=dev)
    if tsum is not None:
        _req(tsum, torch.float32, "tsum", numel=B)
    check(lib().m3_loss_softce_fwd(_p(logits), dt_code(logits.dtype), _p(dense), _p(lab), float(smoothing), B, C, _p(lse),
                                   _p(tsum), _p(ws), _p(record), _stream()), "m3_loss_softce_fwd")
    return record, lse, tsum


def loss_softce_bwd(logits, target, lse, tsum, record, grad_out, smoothing=0.0, *, dlogits=None):
    """d logits of loss_softce_fwd, scaled by the 1-element float32 GPU tensor grad_out (read on the device); in the logits'
    dtype"""
    B, C, dense, lab = _softce_args(logits, target, smoothing)
    _req(lse, torch.float32, "lse", numel=B)
    if dense is not None:
        _req(tsum, torch.float32, "tsum", numel=B)
    _req(record, torch.int32, "record", numel=LOSS_REC_WORDS)
    _req(grad_out, torch.float32, "grad_out", numel=1)
    if dlogits is None:
        dlogits = torch.empty_like(logits)
    _req(dlogits, logits.dtype, "dlogits", numel=B * C)
    check(lib().m3_loss_softce_bwd(_p(logits), dt_code(logits.dtype), _p(dense), _p(lab), float(smoothing), _p(lse),
                                   _p(tsum if dense is not None else None), _p(record), _p(grad_out), B, C, _p(dlogits),
                                   _stream()), "m3_loss_softce_bwd")
    return dlogits


DISTILL_KINDS = {"soft": _lib.M3_DISTILL_SOFT, "hard": _lib.M3_DISTILL_HARD}


def distill_ws_elems(B: int) -> int:
    return int(lib().m3_distill_ws_elems(B))


def _distill_args(logits, teacher, kind, tau):
    """(B, C, kind code) of a distillation-loss call; teacher None: not read (the hard backward)"""
    B, C = _dims(logits, 2, "logits")
    _act(logits, "logits")
    if B < 1 or not 1 <= C <= _lib.M3_SOFTCE_MAX_C:
        raise _lib.M3Error(f"logits must be [B >= 1, 1 <= C <= {_lib.M3_SOFTCE_MAX_C}], got {tuple(logits.shape)}")
    if B * C >= 2 ** 31 - 2 ** 20:
        raise _lib.M3Error(f"{B * C} logits: the kernels index with 32 bits")
    if kind not in DISTILL_KINDS:
        raise _lib.M3Error(f"kind must be 'soft' or 'hard', got {kind!r}")
    if kind == "soft" and not (0.0 < float(tau) < math.inf):
        raise _lib.M3Error(f"tau must be positive and finite, got {tau}")
    if teacher is not None:
        if not isinstance(teacher, torch.Tensor) or tuple(teacher.shape) != (B, C):
            raise _lib.M3Error(f"teacher logits must have the student's shape {(B, C)}, got "
                               f"{tuple(teacher.shape) if isinstance(teacher, torch.Tensor) else type(teacher).__name__}")
        _act(teacher, "teacher", B * C)
        if teacher.device != logits.device:
            raise _lib.M3Error(f"teacher logits live on {teacher.device}, the student's on {logits.device}")
    return B, C, DISTILL_KINDS[kind]


def loss_distill_fwd(logits, teacher, kind, tau=1.0, *, lse=None, aux=None, ws=None, record=None):
    """The teacher term of the distillation loss (m3_loss_distill_fwd): student logits [B, C] and teacher logits [B, C], each
    fp32 / fp16 / bf16; kind "soft" (KL at temperature tau, scaled tau^2 / (B C)) or "hard" (cross-entropy against the
    teacher's argmax).  Returns (record, lse, aux): the int32 loss record, the student rows' log-sum-exp and the teacher's
    side per row (int32 words: the bits of its float32 lse, soft; its argmax, hard), both for the backward."""
    B, C, code = _distill_args(logits, teacher, kind, tau)
    if teacher is None:
        raise _lib.M3Error("teacher logits are required")
    dev = logits.device
    need = distill_ws_elems(B)
    if ws is None:
        ws = torch.empty(need, dtype=torch.float32, device=dev)
    _req(ws, torch.float32, "ws", min_numel=need)
    if record is None:
        record = torch.empty(LOSS_REC_WORDS, dtype=torch.int32, device=dev)
    _req(record, torch.int32, "record", numel=LOSS_REC_WORDS)
    if lse is None:
        lse = torch.empty(B, dtype=torch.float32, device=dev)
    _req(lse, torch.float32, "lse", numel=B)
    if aux is None:
        aux = torch.empty(B, dtype=torch.int32, device=dev)
    _req(aux, torch.int32, "aux", numel=B)
    check(lib().m3_loss_distill_fwd(_p(logits), dt_code(logits.dtype), _p(teacher), dt_code(teacher.dtype), code, float(tau), B, C,
                                    _p(lse), _p(aux), _p(ws), _p(record), _stream()), "m3_loss_distill_fwd")
    return record, lse, aux


def loss_distill_bwd(logits, teacher, kind, lse, aux, record, grad_out, tau=1.0, *, dlogits=None):
    """d logits of loss_distill_fwd, scaled by the 1-element float32 GPU tensor grad_out (read on the device); in the logits'
    dtype.  teacher may be None for kind "hard" (the argmax in aux is all that is read of it)."""
    B, C, code = _distill_args(logits, teacher, kind, tau)
    if teacher is None and kind == "soft":
        raise _lib.M3Error("teacher logits are required for kind 'soft'")
    _req(lse, torch.float32, "lse", numel=B)
    _req(aux, torch.int32, "aux", numel=B)
    _req(record, torch.int32, "record", numel=LOSS_REC_WORDS)
    _req(grad_out, torch.float32, "grad_out", numel=1)
    if dlogits is None:
        dlogits = torch.empty_like(logits)
    _req(dlogits, logits.dtype, "dlogits", numel=B * C)
    tdt = dt_code(teacher.dtype) if teacher is not None else dt_code(logits.dtype)
    check(lib().m3_loss_distill_bwd(_p(logits), dt_code(logits.dtype), _p(teacher), tdt, code, float(tau), _p(lse), _p(aux),
                                    _p(record), _p(grad_out), B, C, _p(dlogits), _stream()), "m3_loss_distill_bwd")
    return dlogits


def cls_eval_ws_elems(B: int) -> int:
    return int(lib().m3_cls_eval_ws_elems(B))


def cls_eval_state(device) -> torch.Tensor:
    """a zeroed evaluation state: int64 words; the first four read through .view(torch.float64) are loss_sum, correct1,
    correct5, count, the fifth counts the bad labels (layout: include/m3vit_hip.h, M3_CLS_EVAL_*)"""
    return torch.zeros(CLS_EVAL_WORDS, dtype=torch.int64, device=device)


def cls_eval_update(logits, label, *, ws=None, state=None):
    """One batch of classification evaluation ADDED to state (m3_cls_eval_update): logits [B, C] fp32 / fp16 / bf16, label
    int64 [B].  Returns state.  Nothing is read back."""
    B, C, _, lab = _softce_args(logits, label, 0.0)
    if lab is None:
        raise _lib.M3Error("label must be int64 [B]")
    need = cls_eval_ws_elems(B)
    if ws is None:
        ws = torch.empty(need, dtype=torch.int32, device=logits.device)
    _req(ws, torch.int32, "ws", min_numel=need)
    if state is None:
        state = cls_eval_state(logits.device)
    _req(state, torch.int64, "state", numel=CLS_EVAL_WORDS)
    check(lib().m3_cls_eval_update(_p(logits), dt_code(logits.dtype), _p(lab), B, C, _p(ws), _p(state), _stream()),
          "m3_cls_eval_update")
    return state


def ema_table(pairs):
    """The device-resident descriptor table of m3_ema_update: pairs = [(ema, src)] float32 contiguous GPU tensors of equal
    element counts.  Returns (table uint8 tensor, n_desc, total_chunks); the caller keeps the tensors alive."""
    if not pairs:
        raise _lib.M3Error("ema_table needs at least one (ema, src) pair")
    rows = []
    for e, s in pairs:
        n = _req(e, torch.float32, "ema tensor").numel()
        _req(s, torch.float32, "source tensor", n)
        if e.device != s.device:
            raise _lib.M3Error("an ema tensor and its source must live on the same device")
        rows.append((e.data_ptr(), s.data_ptr(), 0, 0, n, 0))
    arr, total = optim_table(rows)                   # m, v null: p and g alone decide vec_ok
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(pairs[0][0].device), len(rows), total


def ema_update(table, n_desc, total_chunks, decay):
    """ema = decay * ema + (1 - decay) * src for every pair of an ema_table in one launch; both factors formed here in double"""
    d = float(decay)
    if not 0.0 <= d <= 1.0:
        raise _lib.M3Error(f"decay must be in [0, 1], got {decay}")
    _req(table, torch.uint8, "table", numel=n_desc * ctypes.sizeof(_lib.OptimDesc))
    check(lib().m3_ema_update(_p(table), int(n_desc), int(total_chunks), d, 1.0 - d, _stream()), "m3_ema_update")


# ------------------------------------------------------------------ dense-prediction augmentation (csrc/augment.hip)
AUG_KINDS = {"image": _lib.M3_AUG_IMAGE, "label": _lib.M3_AUG_LABEL, "depth": _lib.M3_AUG_DEPTH, "normals": _lib.M3_AUG_NORMALS}
AUG_MODES = {"nearest": _lib.M3_AUG_NEAREST, "linear": _lib.M3_AUG_LINEAR, "cubic": _lib.M3_AUG_CUBIC}
AUG_BORDERS = {"zero": _lib.M3_AUG_BORDER_ZERO, "replicate": _lib.M3_AUG_BORDER_REPLICATE}
_AUG_SRC_DT = {torch.float32: M3_F32, torch.uint8: _lib.M3_AUG_U8}


def augment_batch(maps, mats, aux, border="zero"):
    """Flip, warp, resize and post-process every map of a raw batch in one launch (m3_augment_batch).  maps: a list of
    (src, dst, kind, mode, quantize, mean, std): src [B,H,W,C] or [B,H,W], float32 or uint8, contiguous; dst [B,C,Ho,Wo]
    contiguous (float32; an image may be float16 / bfloat16); kind, mode and border by name or code; mean / std: three floats
    for an image, None otherwise.  All maps share B, H, W, Ho, Wo.  mats float64 [B,6], aux float32 [B,4], both on the device
    (include/m3vit_hip.h).  What makes no sense (a C that is not the kind's, a cubic class map, more than 8 maps) is refused by
    the library before anything is launched.  Returns the dst tensors."""
    if not maps:
        raise _lib.M3Error("augment_batch needs at least one map")
    arr = (_lib.AugmentDesc * len(maps))()
    shape = None
    for i, (d, (src, dst, kind, mode, quantize, mean, std)) in enumerate(zip(arr, maps)):
        name = f"map {i}"
        if not isinstance(src, torch.Tensor) or src.dim() not in (3, 4) or src.dtype not in _AUG_SRC_DT:
            raise _lib.M3Error(f"{name}: the source must be a float32 or uint8 [B,H,W,C] or [B,H,W] tensor")
        _req(src, name=name + " source")
        B, H, W = src.shape[:3]
        C = src.shape[3] if src.dim() == 4 else 1
        _dims(dst, 4, name + " output")
        _act(dst, name + " output")
        if dst.shape[0] != B or dst.shape[1] != C or dst.device != src.device:
            raise _lib.M3Error(f"{name}: the output must be [{B}, {C}, Ho, Wo] on the source's device, got {tuple(dst.shape)}")
        if shape is None:
            shape = (B, H, W, dst.shape[2], dst.shape[3], src.device)
        elif shape != (B, H, W, dst.shape[2], dst.shape[3], src.device):
            raise _lib.M3Error(f"{name}: all maps of one call share B, H, W, Ho, Wo and the device")
        d.src, d.dst = src.data_ptr(), dst.data_ptr()
        d.kind = AUG_KINDS[kind] if isinstance(kind, str) else int(kind)
        d.mode = AUG_MODES[mode] if isinstance(mode, str) else int(mode)
        d.C, d.src_dtype, d.dst_dtype, d.quantize = C, _AUG_SRC_DT[src.dtype], dt_code(dst.dtype), int(bool(quantize))
        for c in range(3):
            d.mean[c], d.std[c] = (float(mean[c]), float(std[c])) if mean is not None else (0.0, 1.0)
    B, H, W, Ho, Wo, dev = shape
    _req(mats, torch.float64, "mats", numel=6 * B)
    _req(aux, torch.float32, "aux", numel=4 * B)
    if mats.device != dev or aux.device != dev:
        raise _lib.M3Error("mats and aux must live on the maps' device")
    check(lib().m3_augment_batch(arr, len(maps), B, H, W, Ho, Wo, AUG_BORDERS[border] if isinstance(border, str) else int(border),
                                 _p(mats), _p(aux), _stream()), "m3_augment_batch")
    return [m[1] for m in maps]


def cast_f32(src, dst):
    _req(src, torch.float32, "src"); _act(dst, "dst", src.numel())
    check(lib().m3_cast_f32(_p(src), src.numel(), _p(dst), dt_code(dst.dtype), _stream()), "m3_cast_f32")
    return dst


def scale_rows_cast(src, row_scale, div, dst):
    """dst[r, :] = row_scale[r // div] * src[r, :] (src fp32 [rows, cols], dst fp32 / f16)"""
    rows, cols = _dims(src, 2, "src")
    _req(src, torch.float32, "src"); _act(dst, "dst", rows * cols)
    if div < 1:
        raise _lib.M3Error(f"div must be >= 1, got {div}")
    _req(row_scale, torch.float32, "row_scale", min_numel=-(-rows // div))
    check(lib().m3_scale_rows_cast(_p(src), rows, cols, _p(row_scale), div, _p(dst), dt_code(dst.dtype), _stream()),
          "m3_scale_rows_cast")
    return dst


def _nhwc(t, name):
    """t is a [N, C, H, W] tensor in channels-last memory format (its storage is [N, H, W, C])"""
    if t.dim() != 4 or not t.is_contiguous(memory_format=torch.channels_last):
        raise _lib.M3Error(f"{name} must be a 4-d channels-last tensor")
    if not t.is_cuda:
        raise _lib.M3Error(f"{name} must live on the GPU (no CPU path)")
    return t


def relu_up2x_fwd(x, relu=True, out_dtype=None):
    """y = bilinear x2 (align_corners False) of relu(x), channels-last [N, C, H, W] in -> [N, C, 2H, 2W] out (m3_relu_up2x_fwd)"""
    _nhwc(x, "x")
    N, C, H, W = x.shape
    y = torch.empty((N, C, 2 * H, 2 * W), dtype=out_dtype or x.dtype, device=x.device, memory_format=torch.channels_last)
    check(lib().m3_relu_up2x_fwd(_p(x), dt_code(x.dtype), N, H, W, C, 1 if relu else 0, _p(y), dt_code(y.dtype), _stream()),
          "m3_relu_up2x_fwd")
    return y


def relu_up2x_bwd(dy, x, relu=True):
    _nhwc(dy, "dy"); _nhwc(x, "x")
    N, C, H, W = x.shape
    if tuple(dy.shape) != (N, C, 2 * H, 2 * W):
        raise _lib.M3Error(f"dy must be [{N}, {C}, {2 * H}, {2 * W}], got {tuple(dy.shape)}")
    dt_code(dy.dtype)
    dx = torch.empty_like(x, memory_format=torch.channels_last)
    check(lib().m3_relu_up2x_bwd(_p(dy), dt_code(dy.dtype), _p(x), dt_code(x.dtype), N, H, W, C, 1 if relu else 0, _p(dx),
                                 _stream()), "m3_relu_up2x_bwd")
    return dx


# ---- 3 x 3 convolutions of the decoder heads on the GEMM kernels (csrc/conv.hip; include/m3vit_hip.h: m3_conv3x3_*).
# A bordered activation is a contiguous 16-bit tensor [N, H+2, W+2, C] whose border is zero.

def conv3x3_plan(dtype, N, H, W, C, Cout) -> _lib.Conv3x3Plan:
    """m3_conv3x3_plan: .ok / .reason (names: _lib.CONV_REASONS) / .dgrad_ok, the kernel, tile counts and the weight-gradient
    workspace of a [N, C, H, W] -> Cout convolution on the GEMM path.  Host code: launches nothing, needs no GPU."""
    p = _lib.Conv3x3Plan()
    check(lib().m3_conv3x3_plan(dt_code(dtype), N, H, W, C, Cout, byref(p)), "m3_conv3x3_plan")
    return p


_CONV_INDEX = {}


def conv3x3_index(N, H, W, device):
    """the int32 table pixel (n, y, x) -> bordered pixel index, built on the device once per (shape, device)"""
    key = (N, H, W, torch.device(device))
    idx = _CONV_INDEX.get(key)
    if idx is None:
        idx = torch.empty(max(N * H * W, 1), dtype=torch.int32, device=device)
        check(lib().m3_conv3x3_index(N, H, W, _p(idx), _stream()), "m3_conv3x3_index")
        if not torch.cuda.is_current_stream_capturing():
            _CONV_INDEX[key] = idx
    return idx


def _bordered(t, name):
    """(N, H, W, C) of a bordered activation [N, H+2, W+2, C]"""
    N, HB, WB, C = _dims(t, 4, name)
    _req(t, name=name)
    if t.dtype not in (torch.float16, torch.bfloat16):
        raise _lib.M3Error(f"{name} must be float16 or bfloat16, got {t.dtype}")
    if HB < 3 or WB < 3:
        raise _lib.M3Error(f"{name} must be a bordered image [N, H+2, W+2, C], got shape {tuple(t.shape)}")
    return N, HB - 2, WB - 2, C


def pad_border(x, out=None):
    """channels-last [N, C, H, W] (16-bit) -> bordered [N, H+2, W+2, C], the border written as zeros (m3_pad_border_nhwc)"""
    _nhwc(x, "x")
    N, C, H, W = x.shape
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise _lib.M3Error(f"x must be float16 or bfloat16, got {x.dtype}")
    xb = torch.empty((N, H + 2, W + 2, C), dtype=x.dtype, device=x.device) if out is None else out
    _req(xb, x.dtype, "out", numel=N * (H + 2) * (W + 2) * C)
    check(lib().m3_pad_border_nhwc(_p(x), dt_code(x.dtype), N, H, W, C, _p(xb), _stream()), "m3_pad_border_nhwc")
    return xb


def relu_up2x_fwd_bordered(x, relu=True, out=None):
    """bilinear x2 of relu(x), channels-last [N, C, H, W] (16-bit) -> bordered [N, 2H+2, 2W+2, C] (m3_relu_up2x_fwd_bordered).
    out: a bordered buffer whose border is already zero; without it one is allocated and its border zeroed here."""
    _nhwc(x, "x")
    N, C, H, W = x.shape
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise _lib.M3Error(f"x must be float16 or bfloat16, got {x.dtype}")
    if out is None:
        out = torch.empty((N, 2 * H + 2, 2 * W + 2, C), dtype=x.dtype, device=x.device)
        out[:, 0].zero_(); out[:, -1].zero_(); out[:, :, 0].zero_(); out[:, :, -1].zero_()
    _req(out, x.dtype, "out", numel=N * (2 * H + 2) * (2 * W + 2) * C)
    check(lib().m3_relu_up2x_fwd_bordered(_p(x), dt_code(x.dtype), N, H, W, C, 1 if relu else 0, _p(out), _stream()),
          "m3_relu_up2x_fwd_bordered")
    return out


def conv3x3_fwd(xb, w, bias=None, out=None):
    """y [N H W, Cout] = conv3x3(bordered xb [N, H+2, W+2, C], w [Cout, 9 C] in (dy, dx, c) order) (+ bias fp32) - m3_conv3x3_fwd"""
    N, H, W, C = _bordered(xb, "xb")
    Cout = _dims(w, 2, "w")[0]
    _req(w, xb.dtype, "w", numel=Cout * 9 * C)
    if bias is not None:
        _req(bias, torch.float32, "bias", numel=Cout)
    y = torch.empty((N * H * W, Cout), dtype=xb.dtype, device=xb.device) if out is None else out
    _req(y, xb.dtype, "out", numel=N * H * W * Cout)
    check(lib().m3_conv3x3_fwd(_p(xb), dt_code(xb.dtype), N, H, W, C, _p(w), Cout, _p(bias),
                               _p(conv3x3_index(N, H, W, xb.device)), _p(y), _stream()), "m3_conv3x3_fwd")
    return y


def conv3x3_dgrad(dyb, w_flip, out=None):
    """dx [N H W, C] from the bordered dyb [N, H+2, W+2, Cout] and w_flip [C, 9 Cout] = weight.flip(2, 3).permute(1, 2, 3, 0)
    (m3_conv3x3_dgrad)"""
    N, H, W, Cout = _bordered(dyb, "dyb")
    C = _dims(w_flip, 2, "w_flip")[0]
    _req(w_flip, dyb.dtype, "w_flip", numel=C * 9 * Cout)
    dx = torch.empty((N * H * W, C), dtype=dyb.dtype, device=dyb.device) if out is None else out
    _req(dx, dyb.dtype, "out", numel=N * H * W * C)
    check(lib().m3_conv3x3_dgrad(_p(dyb), dt_code(dyb.dtype), N, H, W, C, _p(w_flip), Cout,
                                 _p(conv3x3_index(N, H, W, dyb.device)), _p(dx), _stream()), "m3_conv3x3_dgrad")
    return dx


def conv3x3_wgrad(xb, dy, dw3=None, db=None, ws=None):
    """dw3 fp32 [3, Cout, 3 C] (dw3[dy, co, dx C + c] = d weight[co, c, dy, dx]) and, when db fp32 [Cout] is given, the bias
    gradient, from the bordered xb [N, H+2, W+2, C] and the dense dy [N H W, Cout] (m3_conv3x3_wgrad).  Both are overwritten."""
    N, H, W, C = _bordered(xb, "xb")
    Cout = _dims(dy, 2, "dy")[1]
    _req(dy, xb.dtype, "dy", numel=N * H * W * Cout)
    p = conv3x3_plan(xb.dtype, N, H, W, C, Cout)
    if not p.ok:
        raise _lib.M3Error(f"conv3x3_wgrad: the shape does not take the GEMM path ({_lib.CONV_REASONS[p.reason]})")
    if dw3 is None:
        dw3 = torch.empty((3, Cout, 3 * C), dtype=torch.float32, device=xb.device)
    _req(dw3, torch.float32, "dw3", numel=3 * Cout * 3 * C)
    if db is not None:
        _req(db, torch.float32, "db", numel=Cout)
    if ws is None:
        ws = torch.empty(max(p.wgrad_ws_elems, 4), dtype=torch.float32, device=xb.device)
    _req(ws, torch.float32, "ws", min_numel=p.wgrad_ws_elems)
    check(lib().m3_conv3x3_wgrad(_p(xb), _p(dy), dt_code(xb.dtype), N, H, W, C, Cout, _p(conv3x3_index(N, H, W, xb.device)),
                                 _p(ws), ws.numel(), _p(dw3), _p(db), _stream()), "m3_conv3x3_wgrad")
    return dw3


def im2row(img, P, rows):
    B, Cin, H, W = _dims(img, 4, "img")
    if P < 1 or H % P or W % P:
        raise _lib.M3Error(f"im2row: H, W ({H}, {W}) must be multiples of the patch size {P}")
    _req(img, torch.float32, "img"); _act(rows, "rows", B * (H // P) * (W // P) * Cin * P * P)
    check(lib().m3_im2row(_p(img), B, Cin, H, W, P, _p(rows), dt_code(rows.dtype), _stream()), "m3_im2row")
    return rows


def assemble_tokens(patch, cls, pos, B, np_, D, tokens):
    _req(patch, torch.float32, "patch", B * np_ * D); _req(cls, torch.float32, "cls", D)
    _req(pos, torch.float32, "pos", (np_ + 1) * D); _req(tokens, torch.float32, "tokens", B * (np_ + 1) * D)
    check(lib().m3_assemble_tokens(_p(patch), _p(cls), _p(pos), B, np_, D, _p(tokens), _stream()), "m3_assemble_tokens")
    return tokens


def tokens_bwd(dtok, B, np_, D, dpatch, dpos, dcls, beta=0):
    _req(dtok, torch.float32, "dtok", B * (np_ + 1) * D); _req(dpos, torch.float32, "dpos", (np_ + 1) * D)
    _req(dcls, torch.float32, "dcls", D)
    if dpatch is not None:
        _act(dpatch, "dpatch", B * np_ * D)
    check(lib().m3_tokens_bwd(_p(dtok), B, np_, D, _p(dpatch), dt_code(dpatch.dtype) if dpatch is not None else M3_F32,
                              _p(dpos), _p(dcls), beta, _stream()), "m3_tokens_bwd")


def assemble_tokens2(patch, cls, dist, pos, B, np_, D, tokens):
    """assemble_tokens with two prefix tokens (cls, dist) in front of the patches: a distilled model (m3_assemble_tokens2)"""
    _req(patch, torch.float32, "patch", B * np_ * D); _req(cls, torch.float32, "cls", D); _req(dist, torch.float32, "dist", D)
    _req(pos, torch.float32, "pos", (np_ + 2) * D); _req(tokens, torch.float32, "tokens", B * (np_ + 2) * D)
    check(lib().m3_assemble_tokens2(_p(patch), _p(cls), _p(dist), _p(pos), B, np_, D, _p(tokens), _stream()),
          "m3_assemble_tokens2")
    return tokens


def tokens_bwd2(dtok, B, np_, D, dpatch, dpos, dcls, ddist, beta=0):
    _req(dtok, torch.float32, "dtok", B * (np_ + 2) * D); _req(dpos, torch.float32, "dpos", (np_ + 2) * D)
    _req(dcls, torch.float32, "dcls", D); _req(ddist, torch.float32, "ddist", D)
    if dpatch is not None:
        _act(dpatch, "dpatch", B * np_ * D)
    check(lib().m3_tokens_bwd2(_p(dtok), B, np_, D, _p(dpatch), dt_code(dpatch.dtype) if dpatch is not None else M3_F32,
                               _p(dpos), _p(dcls), _p(ddist), beta, _stream()), "m3_tokens_bwd2")


# ----------------------------------------------------------------------------- token sharing stage (csrc/share.hip)
SHARE_MAX_T, SHARE_MAX_D = _lib.M3_SHARE_MAX_T, _lib.M3_SHARE_MAX_D
SHARE_STAT_WORDS = _lib.M3_SHARE_STAT_WORDS


def _share_tasks(T, what, tmin=2):
    if not tmin <= T <= SHARE_MAX_T:
        raise _lib.M3Error(f"{what}: {T} task tensors; the sharing kernels take {tmin} to {SHARE_MAX_T} tasks")


def _share_rows(ts, P, D, dtype, name, allow_none=False):
    """the table of device addresses of T separate [P, D] task tensors (nothing is stacked or copied)"""
    rows = _lib.ShareRows()
    for t, x in enumerate(ts):
        if x is None and allow_none:
            continue
        _req(x, dtype, f"{name}[{t}]", numel=P * D)
        rows.p[t] = x.data_ptr()
    return rows


def _share_common(xs, w_gate, task_emb, what, tmin=2):
    xs = list(xs)
    _share_tasks(len(xs), what, tmin)
    x0 = _act(xs[0], f"{what}: x[0]")
    D = x0.shape[-1]
    P = x0.numel() // D
    if D % 8 or not 8 <= D <= SHARE_MAX_D:
        raise _lib.M3Error(f"{what}: D={D} must be a multiple of 8 in [8, {SHARE_MAX_D}]")
    Dg = 0 if task_emb is None else task_emb.shape[-1]
    if w_gate is not None:
        _req(w_gate, torch.float32, "w_gate", numel=(D + Dg) * 2)
        if task_emb is not None:
            _req(task_emb, torch.float32, "task_emb", numel=len(xs) * Dg)
    return xs, P, D, Dg


def share_bwd_ws_elems(P, T, D, Dg) -> int:
    return int(lib().m3_share_bwd_ws_elems(P, T, D, Dg))


def share_stage_fwd(xs, w_gate, task_emb, noise, tau, hard, gamma=0.5, eps=1e-6):
    """m3_share_stage_fwd over T separate task tensors [.., D].  task_emb f32 [T, Dg] or None, noise f32 [T, P, 2] or None.
    Returns (ys, shared_x [P, D], bits int64 [P], g f32 [T, P], soft f32 [T, P] or None (soft mode: g is the soft score))."""
    xs, P, D, Dg = _share_common(xs, w_gate, task_emb, "share_stage_fwd")
    T, dt, dev = len(xs), xs[0].dtype, xs[0].device
    if noise is not None:
        _req(noise, torch.float32, "noise", numel=T * P * 2)
    xr = _share_rows(xs, P, D, dt, "x")
    ys = [torch.empty_like(x) for x in xs]
    yr = _share_rows(ys, P, D, dt, "y")
    sx = torch.empty((P, D), dtype=dt, device=dev)
    bits = torch.empty(P, dtype=torch.int64, device=dev)
    g = torch.empty((T, P), dtype=torch.float32, device=dev)
    soft = torch.empty((T, P), dtype=torch.float32, device=dev) if hard else None
    check(lib().m3_share_stage_fwd(byref(xr), dt_code(dt), T, P, D, _p(w_gate), _p(task_emb), Dg, _p(noise), float(tau),
                                   int(bool(hard)), float(gamma), float(eps), byref(yr), _p(sx), _p(bits), _p(g), _p(soft),
                                   _stream()), "m3_share_stage_fwd")
    return ys, sx, bits, g, soft


def share_stage_bwd(xs, w_gate, task_emb, tau, eps, bits, g, soft, sx, dys, d_sx=None, d_g=None, ws=None):
    """m3_share_stage_bwd: (d x_t list, d w_gate [D + Dg, 2], d task_emb [T, Dg] or None).  dys: a list whose None entries
    count as zeros; d_sx dense [P, D] or None; d_g f32 [T, P] or None."""
    xs, P, D, Dg = _share_common(xs, w_gate, task_emb, "share_stage_bwd")
    T, dt, dev = len(xs), xs[0].dtype, xs[0].device
    _req(bits, torch.int64, "shared_bits", numel=P); _req(g, torch.float32, "g", numel=T * P)
    _req(sx, dt, "shared_x", numel=P * D)
    if soft is not None:
        _req(soft, torch.float32, "soft", numel=T * P)
    if d_sx is not None:
        _req(d_sx, dt, "d_shared_x", numel=P * D)
    if d_g is not None:
        _req(d_g, torch.float32, "d_g", numel=T * P)
    xr = _share_rows(xs, P, D, dt, "x")
    dyr = _share_rows(dys, P, D, dt, "dy", allow_none=True)
    dxs = [torch.empty_like(x) for x in xs]
    dxr = _share_rows(dxs, P, D, dt, "dx")
    n_ws = share_bwd_ws_elems(P, T, D, Dg)
    if ws is None:
        ws = torch.empty(max(n_ws, 4), dtype=torch.float32, device=dev)
    _req(ws, torch.float32, "ws", min_numel=n_ws)
    dw = torch.empty((D + Dg, 2), dtype=torch.float32, device=dev)
    demb = torch.empty((T, Dg), dtype=torch.float32, device=dev) if Dg else None
    if P == 0:
        dw.zero_()
        if demb is not None:
            demb.zero_()
    check(lib().m3_share_stage_bwd(byref(xr), dt_code(dt), T, P, D, _p(w_gate), _p(task_emb), Dg, float(tau), float(eps),
                                   _p(bits), _p(g), _p(soft), _p(sx), byref(dyr), _p(d_sx), _p(d_g), byref(dxr), _p(ws),
                                   _p(dw), _p(demb), _stream()), "m3_share_stage_bwd")
    return dxs, dw, demb


def share_predict_fwd(x, w_gate, task_emb, noise, tau, hard):
    """m3_share_predict_fwd: the predictor of one tensor [.., D].  task_emb f32 [Dg] or None, noise f32 [P, 2] or None.
    Returns (g f32 [P], soft f32 [P] or None)."""
    (x,), P, D, Dg = _share_common([x], None, task_emb, "share_predict_fwd", tmin=1)
    _req(w_gate, torch.float32, "w_gate", numel=(D + Dg) * 2)
    if task_emb is not None:
        _req(task_emb, torch.float32, "task_emb", numel=Dg)
    if noise is not None:
        _req(noise, torch.float32, "noise", numel=P * 2)
    g = torch.empty(P, dtype=torch.float32, device=x.device)
    soft = torch.empty(P, dtype=torch.float32, device=x.device) if hard else None
    check(lib().m3_share_predict_fwd(_p(x), dt_code(x.dtype), P, D, _p(w_gate), _p(task_emb), Dg, _p(noise), float(tau),
                                     int(bool(hard)), _p(g), _p(soft), _stream()), "m3_share_predict_fwd")
    return g, soft


def share_predict_bwd(x, w_gate, task_emb, tau, g, soft, d_g, ws=None):
    """m3_share_predict_bwd: (d x, d w_gate, d task_emb [Dg] or None)"""
    (x,), P, D, Dg = _share_common([x], None, task_emb, "share_predict_bwd", tmin=1)
    _req(w_gate, torch.float32, "w_gate", numel=(D + Dg) * 2)
    _req(g, torch.float32, "g", numel=P); _req(d_g, torch.float32, "d_g", numel=P)
    if soft is not None:
        _req(soft, torch.float32, "soft", numel=P)
    dx = torch.empty_like(x)
    n_ws = share_bwd_ws_elems(P, 1, D, Dg)
    if ws is None:
        ws = torch.empty(max(n_ws, 4), dtype=torch.float32, device=x.device)
    _req(ws, torch.float32, "ws", min_numel=n_ws)
    dw = torch.empty((D + Dg, 2), dtype=torch.float32, device=x.device)
    demb = torch.empty(Dg, dtype=torch.float32, device=x.device) if Dg else None
    if P == 0:
        dw.zero_()
        if demb is not None:
            demb.zero_()
    check(lib().m3_share_predict_bwd(_p(x), dt_code(x.dtype), P, D, _p(w_gate), _p(task_emb), Dg, float(tau), _p(g), _p(soft),
                                     _p(d_g), _p(dx), _p(ws), _p(dw), _p(demb), _stream()), "m3_share_predict_bwd")
    return dx, dw, demb


def share_aggregate_fwd(xs, mask_bits, agg_needed, eps=1e-6, want_agg=True):
    """m3_share_aggregate_fwd: (ys, agg [P, D] or None).  mask_bits int64 [P] (bit t: task t's mask), agg_needed bool [P] or
    None (= everywhere)."""
    xs, P, D, _ = _share_common(xs, None, None, "share_aggregate_fwd")
    T, dt, dev = len(xs), xs[0].dtype, xs[0].device
    _req(mask_bits, torch.int64, "mask_bits", numel=P)
    if agg_needed is not None:
        _req(agg_needed, torch.bool, "agg_needed", numel=P)
    xr = _share_rows(xs, P, D, dt, "x")
    ys = [torch.empty_like(x) for x in xs]
    yr = _share_rows(ys, P, D, dt, "y")
    agg = torch.empty((P, D), dtype=dt, device=dev) if want_agg else None
    check(lib().m3_share_aggregate_fwd(byref(xr), dt_code(dt), T, P, D, _p(mask_bits), _p(agg_needed), float(eps), byref(yr),
                                       _p(agg), _stream()), "m3_share_aggregate_fwd")
    return ys, agg


def share_aggregate_bwd(dys, mask_bits, agg_needed, eps=1e-6, d_agg=None):
    """m3_share_aggregate_bwd: the d x_t list from the d y_t list (all given) and d agg (dense or None)"""
    dys, P, D, _ = _share_common(dys, None, None, "share_aggregate_bwd")
    T, dt = len(dys), dys[0].dtype
    _req(mask_bits, torch.int64, "mask_bits", numel=P)
    if agg_needed is not None:
        _req(agg_needed, torch.bool, "agg_needed", numel=P)
    if d_agg is not None:
        _req(d_agg, dt, "d_agg", numel=P * D)
    dyr = _share_rows(dys, P, D, dt, "dy")
    dxs = [torch.empty_like(x) for x in dys]
    dxr = _share_rows(dxs, P, D, dt, "dx")
    check(lib().m3_share_aggregate_bwd(byref(dyr), dt_code(dt), T, P, D, _p(mask_bits), _p(agg_needed), float(eps), _p(d_agg),
                                       byref(dxr), _stream()), "m3_share_aggregate_bwd")
    return dxs


def share_compact(bits, num_tasks, prev_bits=None, want_idx=True):
    """m3_share_compact: (flat_idx int32 [P] ascending then -1, or None; count int32 [1] or None; stats int64
    [M3_SHARE_STAT_WORDS]) of a shared_bits tensor - all on the device, nothing read back."""
    _req(bits, torch.int64, "shared_bits")
    _share_tasks(num_tasks, "share_compact", tmin=1)
    P = bits.numel()
    if prev_bits is not None:
        _req(prev_bits, torch.int64, "prev_shared_bits", numel=P)
    idx = torch.empty(P, dtype=torch.int32, device=bits.device) if want_idx else None
    count = torch.empty(1, dtype=torch.int32, device=bits.device) if want_idx else None
    stats = torch.zeros(SHARE_STAT_WORDS, dtype=torch.int64, device=bits.device)
    check(lib().m3_share_compact(_p(bits), _p(prev_bits), P, num_tasks, _p(idx), _p(count), _p(stats), _stream()),
          "m3_share_compact")
    return idx, count, stats


# ----------------------------------------------------------------------------- token blocks: FFN sublayer (csrc/token_ffn.hip)
TOKEN_FFN_MODES = {"all": _lib.M3_TOKEN_FFN_ALL, "shared": _lib.M3_TOKEN_FFN_SHARED}


def _token_ffn_mode(mode):
    try:
        return TOKEN_FFN_MODES[mode]
    except KeyError:
        raise _lib.M3Error(f"token FFN: mode {mode!r} is neither 'all' nor 'shared'")


def token_ffn_rows_ub(P, T, mode) -> int:
    """the bound on the work rows every buffer and launch is sized by: T * P (mode 'all'), P (mode 'shared')"""
    return int(lib().m3_token_ffn_rows_ub(P, T, _token_ffn_mode(mode)))


class TokenWorkList:
    """Device-resident work list of the token FFN (m3_token_ffn_worklist in include/m3vit_hip.h; no host sync):
    rows i32 [M_ub], slot_of i32 [T + 1, P] (-1: not listed), offsets / tile_starts i32 [2] (group_offsets / tile_starts of a
    grouped GEMM with G = 1), count i32 [1]."""
    __slots__ = ("rows", "slot_of", "offsets", "tile_starts", "count", "M_ub", "P", "T", "mode")


def token_ffn_worklist(bits, T, mode, *, rows=None, slot_of=None, ws=None) -> TokenWorkList:
    """m3_token_ffn_worklist of a shared_bits tensor int64 [P]"""
    _req(bits, torch.int64, "shared_bits")
    _share_tasks(T, "token_ffn_worklist")
    P, dev = bits.numel(), bits.device
    if (T + 1) * P >= 1 << 31:
        raise _lib.M3Error(f"token_ffn_worklist: (T + 1) * B*N = {(T + 1) * P} must stay below 2^31")
    w = TokenWorkList()
    w.P, w.T, w.mode, w.M_ub = P, T, mode, token_ffn_rows_ub(P, T, mode)
    w.rows = torch.empty(w.M_ub, dtype=torch.int32, device=dev) if rows is None else _req(rows, torch.int32, "rows", numel=w.M_ub)
    w.slot_of = (torch.empty((T + 1, P), dtype=torch.int32, device=dev) if slot_of is None
                 else _req(slot_of, torch.int32, "slot_of", numel=(T + 1) * P))
    meta = torch.empty(8, dtype=torch.int32, device=dev)
    w.offsets, w.tile_starts, w.count = meta[0:2], meta[2:4], meta[4:5]
    n_ws = int(lib().m3_token_ffn_list_ws_elems(P, T))
    if ws is None:
        ws = torch.empty(n_ws, dtype=torch.int32, device=dev)
    _req(ws, torch.int32, "ws", min_numel=n_ws)
    check(lib().m3_token_ffn_worklist(_p(bits), P, T, _token_ffn_mode(mode), _p(w.rows), _p(w.slot_of), _p(w.offsets),
                                      _p(w.tile_starts), _p(w.count), _p(ws), _stream()), "m3_token_ffn_worklist")
    return w


def _token_ffn_common(xs, sx, w: TokenWorkList, what):
    xs, P, D, _ = _share_common(xs, None, None, what)
    if len(xs) != w.T or P != w.P:
        raise _lib.M3Error(f"{what}: {len(xs)} task tensors of {P} positions, the work list was built for {w.T} of {w.P}")
    if sx is not None:
        _req(sx, xs[0].dtype, "shared_x", numel=P * D)
    return xs, P, D


def token_ffn_ln_fwd(xs, sx, w: TokenWorkList, gamma, beta, eps=1e-6, *, h=None, mean=None, rstd=None):
    """m3_token_ffn_ln_fwd: (h [M_ub, D] in the activation dtype, mean f32 [M_ub], rstd f32 [M_ub]); rows at and past the
    work list's count are left as they are"""
    xs, P, D = _token_ffn_common(xs, sx, w, "token_ffn_ln_fwd")
    dt, dev = xs[0].dtype, xs[0].device
    _req(gamma, torch.float32, "gamma", numel=D); _req(beta, torch.float32, "beta", numel=D)
    h = torch.empty((w.M_ub, D), dtype=dt, device=dev) if h is None else _req(h, dt, "h", numel=w.M_ub * D)
    mean = torch.empty(w.M_ub, dtype=torch.float32, device=dev) if mean is None else _req(mean, torch.float32, "mean", numel=w.M_ub)
    rstd = torch.empty(w.M_ub, dtype=torch.float32, device=dev) if rstd is None else _req(rstd, torch.float32, "rstd", numel=w.M_ub)
    xr = _share_rows(xs, P, D, dt, "x")
    check(lib().m3_token_ffn_ln_fwd(byref(xr), _p(sx), dt_code(dt), w.T, P, D, _p(w.rows), _p(w.count), w.M_ub, _p(gamma),
                                    _p(beta), float(eps), _p(h), _p(mean), _p(rstd), _stream()), "m3_token_ffn_ln_fwd")
    return h, mean, rstd


def _token_ffn_scales(path_scale, shared_path_scale, P, N, what):
    if N < 1 or P % N:
        raise _lib.M3Error(f"{what}: N={N} tokens per sample must divide B*N={P}")
    if path_scale is not None:
        _req(path_scale, torch.float32, "path_scale", numel=P // N)
    if shared_path_scale is not None:
        _req(shared_path_scale, torch.float32, "shared_path_scale", numel=P)


def token_ffn_scatter_fwd(xs, sx, f, w: TokenWorkList, bits, N, path_scale=None, shared_path_scale=None, *, ys=None):
    """m3_token_ffn_scatter_fwd: the list of y_t.  f [M_ub, D]: the FFN of the work rows; N: tokens per sample (path_scale f32
    [P / N]); shared_path_scale f32 [P]; None = 1."""
    xs, P, D = _token_ffn_common(xs, sx, w, "token_ffn_scatter_fwd")
    dt = xs[0].dtype
    _req(f, dt, "f", numel=w.M_ub * D); _req(bits, torch.int64, "shared_bits", numel=P)
    _token_ffn_scales(path_scale, shared_path_scale, P, N, "token_ffn_scatter_fwd")
    xr = _share_rows(xs, P, D, dt, "x")
    ys = [torch.empty_like(x) for x in xs] if ys is None else ys
    yr = _share_rows(ys, P, D, dt, "y")
    check(lib().m3_token_ffn_scatter_fwd(byref(xr), _p(sx), _p(f), dt_code(dt), w.T, P, N, D, _token_ffn_mode(w.mode),
                                         _p(w.slot_of), _p(bits), _p(path_scale), _p(shared_path_scale), byref(yr), _stream()),
          "m3_token_ffn_scatter_fwd")
    return ys


def token_ffn_gather_bwd(dys, w: TokenWorkList, bits, N, path_scale=None, shared_path_scale=None, *, df=None):
    """m3_token_ffn_gather_bwd: d f [M_ub, D] from the d y_t list; rows at and past the count are left as they are"""
    dys, P, D = _token_ffn_common(dys, None, w, "token_ffn_gather_bwd")
    dt = dys[0].dtype
    _req(bits, torch.int64, "shared_bits", numel=P)
    _token_ffn_scales(path_scale, shared_path_scale, P, N, "token_ffn_gather_bwd")
    df = torch.empty((w.M_ub, D), dtype=dt, device=dys[0].device) if df is None else _req(df, dt, "df", numel=w.M_ub * D)
    dyr = _share_rows(dys, P, D, dt, "dy")
    check(lib().m3_token_ffn_gather_bwd(byref(dyr), dt_code(dt), w.T, P, N, D, _p(w.rows), _p(w.count), w.M_ub, _p(bits),
                                        _p(path_scale), _p(shared_path_scale), _p(df), _stream()), "m3_token_ffn_gather_bwd")
    return df


def token_ffn_bwd_ws_elems(P, D) -> int:
    return int(lib().m3_token_ffn_bwd_ws_elems(P, D))


def token_ffn_scatter_bwd(xs, sx, dys, dh, mean, rstd, w: TokenWorkList, bits, gamma, *, dxs=None, d_sx=None, ws=None):
    """m3_token_ffn_scatter_bwd: (d x_t list, d shared_x [P, D], d gamma f32 [D], d beta f32 [D])"""
    xs, P, D = _token_ffn_common(xs, sx, w, "token_ffn_scatter_bwd")
    dt, dev = xs[0].dtype, xs[0].device
    _req(dh, dt, "dh", numel=w.M_ub * D)
    _req(mean, torch.float32, "mean", numel=w.M_ub); _req(rstd, torch.float32, "rstd", numel=w.M_ub)
    _req(bits, torch.int64, "shared_bits", numel=P); _req(gamma, torch.float32, "gamma", numel=D)
    xr = _share_rows(xs, P, D, dt, "x")
    dyr = _share_rows(list(dys), P, D, dt, "dy")
    dxs = [torch.empty_like(x) for x in xs] if dxs is None else dxs
    dxr = _share_rows(dxs, P, D, dt, "dx")
    d_sx = torch.empty((P, D), dtype=dt, device=dev) if d_sx is None else _req(d_sx, dt, "d_shared_x", numel=P * D)
    n_ws = token_ffn_bwd_ws_elems(P, D)
    if ws is None:
        ws = torch.empty(max(n_ws, 4), dtype=torch.float32, device=dev)
    _req(ws, torch.float32, "ws", min_numel=n_ws)
    dg = torch.empty(D, dtype=torch.float32, device=dev)
    db = torch.empty(D, dtype=torch.float32, device=dev)
    check(lib().m3_token_ffn_scatter_bwd(byref(xr), _p(sx), byref(dyr), _p(dh), _p(mean), _p(rstd), dt_code(dt), w.T, P, D,
                                         _token_ffn_mode(w.mode), _p(w.slot_of), _p(bits), _p(gamma), byref(dxr), _p(d_sx),
                                         _p(ws), _p(dg), _p(db), _stream()), "m3_token_ffn_scatter_bwd")
    return dxs, d_sx, dg, db
