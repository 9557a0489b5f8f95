"""GPU: the fused module path (m3vit_amd/fused.py) delivering its parameter gradients THROUGH AUTOGRAD
(VisionTransformerMoE(fused_grads=...)): under torch DistributedDataParallel the way the reference's trainer wraps the model
with --moe_data_distributed (train_fastmoe.py:463,469: DistributedDataParallel(model, device_ids=[local_rank],
find_unused_parameters=True)), with torch.autograd.grad and with parameter hooks - against the per-op module path
(fused=False) on the same weights; and the default .grad-view delivery left as it was."""
import contextlib

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = a.detach().double().cpu().flatten(); b = b.detach().double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


KW = dict(img_size=(32, 48), embed_dim=64, depth=4, num_heads=2, moe_top_k=2, gate_dim=66, multi_gate=True, moe_experts=4)
TOL = 2e-4


def _model(fused="auto", seed=9, **model_kw):
    from m3vit_amd.vit import VisionTransformerMoE
    from oracle import ref_torch as R
    cfg = R.BackboneCfg(mlp_ratio=4.0, moe_mlp_ratio=1.0, vmoe_noisy_std=0.0, **KW)
    m = VisionTransformerMoE(mlp_ratio=4.0, moe_mlp_ratio=1, vmoe_noisy_std=0.0, fused=fused, **KW, **model_kw).cuda()
    m.load_state_dict(R.init_backbone_params(cfg, seed=seed))
    m.train()
    return m, cfg


class Joint(nn.Module):
    """the backbone called once per task inside ONE forward, as heads.MultiTaskModel does (models/models.py:299-320)"""

    def __init__(self, backbone):
        super().__init__()
        self.backbone = backbone

    def forward(self, x, tasks=(0, 1)):
        return [self.backbone(x, task_id=t) for t in tasks]


def _loss(outs, dtok):
    return sum((tok * dtok).sum() + 0.01 * cv for tok, cv in outs)


def _grad(p):
    return torch.zeros_like(p) if p.grad is None else p.grad


def _batch(g, cfg, B=3):
    return torch.randn(B, 3, 32, 48, generator=g).cuda(), (torch.randn(B, cfg.num_tokens, 64, generator=g) * 0.1).cuda()


# ---------------------------------------------------------------------------------------------- two ranks, torch DDP
def _ddp_variant(variant, rank, world):
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel
    m, cfg = _model(use_checkpointing=(variant == "checkpointing"))
    ref, _ = _model(fused=False)
    kw = dict(find_unused_parameters=True)
    if variant == "static_bucket_view":
        kw = dict(find_unused_parameters=False, gradient_as_bucket_view=True)
    w = DistributedDataParallel(Joint(m), device_ids=[0], **kw)
    rj = Joint(ref)
    micro = 3 if variant == "no_sync" else 1
    one_by_one = variant == "one_by_one"
    g = torch.Generator().manual_seed(300 + rank)                    # every rank its own images
    for step in range(3):                                            # eager, hipGraph capture, replay
        batches = [_batch(g, cfg) for _ in range(micro)]
        for p in list(m.parameters()) + list(ref.parameters()):
            p.grad = None                                            # optimizer.zero_grad(set_to_none=True)
        for img, dtok in batches:                                    # per-op, unwrapped: this rank's summed gradients
            for tasks in (((0,), (1,)) if one_by_one else ((0, 1),)):
                _loss(rj(img, tasks), dtok).backward()
        for i, (img, dtok) in enumerate(batches):
            with (w.no_sync() if i < micro - 1 else contextlib.nullcontext()):
                for tasks in (((0,), (1,)) if one_by_one else ((0, 1),)):
                    _loss(w(img, tasks), dtok).backward()
                    assert m.fused_fallback_reason is None, m.fused_fallback_reason
        torch.cuda.synchronize()
        assert m._fused.slots[0].eng.checkpoint == (variant == "checkpointing")
        bad = []
        for (n, p), (_, r) in zip(m.named_parameters(), ref.named_parameters()):
            want = _grad(r).detach().clone()
            dist.all_reduce(want)                                    # (every rank runs all of them before it asserts)
            want /= world
            if p.grad is None or rel(p.grad, want) > TOL:
                bad.append((n, None if p.grad is None else rel(p.grad, want)))
        assert not bad, (variant, step, bad)
        assert m.fused_grads_used == "autograd", m.fused_grads_used
        with torch.no_grad():                                        # an optimizer step: the same on both ranks
            for p, r in zip(m.parameters(), ref.parameters()):
                p.add_(p.grad, alpha=-0.05)
                r.copy_(p)
    fb = m._fused
    assert fb.slots[0].graphs_f and fb.slots[0].graphs_b, "steps 2.. must have replayed hipGraphs"


def _ddp_worker(rank, world, port, q, variants):
    import datetime
    import os
    import traceback
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    # a rank that fails leaves the other one waiting in a collective: that wait ends after two minutes, not gloo's thirty
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    res = []
    try:
        torch.cuda.set_device(0)
        for v in variants:
            try:
                _ddp_variant(v, rank, world)
                res.append((v, "ok"))
            except Exception:
                res.append((v, "FAIL: " + traceback.format_exc()))
                break                                                # (the ranks' collectives no longer match)
    finally:
        q.put((rank, res))
        dist.destroy_process_group()


def _two_ranks(variants):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q, variants)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=480) for _ in procs]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
                p.join(timeout=30)
    for rank, out in res:
        assert [v for v, _ in out] == list(variants) and all(r == "ok" for _, r in out), (rank, out)


def test_torch_ddp_joint_multitask_step_two_ranks_one_gpu():
    """DistributedDataParallel(model, device_ids=[0], find_unused_parameters=True), both task passes in one DDP forward, one
    backward: every parameter's .grad is the rank-mean of the per-op gradients"""
    _need_gpu()
    _two_ranks(["joint"])


def test_torch_ddp_variants_two_ranks_one_gpu():
    """find_unused_parameters=False with gradient_as_bucket_view=True; use_checkpointing=True; one task at a time (a DDP
    forward and backward per task); two micro-batches under no_sync() and a synced one (the gradients handed to autograd
    are accumulated into across backward calls: no executor launch may write them again)"""
    _need_gpu()
    _two_ranks(["static_bucket_view", "checkpointing", "one_by_one", "no_sync"])


# ---------------------------------------------------------------------------------------------- one process, no DDP
def test_autograd_grad_and_post_accumulate_hooks():
    """fused_grads="autograd": torch.autograd.grad(loss, params) gives the per-op gradients (and leaves .grad alone);
    fused_grads="auto" with a post-accumulate-grad hook on every parameter: each hook fires once per parameter and
    backward(), with the per-op gradient"""
    _need_gpu()
    a, cfg = _model(fused_grads="autograd")
    ref, _ = _model(fused=False)
    params, rparams = list(a.parameters()), list(ref.parameters())
    g = torch.Generator().manual_seed(5)
    for step in range(3):
        img, dtok = _batch(g, cfg)
        got = torch.autograd.grad(_loss(Joint(a)(img), dtok), params)
        assert a.fused_fallback_reason is None and a.fused_grads_used == "autograd"
        want = torch.autograd.grad(_loss(Joint(ref)(img), dtok), rparams, allow_unused=True)
        torch.cuda.synchronize()
        assert all(p.grad is None for p in params)
        want = [torch.zeros_like(x) if y is None else y for x, y in zip(got, want)]
        bad = [(n, rel(x, y)) for (n, _), x, y in zip(ref.named_parameters(), got, want) if rel(x, y) > TOL]
        assert not bad, (step, bad)

    h, cfg = _model()
    ref, _ = _model(fused=False)
    seen = {}

    def hook(n):
        def f(p):
            seen.setdefault(n, []).append(p.grad.detach().clone())
        return f
    handles = [p.register_post_accumulate_grad_hook(hook(n)) for n, p in h.named_parameters()]
    for step in range(3):
        img, dtok = _batch(g, cfg)
        seen.clear()
        h.zero_grad(set_to_none=True)
        ref.zero_grad(set_to_none=True)
        _loss(Joint(h)(img), dtok).backward()
        assert h.fused_fallback_reason is None and h.fused_grads_used == "autograd"
        _loss(Joint(ref)(img), dtok).backward()
        torch.cuda.synchronize()
        names = [n for n, _ in h.named_parameters()]
        assert sorted(seen) == sorted(names) and all(len(v) == 1 for v in seen.values()), (step, {n: len(v) for n, v in seen.items()})
        bad = [(n, rel(seen[n][0], _grad(r))) for n, r in ref.named_parameters() if rel(seen[n][0], _grad(r)) > TOL]
        assert not bad, (step, bad)
        assert all(rel(p.grad, seen[n][0]) == 0.0 for n, p in h.named_parameters())
    for x in handles:
        x.remove()
    img, _ = _batch(g, cfg)
    h(img, task_id=0)
    assert h.fused_grads_used == "views"                              # no hook left: back to the .grad views


def test_autograd_delivery_partial_backward_and_frozen_parameters():
    """fused_grads="autograd": a backward over only one of two pending task passes delivers that pass alone (the other task's
    gate gets a zero gradient, not None), the second backward adds the other pass; frozen parameters keep .grad = None"""
    _need_gpu()
    a, cfg = _model(fused_grads="autograd")
    ref, _ = _model(fused=False)
    g = torch.Generator().manual_seed(7)
    for step in range(3):
        img, dtok = _batch(g, cfg)
        a.zero_grad(set_to_none=True)
        ref.zero_grad(set_to_none=True)
        outs = Joint(a)(img)
        routs = Joint(ref)(img)
        for i in (0, 1):
            _loss([outs[i]], dtok).backward()
            _loss([routs[i]], dtok).backward()
            torch.cuda.synchronize()
            bad = [(n, rel(p.grad, _grad(r))) for (n, p), (_, r) in zip(a.named_parameters(), ref.named_parameters())
                   if p.grad is None or rel(p.grad, _grad(r)) > TOL]
            assert not bad, (step, i, bad)
        assert a.fused_fallback_reason is None and a.fused_grads_used == "autograd"
        assert not any(s.busy for s in a._fused.slots)
    gate1 = a.blocks[1].mlp.gate[1].w_gate
    a.zero_grad(set_to_none=True)
    img, dtok = _batch(g, cfg)
    _loss(Joint(a)(img, (0,)), dtok).backward()
    assert gate1.grad is not None and float(gate1.grad.abs().max()) == 0.0
    frozen = [p for n, p in a.named_parameters() if n.startswith("blocks.0.")]
    for p in frozen:
        p.requires_grad_(False)
    a.zero_grad(set_to_none=True)
    _loss(Joint(a)(img), dtok).backward()
    assert all(p.grad is None for p in frozen)
    assert all(p.grad is not None for p in a.parameters() if p.requires_grad)


def test_views_delivery_is_the_default_and_unchanged():
    """a plain model under fused_grads="auto" keeps the .grad-view delivery: its .grad tensors lie inside the executor's
    sum buffer, no parameter is an input of the node"""
    _need_gpu()
    m, cfg = _model()
    g = torch.Generator().manual_seed(11)
    for step in range(3):
        img, dtok = _batch(g, cfg)
        m.zero_grad(set_to_none=True)
        _loss(Joint(m)(img), dtok).backward()
        assert m.fused_fallback_reason is None and m.fused_grads_used == "views"
    fb = m._fused
    lo, hi = fb.gsum.data_ptr(), fb.gsum.data_ptr() + fb.gsum.numel() * fb.gsum.element_size()
    assert all(lo <= p.grad.data_ptr() < hi for p in m.parameters())
    tok, _ = m(img, task_id=0)
    assert tok.grad_fn is not None and not fb.ag_nodes and fb.ag_acc is None      # (autograd delivery registers its nodes)
