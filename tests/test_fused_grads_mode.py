"""Which gradient delivery the fused module path chooses (VisionTransformerMoE(fused_grads=...), m3vit_amd/fused.py
FusedBackbone.grads_mode) - decided without touching the GPU: "views" by default, "autograd" inside a torch
DistributedDataParallel forward that wraps the model or when a trainable parameter carries a hook, and the per-op path
when autograd delivery meets an expert parallel layer."""
import pytest
import torch

KW = dict(img_size=(32, 32), embed_dim=64, depth=2, num_heads=2, moe_mlp_ratio=1, moe_experts=4, moe_top_k=2, gate_dim=66,
          multi_gate=True)


class FakeCuda(torch.Tensor):                         # (is_cuda is all `unsupported` looks at before the shape)
    is_cuda = True


def test_fused_grads_argument_and_hook_detection():
    from m3vit_amd.fused import FusedBackbone
    from m3vit_amd.vit import VisionTransformerMoE
    m = VisionTransformerMoE(**KW)
    assert m.fused_grads == "auto" and m.fused_grads_used is None
    assert FusedBackbone.grads_mode(m) == "views"
    for mode in ("views", "autograd"):
        assert FusedBackbone.grads_mode(VisionTransformerMoE(fused_grads=mode, **KW)) == mode
    with pytest.raises(AssertionError, match="fused_grads"):
        VisionTransformerMoE(fused_grads="grads", **KW)
    p = m.blocks[1].mlp.gate[1].w_gate
    h = p.register_hook(lambda g: g)
    assert FusedBackbone.grads_mode(m) == "autograd"
    h.remove()
    assert FusedBackbone.grads_mode(m) == "views"
    h = m.pos_embed.register_post_accumulate_grad_hook(lambda t: None)
    assert FusedBackbone.grads_mode(m) == "autograd"
    m.pos_embed.requires_grad_(False)                 # a frozen parameter's hook never fires: it does not count
    assert FusedBackbone.grads_mode(m) == "views"
    m.pos_embed.requires_grad_(True)
    h.remove()
    assert FusedBackbone.grads_mode(m) == "views"


def test_fused_grads_auto_inside_a_torch_ddp_forward():
    """DistributedDataParallel (gloo, one rank, CPU) around a module that holds the backbone: inside its forward the
    backbone asks for autograd delivery, outside it (and inside another model's DDP forward) for views"""
    import torch.distributed as dist
    import torch.nn as nn
    from torch.nn.parallel import DistributedDataParallel
    from m3vit_amd.fused import FusedBackbone
    from m3vit_amd.vit import VisionTransformerMoE

    class Probe(nn.Module):
        def __init__(self, backbone):
            super().__init__()
            self.backbone = backbone
            self.seen, self.target = None, [backbone]     # (a list: not registered as a submodule)

        def forward(self, x):
            self.seen = FusedBackbone.grads_mode(self.target[0])
            return (self.backbone.pos_embed * x).sum()

    dist.init_process_group("gloo", rank=0, world_size=1, store=dist.HashStore())
    try:
        m, other = VisionTransformerMoE(**KW), VisionTransformerMoE(**KW)
        probe = Probe(m)
        ddp = DistributedDataParallel(probe, find_unused_parameters=True)
        ddp(torch.ones(()))
        assert probe.seen == "autograd"
        probe.target[0] = other                       # not wrapped by the active DDP module
        ddp(torch.ones(()))
        assert probe.seen == "views"
        assert FusedBackbone.grads_mode(m) == "views"      # outside the DDP forward
    finally:
        dist.destroy_process_group()


def test_autograd_delivery_with_sharded_experts_takes_the_per_op_path():
    import torch.distributed as dist
    from m3vit_amd.fused import FusedBackbone
    from m3vit_amd.vit import VisionTransformerMoE
    xc = torch.zeros(2, 3, 32, 32).as_subclass(FakeCuda)
    dist.init_process_group("gloo", rank=0, world_size=1, store=dist.HashStore())
    try:
        m = VisionTransformerMoE(world_size=2, **KW)
        assert FusedBackbone.unsupported(m, xc, None, 0, None, "views") is None
        assert FusedBackbone.unsupported(m, xc, None, 0, None) is None
        why = FusedBackbone.unsupported(m, xc, None, 0, None, "autograd")
        assert why is not None and "autograd" in why and "expert parallel" in why
        assert FusedBackbone.unsupported(VisionTransformerMoE(**KW), xc, None, 0, None, "autograd") is None
    finally:
        dist.destroy_process_group()
