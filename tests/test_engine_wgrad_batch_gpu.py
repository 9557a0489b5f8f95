"""GPU: the engine's batched weight gradients (BackboneEngine._plan_wgrad_batch: one ops.wgrad_multi launch per block backward
for the dense-row weights) against the per-weight path on the same step - one dense and one MoE block at the ViT-S width,
both task passes accumulated, with and without DropPath factors - and the conditions under which the per-weight path stays.
Only the fp32 summation order of the weight gradients differs between the two paths (other row parts), so every parameter
gradient must agree within the fp16 weight-gradient bound of tests/test_wgrad_dma.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-3                                   # relative Frobenius per parameter, fp16
B, TASKS = 2, (0, 1)


def rel(a, b):
    a = a.double().flatten().cpu(); b = b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import ref_torch as R
    # 352 x 368 pixels: 507 tokens, 1014 rows = 32 steps of 32 rows - the smallest at which the plan cuts the rows in two parts
    cfg = R.BackboneCfg(img_size=(352, 368), embed_dim=384, depth=2, num_heads=12, mlp_ratio=4.0, moe_mlp_ratio=1.0,
                        moe_experts=16, moe_top_k=4, gate_dim=386, multi_gate=True)
    P = R.init_backbone_params(cfg, seed=5)
    g = torch.Generator().manual_seed(1)
    img = torch.randn(B, 3, *cfg.img_size, generator=g).cuda()
    dtok = (torch.randn(B, cfg.num_tokens, 384, generator=g) * 0.1).cuda()
    keep = 0.7
    ps = {i: tuple((torch.floor(keep + torch.rand(B, generator=g)) / keep).cuda() for _ in range(2)) for i in range(cfg.depth)}
    return cfg, P, img, dtok, ps


def step(setup, monkeypatch, batch, dtype=torch.float16, drop_path=False, **kw):
    """gradients of one step (both task passes), and the engine"""
    from m3vit_amd.engine import BackboneEngine
    cfg, P, img, dtok, ps = setup
    monkeypatch.setenv("M3_WGRAD_BATCH", "1" if batch else "0")
    eng = BackboneEngine(cfg, P, batch=B, dtype=dtype, **kw)
    eng.zero_grad()
    for task in TASKS:
        eng.forward(img, task, path_scales=ps if drop_path else None)
        eng.backward(dtok, cv_weight=0.01)
    torch.cuda.synchronize()
    return {n: g.clone() for n, g in eng.grads.items()}, eng


_OFF = {}


def per_weight(setup, monkeypatch, drop_path):
    """the per-weight path's gradients: computed once per variant, shared, never written"""
    if drop_path not in _OFF:
        grads, eng = step(setup, monkeypatch, False, drop_path=drop_path)
        assert not eng.wgrad_batched and eng.wgrad_batch_why == "M3_WGRAD_BATCH=0" and eng.wgrad_multi_calls == 0
        _OFF[drop_path] = grads
    return _OFF[drop_path]


@pytest.mark.parametrize("drop_path", [False, True], ids=["plain", "drop-path"])
def test_batched_path_matches_the_per_weight_path(setup, monkeypatch, drop_path):
    want = per_weight(setup, monkeypatch, drop_path)
    got, eng = step(setup, monkeypatch, True, drop_path=drop_path)
    assert eng.wgrad_batched and eng.wgrad_batch_why is None
    assert eng.wgrad_multi_calls == 2 * len(TASKS)                       # one launch per block and pass
    from m3vit_amd import ops
    assert ops.wgrad_multi_plan(eng._wgrad_batch_shapes()["dense"], eng.T, eng.dt).parts == 2
    bad = [(n, rel(got[n], want[n])) for n in want if float(want[n].abs().max()) > 0 and not rel(got[n], want[n]) < TOL]
    assert not bad, bad
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    moved = [n for n in want if ".attn.qkv.weight" in n or ".mlp.fc1.weight" in n]
    assert len(moved) == 3 and all(float(want[n].abs().max()) > 0 for n in moved)


@pytest.mark.parametrize("why,dtype,kw", [("weight-gradient side stream", torch.float16, dict(wgrad_stream=True)),
                                          ("activation checkpointing", torch.float16, dict(checkpoint=True)),
                                          ("refused by m3_wgrad_multi_plan", torch.float32, dict())],
                         ids=["side-stream", "checkpoint", "fp32"])
def test_per_weight_path_stays_where_the_batch_cannot_run(setup, monkeypatch, why, dtype, kw):
    got, eng = step(setup, monkeypatch, True, dtype=dtype, **kw)
    assert not eng.wgrad_batched and eng.wgrad_batch_why == why and eng.wgrad_multi_calls == 0 and eng.s_dx_tb is None
    if dtype == torch.float16:                   # the same step as the forced per-weight path
        want = per_weight(setup, monkeypatch, False)
        bad = [(n, rel(got[n], want[n])) for n in want if float(want[n].abs().max()) > 0 and not rel(got[n], want[n]) < TOL]
        assert not bad, bad


def test_expert_parallel_engines_keep_the_per_weight_path():
    """(the rule itself; the expert-parallel step is run by tests/test_ep_*.py)"""
    from m3vit_amd.engine import BackboneEngine

    class E:
        wg_stream, checkpoint, ep_world, T, dt, D, Hd = None, False, 2, 1014, torch.float16, 384, 1536
    e = E()
    e._wgrad_batch_shapes = lambda: BackboneEngine._wgrad_batch_shapes(e)
    BackboneEngine._plan_wgrad_batch(e)
    assert not e.wgrad_batched and e.wgrad_batch_why == "expert parallelism"
    e.ep_world = 1
    BackboneEngine._plan_wgrad_batch(e)
    assert e.wgrad_batched
