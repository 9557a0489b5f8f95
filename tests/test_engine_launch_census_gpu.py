"""GPU: a census of what BackboneEngine launches, tied to the kernel contract tests.

The contract modules (test_contract_gemm / _wgrad / _attention, test_wgrad_multi) check each kernel elementwise against
fp64, at cases chosen per kernel.  This module checks that the cases are the ones the engine needs: it records, at the
C-ABI boundary (the argument struct as `ops` filled it), every m3_gemm_nt, m3_wgrad_tn, m3_wgrad_multi and
m3_attention_fwd / _bwd call of one forward + backward of the engine in BASELINE configs[1], [3] and [4] at their real
widths and token counts (depth 2: one dense and one MoE block; batch 2), multi-gate and task-conditioned, with and
without DropPath factors, with and without activation checkpointing, in fp32, fp16 and bf16; reduces each call to its
signature (launch_signature.py: what the library's plan reports plus the option pattern); plans each call a second time
with its rows scaled to the configuration's benchmarked batch (host code: the kernel choice depends on M); and asserts that
every signature is the signature of a contract case, computed the same way from the contract modules' own tables.

    M3_CENSUS_OUT=<file> python -m pytest tests/test_engine_launch_census_gpu.py -m gpu

also writes the census per configuration (profiles/launch_census.txt is such a file)."""
import os

import pytest
import torch

import launch_signature as ls

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
BATCH = 2
REPORT = {}


def workloads():
    import bench                                               # the benchmarked configurations and their batch sizes
    return {c: (dict(w["cfg"]), w["batch"]) for c, w in bench.WORKLOADS.items()}


def engine_cfg(config, gate):
    """configs[config] with depth 2 (block 0 dense, block 1 MoE); gate: "multi" (one w_gate per task) or "taskcond" (one shared
    gate fed cat(token, task embedding), BASELINE configs[2]'s structure with gate_task_specific_dim 16)"""
    from m3vit_amd.config import BackboneConfig
    kw, bench_batch = workloads()[config]
    kw["depth"] = 2
    D = kw["embed_dim"]
    if gate == "multi":
        kw.update(multi_gate=True, gate_dim=D + 2, gate_task_specific_dim=-1)
    else:
        kw.update(multi_gate=False, gate_dim=D + 2, gate_task_specific_dim=16)
    return BackboneConfig(**kw), bench_batch


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    yield _ops
    out = os.environ.get("M3_CENSUS_OUT")
    if out and REPORT:
        with open(out, "w") as f:
            f.write(render(REPORT))


@pytest.fixture(scope="module")
def contract(ops):
    """the signatures of the contract cases, from the contract modules' tables (dummy structs, host code)"""
    return contract_signatures(ops)


def contract_signatures(ops):
    import test_contract_attention as ca
    import test_contract_gemm as cg
    import test_contract_wgrad as cw
    import test_wgrad_multi as cm
    have = {}
    for cid, (sig, _band) in cg.case_signatures(ops).items():
        have.setdefault(sig, "test_contract_gemm " + cid)
    for cid, sig in cw.case_signatures(ops).items():
        have.setdefault(sig, "test_contract_wgrad " + cid)
    for cid, sig in ca.case_signatures(ops).items():
        have.setdefault(sig, "test_contract_attention " + cid)
    for cid, sig in cm.case_signatures(ops).items():
        have.setdefault(sig, "test_wgrad_multi " + cid)
    return have


_PARAMS = {}


def params(config, gate):
    """one set of parameters per (configuration, gate kind), kept on the device for the variants that use it"""
    from m3vit_amd.config import init_params
    if (config, gate) not in _PARAMS:
        _PARAMS.clear()                                        # (one ViT-Base set at a time: 0.6 GB)
        cfg, _ = engine_cfg(config, gate)
        _PARAMS[(config, gate)] = {n: p.cuda() for n, p in init_params(cfg, seed=3, zero_bias=False).items()}
    return _PARAMS[(config, gate)]


def one_step(ops, config, gate, dtype, drop_path, checkpoint):
    """the recorded calls of one forward + backward"""
    from m3vit_amd.engine import BackboneEngine
    cfg, _ = engine_cfg(config, gate)
    eng = BackboneEngine(cfg, params(config, gate), batch=BATCH, dtype=dtype, checkpoint=checkpoint)
    eng.zero_grad()
    g = torch.Generator().manual_seed(config)
    img = torch.randn(BATCH, 3, *cfg.img_size, generator=g).cuda()
    dtok = (torch.randn(BATCH, cfg.num_tokens, cfg.embed_dim, generator=g) * 0.1).cuda()
    ps = None
    if drop_path:                                             # sample 0 keeps both branches (1 / keep), sample 1 drops them
        ps = {i: (torch.tensor([2.0, 0.0]).cuda(), torch.tensor([0.0, 2.0]).cuda()) for i in range(cfg.depth)}
    with ls.Recorder(ops) as rec:
        eng.forward(img, 0, path_scales=ps)
        eng.backward(dtok, cv_weight=0.01)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in eng.grads.values())
    return rec.calls


VARIANTS = [(dp, ck) for dp in (False, True) for ck in (False, True)]


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("gate", ["multi", "taskcond"])
@pytest.mark.parametrize("config", [1, 3, 4])
def test_every_engine_launch_has_a_contract_case(ops, contract, config, gate, dtype):
    _, bench_batch = engine_cfg(config, gate)
    missing = {}
    for drop_path, checkpoint in VARIANTS:
        calls = one_step(ops, config, gate, dtype, drop_path, checkpoint)
        assert {n for n, _, _ in calls} >= {"m3_gemm_nt", "m3_attention_fwd", "m3_attention_bwd"}
        name = f"configs[{config}] {gate} {ls.DT_NAME[ops.dt_code(dtype)]}" + (" drop_path" if drop_path else "") + (" checkpoint" if checkpoint else "")
        for size, (num, den) in (("batch %d (run)" % BATCH, (1, 1)), ("batch %d (planned)" % bench_batch, (bench_batch, BATCH))):
            cen = ls.census(ops, calls, num, den)
            REPORT[(name, size)] = cen
            for sig in cen:
                if sig not in contract:
                    missing.setdefault(sig, []).append(f"{name}, {size}")
    assert not missing, "launches of the engine without a contract case:\n" + "\n".join(f"  {s}\n      {w[0]} (+{len(w) - 1})" for s, w in missing.items())


def test_recording_changes_nothing(ops):
    """the same step with and without the recorder: the same bits in every gradient"""
    from m3vit_amd.engine import BackboneEngine
    cfg, _ = engine_cfg(1, "multi")
    out = []
    for record in (False, True):
        eng = BackboneEngine(cfg, params(1, "multi"), batch=BATCH, dtype=F16)
        eng.zero_grad()
        g = torch.Generator().manual_seed(1)
        img = torch.randn(BATCH, 3, *cfg.img_size, generator=g).cuda()
        dtok = (torch.randn(BATCH, cfg.num_tokens, cfg.embed_dim, generator=g) * 0.1).cuda()
        if record:
            with ls.Recorder(ops) as rec:
                tok, _ = eng.forward(img, 0)
                eng.backward(dtok, cv_weight=0.01)
            assert len(rec.calls) > 10
        else:
            tok, _ = eng.forward(img, 0)
            eng.backward(dtok, cv_weight=0.01)
        torch.cuda.synchronize()
        out.append((tok.clone(), eng.flat_grads.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def render(report):
    """the census as text: the distinct signatures, numbered, then per configuration and size `launches x signature number`"""
    sigs = sorted({str(s) for cen in report.values() for s in cen})
    num = {s: i + 1 for i, s in enumerate(sigs)}
    lines = ["Launches of one forward + backward of BackboneEngine (depth 2: one dense, one MoE block), as signatures",
             "(tests/launch_signature.py) with their launch counts.  Written by tests/test_engine_launch_census_gpu.py", "",
             f"{len(sigs)} distinct signatures in {len(report)} (configuration, size) entries", ""]
    lines += [f"#{i + 1:<3d} {s}" for i, s in enumerate(sigs)]
    lines += ["", "Per configuration and size (configurations that launch the same are listed together): launches x #signature", ""]
    groups = {}
    for (name, size), cen in report.items():
        groups.setdefault(tuple(sorted((num[str(s)], n) for s, n in cen.items())), []).append(f"{name}, {size}")
    for cen, names in groups.items():
        lines += names
        lines.append("    " + "  ".join(f"{n}x#{i}" for i, n in cen))
        lines.append("")
    return "\n".join(lines)
