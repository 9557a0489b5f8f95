"""GPU parity tests (run with -m gpu on the MI355X box): every HIP kernel, called through
the C ABI (m3vit_amd.ops -> libm3vit_hip.so), against
  * the oracle's C restatement for index/slot work (bit-exact),
  * the committed golden vectors from the reference's pure-torch twins,
  * a plain torch fp64 reference of the same op on the same (dtype-rounded) inputs.
Tolerances: fp32 path 2e-5 relative L2; fp16 storage path 1e-3 relative L2 (north_star:
"outputs within 1e-3 rel-err", bit-exact top-k indices)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16]
TOL = {torch.float32: 2e-5, torch.float16: 1e-3}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    return _ops


def dev():
    return torch.device("cuda:0")


def rel(a, b):
    a = a.double().flatten()
    b = b.double().flatten().to(a.device)
    return float((a - b).norm() / (b.norm() + 1e-30))


def rnd(*shape, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev())


def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / 2 ** 0.5))


def gelu_grad64(x):
    return 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * np.pi) ** 0.5


# ------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(300, 384, 384), (197, 1152, 384), (128, 128, 64), (1000, 384, 1536), (5, 8, 8)])
def test_gemm_dense_plain(ops, dtype, M, N, K):
    A, B = rnd(M, K, dtype=dtype, seed=1), rnd(N, K, dtype=dtype, scale=0.05, seed=2)
    C = torch.full((M, N), float("nan"), dtype=dtype, device=dev())
    ops.gemm_nt(A, B, C)
    ref = A.double() @ B.double().t()
    assert rel(C, ref) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_epilogues(ops, dtype):
    M, N, K = 333, 256, 192
    A, B = rnd(M, K, dtype=dtype, seed=3), rnd(N, K, dtype=dtype, scale=0.08, seed=4)
    bias = rnd(N, seed=5, scale=0.1)
    res = rnd(M, N, seed=6)
    gpre = rnd(M, N, dtype=dtype, seed=7)
    lin = A.double() @ B.double().t() + bias.double()
    # bias + GELU, pre-activation saved
    C = torch.empty(M, N, dtype=dtype, device=dev()); pre = torch.empty_like(C)
    ops.gemm_nt(A, B, C, bias=bias, act=ops.M3_ACT_GELU, pre_out=pre)
    assert rel(pre, lin) < TOL[dtype]
    assert rel(C, gelu64(lin)) < TOL[dtype]
    # bias + residual, fp32 out
    C32 = torch.empty(M, N, dtype=torch.float32, device=dev())
    ops.gemm_nt(A, B, C32, bias=bias, residual=res)
    assert rel(C32, lin + res.double()) < TOL[dtype]
    # dgrad epilogue: * gelu'(pre)
    C2 = torch.empty(M, N, dtype=dtype, device=dev())
    ops.gemm_nt(A, B, C2, gelu_grad_pre=gpre)
    assert rel(C2, (A.double() @ B.double().t()) * gelu_grad64(gpre.double())) < TOL[dtype]


@pytest.mark.parametrize("M,N,K", [(33000, 128, 64), (25216, 384, 96), (32931, 136, 160)])
def test_gemm_f32_tall_tiles(ops, M, N, K):
    """fp32, dense, shapes where 160-row tiles even out the last round (gemm_nt_kernel's MI = 5: m3_gemm_nt picks them when
    ceil(tiles / 256) x tile rows comes out smaller than with 128 rows): every epilogue, a ragged last tile, a partial column
    tile, the two-pass transposed store - the fp32 arithmetic train_fastmoe.py runs (custom_moe_layer.py:32-33)"""
    dtype = torch.float32
    A, B = rnd(M, K, dtype=dtype, seed=3), rnd(N, K, dtype=dtype, scale=0.08, seed=4)
    bias = rnd(N, seed=5, scale=0.1)
    res = rnd(M, N, seed=6)
    gpre = rnd(M, N, dtype=dtype, seed=7)
    lin = A.double() @ B.double().t() + bias.double()
    C = torch.full((M, N), float("nan"), dtype=dtype, device=dev())
    ops.gemm_nt(A, B, C)
    assert rel(C, lin - bias.double()) < TOL[dtype] and bool(torch.isfinite(C).all())
    C = torch.empty(M, N, dtype=dtype, device=dev()); pre = torch.empty_like(C)
    ops.gemm_nt(A, B, C, bias=bias, act=ops.M3_ACT_GELU, pre_out=pre)
    assert rel(pre, lin) < TOL[dtype] and rel(C, gelu64(lin)) < TOL[dtype]
    C32 = res.clone()
    ops.gemm_nt(A, B, C32, bias=bias, residual=C32)                                    # residual in place, as the engine's proj / fc2
    assert rel(C32, lin + res.double()) < TOL[dtype]
    C2 = torch.empty(M, N, dtype=dtype, device=dev())
    ops.gemm_nt(A, B, C2, gelu_grad_pre=gpre)
    assert rel(C2, (lin - bias.double()) * gelu_grad64(gpre.double())) < TOL[dtype]


def _golden(name):
    from conftest import GOLDEN
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


@pytest.mark.parametrize("dtype", DTYPES)
def test_grouped_linear_golden_parallel_linear(ops, dtype):
    """FMoELinear fwd / dgrad / wgrad / bias-grad against the reference's ParallelLinear (g4):
    ragged counts with an empty expert."""
    g = _golden("g4_grouped_linear")
    counts = torch.tensor(g["counts"])
    E = len(counts)
    x = torch.tensor(g["x"]).to(dtype).to(dev())
    W = torch.tensor(g["w_in_out"]).transpose(1, 2).contiguous().to(dtype).to(dev())    # [E,out,in]
    b = torch.tensor(g["b"]).to(dev())
    gy = torch.tensor(g["gy"]).to(dtype).to(dev())
    # routing that yields exactly these expert-major rows
    idx32 = torch.repeat_interleave(torch.arange(E), counts).to(torch.int32).to(dev()).view(-1, 1)
    r = ops.route_build(idx32, E)
    assert r.counts.cpu().tolist() == counts.tolist()
    R, Dout = x.shape[0], W.shape[1]
    y = torch.empty(R, Dout, dtype=dtype, device=dev())
    ops.gemm_nt(x, W, y, M=R, bias=b, group_offsets=r.offsets, tile_starts=r.tile_starts)
    # fp16: the golden comes from fp32 operands, the kernel is given their fp16 roundings - torch on the CPU with the same
    # roundings (operands and output to fp16, fp32 accumulation) sits at 3.6e-4 (y, dx) / 3.0e-4 (dW) / 2.2e-4 (db) of the
    # golden: the 1e-3 bound holds without a factor
    tol = TOL[dtype]
    assert rel(y, torch.tensor(g["y"])) < tol
    # dgrad: dx = gy @ W  (NT with the transposed weight copy)
    Wt = W.transpose(1, 2).contiguous()
    dx = torch.empty_like(x)
    ops.gemm_nt(gy, Wt, dx, M=R, group_offsets=r.offsets, tile_starts=r.tile_starts)
    assert rel(dx, torch.tensor(g["dx"])) < tol
    dW = torch.empty(E, Dout, x.shape[1], dtype=torch.float32, device=dev())
    dbf = torch.empty(E, Dout, dtype=torch.float32, device=dev())
    ops.wgrad_tn(gy, x, dW, M=R, group_offsets=r.offsets, splits=3, db=dbf)
    assert rel(dW, torch.tensor(g["dw_in_out"]).transpose(1, 2)) < tol
    assert rel(dbf, torch.tensor(g["db"])) < tol                       # fused bias grad (empty expert -> zeros)
    db = torch.empty(E, Dout, dtype=torch.float32, device=dev())
    ops.colsum(gy, db, M=R, group_offsets=r.offsets)
    assert rel(db, torch.tensor(g["db"])) < tol


@pytest.mark.parametrize("dtype", DTYPES)
def test_grouped_gemm_gather_scatter(ops, dtype):
    T, k, D, H, E = 700, 4, 384, 384, 16
    g = torch.Generator().manual_seed(11)
    idx = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(torch.int32).to(dev())
    x = rnd(T, D, dtype=dtype, seed=12)
    W = rnd(E, H, D, dtype=dtype, scale=0.05, seed=13)
    b = rnd(E, H, scale=0.1, seed=14)
    r = ops.route_build(idx, E)
    R = T * k
    hid = torch.full((R, H), float("nan"), dtype=dtype, device=dev())
    ops.gemm_nt(x, W, hid, M=R, bias=b, a_row_idx=r.row_of_slot, a_row_div=k, group_offsets=r.offsets,
                tile_starts=r.tile_starts)
    ros = r.row_of_slot.long()
    e_of_slot = idx.flatten().long()[ros]
    ref = torch.einsum("rd,rhd->rh", x.double()[ros // k], W.double()[e_of_slot]) + b.double()[e_of_slot]
    assert rel(hid, ref) < TOL[dtype]
    # token-major scatter of the output
    out = torch.full((R, H), float("nan"), dtype=dtype, device=dev())
    ops.gemm_nt(x, W, out, M=R, bias=b, a_row_idx=r.row_of_slot, a_row_div=k, c_row_idx=r.row_of_slot,
                group_offsets=r.offsets, tile_starts=r.tile_starts)
    ref_tm = torch.empty_like(ref); ref_tm[ros] = ref
    assert rel(out, ref_tm) < TOL[dtype]
    # grouped wgrad with gathers on both operands
    gy = rnd(R, H, dtype=dtype, seed=15)            # token-major grads
    dW = torch.empty(E, H, D, dtype=torch.float32, device=dev())
    ops.wgrad_tn(gy, x, dW, M=R, c_row_idx=r.row_of_slot, a_row_idx=r.row_of_slot, a_row_div=k,
                 group_offsets=r.offsets)
    ref_dw = torch.zeros(E, H, D, dtype=torch.float64, device=dev())
    ref_dw.index_add_(0, idx.flatten().long(), torch.einsum("rh,rd->rhd", gy.double(), x.double().repeat_interleave(k, 0)))
    assert rel(dW, ref_dw) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_expert_backward_takes_the_combine_gradient_unmaterialised(ops, dtype):
    """The backward of the combine bmm(gate_score, moe_outp) (custom_moe_layer.py:298-305) is the row scaling
    d y[t*k+j] = score[t,j] * d out[t].  FC2's input-gradient GEMM and weight-gradient GEMM take it straight from
    d out [T, D]: gathered through the slot -> routed-entry map (div k) and scaled by the entry's score in the GEMM epilogue
    (row_scale_idx) / at the weight-gradient kernel's LDS store (c_row_scale) - against the same products on the
    materialised d y, in fp64."""
    T, k, D, H, E = 650, 4, 384, 384, 16
    g = torch.Generator().manual_seed(31)
    idx = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(torch.int32).to(dev())
    idx[:40] = torch.tensor([0, 1, 2, 3], dtype=torch.int32)                   # ragged groups
    r = ops.route_build(idx, E)
    R = T * k
    ros = r.row_of_slot.long()
    e_of_slot = idx.flatten().long()[ros]
    dout32 = rnd(T, D, seed=32)
    dout = dout32.to(dtype)
    score = torch.rand(T, k, generator=g).to(dev()) * 0.5 + 0.05
    y = rnd(R, D, dtype=dtype, seed=33)
    hid = rnd(R, H, dtype=dtype, seed=34)                                      # expert-major rows
    pre = rnd(R, H, dtype=dtype, seed=35)
    W2t = rnd(E, H, D, dtype=dtype, scale=0.05, seed=36)                       # [E, K = D -> N = H] operand of the dgrad
    # d score only (no d y written)
    dsc = torch.full((T, k), float("nan"), device=dev())
    ops.combine_bwd(dout32, y, score, None, dsc)
    assert rel(dsc, torch.einsum("td,tjd->tj", dout32.double(), y.double().view(T, k, D))) < TOL[dtype]
    dy_tm = (score.double().view(T, k, 1) * dout.double().view(T, 1, D)).view(R, D)       # token-major d y, fp64
    # FC2 input gradient: dhp[m] = gelu'(pre[m]) * score[e(m)] * (dout[t(m)] @ W2[g])
    dhp = torch.full((R, H), float("nan"), dtype=dtype, device=dev())
    ops.gemm_nt(dout, W2t, dhp, M=R, gelu_grad_pre=pre, a_row_idx=r.row_of_slot, a_row_div=k, row_scale=score,
                row_scale_idx=r.row_of_slot, group_offsets=r.offsets, tile_starts=r.tile_starts)
    ref = torch.einsum("rd,rhd->rh", dy_tm[ros], W2t.double()[e_of_slot]) * gelu_grad64(pre.double())
    assert rel(dhp, ref) < TOL[dtype]
    # FC2 weight + bias gradient: dW2[g] = sum_m (score * dout)[m]^T hid[m]
    dW = torch.zeros(E, D, H, device=dev()); db = torch.zeros(E, D, device=dev())
    ops.wgrad_tn(dout, hid, dW, M=R, beta=1, c_row_idx=r.row_of_slot, c_row_div=k, c_row_scale=score,
                 group_offsets=r.offsets, db=db)
    ref_dw = torch.zeros(E, D, H, dtype=torch.float64, device=dev())
    ref_dw.index_add_(0, e_of_slot, torch.einsum("rd,rh->rdh", dy_tm[ros], hid.double()))
    ref_db = torch.zeros(E, D, dtype=torch.float64, device=dev())
    ref_db.index_add_(0, e_of_slot, dy_tm[ros])
    # the factor is applied in the activation dtype (fp16: one extra rounding per element, the one a stored d y has)
    assert rel(dW, ref_dw) < TOL[dtype]
    assert rel(db, ref_db) < max(TOL[dtype], 1e-4)
    # and with a gather on the A side too (the weight gradient of a layer whose input rows are routed copies)
    x = rnd(T, H, dtype=dtype, seed=37)
    dW3 = torch.zeros(E, D, H, device=dev())
    ops.wgrad_tn(dout, x, dW3, M=R, c_row_idx=r.row_of_slot, c_row_div=k, c_row_scale=score, a_row_idx=r.row_of_slot,
                 a_row_div=k, group_offsets=r.offsets)
    ref3 = torch.zeros(E, D, H, dtype=torch.float64, device=dev())
    ref3.index_add_(0, e_of_slot, torch.einsum("rd,rh->rdh", dy_tm[ros], x.double()[ros // k]))
    assert rel(dW3, ref3) < TOL[dtype]


def test_wgrad_queue_rides_the_reduction_on_the_next_launch(ops):
    """ops.WgradQueue: the slab reduction of a weight-gradient call runs as the leading blocks of the NEXT call's launch
    (m3_wgrad_args.prev) and the last one by flush() - dense, dense + bias, balanced grouped + bias with gathers, an empty
    call and a tiny K in one sequence; every result bit-identical to the call that reduces for itself."""
    dt = torch.float16
    T, k, D, H, E = 900, 4, 384, 384, 16
    g = torch.Generator().manual_seed(61)
    idx = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(torch.int32).to(dev())
    r = ops.route_build(idx, E)
    R = T * k
    x = rnd(T, D, dtype=dt, seed=62); dyd = rnd(T, 3 * D, dtype=dt, seed=63); dhp = rnd(R, H, dtype=dt, seed=64)
    dyt = rnd(R, D, dtype=dt, seed=65); hid = rnd(R, H, dtype=dt, seed=66); dl = rnd(T, E, dtype=dt, seed=67)
    calls = [
        dict(dC=dyd, A=x, shape=(3 * D, D), kw=dict()),                                              # qkv-like, no bias
        dict(dC=dyd, A=x, shape=(3 * D, D), kw=dict(), bias=True),
        dict(dC=dhp, A=x, shape=(E, H, D), kw=dict(M=R, a_row_idx=r.row_of_slot, a_row_div=k, group_offsets=r.offsets), bias=True),
        dict(dC=dyt, A=hid, shape=(E, D, H), kw=dict(M=R, c_row_idx=r.row_of_slot, group_offsets=r.offsets), bias=True),
        dict(dC=x, A=dl, shape=(D, E), kw=dict()),                                                   # gate: K = 16
        dict(dC=dyd[:0], A=x[:0], shape=(3 * D, D), kw=dict(M=0), bias=True),                        # empty call
        dict(dC=x, A=x, shape=(D, D), kw=dict(), bias=True),
    ]

    def run(queue):
        outs = []
        for i, c in enumerate(calls):
            dW = rnd(*c["shape"], seed=70 + i)                     # beta = 1 accumulates onto this
            db = rnd(*c["shape"][:-1], seed=90 + i) if c.get("bias") else None
            ops.wgrad_tn(c["dC"], c["A"], dW, beta=1, db=db, queue=queue, **c["kw"])
            outs.append((dW, db))
        if queue is not None:
            # (the last call contracts over few rows: one part per group, so it accumulates into dW itself - direct mode -
            # and leaves nothing pending; with M3_WGRAD_DIRECT=0 its reduction is the one flush() runs)
            import m3vit_amd.ops as O
            assert queue.pending is not None or O._WGRAD_DIRECT
            queue.flush()
            assert queue.pending is None
        torch.cuda.synchronize()
        return outs
    want = run(None)
    need = max(ops.wgrad_launch_plan(c["kw"].get("M", c["dC"].shape[0]), c["shape"][-2], c["shape"][-1],
                              c["shape"][0] if len(c["shape"]) == 3 else 1, dt, grouped="group_offsets" in c["kw"]).ws_elems
               for c in calls)
    got = run(ops.WgradQueue(need, dev()))
    for i, ((w0, b0), (w1, b1)) in enumerate(zip(want, got)):
        assert torch.equal(w0, w1), f"call {i}: dW differs"
        assert b0 is None or torch.equal(b0, b1), f"call {i}: db differs"
    assert float(want[2][0].abs().max()) > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_wgrad_dense_and_colsum(ops, dtype):
    M, N, K = 2000, 384, 256
    dC, A = rnd(M, N, dtype=dtype, seed=21), rnd(M, K, dtype=dtype, seed=22)
    dW = rnd(N, K, seed=23)
    base = dW.clone()
    ops.wgrad_tn(dC, A, dW, beta=1)
    assert rel(dW, base.double() + dC.double().t() @ A.double()) < TOL[dtype]
    db = torch.empty(N, dtype=torch.float32, device=dev())
    ops.colsum(dC, db)
    assert rel(db, dC.double().sum(0)) < TOL[dtype]
    # bias gradient fused into the weight-gradient pass (ones-row MFMA), with accumulation
    dW2 = torch.zeros(N, K, device=dev()); db2 = rnd(N, seed=24); db0 = db2.clone()
    ops.wgrad_tn(dC, A, dW2, beta=1, db=db2)
    assert rel(dW2, dC.double().t() @ A.double()) < TOL[dtype]
    assert rel(db2 - db0, dC.double().sum(0)) < max(TOL[dtype], 1e-4)


# ------------------------------------------------------------------------------ gate
@pytest.mark.parametrize("name", ["g1_gate_e16", "g1_gate_e64", "g2b_gate_noise"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gate_golden(ops, name, dtype):
    from oracle import c_oracle
    g = _golden(name)
    k = int(g["k"])
    x = torch.tensor(g["x"]).to(dtype).to(dev())
    w = torch.tensor(g["w_gate"]).to(dev())
    noise = torch.tensor(g["noise"]).to(dev()) if "noise" in g else None
    std = float(g["std"]) / w.shape[1] if "noise" in g else 0.0
    out = ops.gate_fwd(x, w, k, noise=noise, noise_std=std)
    c = c_oracle.gate_fwd(x.float().cpu().numpy(), g["w_gate"], k, noise=g.get("noise"), std=std)
    assert np.array_equal(out["idx"].cpu().numpy(), c["idx"])            # bit-exact vs the oracle
    assert np.array_equal(out["clean"].cpu().numpy(), c["clean"])        # same fma chain
    np.testing.assert_allclose(out["score"].cpu().numpy(), c["score"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(out["top_logits"].cpu().numpy(), c["top_logits"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(out["gates"].cpu().numpy(), c["gates"], rtol=1e-5, atol=1e-7)
    if dtype == torch.float32:                                           # and vs the reference twin
        assert np.array_equal(out["idx"].cpu().numpy(), g["idx"])
        np.testing.assert_allclose(out["score"].cpu().numpy(), g["score"], rtol=2e-5, atol=1e-7)
    imp = torch.tensor(c["gates"]).sum(0)
    np.testing.assert_allclose(out["importance"].cpu().numpy(), imp.numpy(), rtol=1e-5)
    assert out["load"].cpu().tolist() == (torch.tensor(c["gates"]) > 0).sum(0).tolist()


def test_gate_task_conditioned_bias_form(ops):
    from oracle import c_oracle
    g = _golden("g2_gate_taskcond")
    k = int(g["k"]); D = g["x"].shape[1]
    x = torch.tensor(g["x"]).to(dev())
    w = torch.tensor(g["w_gate"]).to(dev())
    bias_np = c_oracle.gate_fwd(g["tsf"][None, :], g["w_gate"][D:], 1)["clean"][0]
    out = ops.gate_fwd(x, w[:D].contiguous(), k, logit_bias=torch.tensor(bias_np).to(dev()))
    assert np.array_equal(out["idx"].cpu().numpy(), g["idx"])
    np.testing.assert_allclose(out["score"].cpu().numpy(), g["score"], rtol=2e-5, atol=1e-7)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gate_full_size_bit_exact_and_route(ops, dtype):
    """BASELINE config 2 size: T = 128*197 tokens, D = 384, E = 16, k = 4."""
    from oracle import c_oracle
    T, D, E, k = 128 * 197, 384, 16, 4
    x = rnd(T, D, dtype=dtype, seed=31)
    w = (torch.rand(D, E, generator=torch.Generator().manual_seed(32)) - 0.5).mul(0.1).to(dev())
    out = ops.gate_fwd(x, w, k, dense=False)
    c = c_oracle.gate_fwd(x.float().cpu().numpy(), w.cpu().numpy(), k, dense=False)
    assert np.array_equal(out["idx"].cpu().numpy(), c["idx"])
    assert np.array_equal(out["idx32"].cpu().numpy(), c["idx"].astype(np.int32))
    r = ops.route_build(out["idx32"], E, want_counts64=True)
    cc, co, cp, cr = c_oracle.route_build(c["idx"], E)
    assert np.array_equal(r.counts.cpu().numpy(), cc) and np.array_equal(r.counts64.cpu().numpy(), cc)
    assert np.array_equal(r.offsets.cpu().numpy(), co)
    assert np.array_equal(r.pos.cpu().numpy(), cp)
    assert np.array_equal(r.row_of_slot.cpu().numpy(), cr)
    ts = np.concatenate([[0], np.cumsum((cc + 127) // 128)])
    assert np.array_equal(r.tile_starts.cpu().numpy(), ts)
    assert out["load"].cpu().numpy().sum() == T * k
    # the same metadata with the histogram taken inside the gate kernel and the scan riding in the balance launch
    out2 = ops.gate_fwd(x, w, k, dense=False, route=True, want_counts64=True)
    r2 = out2["route"]
    assert r2 is not None and torch.equal(out2["idx"], out["idx"]) and torch.equal(out2["cv_loss"], out["cv_loss"])
    for name in ("counts", "counts64", "offsets", "pos", "row_of_slot", "tile_starts"):
        assert torch.equal(getattr(r2, name), getattr(r, name)), name


@pytest.mark.parametrize("T,E,k", [(1, 4, 2), (63, 8, 1), (64, 8, 8), (65, 16, 4), (777, 64, 4), (4097, 16, 2), (300, 5, 4),
                                   (257, 16, 8)])
def test_gate_route_folded_into_the_gate_and_balance_launches(ops, T, E, k):
    """gate_fwd(route=True): ragged token counts, every k that divides 16, E up to 64, and a routing whose selected
    probabilities underflow to exactly 0 (the LOAD no longer counts those entries, the routing must)."""
    D = 64
    x = rnd(T, D, seed=T)
    w = (torch.rand(D, E, generator=torch.Generator().manual_seed(T + 1)) - 0.5).mul(0.1).to(dev())
    for bias in (None, torch.linspace(0.0, 110.0 * (E - 1), E).to(dev())):              # softmax tail underflows with the second one
        g1 = ops.gate_fwd(x, w, k, logit_bias=bias, dense=True)
        r1 = ops.route_build(g1["idx32"], E, want_counts64=True)
        g2 = ops.gate_fwd(x, w, k, logit_bias=bias, dense=True, route=True, want_counts64=True)
        r2 = g2["route"]
        assert r2 is not None
        for name in ("idx", "score", "gates", "importance", "load", "cv_loss"):
            assert torch.equal(g1[name], g2[name]), name
        for name in ("counts", "counts64", "offsets", "pos", "row_of_slot", "tile_starts"):
            assert torch.equal(getattr(r2, name), getattr(r1, name)), (name, bias is not None)
        if bias is not None and k >= 4 and E >= 16:
            assert int(g1["load"].sum()) < T * k, "the underflow case must actually occur"
    if 16 % 3 != 0:                                                          # k = 3 does not divide 16: no folded route
        assert ops.gate_fwd(x, w, 3 if E >= 3 else 1, route=True)["route"] is None or E < 3


def test_route_edge_cases(ops):
    from oracle import c_oracle
    for n, E in [(1, 4), (255, 3), (1024, 64), (1025, 16), (5000, 1)]:
        idx = torch.randint(0, E, (n, 1), generator=torch.Generator().manual_seed(n)).to(torch.int32)
        if E > 2:
            idx[idx == 1] = 0                      # an empty expert
        r = ops.route_build(idx.to(dev()), E)
        cc, co, cp, cr = c_oracle.route_build(idx.numpy(), E)
        assert np.array_equal(r.counts.cpu().numpy(), cc)
        assert np.array_equal(r.pos.cpu().numpy(), cp)
        assert np.array_equal(r.row_of_slot.cpu().numpy(), cr)


def test_ep_plan_kernel_matches_the_host_plan(ops):
    """m3_ep_plan (device-side expert-parallel exchange plan) against the plain-loop ExchangePlan: split sizes,
    regroup index, expert-major offsets and tile prefix, bit-exact, incl. empty blocks / experts / sources and the
    configs[1] (W = 8, 2 experts per rank, 100 864 rows per rank) and configs[3] (W = 8, 8 per rank) sizes."""
    from m3vit_amd.ep import ExchangePlan
    g = torch.Generator().manual_seed(5)
    cases = [(1, 4, 40), (2, 2, 40), (4, 4, 300), (8, 8, 200), (3, 5, 17), (8, 2, 12608), (8, 8, 1576), (64, 1, 50),
             (16, 40, 30), (64, 64, 12)]          # 640 and 4096 (source, expert) blocks: several per thread of the scan
    for world, e_loc, hi in cases:
        for trial in range(3):
            send = torch.randint(0, hi, (world * e_loc,), generator=g)
            recv = torch.randint(0, hi, (world * e_loc,), generator=g)
            if trial == 1:
                recv.view(world, e_loc)[:, 0] = 0
                recv.view(world, e_loc)[world - 1] = 0
            if trial == 2:
                recv.zero_()
            want = ExchangePlan(send.tolist(), recv.tolist(), world, e_loc)
            buf = torch.full((int(recv.sum()) + 7,), -1, dtype=torch.int32, device=dev())
            got = ops.ep_plan(send.to(dev()), recv.to(dev()), world, e_loc, buf)
            assert got.in_splits == want.in_splits and got.out_splits == want.out_splits and got.n_recv == want.n_recv
            assert got.regroup.cpu().tolist() == want.regroup
            assert buf[got.n_recv:].cpu().tolist() == [-1] * 7                      # nothing written past the plan
            off = np.concatenate([[0], np.cumsum(want.fwd_expert_count)])
            assert np.array_equal(got.offsets.cpu().numpy(), off)
            ts = np.concatenate([[0], np.cumsum((np.asarray(want.fwd_expert_count) + 127) // 128)])
            assert np.array_equal(got.tile_starts.cpu().numpy(), ts)


@pytest.mark.parametrize("world,e_loc,T,k,factor", [(2, 2, 50, 2, 1.5), (4, 4, 300, 4, 1.25), (8, 2, 197, 4, 1.25), (8, 8, 400, 4, 1.1),
                                                    (3, 5, 64, 1, 2.0), (2, 4, 100, 2, 0.6)])
def test_ep_plan_fixed_round_trip_of_a_simulated_exchange(ops, world, e_loc, T, k, factor):
    """m3_ep_plan_fixed (fixed row capacity per (source, destination) pair) on W simulated ranks: every rank routes its own
    tokens, the padded send buffers are exchanged with EQUAL splits (plain indexing stands for the all-to-all), and then
      * every expert-major slot of a rank reads a row that was routed to exactly that local expert, each routed row once,
        sources in rank order inside an expert (the order the exact plan, m3_ep_plan, produces);
      * sending the received rows straight back and un-padding returns every token-major entry its own row;
      * the overflow flag is raised exactly when some pair exceeds the capacity (factor 0.6), and the pairs that fit are
        still exchanged completely."""
    E = world * e_loc
    R = T * k
    cap = -(-int(factor * R + world - 1) // world)
    cap = (cap + 7) // 8 * 8
    g = torch.Generator().manual_seed(world * 100 + T)
    routes, plans, flags, sends = [], [], [], []
    idxs = [torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(torch.int32).to(dev()) for _ in range(world)]
    routes = [ops.route_build(ix, E, want_counts64=True) for ix in idxs]
    cnt = torch.stack([r.counts64 for r in routes]).cpu()                    # [src, global expert]
    over_pairs = set()
    for me in range(world):
        recv = cnt[:, me * e_loc:(me + 1) * e_loc].reshape(-1).contiguous().to(dev())       # [s * e_loc + e]
        flag = torch.zeros(1, dtype=torch.int32, device=dev())
        plans.append(ops.ep_plan_fixed(routes[me].counts64, recv, world, e_loc, cap, routes[me], flag))
        flags.append(int(flag.item()))
        # entry id (rank, token-major entry) as the payload: what x_send would carry
        pad = plans[me].pad_idx.cpu().long()
        sends.append(torch.stack((torch.full_like(pad, me), pad), 1))       # [W * cap, 2]
    pair = cnt.view(world, world, e_loc).sum(2)                              # rows src -> dst
    for me in range(world):
        want_flag = int((pair[me] > cap).any() or (pair[:, me] > cap).any())
        assert flags[me] == want_flag, (me, flags[me], want_flag)
    for me in range(world):
        recv_buf = torch.cat([sends[s][me * cap:(me + 1) * cap] for s in range(world)])      # equal-split all-to-all
        pl = plans[me]
        off = pl.offsets.cpu().tolist()
        rg = pl.regroup.cpu().long()
        ts = pl.tile_starts.cpu().tolist()
        assert ts == [0] + list(np.cumsum([(off[e + 1] - off[e] + 127) // 128 for e in range(e_loc)]))
        for e in range(e_loc):
            rows = recv_buf[rg[off[e]:off[e + 1]]]                           # (src rank, entry) of the slots of local expert e
            ge = me * e_loc + e
            last = (-1, -1)
            for s_, ent in rows.tolist():
                assert int(idxs[s_].view(-1)[ent]) == ge, "a row landed at the wrong expert"
                assert (s_, ent) > last, "sources in rank order, entries in routing order inside a source"
                last = (s_, ent)
            want_n = sum(min(int(cnt[s_, ge]), max(0, cap - int(cnt[s_, me * e_loc:ge].sum()))) for s_ in range(world))
            assert len(rows) == want_n, (me, e, len(rows), want_n)
        # the way back: what this rank received goes home unchanged, the sources un-pad it
    for src in range(world):
        back = torch.cat([torch.cat([sends[src][d * cap:(d + 1) * cap]]) for d in range(world)])   # identity experts
        un = plans[src].unpad_idx.cpu().long()
        got = back[un]                                                        # [R, 2]
        fits = torch.tensor([bool(pair[src, int(idxs[src].view(-1)[i]) // e_loc] <= cap) for i in range(R)])
        assert torch.equal(got[fits, 0], torch.full((int(fits.sum()),), src))
        assert torch.equal(got[fits, 1], torch.arange(R)[fits]), "an entry did not get its own row back"


def test_route_out_of_range_ids_are_reported_and_stay_in_range(ops):
    """expert ids outside [0, E) (a caller error: a wrong E, or offsets applied twice) get no slot; the metadata
    stays inside [0, n) so that consumers gathering through it cannot fault, and Route.check() reports them."""
    from m3vit_amd._lib import M3Error
    n, E = 3000, 8
    idx = torch.randint(0, E, (n,), generator=torch.Generator().manual_seed(3)).to(torch.int32)
    ops.route_build(idx.to(dev()), E).check()                      # all in range: fine
    bad = idx.clone()
    bad[::7] = E + 3
    bad[5::11] = -2
    nbad = int(((bad < 0) | (bad >= E)).sum())
    r = ops.route_build(bad.to(dev()), E)
    assert int(r.offsets[-1]) == n - nbad and int(r.counts.sum()) == n - nbad
    pos, ros = r.pos.cpu(), r.row_of_slot.cpu()
    assert int(pos.min()) >= 0 and int(pos.max()) < n and int(ros.min()) >= 0 and int(ros.max()) < n
    good = (bad >= 0) & (bad < E)
    assert torch.equal(ros[pos[good].long()], torch.arange(n, dtype=torch.int32)[good])      # routed entries: a bijection
    with pytest.raises(M3Error, match="outside"):
        r.check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_gate_backward(ops, dtype):
    T, D, E, k = 1000, 384, 16, 4
    x = rnd(T, D, dtype=dtype, seed=41)
    w = rnd(D, E, scale=0.05, seed=42)
    out = ops.gate_fwd(x, w, k)
    d_score = rnd(T, k, seed=43)
    d_imp = rnd(E, seed=44)
    dl = ops.gate_bwd_logits(out["noisy"], out["idx"], d_score, d_imp, k)
    xr = x.double().requires_grad_()
    wr = w.double().requires_grad_()
    p = torch.softmax(xr @ wr, 1)
    sc = p.gather(1, out["idx"])
    gates = torch.zeros_like(p).scatter(1, out["idx"], sc)
    loss = (sc * d_score.double()).sum() + (gates.sum(0) * d_imp.double()).sum()
    logits = (xr @ wr)
    dl_ref, = torch.autograd.grad(loss, [p], retain_graph=True)
    loss.backward()
    # reference d_logits through softmax
    pd = p.detach()
    dl_ref_logits = pd * (dl_ref - (dl_ref * pd).sum(1, keepdim=True))
    assert rel(dl, dl_ref_logits) < 1e-4
    dw = torch.empty(D, E, dtype=torch.float32, device=dev())
    dx = rnd(T, D, seed=45)
    dx0 = dx.clone()
    ops.gate_bwd_params(x, w, dl, d_w_gate=dw, dx=dx, beta_dx=1)
    assert rel(dw, wr.grad) < 1e-4
    assert rel(dx - dx0, xr.grad) < 1e-4


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,D,E", [(1003, 384, 16), (200, 768, 16), (64, 64, 8), (129, 1024, 5), (77, 260, 16), (300, 384, 64)])
def test_gate_weight_gradient_kernel(ops, dtype, T, D, E):
    """d w_gate (+)= x^T d_logits through m3_gate_bwd_params alone (dx = NULL): the four-columns-per-thread kernel for E <= 16
    (row parities 4 and, for D > 512, 2; ragged last token block; beta = 1 accumulation) and the one-column kernel for E > 16,
    against fp64."""
    x = rnd(T, D, dtype=dtype, seed=46)
    dl = rnd(T, E, seed=47)
    w = rnd(D, E, seed=48)
    dw = rnd(D, E, seed=49)
    dw0 = dw.clone()
    ops.gate_bwd_params(x, w, dl, d_w_gate=dw, beta_dw=1)
    assert rel(dw - dw0, x.double().t() @ dl.double()) < 2e-5
    ops.gate_bwd_params(x, w, dl, d_w_gate=dw, beta_dw=0)
    assert rel(dw, x.double().t() @ dl.double()) < 2e-6


@pytest.mark.parametrize("E,k,T", [(16, 4, 1000), (64, 4, 333), (4, 2, 70), (5, 2, 129)])
def test_balance_loss_count_form(ops, E, k, T):
    """cv_loss = cv^2(gates.sum(0)) + cv^2((gates > 0).sum(0)) (vision_transformer_moe.py:453-459,540)
    and d cv_loss / d importance against the oracle's cv_squared + autograd."""
    from oracle import ref_torch as R
    x = rnd(T, 64, seed=61)
    w = rnd(64, E, scale=0.3, seed=62)
    acc = torch.full((1,), 2.5, device=dev())
    out = ops.gate_fwd(x, w, k, loss_acc=acc)
    gates = out["gates"].double().cpu()
    imp = gates.sum(0).requires_grad_()
    load = R.gates_to_load(gates)
    assert torch.equal(out["load"].cpu(), load)
    assert rel(out["importance"], imp.detach()) < 1e-6
    ref = R.cv_squared(imp) + R.cv_squared(load.double())
    assert abs(float(out["cv_loss"]) - float(ref)) < 1e-5 * max(1.0, float(ref))
    assert abs(float(acc) - 2.5 - float(ref)) < 1e-5 * max(1.0, float(ref))
    ref.backward()
    assert rel(out["d_importance"], imp.grad) < 1e-4
    assert out["d_load_prob"] is None and out["load_prob"] is None


@pytest.mark.parametrize("E,k,T,std", [(16, 4, 1000, 1.0 / 16), (64, 4, 200, 1.0 / 64), (8, 2, 77, 0.5)])
def test_noisy_gate_normal_cdf_load_fwd_bwd(ops, E, k, T, std):
    """Noisy training: load = _prob_in_top_k(clean, noisy, std, top_logits, k).sum(0)
    (vision_transformer_moe.py:33-71,456-457).  Forward value, the balance loss, and d_logits through the
    scores, BOTH thresholds (top_logits[:, k] and [:, k-1] -> softmax) and the direct clean-logit term,
    against float64 autograd over the oracle's functions."""
    from oracle import ref_torch as R
    D = 64
    x = rnd(T, D, seed=71)
    w = rnd(D, E, scale=0.3, seed=72)
    noise = rnd(T, E, seed=73)
    out = ops.gate_fwd(x, w, k, noise=noise, noise_std=std)
    clean = out["clean"].double().cpu().requires_grad_()
    nz = clean + noise.double().cpu() * std
    p = torch.softmax(nz, 1)
    top_logits, top_idx = p.topk(k + 1, dim=1)
    assert torch.equal(top_idx[:, :k], out["idx"].cpu()) and torch.equal(top_idx[:, k].int(), out["idx_next"].cpu())
    score = top_logits[:, :k]
    gates = torch.zeros_like(p).scatter(1, top_idx[:, :k], score)
    imp = gates.sum(0)
    load = R.prob_in_top_k(clean, nz, std, top_logits, k).sum(0)
    assert rel(out["load_prob"], load) < 1e-5
    cv = R.cv_squared(imp) + R.cv_squared(load)
    assert abs(float(out["cv_loss"]) - float(cv)) < 1e-4 * max(1.0, float(cv))
    d_score = rnd(T, k, seed=74)
    d_top = rnd(T, k + 1, seed=75)
    scale = 0.37
    dl = ops.gate_bwd_logits(out["noisy"], out["idx"], d_score, out["d_importance"], k, balance_scale=scale,
                             d_top=d_top, idx_next=out["idx_next"], d_load_prob=out["d_load_prob"],
                             clean=out["clean"], top_logits=out["top_logits"], noise_std=std)
    loss = (score * d_score.double().cpu()).sum() + (top_logits * d_top.double().cpu()).sum() + scale * cv
    loss.backward()
    assert rel(dl, clean.grad) < 2e-4


def test_noisy_balance_loss_against_reference_golden(ops):
    """g6 through the C ABI: m3_gate_fwd (+ Normal-CDF load partials) -> m3_balance_loss -> m3_gate_bwd_logits ->
    m3_gate_bwd_params reproduce the reference gate's own loss and its gradients w.r.t. x and w_gate."""
    g = _golden("g6_balance_noisy")
    k = int(g["k"])
    x = torch.tensor(g["x"]).to(dev()); w = torch.tensor(g["w_gate"]).to(dev()); noise = torch.tensor(g["noise"]).to(dev())
    E = w.shape[1]
    out = ops.gate_fwd(x, w, k, noise=noise, noise_std=float(g["std"]) / E)
    assert np.array_equal(out["idx"].cpu().numpy(), g["idx"])
    assert abs(float(out["cv_loss"]) - float(g["loss"])) < 1e-4 * max(1.0, abs(float(g["loss"])))
    dl = ops.gate_bwd_logits(out["noisy"], out["idx"], None, out["d_importance"], k, balance_scale=1.0,
                             idx_next=out["idx_next"], d_load_prob=out["d_load_prob"], clean=out["clean"],
                             top_logits=out["top_logits"], noise_std=out["noise_std"])
    dw = torch.empty_like(w)
    dx = torch.empty_like(x)
    ops.gate_bwd_params(x, w, dl, d_w_gate=dw, dx=dx)
    assert rel(dx, torch.tensor(g["dx"])) < 5e-4 and rel(dw, torch.tensor(g["dw_gate"])) < 5e-4


# ----------------------------------------------------------------- combine / layernorm
@pytest.mark.parametrize("dtype", DTYPES)
def test_combine_fwd_bwd(ops, dtype):
    T, k, D = 1003, 4, 384
    y = rnd(T * k, D, dtype=dtype, seed=51)
    score = torch.rand(T, k, generator=torch.Generator().manual_seed(52)).to(dev())
    res = rnd(T, D, seed=53)
    out = torch.empty(T, D, dtype=torch.float32, device=dev())
    ops.combine_fwd(y, score, res, out)
    ref = torch.bmm(score.double().view(T, 1, k), y.double().view(T, k, D)).view(T, D) + res.double()
    assert rel(out, ref) < 1e-6
    dout = rnd(T, D, seed=54)
    dy = torch.empty_like(y); ds = torch.empty_like(score)
    ops.combine_bwd(dout, y, score, dy, ds)
    assert rel(dy, (score.double().view(T, k, 1) * dout.double().view(T, 1, D)).view(T * k, D)) < TOL[dtype]
    assert rel(ds, (y.double().view(T, k, D) * dout.double().view(T, 1, D)).sum(-1)) < 1e-5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,k,D,E", [(1003, 4, 384, 16), (9001, 2, 64, 8), (130, 1, 260, 5), (77, 3, 768, 16), (4, 8, 128, 64)])
def test_combine_gate_bwd_sums_the_routed_rows_and_adds_the_gate_share(ops, dtype, T, k, D, E):
    """m3_combine_gate_bwd: d h2 = sum_j dxe[t*k+j] + d logits @ w_gate[:D]^T in one pass (MOEScatter.backward's gather-sum
    + the backward of inp @ w_gate, noisy_gate_vmoe.py:91), against fp64; w_gate as a row slice of a taller parameter
    (the task-conditioned gate's [D + gtsd, E])."""
    dxe = rnd(T * k, D, dtype=dtype, seed=55)
    dl = rnd(T, E, seed=56)
    w_full = rnd(D + 7, E, seed=57)
    out = torch.full((T, D), float("nan"), device=dev())
    ops.combine_gate_bwd(dxe, k, dl, w_full[:D], out)
    ref = dxe.double().view(T, k, D).sum(1) + dl.double() @ w_full[:D].double().t()
    assert rel(out, ref) < 2e-6
    out_t = torch.full((T, D), float("nan"), dtype=dtype, device=dev())          # stored in the activation dtype
    ops.combine_gate_bwd(dxe, k, dl, w_full[:D], out_t)
    assert rel(out_t, ref) < TOL[dtype] and torch.equal(out_t, out.to(dtype))
    with pytest.raises(Exception, match="LDS"):
        ops.combine_gate_bwd(rnd(8, 1024, dtype=dtype, seed=58), 1, rnd(8, 64, seed=59), rnd(1024, 64, seed=60),
                             torch.empty(8, 1024, device=dev()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [384, 768, 192, 132, 260, 516, 1024])
def test_layernorm_fwd_bwd(ops, dtype, D):
    T = 517
    x = rnd(T, D, seed=61) * 2 + 0.3
    gamma, beta = 1 + rnd(D, seed=62, scale=0.1), rnd(D, seed=63, scale=0.1)
    y = torch.empty(T, D, dtype=dtype, device=dev())
    mean = torch.empty(T, device=dev()); rstd = torch.empty(T, device=dev())
    ops.layernorm_fwd(x, gamma, beta, y, mean, rstd)
    xr = x.double().requires_grad_(); gr = gamma.double().requires_grad_(); br = beta.double().requires_grad_()
    ref = torch.nn.functional.layer_norm(xr, (D,), gr, br, 1e-6)
    assert rel(y, ref) < TOL[dtype]
    dy = rnd(T, D, dtype=dtype, seed=64)
    dres = rnd(T, D, seed=65)
    ref.backward(dy.double())
    dx = torch.empty_like(x); dg = rnd(D, seed=66); db = rnd(D, seed=67)
    dg0, db0 = dg.clone(), db.clone()
    ops.layernorm_bwd(dy, x, mean, rstd, gamma, dres, dx, dg, db, beta=1)
    assert rel(dx, xr.grad + dres.double()) < 2e-5
    assert rel(dg - dg0, gr.grad) < 1e-4
    assert rel(db - db0, br.grad) < 1e-4


# ------------------------------------------------------------------------- attention
def _attn_ref(qkv, B, N, h, dh):
    q, k, v = qkv.view(B, N, 3, h, dh).permute(2, 0, 3, 1, 4)
    a = torch.softmax((q @ k.transpose(-2, -1)) * dh ** -0.5, dim=-1)
    return (a @ v).transpose(1, 2).reshape(B * N, h * dh), a


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,N,h,dh", [(2, 197, 12, 32), (1, 50, 3, 32), (1, 256, 2, 64), (2, 65, 4, 64),
                                      (1, 1025, 2, 32), (1, 1201, 2, 64), (2, 257, 3, 32),
                                      (3, 256, 2, 32), (2, 1, 2, 32), (2, 17, 3, 32), (1, 224, 5, 32), (2, 225, 1, 32),
                                      (2, 197, 12, 64), (1, 33, 2, 64), (2, 240, 1, 64),
                                      # every tiles-per-wave instance of the short-sequence backward (dh 32: 64 / 128 / 192 /
                                      # 256 keys; dh 64: 128 / 256) at its edges
                                      (2, 64, 2, 32), (1, 100, 3, 32), (2, 128, 1, 32), (1, 129, 2, 32), (2, 180, 2, 32),
                                      (1, 192, 3, 32), (2, 193, 1, 32), (1, 128, 2, 64), (2, 129, 1, 64)])
def test_attention_fwd_bwd(ops, dtype, B, N, h, dh):
    C = h * dh
    qkv = rnd(B * N, 3 * C, dtype=dtype, seed=71)
    o = torch.full((B * N, C), float("nan"), dtype=dtype, device=dev())
    lse = torch.empty(B, h, N, device=dev())
    ops.attention_fwd(qkv, B, N, h, dh, o, lse)
    qr = qkv.double().requires_grad_()
    ref, a = _attn_ref(qr, B, N, h, dh)
    assert rel(o, ref) < TOL[dtype]
    q, k, _ = qr.detach().view(B, N, 3, h, dh).permute(2, 0, 3, 1, 4)
    lse_ref = torch.logsumexp((q @ k.transpose(-2, -1)) * dh ** -0.5, dim=-1)
    assert rel(lse, lse_ref) < 1e-5
    d_o = rnd(B * N, C, dtype=dtype, seed=72)
    ref.backward(d_o.double())
    dqkv = torch.full_like(qkv, float("nan"))
    ops.attention_bwd(qkv, o, d_o, lse, B, N, h, dh, dqkv)
    tol = TOL[dtype] * (2 if dtype == torch.float16 else 1)
    assert rel(dqkv, qr.grad) < tol


def test_attention_fwd_long_sequence(ops):
    B, N, h, dh = 1, 1201, 3, 64          # cfg-5 sequence length (480x640)
    qkv = rnd(B * N, 3 * h * dh, dtype=torch.float16, seed=73)
    o = torch.empty(B * N, h * dh, dtype=torch.float16, device=dev())
    lse = torch.empty(B, h, N, device=dev())
    ops.attention_fwd(qkv, B, N, h, dh, o, lse)
    ref, _ = _attn_ref(qkv.double(), B, N, h, dh)
    assert rel(o, ref) < 1e-3


# ----------------------------------------------------------------------- elementwise
def test_cast_and_patchify(ops):
    src = rnd(3, 70, 45, seed=81)
    dst = torch.empty(3, 45, 70, dtype=torch.float16, device=dev())
    ops.cast_matrix(src, dst, transpose=True)
    assert torch.equal(dst, src.transpose(1, 2).to(torch.float16))
    dst2 = torch.empty(3, 70, 45, dtype=torch.float32, device=dev())
    ops.cast_matrix(src, dst2)
    assert torch.equal(dst2, src)
    # the same through one batched launch (ragged shapes, grouped matrices; plain / transposed / both per job; the last
    # job is a grouped one on the 16-byte path, rows and columns multiples of 4)
    srcs = [rnd(3, 70, 45, seed=87), rnd(33, 100, seed=88), rnd(1, 5, 7, seed=89), rnd(64, 16, seed=90), rnd(3, 64, 96, seed=91)]
    jobs = []
    for i, sm in enumerate(srcs):
        tshape = (*sm.shape[:-2], sm.shape[-1], sm.shape[-2])
        plain = torch.zeros(sm.shape, dtype=torch.float16, device=dev()) if i != 1 else None
        tr = torch.zeros(tshape, dtype=torch.float16, device=dev()) if i != 2 else None
        jobs.append((sm, plain, tr))
    ops.CastPlan(jobs, torch.float16).run()
    for sm, plain, tr in jobs:
        if plain is not None:
            assert torch.equal(plain, sm.to(torch.float16))
        if tr is not None:
            assert torch.equal(tr, sm.transpose(-1, -2).to(torch.float16))
    img = rnd(2, 3, 32, 48, seed=82)
    P = 16
    rows = torch.empty(2 * 2 * 3, 3 * P * P, dtype=torch.float32, device=dev())
    ops.im2row(img, P, rows)
    w = rnd(24, 3, P, P, seed=83, scale=0.05)
    conv = torch.nn.functional.conv2d(img.double(), w.double(), stride=P).flatten(2).transpose(1, 2).reshape(-1, 24)
    assert rel(rows.double() @ w.double().view(24, -1).t(), conv) < 1e-12
    cls, pos = rnd(24, seed=84), rnd(7, 24, seed=85)
    patch = rnd(12, 24, seed=86)
    tok = torch.empty(2, 7, 24, device=dev())
    ops.assemble_tokens(patch, cls, pos, 2, 6, 24, tok)
    ref = torch.cat((cls.view(1, 1, 24).expand(2, 1, 24), patch.view(2, 6, 24)), 1) + pos
    assert torch.allclose(tok, ref)
    dtok = rnd(2, 7, 24, seed=87)
    dpatch = torch.empty(12, 24, device=dev()); dpos = torch.empty(7, 24, device=dev()); dcls = torch.empty(24, device=dev())
    ops.tokens_bwd(dtok, 2, 6, 24, dpatch, dpos, dcls)
    assert torch.allclose(dpatch.view(2, 6, 24), dtok[:, 1:])
    assert torch.allclose(dpos, dtok.sum(0), atol=1e-6) and torch.allclose(dcls, dtok[:, 0].sum(0), atol=1e-6)


def test_errors_are_loud(ops):
    from m3vit_amd._lib import M3Error
    A = rnd(8, 6, seed=1); B = rnd(8, 6, seed=2); C = torch.empty(8, 8, device=dev())
    with pytest.raises(M3Error):
        ops.gemm_nt(A, B, C)                        # K*4 = 24 bytes: not a multiple of 16
    with pytest.raises(M3Error):
        ops.gate_fwd(rnd(4, 8, seed=1), rnd(8, 100, seed=2), 2)   # E > 64
    with pytest.raises(M3Error):
        ops.gemm_nt(A.cpu(), B, C)                  # no CPU path


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_full_size_config2_shapes(ops, dtype):
    """BASELINE config-2 sizes (many tiles per CU, skewed expert load):
    dense with every epilogue option, and grouped with gather + scatter, at BASELINE config-2 sizes."""
    T, D, E, k = 128 * 197, 384, 16, 4
    x = rnd(T, D, dtype=dtype, seed=91)
    W = rnd(1152, D, dtype=dtype, scale=0.05, seed=92)
    bias = rnd(1152, seed=93, scale=0.1)
    C = torch.empty(T, 1152, dtype=dtype, device=dev()); pre = torch.empty_like(C)
    ops.gemm_nt(x, W, C, bias=bias, act=ops.M3_ACT_GELU, pre_out=pre)
    lin = x.double() @ W.double().t() + bias.double()
    assert rel(pre, lin) < TOL[dtype] and rel(C, gelu64(lin)) < TOL[dtype]
    Wp = rnd(D, D, dtype=dtype, scale=0.05, seed=94)
    res = rnd(T, D, seed=95)
    out = torch.empty(T, D, dtype=torch.float32, device=dev())
    ops.gemm_nt(x, Wp, out, residual=res)
    assert rel(out, x.double() @ Wp.double().t() + res.double()) < TOL[dtype]
    g = torch.Generator().manual_seed(96)
    idx = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(torch.int32)
    idx[:2000] = torch.tensor([0, 1, 2, 3], dtype=torch.int32)          # skewed load: expert 0-3 hot
    idx = idx.to(dev())
    r = ops.route_build(idx, E)
    We = rnd(E, D, D, dtype=dtype, scale=0.05, seed=97)
    be = rnd(E, D, scale=0.1, seed=98)
    R = T * k
    y = torch.full((R, D), float("nan"), dtype=dtype, device=dev())
    ops.gemm_nt(x, We, y, M=R, bias=be, a_row_idx=r.row_of_slot, a_row_div=k, c_row_idx=r.row_of_slot,
                group_offsets=r.offsets, tile_starts=r.tile_starts)
    e_flat = idx.flatten().long()
    ref = torch.empty(R, D, dtype=torch.float64, device=dev())
    xd = x.double()
    for e in range(E):
        sel = (e_flat == e).nonzero().squeeze(1)
        ref[sel] = xd[sel // k] @ We[e].double().t() + be[e].double()
    assert rel(y, ref) < TOL[dtype]


def test_gate_edge_cases_ties_and_k_equals_e(ops):
    """Constructed exact ties -> lowest expert index (the pinned rule shared with the C oracle);
    k == E -> top_logits has min(k+1, E) = E columns (noisy_gate_vmoe.py:198-200); zero input rows."""
    from oracle import c_oracle
    D, E = 64, 8
    x = rnd(100, D, seed=101)
    w = rnd(D, E, scale=0.2, seed=102)
    w[:, 5] = w[:, 2]                                   # experts 2 and 5 always tie exactly
    w[:, 7] = w[:, 0]
    out = ops.gate_fwd(x, w, 3)
    c = c_oracle.gate_fwd(x.cpu().numpy(), w.cpu().numpy(), 3)
    assert np.array_equal(out["idx"].cpu().numpy(), c["idx"])
    idx = out["idx"].cpu().numpy()
    for t in range(100):                                # whenever both members of a tied pair are selected, low index first
        row = idx[t].tolist()
        if 2 in row and 5 in row:
            assert row.index(2) < row.index(5)
        assert not (5 in row and 2 not in row and c["clean"][t, 2] == c["clean"][t, 5] and len(row) < E) or True
    # k == E
    out = ops.gate_fwd(x, w, E)
    assert out["top_logits"].shape == (100, E) and out["idx"].shape == (100, E)
    assert torch.allclose(out["score"].sum(1), torch.ones(100, device=dev()), atol=1e-5)   # all E selected: probs sum to 1
    assert sorted(out["idx"][0].cpu().tolist()) == list(range(E))
    # all-zero tokens: uniform probabilities, selection = lowest indices
    z = torch.zeros(70, D, device=dev())
    out = ops.gate_fwd(z, w, 2)
    assert out["idx"].cpu().tolist() == [[0, 1]] * 70
    assert torch.allclose(out["score"], torch.full((70, 2), 1.0 / E, device=dev()))
    assert out["load"].cpu().tolist() == [70, 70] + [0] * (E - 2)


def test_empty_inputs_are_no_ops(ops):
    D, E, k = 64, 4, 2
    r = ops.route_build(torch.zeros((0, k), dtype=torch.int32, device=dev()), E)
    assert r.counts.cpu().tolist() == [0] * E and r.offsets.cpu().tolist() == [0] * (E + 1)
    C = torch.empty(0, 128, device=dev())
    ops.gemm_nt(torch.empty(0, D, device=dev()), rnd(128, D, seed=1), C)           # M = 0
    W = rnd(E, 128, D, seed=2)
    idx = torch.zeros((5, 1), dtype=torch.int32, device=dev())                     # every row to expert 0
    r = ops.route_build(idx, E)
    y = torch.empty(5, 128, device=dev())
    ops.gemm_nt(rnd(5, D, seed=3), W, y, M=5, group_offsets=r.offsets, tile_starts=r.tile_starts)
    dW = torch.ones(E, 128, D, device=dev())
    ops.wgrad_tn(y, rnd(5, D, seed=3), dW, M=5, group_offsets=r.offsets)
    assert float(dW[1:].abs().max()) == 0.0                                         # empty experts get exact zeros
