"""GPU contract tests of the row kernels: LayerNorm forward at every NCH with a partial last vector and at large row offsets
(under the centring-aware bound of kernel_contract.layernorm_bound), the backward in slot mode and the batched parameter
reduction over a subset of layers, the casts, the row-scaled cast, the fp32 add with its single-thread tail - every output
guarded, every input bit-unchanged; and every leg of the host's instance choices (top-k constants, dx_act pairings, wave
counts, dtypes) by value."""
import os
import subprocess
import sys

import pytest
import torch

import kernel_contract as kc

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
WORST = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    yield _ops
    if WORST:
        print("\nrow kernels worst err/bound:", max(WORST.values()), max(WORST, key=WORST.get))


def rnd(*shape, dtype=F32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
@pytest.mark.parametrize("D", [4, 132, 260, 516, 772, 1024])
@pytest.mark.parametrize("offset,std", [(0.3, 2.0), (300.0, 1.0), (1000.0, 0.05)])
def test_layernorm_fwd_contract(ops, dtype, D, offset, std):
    """NCH = ceil(D / 256) = 1..4, each with a partial last 4-wide vector (D = 1024: full); rows with a per-row offset of
    10^2 - 10^3 around which the values spread by std 1 / 0.05 - where a one-pass variance fails"""
    T = 203
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(T, D, generator=g) * std + offset * (1 + torch.rand(T, 1, generator=g))).cuda()
    gamma, beta = 1 + rnd(D, seed=2, scale=0.1), rnd(D, seed=3, scale=0.1)
    y, ycheck = kc.guarded(T, D, dtype)
    mean, mcheck = kc.guarded(1, T, F32)
    rstd, rcheck = kc.guarded(1, T, F32)
    snap = kc.snapshot(x=x, gamma=gamma, beta=beta)
    ops.layernorm_fwd(x, gamma, beta, y, mean.view(T), rstd.view(T))
    torch.cuda.synchronize()
    kc.unchanged(snap)
    ycheck(); mcheck(); rcheck()
    x64 = x.double()
    ref = torch.nn.functional.layer_norm(x64, (D,), gamma.double(), beta.double(), 1e-6)
    w = kc.assert_within(y, ref, kc.layernorm_bound(x, gamma, beta, ref, dtype), what="y")
    mu = x64.mean(-1)
    rs = 1 / (x64.var(-1, unbiased=False) + 1e-6).sqrt()
    h = -(-D // 64) + 6
    w = max(w, kc.assert_within(mean.view(T), mu, kc.SAFETY * h * kc.U32 * x64.abs().mean(-1), what="mean"))
    # rstd: the variance of centred values (relative error (h + 2) u32 plus the centring error squared), half in the sqrt
    drs = ((h + 2) * kc.U32 + (h * kc.U32 * x64.abs().mean(-1) * rs) ** 2 + 2 * kc.U32) * rs
    w = max(w, kc.assert_within(rstd.view(T), rs, kc.SAFETY * drs, what="rstd"))
    WORST[f"ln_fwd/{dtype}/{D}/{offset}"] = w


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("D", [4, 132, 260, 516, 772, 1024])
def test_layernorm_bwd_slot_mode_and_subset_reduce(ops, dtype, D):
    """layernorm_bwd with dgamma = dbeta = None leaves its per-block partials in a workspace slot; layernorm_bwd_reduce then
    sums the slots of layers [first, first + count) - with beta 0 and 1 - and the table entries outside the subset keep their
    bits (engine.py runs both every backward)"""
    T, L = 150, 4
    nblk = ops.lib().m3_ln_bwd_blocks(T, D)
    ws_all, wcheck = kc.guarded_ws(L * 2 * nblk * D)
    ws4 = ws_all.view(L, 2, nblk, D)
    gamma = 1 + rnd(D, seed=11, scale=0.1)
    refs = []
    for j in range(L):
        x = rnd(T, D, seed=20 + j) * 2 + 0.5
        mean, rstd = torch.empty(T, device="cuda"), torch.empty(T, device="cuda")
        ops.layernorm_fwd(x, gamma, torch.zeros(D, device="cuda"), torch.empty(T, D, device="cuda"), mean, rstd)
        dy = rnd(T, D, dtype=dtype, seed=30 + j)
        dres = rnd(T, D, seed=40 + j)
        dx, dxcheck = kc.guarded(T, D, F32)
        dxa, dxacheck = kc.guarded(T, D, dtype)
        snap = kc.snapshot(dy=dy, x=x, mean=mean, rstd=rstd, gamma=gamma, dres=dres)
        ops.layernorm_bwd(dy, x, mean, rstd, gamma, dres, dx, None, None, ws=ws4[j].reshape(-1), dx_act=dxa)
        torch.cuda.synchronize()
        kc.unchanged(snap)
        dxcheck(); dxacheck()
        xr = x.double().requires_grad_(); gr = gamma.double().requires_grad_(); br = torch.zeros(D, dtype=torch.float64,
                                                                                                  device="cuda", requires_grad=True)
        torch.nn.functional.layer_norm(xr, (D,), gr, br, 1e-6).backward(dy.double())
        assert torch.equal(dxa, dx.to(dtype))
        ref_dx = xr.grad + dres.double()
        # dx = dres + rstd (g dy - mean(g dy) - xhat mean(g dy xhat)): row means over D terms in fp32
        bdx = kc.SAFETY * ((D + 8) * kc.U32 * (rstd.double().unsqueeze(1) * (gr.detach().abs() * dy.double().abs()).mean(-1, keepdim=True)
                                              * (1 + (x.double() - mean.double().unsqueeze(1)).abs() * rstd.double().unsqueeze(1)) * 3)
                           + 4 * kc.U32 * (ref_dx.abs() + dres.double().abs()))
        WORST[f"ln_bwd_dx/{dtype}/{D}"] = kc.assert_within(dx, ref_dx, bdx, what="dx")
        refs.append((gr.grad, br.grad, (dy.double().abs() * ((x.double() - mean.double().unsqueeze(1)).abs()
                                                           * rstd.double().unsqueeze(1))).sum(0), dy.double().abs().sum(0)))
    wcheck()
    pairs = [(torch.full((D,), 7.0, device="cuda"), torch.full((D,), -3.0, device="cuda")) for _ in range(L)]
    table = ops.LnGradTable(pairs, "cuda")
    before = [(g.clone(), b.clone()) for g, b in pairs]
    ws_snap = kc.snapshot(ws=ws_all)
    first, count = 1, 2
    ops.layernorm_bwd_reduce(ws4, nblk, D, table, first, count, beta=0)
    ops.layernorm_bwd_reduce(ws4, nblk, D, table, first + 1, 1, beta=1)     # layer 2 again, accumulated
    torch.cuda.synchronize()
    kc.unchanged(ws_snap)
    for j in range(L):
        g, b = pairs[j]
        if not first <= j < first + count:
            assert kc.same_bits(g, before[j][0]) and kc.same_bits(b, before[j][1]), f"layer {j} outside the subset changed"
            continue
        times = 2 if j == first + 1 else 1
        rg, rb, ag, ab = refs[j]
        w = kc.assert_within(g, times * rg, kc.sum_bound(times * ag, T + 8, rg, F32), what=f"dgamma[{j}]")
        w = max(w, kc.assert_within(b, times * rb, kc.sum_bound(times * ab, T + 8, rb, F32), what=f"dbeta[{j}]"))
        WORST[f"ln_reduce/{dtype}/{D}/{j}"] = w


@pytest.mark.parametrize("dtype", [F16, BF16, F32])
def test_cast_f32_and_scale_rows_cast(ops, dtype):
    rows, cols = 394, 132
    src = rnd(rows, cols, seed=50)
    dst, check = kc.guarded(rows, cols, dtype)
    snap = kc.snapshot(src=src)
    ops.cast_f32(src, dst)
    torch.cuda.synchronize()
    kc.unchanged(snap); check()
    assert torch.equal(dst, src.to(dtype))
    for div in (1, 197):
        rs = torch.rand(-(-rows // div), generator=torch.Generator().manual_seed(div)).cuda() + 0.5
        dst, check = kc.guarded(rows, cols, dtype)
        ops.scale_rows_cast(src, rs, div, dst)
        torch.cuda.synchronize()
        check()
        ref = rs.double().repeat_interleave(div)[:rows].unsqueeze(1) * src.double()
        WORST[f"scale_rows_cast/{dtype}/{div}"] = kc.assert_within(dst, ref, kc.SAFETY * (kc.U32 * ref.abs() + kc.store(dtype, ref)))


@pytest.mark.parametrize("n", [1, 2, 3, 5, 4 * 1000 + 3])
def test_add_f32_tail(ops, n):
    dst0, src = rnd(1, n, seed=60), rnd(1, n, seed=61)
    dst, check = kc.guarded(1, n, F32)
    dst.copy_(dst0)
    snap = kc.snapshot(src=src)
    ops.add_f32(dst.view(n), src.view(n))
    torch.cuda.synchronize()
    kc.unchanged(snap); check()
    assert torch.equal(dst, dst0 + src)


def test_cast_matrix_gather_and_combine_guarded(ops):
    src = rnd(3, 70, 44, seed=70)
    dst, check = kc.guarded(3 * 44, 70, F16)
    ops.cast_matrix(src, dst.view(3, 44, 70), transpose=True)
    torch.cuda.synchronize()
    check()
    assert torch.equal(dst.view(3, 44, 70), src.transpose(1, 2).to(F16))
    T, k, D = 77, 3, 1024
    y = rnd(T * k, D, dtype=F16, seed=71)
    score = torch.rand(T, k, generator=torch.Generator().manual_seed(72)).cuda()
    res = rnd(T, D, seed=73)
    out, ocheck = kc.guarded(T, D, F32)
    snap = kc.snapshot(y=y, score=score, res=res)
    ops.combine_fwd(y, score, res, out)
    torch.cuda.synchronize()
    kc.unchanged(snap); ocheck()
    terms = (score.double().unsqueeze(2) * y.double().view(T, k, D))
    ref = terms.sum(1) + res.double()
    WORST["combine_fwd"] = kc.assert_within(out, ref, kc.sum_bound(terms.abs().sum(1) + res.double().abs(), k + 1, ref, F32))
    dout = rnd(T, D, seed=74)
    dy, dycheck = kc.guarded(T * k, D, F16)
    ds, dscheck = kc.guarded(T, k, F32)
    ops.combine_bwd(dout, y, score, dy, ds)
    torch.cuda.synchronize()
    dycheck(); dscheck()
    rdy = (score.double().unsqueeze(2) * dout.double().unsqueeze(1)).reshape(T * k, D)
    WORST["combine_bwd_dy"] = kc.assert_within(dy, rdy, kc.SAFETY * (kc.U32 * rdy.abs() + kc.store(F16, rdy)))
    prod = y.double().view(T, k, D) * dout.double().unsqueeze(1)
    WORST["combine_bwd_ds"] = kc.assert_within(ds, prod.sum(-1), kc.sum_bound(prod.abs().sum(-1), D, prod.sum(-1), F32))
    idx = torch.randint(0, T * k * 2, (T * k,), generator=torch.Generator().manual_seed(75), dtype=torch.int32).cuda()
    g_out, gcheck = kc.guarded(T, D, F16)
    ops.gather_rows(y, idx, g_out, div=2, k=k)
    torch.cuda.synchronize()
    gcheck()
    terms = y.double()[(idx.long() // 2)].view(T, k, D)
    ref = terms.sum(1)
    WORST["gather_rows"] = kc.assert_within(g_out, ref, kc.sum_bound(terms.abs().sum(1), k, ref, F16))


def test_patchify_tokens_and_upsample_guarded(ops):
    B, P, H, W, D = 2, 16, 32, 48, 64
    img = rnd(B, 3, H, W, seed=80)
    np_ = (H // P) * (W // P)
    rows, rcheck = kc.guarded(B * np_, 3 * P * P, F16)
    ops.im2row(img, P, rows)
    torch.cuda.synchronize()
    rcheck()
    ref = img.unfold(2, P, P).unfold(3, P, P).permute(0, 2, 3, 1, 4, 5).reshape(B * np_, 3 * P * P)
    assert torch.equal(rows, ref.to(F16))
    patch, cls, pos = rnd(B * np_, D, seed=81), rnd(D, seed=82), rnd(np_ + 1, D, seed=83)
    tok, tcheck = kc.guarded(B * (np_ + 1), D, F32)
    ops.assemble_tokens(patch, cls, pos, B, np_, D, tok)
    torch.cuda.synchronize()
    tcheck()
    ref = torch.cat([cls.view(1, 1, D).expand(B, 1, D), patch.view(B, np_, D)], 1) + pos
    assert torch.equal(tok.view(B, np_ + 1, D), ref)
    dtok = rnd(B * (np_ + 1), D, seed=84)
    dpatch, dpcheck = kc.guarded(B * np_, D, F16)
    dpos, dposcheck = kc.guarded(np_ + 1, D, F32)
    dcls, dclscheck = kc.guarded(1, D, F32)
    ops.tokens_bwd(dtok, B, np_, D, dpatch, dpos, dcls.view(D), beta=0)
    torch.cuda.synchronize()
    dpcheck(); dposcheck(); dclscheck()
    d3 = dtok.view(B, np_ + 1, D)
    assert torch.equal(dpatch.view(B, np_, D), d3[:, 1:].to(F16))
    WORST["tokens_bwd"] = kc.assert_within(dpos, d3.double().sum(0), kc.sum_bound(d3.double().abs().sum(0), B, d3.double().sum(0), F32))

@pytest.mark.parametrize("dtype,C", [(F16, 24), (BF16, 16), (F32, 12)])
def test_relu_up2x_fwd_bwd_guarded(ops, dtype, C):
    """the decoder-head stage through the C ABI with a guarded output (the wrapper allocates its own), and its backward: a
    bilinear tap is a weighted sum of 4 inputs (weights 9/16, 3/16, 3/16, 1/16), an input gradient one of up to 16 outputs"""
    Nb, H, W = 2, 5, 7
    x = rnd(Nb, H, W, C, dtype=dtype, seed=85).permute(0, 3, 1, 2)             # [N, C, H, W] channels-last
    y, ycheck = kc.guarded(Nb * 2 * H * 2 * W, C, dtype)
    snap = kc.snapshot(x=x)
    ops.check(ops.lib().m3_relu_up2x_fwd(ops._p(x), ops.dt_code(dtype), Nb, H, W, C, 1, ops._p(y), ops.dt_code(dtype),
                                         ops._stream()), "m3_relu_up2x_fwd")
    torch.cuda.synchronize()
    kc.unchanged(snap); ycheck()
    xr = torch.relu(x.double()).requires_grad_()
    ref = torch.nn.functional.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=False)
    aref = torch.nn.functional.interpolate(xr.detach().abs(), scale_factor=2, mode="bilinear", align_corners=False)
    got = y.view(Nb, 2 * H, 2 * W, C).permute(0, 3, 1, 2)
    w = kc.assert_within(got, ref.detach(), kc.sum_bound(aref, 4, ref.detach(), dtype), what="y")
    dy = rnd(Nb, 2 * H, 2 * W, C, dtype=dtype, seed=86).permute(0, 3, 1, 2)
    snap = kc.snapshot(x=x, dy=dy)
    dx = ops.relu_up2x_bwd(dy, x, relu=True)
    torch.cuda.synchronize()
    kc.unchanged(snap)
    ref.backward(dy.double())
    mask = (x.double() > 0).double()
    xa = xr.detach().clone().requires_grad_()
    torch.nn.functional.interpolate(xa, scale_factor=2, mode="bilinear", align_corners=False).backward(dy.double().abs())
    rdx = xr.grad * mask
    w = max(w, kc.assert_within(dx, rdx, kc.sum_bound(xa.grad * mask, 16, rdx, dtype), what="dx"))
    WORST[f"relu_up2x/{dtype}"] = w


def combine_gate_bwd_case(ops, dxe_dtype, dh_dtype, T, k, D, E):
    """dh = sum_j dxe[t*k+j] + d_logits @ w_gate[:D]^T: k + E terms summed in fp32, stored as dh_dtype"""
    dxe = rnd(T * k, D, dtype=dxe_dtype, seed=90)
    dl, wg = rnd(T, E, seed=91), rnd(D, E, seed=92)
    dh, check = kc.guarded(T, D, dh_dtype)
    snap = kc.snapshot(dxe=dxe, dl=dl, wg=wg)
    ops.combine_gate_bwd(dxe, k, dl, wg, dh)
    torch.cuda.synchronize()
    kc.unchanged(snap); check()
    x3 = dxe.double().view(T, k, D)
    ref = x3.sum(1) + dl.double() @ wg.double().t()
    aref = x3.abs().sum(1) + dl.double().abs() @ wg.double().abs().t()
    WORST[f"combine_gate_bwd/{dxe_dtype}/{dh_dtype}/{k}/{D}"] = kc.assert_within(dh, ref, kc.sum_bound(aref, k + E, ref, dh_dtype),
                                                                              what="dh")


# (9, 2, 132, 4) and (9, 2, 516, 4): the k = 2 instance, and one and three 256-column chunks (the others: k = 4 and run-time k,
# two and four chunks)
@pytest.mark.parametrize("dh_dtype", [F32, F16])
@pytest.mark.parametrize("T,k,D,E", [(77, 3, 1024, 8), (130, 1, 260, 5), (64, 4, 384, 16), (9, 2, 132, 4), (9, 2, 516, 4)])
def test_combine_gate_bwd_guarded(ops, dh_dtype, T, k, D, E):
    combine_gate_bwd_case(ops, F16, dh_dtype, T, k, D, E)


@pytest.mark.parametrize("dxe_dtype,dh_dtype", [(F32, F32), (BF16, BF16), (BF16, F32)])
@pytest.mark.parametrize("k", [4, 2, 3])
def test_combine_gate_bwd_other_dtypes(ops, dxe_dtype, dh_dtype, k):
    combine_gate_bwd_case(ops, dxe_dtype, dh_dtype, 9, k, 260, 4)


# ------------------------------------------------------------------------------------ every leg of an instance choice
@pytest.mark.parametrize("dtype", [F32, F16, BF16])
@pytest.mark.parametrize("k", [1, 2, 4, 8, 3])
def test_combine_every_top_k_instance(ops, dtype, k):
    """combine_fwd / combine_bwd with top-k as a template constant (1, 2, 4, 8) and at run time (3), and the k-way gather: T = 9
    is two full workgroups and a partial one, D = 260 a second column chunk of one 4-wide vector"""
    T, D = 9, 260
    y = rnd(T * k, D, dtype=dtype, seed=71)
    score = torch.rand(T, k, generator=torch.Generator().manual_seed(72)).cuda()
    res = rnd(T, D, seed=73)
    out, ocheck = kc.guarded(T, D, F32)
    snap = kc.snapshot(y=y, score=score, res=res)
    ops.combine_fwd(y, score, res, out)
    torch.cuda.synchronize()
    kc.unchanged(snap); ocheck()
    terms = (score.double().unsqueeze(2) * y.double().view(T, k, D))
    ref = terms.sum(1) + res.double()
    w = kc.assert_within(out, ref, kc.sum_bound(terms.abs().sum(1) + res.double().abs(), k + 1, ref, F32), what="out")
    dout = rnd(T, D, seed=74)
    dy, dycheck = kc.guarded(T * k, D, dtype)
    ds, dscheck = kc.guarded(T, k, F32)
    ops.combine_bwd(dout, y, score, dy, ds)
    torch.cuda.synchronize()
    dycheck(); dscheck()
    rdy = (score.double().unsqueeze(2) * dout.double().unsqueeze(1)).reshape(T * k, D)
    w = max(w, kc.assert_within(dy, rdy, kc.SAFETY * (kc.U32 * rdy.abs() + kc.store(dtype, rdy)), what="dy"))
    prod = y.double().view(T, k, D) * dout.double().unsqueeze(1)
    w = max(w, kc.assert_within(ds, prod.sum(-1), kc.sum_bound(prod.abs().sum(-1), D, prod.sum(-1), F32), what="dscore"))
    idx = torch.randint(0, T * k * 2, (T * k,), generator=torch.Generator().manual_seed(75), dtype=torch.int32).cuda()
    g_out, gcheck = kc.guarded(T, D, dtype)
    ops.gather_rows(y, idx, g_out, div=2, k=k)
    torch.cuda.synchronize()
    gcheck()
    terms = y.double()[(idx.long() // 2)].view(T, k, D)
    w = max(w, kc.assert_within(g_out, terms.sum(1), kc.sum_bound(terms.abs().sum(1), k, terms.sum(1), dtype), what="gather"))
    WORST[f"combine/{dtype}/k{k}"] = w


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_casts_and_token_plumbing_in_every_dtype(ops, dtype):
    """the dtype leg of cast_matrix (plain and transposed), cast_f32, cast_batch, im2row and tokens_bwd: exact copies, rounded
    once"""
    src = rnd(2, 37, 44, seed=70)
    for tr in (False, True):
        shape = (2, 44, 37) if tr else (2, 37, 44)
        dst, check = kc.guarded(shape[0] * shape[1], shape[2], dtype)
        ops.cast_matrix(src, dst.view(*shape), transpose=tr)
        torch.cuda.synchronize()
        check()
        assert torch.equal(dst.view(*shape), (src.transpose(1, 2) if tr else src).to(dtype))
    dst, check = kc.guarded(37, 44, dtype)
    ops.cast_f32(src[0], dst)
    torch.cuda.synchronize()
    check()
    assert torch.equal(dst, src[0].to(dtype))
    # cast_batch: one launch, three jobs - plain + transposed from one read (37 x 44: the scalar tiles), plain only and
    # transposed only (40 x 36: the 16-byte tiles)
    src2 = rnd(40, 36, seed=76)
    d0, c0 = kc.guarded(2 * 37, 44, dtype)
    t0, ct0 = kc.guarded(2 * 44, 37, dtype)
    d1, c1 = kc.guarded(40, 36, dtype)
    t2, ct2 = kc.guarded(36, 40, dtype)
    plan = ops.CastPlan([(src, d0.view(2, 37, 44), t0.view(2, 44, 37)), (src2, d1, None), (src2, None, t2)], dtype)
    snap = kc.snapshot(src=src, src2=src2)
    plan.run()
    torch.cuda.synchronize()
    kc.unchanged(snap)
    c0(); ct0(); c1(); ct2()
    assert torch.equal(d0.view(2, 37, 44), src.to(dtype)) and torch.equal(t0.view(2, 44, 37), src.transpose(1, 2).to(dtype))
    assert torch.equal(d1, src2.to(dtype)) and torch.equal(t2, src2.t().to(dtype))
    B, P, H, W, D = 2, 4, 8, 12, 8
    img = rnd(B, 3, H, W, seed=80)
    np_ = (H // P) * (W // P)
    rows, rcheck = kc.guarded(B * np_, 3 * P * P, dtype)
    ops.im2row(img, P, rows)
    torch.cuda.synchronize()
    rcheck()
    assert torch.equal(rows, img.unfold(2, P, P).unfold(3, P, P).permute(0, 2, 3, 1, 4, 5).reshape(B * np_, 3 * P * P).to(dtype))
    dtok = rnd(B * (np_ + 1), D, seed=84)
    dpatch, dpcheck = kc.guarded(B * np_, D, dtype)
    dpos, dcls = torch.empty(np_ + 1, D, device="cuda"), torch.empty(D, device="cuda")
    ops.tokens_bwd(dtok, B, np_, D, dpatch, dpos, dcls, beta=0)
    torch.cuda.synchronize()
    dpcheck()
    d3 = dtok.view(B, np_ + 1, D)
    assert torch.equal(dpatch.view(B, np_, D), d3[:, 1:].to(dtype))
    assert torch.equal(dpos, d3[0] + d3[1]) and torch.equal(dcls, dpos[0])


# dy dtype, dx_act dtype: every pairing m3_layernorm_bwd builds (fp32 dy with any copy; 16-bit dy with its own dtype or fp32)
LN_PAIRS = [(F32, F16), (F32, BF16), (F32, F32), (F16, F16), (F16, F32), (BF16, BF16), (BF16, F32)]
LN_T = 150


def ln_bwd_case(ops, dy_dtype, act_dtype, D):
    """one layernorm_bwd that reduces dgamma / dbeta itself and writes a dx_act copy, against float64 autograd (the bounds of
    test_layernorm_bwd_slot_mode_and_subset_reduce)"""
    T = LN_T
    gamma = 1 + rnd(D, seed=11, scale=0.1)
    x = rnd(T, D, seed=20) * 2 + 0.5
    mean, rstd = torch.empty(T, device="cuda"), torch.empty(T, device="cuda")
    ops.layernorm_fwd(x, gamma, torch.zeros(D, device="cuda"), torch.empty(T, D, device="cuda"), mean, rstd)
    dy, dres = rnd(T, D, dtype=dy_dtype, seed=30), rnd(T, D, seed=40)
    dx, dxcheck = kc.guarded(T, D, F32)
    dxa, dxacheck = kc.guarded(T, D, act_dtype)
    dg, dgcheck = kc.guarded(1, D, F32)
    db, dbcheck = kc.guarded(1, D, F32)
    snap = kc.snapshot(dy=dy, x=x, mean=mean, rstd=rstd, gamma=gamma, dres=dres)
    ops.layernorm_bwd(dy, x, mean, rstd, gamma, dres, dx, dg.view(D), db.view(D), dx_act=dxa)
    torch.cuda.synchronize()
    kc.unchanged(snap)
    dxcheck(); dxacheck(); dgcheck(); dbcheck()
    xr, gr = x.double().requires_grad_(), gamma.double().requires_grad_()
    br = torch.zeros(D, dtype=torch.float64, device="cuda", requires_grad=True)
    torch.nn.functional.layer_norm(xr, (D,), gr, br, 1e-6).backward(dy.double())
    assert torch.equal(dxa, dx.to(act_dtype))
    ref_dx = xr.grad + dres.double()
    xh = (x.double() - mean.double().unsqueeze(1)).abs() * rstd.double().unsqueeze(1)
    bdx = kc.SAFETY * ((D + 8) * kc.U32 * (rstd.double().unsqueeze(1) * (gr.detach().abs() * dy.double().abs()).mean(-1, keepdim=True)
                                          * (1 + xh) * 3) + 4 * kc.U32 * (ref_dx.abs() + dres.double().abs()))
    w = kc.assert_within(dx, ref_dx, bdx, what="dx")
    w = max(w, kc.assert_within(dg.view(D), gr.grad, kc.sum_bound((dy.double().abs() * xh).sum(0), T + 8, gr.grad, F32), what="dgamma"))
    w = max(w, kc.assert_within(db.view(D), br.grad, kc.sum_bound(dy.double().abs().sum(0), T + 8, br.grad, F32), what="dbeta"))
    return w


@pytest.mark.parametrize("pair", LN_PAIRS, ids=lambda p: f"{str(p[0])[6:]}-{str(p[1])[6:]}")
@pytest.mark.parametrize("D", [4, 132, 260, 516, 772, 1024])
def test_layernorm_bwd_every_dx_act_pairing(ops, pair, D):
    """each (dy, dx_act) dtype pairing at each NCH = 1..4 (the default 8 waves per workgroup)"""
    assert ops.lib().m3_ln_bwd_blocks(LN_T, D) == -(-LN_T // 64), "not the default geometry: M3_LN_WAVES / M3_LN_ROWS are set"
    WORST[f"ln_bwd_pair/{pair}/{D}"] = ln_bwd_case(ops, pair[0], pair[1], D)


@pytest.mark.parametrize("dy_dtype,act_dtype", [(F16, BF16), (BF16, F16)])
def test_layernorm_bwd_rejects_the_mixed_16bit_pair(ops, dy_dtype, act_dtype):
    T, D = 8, 132
    x, dy = rnd(T, D, seed=1), rnd(T, D, dtype=dy_dtype, seed=2)
    mean, rstd = torch.zeros(T, device="cuda"), torch.ones(T, device="cuda")
    dx, dxcheck = kc.guarded(T, D, F32)
    dxa, dxacheck = kc.guarded(T, D, act_dtype)
    with pytest.raises(ops._lib.M3Error, match=r"dy fp16 with dx_act bf16 \(or the reverse\) is not supported"):
        ops.layernorm_bwd(dy, x, mean, rstd, torch.ones(D, device="cuda"), None, dx, None, None, dx_act=dxa)
    torch.cuda.synchronize()
    dxcheck(keep_rows=list(range(T))); dxacheck(keep_rows=list(range(T)))


@pytest.mark.parametrize("nw", [4, 16])
def test_layernorm_bwd_forced_wave_counts(nw):
    """M3_LN_WAVES = 4 / 16 (read once per process, so in a child): the other two LNB_WAVES instances, at every NCH they can
    run at (16 waves only up to D = 512), fp32 and fp16 gradients"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    here = os.path.dirname(os.path.abspath(__file__))
    dims = [132, 260, 516, 1024] if nw == 4 else [132, 260]
    code = (f"import sys; sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]\n"
            "import torch; from m3vit_amd import ops; import test_contract_rowops as t\n"
            f"assert ops.lib().m3_ln_bwd_blocks(t.LN_T, 132) == -(-t.LN_T // ({nw} * 8)), 'M3_LN_WAVES not in force'\n"
            f"print(max(t.ln_bwd_case(ops, dy, act, D) for D in {dims!r} for dy, act in ((t.F32, t.F16), (t.F16, t.F16))))\n")
    env = dict(os.environ, M3_LN_WAVES=str(nw))
    env.pop("M3_LN_ROWS", None)
    r = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    WORST[f"ln_bwd_waves/{nw}"] = float(r.stdout.split()[-1])


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("dtype", [F16, BF16])
def test_relu_up2x_fp32_output_and_gradient_of_a_16bit_input(ops, dtype, relu):
    """the (16-bit x, fp32 y) and (16-bit x, fp32 dy) instances, with and without the ReLU"""
    Nb, H, W, C = 2, 5, 7, 16
    x = rnd(Nb, H, W, C, dtype=dtype, seed=85)
    y, ycheck = kc.guarded(Nb * 2 * H * 2 * W, C, F32)
    snap = kc.snapshot(x=x)
    ops.check(ops.lib().m3_relu_up2x_fwd(ops._p(x), ops.dt_code(dtype), Nb, H, W, C, relu, ops._p(y), ops.dt_code(F32),
                                         ops._stream()), "m3_relu_up2x_fwd")
    torch.cuda.synchronize()
    kc.unchanged(snap); ycheck()
    xc = x.double().permute(0, 3, 1, 2)
    xr = (torch.relu(xc) if relu else xc.clone()).requires_grad_()
    ref = torch.nn.functional.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=False)
    aref = torch.nn.functional.interpolate(xr.detach().abs(), scale_factor=2, mode="bilinear", align_corners=False)
    got = y.view(Nb, 2 * H, 2 * W, C).permute(0, 3, 1, 2)
    w = kc.assert_within(got, ref.detach(), kc.sum_bound(aref, 4, ref.detach(), F32), what="y")
    dy = rnd(Nb, 2 * H, 2 * W, C, seed=86)
    dx, dxcheck = kc.guarded(Nb * H * W, C, dtype)
    snap = kc.snapshot(x=x, dy=dy)
    ops.check(ops.lib().m3_relu_up2x_bwd(ops._p(dy), ops.dt_code(F32), ops._p(x), ops.dt_code(dtype), Nb, H, W, C, relu,
                                         ops._p(dx), ops._stream()), "m3_relu_up2x_bwd")
    torch.cuda.synchronize()
    kc.unchanged(snap); dxcheck()
    dyc = dy.double().permute(0, 3, 1, 2)
    ref.backward(dyc)
    mask = (xc > 0).double() if relu else torch.ones_like(xc)
    xa = xr.detach().clone().requires_grad_()
    torch.nn.functional.interpolate(xa, scale_factor=2, mode="bilinear", align_corners=False).backward(dyc.abs())
    rdx = xr.grad * mask
    gdx = dx.view(Nb, H, W, C).permute(0, 3, 1, 2)
    w = max(w, kc.assert_within(gdx, rdx, kc.sum_bound(xa.grad * mask, 16, rdx, dtype), what="dx"))
    WORST[f"relu_up2x_f32side/{dtype}/{relu}"] = w
