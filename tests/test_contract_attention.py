"""GPU contract tests of m3_attention_fwd / m3_attention_bwd: guarded o, lse and dqkv, a dQ workspace of exactly
m3_attention_bwd_ws_elems sentinel-filled floats, four input distributions (flat logits; peaked, logit std ~ 8; near one-hot,
where each query's own key dominates; V offset by +50) in f16 / bf16 / f32 at sequence lengths that reach every
tiles-per-wave instance of the LDS-resident kernels (N <= 256) and the streamed ones.  o and lse are checked elementwise
(kernel_contract.attention_fwd_bounds), dqkv by relative L2 and elementwise (attention_bwd_bounds); the backward must be
bitwise repeatable under a different workspace fill.

Which kernel family and which template instance a shape runs is not worked out here: SHAPES states it per shape and the test
asserts it through m3_attention_plan, the host code the launchers take their instance from.  The shapes also cover what the
padding of the resident forward can get wrong - the product's N = 197 (three wholly masked key tiles and one with 5 valid
keys), N = 17 (two wholly masked tiles and one with a single key), N = 16 (one exact tile) and N = 1."""
import pytest
import torch

import kernel_contract as kc
import launch_signature as ls

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
REL = {F32: 2e-5, F16: 2e-3, BF16: 1.2e-2}
WORST = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    yield _ops
    if WORST:
        print("\nattention worst err/bound:", max(WORST.values()), max(WORST, key=WORST.get))


def make_qkv(B, N, h, dh, dist, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, N, h, dh, generator=g) for _ in range(3))
    if dist == "peaked":                    # logits q k^T dh^-0.5 with std ~ 8
        q = q * 8
    elif dist == "onehot":                  # the own key dominates: s_ii ~ 3 sqrt(dh) against std-3 off-diagonal logits
        q = 3 * k + 0.3 * q
    elif dist == "voffset":
        v = v + 50
    return torch.stack([q, k, v], 2).reshape(B * N, 3 * h * dh).to(dtype).cuda()


def heads(t, B, N, h, dh, parts):
    """[B*N, parts*h*dh] -> parts x [B, h, N, dh]"""
    x = t.view(B, N, parts, h, dh).permute(2, 0, 3, 1, 4)
    return [x[i] for i in range(parts)]


# (B, N, heads, dh) -> the instance of the LDS-resident 16-bit kernels (attention_b16.hip) the shape is meant to run: forward
# key tiles nkt (16-key tiles rounded up to a multiple of 4; the tiles past ceil(N / 16) are wholly masked), backward tiles
# per wave kte; None: N > 256, the streamed 16-bit kernels.  fp32 takes attention_f32.hip at every N.
SHAPES = {
    (2, 64, 2, 32): (4, 1), (1, 120, 1, 32): (8, 2), (1, 180, 2, 32): (12, 3), (1, 256, 1, 32): (16, 4),
    (1, 50, 1, 64): (4, 1), (2, 100, 1, 64): (8, 1), (1, 180, 1, 64): (12, 2), (1, 256, 1, 64): (16, 2),
    (1, 257, 2, 32): None, (1, 1025, 1, 64): None, (1, 1201, 1, 32): None,
    (2, 197, 1, 32): (16, 4), (1, 197, 2, 64): (16, 2),                # the product's N: 13 key tiles, the last with 5 keys, 3 masked
    (2, 17, 1, 32): (4, 1), (1, 17, 1, 64): (4, 1),                    # 2 key tiles, the second with one key, 2 masked
    (1, 16, 2, 32): (4, 1), (1, 16, 1, 64): (4, 1),                    # one exact tile, 3 masked
    (1, 1, 2, 32): (4, 1), (2, 1, 1, 64): (4, 1),                      # softmax over one key: o = v, dq = dk = 0
}
DTYPES = [F16, BF16, F32]


def stated_plan(dtype, shape):
    """(forward family, forward key tiles, backward family, backward tiles per wave) a (dtype, shape) case states"""
    if dtype == F32:
        return ("f32", 0, "f32", 0)
    inst = SHAPES[shape]
    return ("streamed", 0, "streamed", 0) if inst is None else ("resident", inst[0], "resident", inst[1])


def planned(ops, dtype, shape):
    from m3vit_amd import _lib
    p = ops.attention_plan(dtype, shape[1], shape[3])
    return (_lib.ATTN_FAMILIES[p.fwd_family], p.fwd_key_tiles, _lib.ATTN_FAMILIES[p.bwd_family], p.bwd_tiles_per_wave)


def case_signatures(ops):
    """{case id: signature} of the forward and the backward launch of every (dtype, shape).  Host only"""
    out = {}
    for dtype in DTYPES:
        for shape in SHAPES:
            for which in ("fwd", "bwd"):
                out[f"{which}/{dtype}/{shape}"] = ls.attention_signature(ops, which, ops.dt_code(dtype), shape[1], shape[3])
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dist", ["flat", "peaked", "onehot", "voffset"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_contract(ops, dtype, dist, shape):
    B, N, h, dh = shape
    C = h * dh
    assert planned(ops, dtype, shape) == stated_plan(dtype, shape)
    qkv = make_qkv(B, N, h, dh, dist, dtype, seed=N + dh)
    o, ocheck = kc.guarded(B * N, C, dtype)
    lse, lcheck = kc.guarded(B * h, N, F32)
    snap = kc.snapshot(qkv=qkv)
    ops.attention_fwd(qkv, B, N, h, dh, o, lse.view(B, h, N))
    torch.cuda.synchronize()
    kc.unchanged(snap); ocheck(); lcheck()
    qr = qkv.double().requires_grad_()
    q, k, v = heads(qr, B, N, h, dh, 3)
    s = (q @ k.transpose(-2, -1)) * dh ** -0.5
    o_ref = torch.softmax(s, -1) @ v
    lse_ref = torch.logsumexp(s, -1)
    qd, kd, vd = (t.detach() for t in (q, k, v))
    ob, lb = kc.attention_fwd_bounds(qd, kd, vd, o_ref.detach(), lse_ref.detach(), dtype)
    (o_k,) = heads(o, B, N, h, dh, 1)
    w = kc.assert_within(o_k, o_ref.detach(), ob, what="o")
    w = max(w, kc.assert_within(lse.view(B, h, N), lse_ref.detach(), lb, what="lse"))
    WORST[f"fwd/{dtype}/{dist}/{shape}"] = w
    # backward
    d_o = (torch.randn(B * N, C, generator=torch.Generator().manual_seed(7)).to(dtype)).cuda()
    (do_h,) = heads(d_o.double(), B, N, h, dh, 1)
    o_ref.backward(do_h)
    need = int(ops.lib().m3_attention_bwd_ws_elems(B, N, h, dh))
    ws, wcheck = kc.guarded_ws(need) if need else (None, None)
    dqkv, dcheck = kc.guarded(B * N, 3 * C, dtype)
    o_in = o.clone()
    snap = kc.snapshot(qkv=qkv, o=o_in, d_o=d_o, lse=lse)
    ops.attention_bwd(qkv, o_in, d_o, lse.view(B, h, N), B, N, h, dh, dqkv, dq_ws=ws)
    torch.cuda.synchronize()
    kc.unchanged(snap); dcheck()
    if wcheck:
        wcheck()
    ref = qr.grad
    if dist != "voffset":
        # (V offset by +50: dS = P (dP - rowsum(dO o O)) cancels two terms ~50x its size - and O is read as stored, in the
        # activation dtype - so the relative L2 of the flat case does not apply; the elementwise bound models both)
        assert float((dqkv.double() - ref).norm() / ref.norm()) < REL[dtype]
    dq, dk, dv = heads(dqkv, B, N, h, dh, 3)
    rq, rk, rv = heads(ref, B, N, h, dh, 3)
    if N == 1:
        # one key: P = 1 whatever the logit, dS = P (dP - rowsum(dO o O)) = 0 - the reference's dQ and dK are exactly zero, so
        # their own relative norm says nothing; they are checked element by element against the bound below
        assert float(rq.abs().max()) == 0.0 and float(rk.abs().max()) == 0.0
    (o_h,) = heads(o_in.double(), B, N, h, dh, 1)
    bq, bk, bv = kc.attention_bwd_bounds(qd, kd, vd, o_h, do_h, rq, rk, rv, dtype)
    w = max(kc.assert_within(dq, rq, bq, what="dq"), kc.assert_within(dk, rk, bk, what="dk"), kc.assert_within(dv, rv, bv, what="dv"))
    WORST[f"bwd/{dtype}/{dist}/{shape}"] = w
    # bitwise repeatable under a different workspace fill
    if dist == "peaked":
        again = torch.zeros_like(dqkv)
        if ws is not None:
            ws.normal_()
        ops.attention_bwd(qkv, o_in, d_o, lse.view(B, h, N), B, N, h, dh, again, dq_ws=ws)
        torch.cuda.synchronize()
        assert kc.same_bits(again, dqkv.contiguous())
