"""GPU: the two-prefix token kernels (m3_assemble_tokens2 / m3_tokens_bwd2: cls and dist in front of the patches) against
float64, with guarded outputs, run-to-run bits and the one-prefix kernels as a second reference for the patch rows."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_contract as kc                                       # noqa: E402

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
# (B, np, D): one 16-byte element; several workgroups; B = 9 is past the eight batch lanes; the real sequence (N = 198)
SHAPES = [(1, 1, 4), (3, 6, 64), (9, 6, 64), (2, 196, 384)]


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _inputs(B, np_, D):
    return rnd(B * np_, D, seed=1), rnd(D, seed=2), rnd(D, seed=3), rnd(np_ + 2, D, seed=4)


@pytest.mark.parametrize("B,np_,D", SHAPES, ids=str)
def test_assemble_tokens2(B, np_, D):
    from m3vit_amd import ops
    patch, cls, dist, pos = _inputs(B, np_, D)
    snap = kc.snapshot(patch=patch, cls=cls, dist=dist, pos=pos)
    tok, tcheck = kc.guarded(B * (np_ + 2), D, F32)
    ops.assemble_tokens2(patch, cls, dist, pos, B, np_, D, tok)
    torch.cuda.synchronize()
    tcheck(what="tokens")
    kc.unchanged(snap)
    ref = torch.cat([cls.view(1, 1, D).expand(B, 1, D), dist.view(1, 1, D).expand(B, 1, D), patch.view(B, np_, D)], 1) + pos
    assert torch.equal(tok.view(B, np_ + 2, D), ref)               # one fp32 addition per element: the same bits as torch's
    again = torch.empty_like(tok)
    ops.assemble_tokens2(patch, cls, dist, pos, B, np_, D, again)
    assert kc.same_bits(tok.contiguous(), again)
    # dist = cls and pos row 1 a copy of row 0: the patch rows (and row 0) are the one-prefix kernel's, bit for bit
    pos1 = torch.cat([pos[:1], pos[2:]], 0).contiguous()
    pos2 = torch.cat([pos[:1], pos[:1], pos[2:]], 0).contiguous()
    one, two = torch.empty(B, np_ + 1, D, device="cuda"), torch.empty(B, np_ + 2, D, device="cuda")
    ops.assemble_tokens(patch, cls, pos1, B, np_, D, one)
    ops.assemble_tokens2(patch, cls, cls.clone(), pos2, B, np_, D, two)
    assert kc.same_bits(two[:, 2:].contiguous(), one[:, 1:].contiguous())
    assert kc.same_bits(two[:, 0].contiguous(), one[:, 0].contiguous()) and kc.same_bits(two[:, 1].contiguous(), one[:, 0].contiguous())


@pytest.mark.parametrize("dtype", [F32, F16, BF16, None], ids=lambda d: "no-dpatch" if d is None else str(d).split(".")[-1])
@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("B,np_,D", SHAPES, ids=str)
def test_tokens_bwd2(B, np_, D, beta, dtype):
    from m3vit_amd import ops
    N = np_ + 2
    dtok = rnd(B * N, D, seed=5)
    prev = [rnd(N, D, seed=6), rnd(1, D, seed=7), rnd(1, D, seed=8)]

    def run():
        dpatch, dpcheck = kc.guarded(B * np_, D, dtype) if dtype is not None else (None, None)
        outs = [kc.guarded(N, D, F32), kc.guarded(1, D, F32), kc.guarded(1, D, F32)]
        for (o, _), p in zip(outs, prev):
            o.copy_(p)                                             # beta = 1 adds to these; beta = 0 must overwrite them
        ops.tokens_bwd2(dtok, B, np_, D, dpatch, outs[0][0], outs[1][0].view(D), outs[2][0].view(D), beta=beta)
        torch.cuda.synchronize()
        for (_, chk), what in zip(outs, ("dpos", "dcls", "ddist")):
            chk(what=what)
        if dpcheck is not None:
            dpcheck(what="dpatch")
        return dpatch, [o.clone() for o, _ in outs]

    snap = kc.snapshot(dtok=dtok)
    dpatch, (dpos, dcls, ddist) = run()
    kc.unchanged(snap)
    d3 = dtok.view(B, N, D)
    if dtype is not None:
        assert torch.equal(dpatch.view(B, np_, D), d3[:, 2:].to(dtype))
    s64, a64 = d3.double().sum(0), d3.double().abs().sum(0)
    base = [p.double() * beta for p in prev]
    # B terms and, with beta = 1, the old value: B + 1 fp32 additions
    bound = kc.sum_bound(a64 + base[0].abs(), B + 1, s64 + base[0], F32)
    kc.assert_within(dpos, s64 + base[0], bound, "dpos")
    kc.assert_within(dcls, s64[:1] + base[1], kc.sum_bound(a64[:1] + base[1].abs(), B + 1, s64[:1] + base[1], F32), "dcls")
    kc.assert_within(ddist, s64[1:2] + base[2], kc.sum_bound(a64[1:2] + base[2].abs(), B + 1, s64[1:2] + base[2], F32), "ddist")
    if beta == 0:                                                  # the prefix gradients are the sums the pos rows got
        assert kc.same_bits(dcls, dpos[:1]) and kc.same_bits(ddist, dpos[1:2])
    dpatch2, again = run()
    for a, b in zip((dpos, dcls, ddist), again):
        assert kc.same_bits(a, b), "a second run gave other bits"
    if dtype is not None:
        assert kc.same_bits(dpatch.contiguous(), dpatch2.contiguous())


def test_tokens_bwd2_matches_the_one_prefix_kernel_on_the_patch_rows():
    """dtok row 1 a copy of row 0: dpatch and the patch rows of dpos equal m3_tokens_bwd's on [row 0, patches], bit for bit"""
    from m3vit_amd import ops
    B, np_, D = 9, 6, 64
    d1 = rnd(B, np_ + 1, D, seed=9)
    d2 = torch.cat([d1[:, :1], d1[:, :1], d1[:, 1:]], 1).contiguous()
    dp1, dp2 = torch.empty(B * np_, D, device="cuda", dtype=F16), torch.empty(B * np_, D, device="cuda", dtype=F16)
    pos1, cls1 = torch.empty(np_ + 1, D, device="cuda"), torch.empty(D, device="cuda")
    pos2, cls2, dist2 = torch.empty(np_ + 2, D, device="cuda"), torch.empty(D, device="cuda"), torch.empty(D, device="cuda")
    ops.tokens_bwd(d1.view(-1, D), B, np_, D, dp1, pos1, cls1)
    ops.tokens_bwd2(d2.view(-1, D), B, np_, D, dp2, pos2, cls2, dist2)
    assert kc.same_bits(dp1, dp2) and kc.same_bits(pos1[1:].contiguous(), pos2[2:].contiguous())
    assert kc.same_bits(cls1, cls2) and kc.same_bits(cls1, dist2)


def test_token2_wrappers_refuse_bad_arguments():
    from m3vit_amd import _lib, ops
    B, np_, D = 2, 4, 8
    z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device="cuda")              # noqa: E731
    good = dict(patch=z(B * np_, D), cls=z(D), dist=z(D), pos=z(np_ + 2, D), tok=z(B * (np_ + 2), D))

    def asm(**kw):
        a = dict(good, **kw)
        return lambda: ops.assemble_tokens2(a["patch"], a["cls"], a["dist"], a["pos"], B, np_, D, a["tok"])
    bad = [asm(pos=z(np_ + 1, D)), asm(dist=z(D + 4)), asm(dist=z(D).cpu()), asm(cls=z(D, dt=F16)), asm(tok=z(B * (np_ + 1), D)),
           lambda: ops.tokens_bwd2(z(B * (np_ + 2), D), B, np_, D, None, z(np_ + 1, D), z(D), z(D)),
           lambda: ops.tokens_bwd2(z(B * (np_ + 2), D), B, np_, D, None, z(np_ + 2, D), z(D), z(D + 4)),
           lambda: ops.tokens_bwd2(z(B * (np_ + 2), D), B, np_, D, z(B * np_, D, dt=torch.int32), z(np_ + 2, D), z(D), z(D)),
           lambda: ops.tokens_bwd2(z(B * (np_ + 1), D), B, np_, D, None, z(np_ + 2, D), z(D), z(D))]
    for f in bad:
        with pytest.raises(_lib.M3Error):
            f()
    D = 6                                                          # D % 4 != 0: refused by the library
    with pytest.raises(_lib.M3Error):
        ops.assemble_tokens2(z(B * np_, D), z(D), z(D), z(np_ + 2, D), B, np_, D, z(B * (np_ + 2), D))
