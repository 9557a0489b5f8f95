"""m3_set_cache_hints moves no arithmetic: for every family that has a non-temporal instance, the entry point is run with the
hints off (mask 0) and on (its bit) and every output must be equal bit for bit.  Outputs sit inside guard bands
(tests/kernel_contract.py), so a hinted store that strays is seen.  Shapes are the smallest that cover what can go wrong:
two row tiles with a clamped tail (the duplicate-row stores of the specialised epilogues go through the hinted store), a
column tile that is partly off, one and several K slices, grouped calls with an empty group and a gathered A."""
import pytest
import torch

import kernel_contract as kc
import launch_signature as ls

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    yield _ops
    _ops.set_cache_hints(-1)


def rnd(*shape, dtype=F32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def off_and_on(ops, bit, run):
    """run() -> list of (name, output view, guard check) under mask 0 and under `bit`; the two lists must agree bitwise"""
    outs = []
    for mask in (0, bit):
        ops.set_cache_hints(mask)
        try:
            res = run()
            torch.cuda.synchronize()
        finally:
            ops.set_cache_hints(-1)
        for name, view, check in res:
            check(what=f"{name} (mask {mask})")
        outs.append(res)
    for (name, a, _), (_, b, _) in zip(*outs):
        assert kc.same_bits(a, b), f"{name}: hints on and off differ"
        assert not kc.same_bits(a, kc.sentinel_like(a)), f"{name}: never written"


def test_mask_range(ops):
    from m3vit_amd import _lib
    assert _lib.M3_HINT_DEFAULT & ~_lib.M3_HINT_ALL == 0
    with pytest.raises(_lib.M3Error):
        ops.set_cache_hints(_lib.M3_HINT_ALL + 1)
    with pytest.raises(_lib.M3Error):
        ops.set_cache_hints(-2)
    ops.set_cache_hints(-1)


GROUPS = (130, 0, 5)


@pytest.mark.parametrize("grouped", [False, True], ids=["dense", "grouped"])
@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("kind", ["gelu", "gpre"])
def test_gemm(ops, kind, dtype, K, grouped):
    from m3vit_amd import _lib
    N = 136
    M = sum(GROUPS) if grouped else 130
    G = len(GROUPS) if grouped else 1
    B = rnd(G, N, K, dtype=dtype, scale=0.06, seed=2)
    kw = {}
    if grouped:
        off, ts = [0], [0]
        for c in GROUPS:
            off.append(off[-1] + c)
            ts.append(ts[-1] + (c + 127) // 128)
        a_div = 4
        a_rows = (M + a_div - 1) // a_div + 3
        A = rnd(a_rows, K, dtype=dtype, seed=1)
        idx = torch.randint(0, a_rows * a_div, (M,), generator=torch.Generator().manual_seed(3), dtype=torch.int32).cuda()
        kw = dict(a_row_idx=idx, a_row_div=a_div, group_offsets=torch.tensor(off, dtype=torch.int32).cuda(),
                  tile_starts=torch.tensor(ts, dtype=torch.int32).cuda())
    else:
        A = rnd(M, K, dtype=dtype, seed=1)
        B = B[0]
    bias = rnd(G * N, scale=0.1, seed=5)
    gpre = rnd(M, N, dtype=dtype, seed=6)
    bit = _lib.M3_HINT_GEMM_PRE if kind == "gelu" else _lib.M3_HINT_GEMM_GPRE

    def run():
        C, c_check = kc.guarded(M, N, dtype)
        with ls.Recorder(ops) as rec:
            if kind == "gelu":
                pre, pre_check = kc.guarded(M, N, dtype)
                ops.gemm_nt(A, B, C, M=M, bias=bias, act=ops.M3_ACT_GELU, pre_out=pre, **kw)
                res = [("C", C, c_check), ("pre_out", pre, pre_check)]
            else:
                ops.gemm_nt(A, B, C, M=M, gelu_grad_pre=gpre, **kw)
                res = [("C", C, c_check)]
        sig = ls.gemm_signature(ops, rec.calls[0][1])
        assert (sig.get("kernel"), sig.get("epi")) == ("dma", kind), str(sig)     # the kernel that has the hinted instance
        return res
    off_and_on(ops, bit, run)
