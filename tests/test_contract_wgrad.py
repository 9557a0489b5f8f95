"""GPU contract tests of m3_wgrad_tn and its reductions: the register-staged (wgrad_set_dma(0)), LDS-DMA (wgrad_set_dma(2)),
256 x 256 and skinny (K = 16 / 32) kernels; slab mode with 1 (direct) to 7 row splits, balanced units with an empty and a hot
expert, direct mode, a WgradQueue ride-along, G > 64; beta = 1 onto a non-zero prior dW; padded lddc / lda through the C ABI
with m3_wgrad_reduce, m3_wgrad_reduce_grouped and m3_wgrad_bias_reduce called directly; m3_colsum.  Every workspace is
exactly the size the library reports and sentinel-NaN-filled (a read of a slab slot nobody wrote shows as NaN), every output
is guarded, inputs keep their bits, and a second call under a different workspace fill must give the same bits (the slab
sums run in a fixed order).

Every run() call states the kernel it is meant to land on AFTER the library's step-downs (wgrad.hip: wgrad_demote) and
asserts it, with the instance flags (gathered dC rows, gathered A rows, per-row factor), through m3_wgrad_kernel on the
argument struct ops.wgrad_tn fills and launches.  plan_args() builds the same struct from dummy addresses (no GPU):
tests/test_launch_paths_cpu.py pins the cases with it, tests/test_engine_launch_census_gpu.py compares the engine's
launches with them (cases())."""
from ctypes import byref

import pytest
import torch

import kernel_contract as kc
import launch_signature as ls

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
        print("\nweight gradient worst err/bound:", max(WORST.values()), max(WORST, key=WORST.get))


def rnd(*shape, dtype=F32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def routing(G, counts):
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    grp = torch.repeat_interleave(torch.arange(G), torch.tensor(counts)).cuda()
    return torch.tensor(off, dtype=torch.int32).cuda(), grp, off[-1]


def reference(dC, A, N, K, G, grp, Mv, splits, dtype, c_idx=None, c_div=1, c_scale=None, a_idx=None, a_div=1):
    """fp64 dW [G, N, K], db [G, N] and their bounds: an fp32 sum over the rows of a group (plus the slab / unit partial sums
    and one prior): (rows_g + splits + 2) u32 sum |dC| |A|; a c_row_scale row is rounded to the operand dtype on its way in:
    u_act |s dC|^T |A|; the store is fp32"""
    f64 = torch.float64
    rc = (c_idx.long()[:Mv] // c_div) if c_idx is not None else torch.arange(Mv, device="cuda")
    ra = (a_idx.long()[:Mv] // a_div) if a_idx is not None else torch.arange(Mv, device="cuda")
    L, R = dC.to(f64)[rc], A.to(f64)[ra]
    if c_scale is not None:
        L = L * c_scale.to(f64)[c_idx.long()[:Mv]].unsqueeze(1)
    W = torch.zeros(G, N, K, dtype=f64, device="cuda"); aW = torch.zeros_like(W)
    db = torch.zeros(G, N, dtype=f64, device="cuda"); adb = torch.zeros_like(db)
    n = torch.zeros(G, 1, 1, dtype=f64, device="cuda")
    for g in range(G):
        sel = (grp[:Mv] == g).nonzero().flatten()
        if sel.numel():
            W[g] = L[sel].t() @ R[sel]; aW[g] = L[sel].abs().t() @ R[sel].abs()
            db[g] = L[sel].sum(0); adb[g] = L[sel].abs().sum(0)
            n[g] = sel.numel()
    rnd_in = kc.u(dtype) if c_scale is not None else 0.0
    bW = kc.gemm_bound(None, None, W, F32, K=n + splits + 2, extra=rnd_in * aW, absacc=aW)
    bdb = kc.SAFETY * ((n[:, :, 0] + splits + 2) * kc.U32 * adb + rnd_in * adb + kc.store(F32, db))
    return W, db, bW, bdb


def plan_args(ops, dtype, M, N, K, *, G=1, grouped=False, splits=None, want_db=True, gc=False, c_div=1, sc=False, ga=False,
              a_div=1):
    """the argument struct ops.wgrad_tn fills for a run() call, with dummy addresses in place of the operands: the same
    m3_wgrad_plan request, the same mode fields.  Host only"""
    p = ops.wgrad_launch_plan(M, N, K, G, dtype, grouped=grouped, bias=want_db, splits=splits or 0, direct_ok=ops._WGRAD_DIRECT)
    on = lambda cond: ls.DUMMY if cond else None                                  # noqa: E731
    a = ops.WgradArgs()
    a.dC, a.lddc, a.c_row_idx, a.c_row_div, a.c_row_scale = ls.DUMMY, N, on(gc), c_div, on(sc)
    a.A, a.lda, a.a_row_idx, a.a_row_div = ls.DUMMY, K, on(ga), a_div
    a.M, a.N, a.K, a.G = M, N, K, G
    a.group_offsets = on(grouped)
    a.splits, a.chunk_rows, a.units = p.splits, p.chunk_rows, p.units
    a.ws, a.dtype = ls.DUMMY, ops.dt_code(dtype)
    a.direct_dW, a.direct_db = on(p.direct), on(p.direct and want_db)
    a.bias_ws = on(want_db and not p.direct)
    return a


def run(ops, dtype, M, N, K, *, kernel, G=1, counts=None, splits=None, beta=0, want_db=True, c_idx=None, c_div=1, c_scale=None,
        a_idx=None, a_div=1, dC=None, A=None, tag=""):
    """one ops.wgrad_tn call with guarded dW / db and an exactly sized, sentinel-filled workspace; checks values, guards,
    inputs and bitwise repeatability under a different workspace fill.  kernel: the one the call is meant to land on after
    the library's step-downs - asserted, with the instance flags, on the struct that is launched.  Returns the worst
    err / bound ratio."""
    flags = dict(gc=c_idx is not None, ga=a_idx is not None, sc=c_scale is not None)
    want = ls.wgrad_signature(ops, plan_args(ops, dtype, M, N, K, G=G, grouped=counts is not None, splits=splits, want_db=want_db,
                                             c_div=c_div, a_div=a_div, **flags))
    assert (want.get("kernel"), want.get("gc"), want.get("ga"), want.get("sc")) == (kernel, *map(int, flags.values())), f"{want} is not {kernel} {flags}"
    if counts is not None:
        off, grp, Mv = routing(G, counts)
    else:
        off, grp, Mv = None, torch.zeros(M, dtype=torch.long, device="cuda"), M
    rows_c = M if c_idx is None else int(c_idx.max()) // c_div + 1
    rows_a = M if a_idx is None else int(a_idx.max()) // a_div + 1
    dC = rnd(rows_c, N, dtype=dtype, seed=1) if dC is None else dC
    A = rnd(rows_a, K, dtype=dtype, seed=2) if A is None else A
    grouped = off is not None
    p = ops.wgrad_launch_plan(M, N, K, G, dtype, grouped=grouped, bias=want_db, splits=splits or 0)
    sp, need = p.splits, p.ws_elems                               # (slabs: this workspace is sized as for a call without direct mode)
    assert need == p.units * N * (K + (1 if want_db else 0))
    if splits is None:
        assert need == ops.wgrad_ws_elems(M, N, K, G, grouped, bias=want_db, dtype=dtype)
    ws, wcheck = kc.guarded_ws(need)
    prior = rnd(G * N, K, seed=3) if beta else None
    prior_db = rnd(G, N, seed=4) if beta else None
    dW, dWcheck = kc.guarded(G * N, K, F32)
    db, dbcheck = kc.guarded(G, N, F32) if want_db else (None, None)
    if beta:
        dW.copy_(prior)
        if want_db:
            db.copy_(prior_db)
    snap = kc.snapshot(dC=dC, A=A, c_idx=c_idx, c_scale=c_scale, a_idx=a_idx, off=off)
    shape = (G, N, K) if G > 1 else (N, K)
    kw = dict(M=M, beta=beta, splits=sp, ws=ws, c_row_idx=c_idx, c_row_div=c_div, c_row_scale=c_scale, a_row_idx=a_idx,
              a_row_div=a_div, group_offsets=off)
    with ls.Recorder(ops) as rec:
        ops.wgrad_tn(dC, A, dW.view(shape), db=db.view(G, N) if want_db and G > 1 else (db.view(N) if want_db else None), **kw)
    ((_, launched, _),) = rec.calls
    got = ls.wgrad_signature(ops, launched)
    assert got == want, f"the call ran\n  {got}\nand states\n  {want}"
    torch.cuda.synchronize()
    kc.unchanged(snap); wcheck(); dWcheck()
    if want_db:
        dbcheck()
    W, rdb, bW, bdb = reference(dC, A, N, K, G, grp, Mv, sp, dtype, c_idx, c_div, c_scale, a_idx, a_div)
    if beta:
        W = W + prior.double().view(G, N, K)
        bW = bW + kc.SAFETY * kc.U32 * W.abs()
        if want_db:
            rdb = rdb + prior_db.double()
            bdb = bdb + kc.SAFETY * kc.U32 * rdb.abs()
    w = kc.assert_within(dW.view(G, N, K), W, bW, what="dW")
    if want_db:
        w = max(w, kc.assert_within(db, rdb, bdb, what="db"))
    if not beta:
        # the same call again with the workspace full of other garbage: the same bits
        ws.normal_()
        dW2 = torch.full((G * N, K), 3.0, device="cuda")
        db2 = torch.full((G, N), 3.0, device="cuda") if want_db else None
        ops.wgrad_tn(dC, A, dW2.view(shape), db=(db2.view(G, N) if G > 1 else db2.view(N)) if want_db else None, **kw)
        torch.cuda.synchronize()
        assert kc.same_bits(dW2, dW.contiguous()), "dW depends on the workspace's prior contents"
        if want_db:
            assert kc.same_bits(db2, db.contiguous()), "db depends on the workspace's prior contents"
    WORST[tag] = w
    return w


class knobs:
    """wgrad_set_dma / wgrad_set_big for the duration of a test, restored in any case"""

    def __init__(self, ops, dma=None, big=None):
        self.ops, self.dma, self.big = ops, dma, big

    def __enter__(self):
        if self.dma is not None:
            self.ops.wgrad_set_dma(self.dma)
        if self.big is not None:
            self.ops.wgrad_set_big(self.big)

    def __exit__(self, *exc):
        if self.dma is not None:
            self.ops.wgrad_set_dma(-1)
        if self.big is not None:
            self.ops.wgrad_set_big(-1)


# kernel id: dtype, N, K, wgrad_set_dma, wgrad_set_big, bias column sums, the kernel a plain call is meant to run
KERNELS = {
    "staged_f16": (F16, 384, 192, 0, 0, True, "staged"),
    "staged_bf16": (BF16, 132 + 4, 200, 0, 0, True, "staged"),
    "staged_f32": (F32, 132, 68, 0, 0, True, "staged"),
    "dma_f16": (F16, 384, 192, 2, 0, True, "dma"),
    "dma_bf16": (BF16, 136, 200, 2, 0, True, "dma"),
    "dma_f32": (F32, 132, 68, 2, 0, True, "dma"),
    "big_f16": (F16, 256, 512, None, 1, True, "big"),
    "big_bf16": (BF16, 512, 256, None, 1, True, "big"),
    "skinny16_f16": (F16, 384, 16, None, None, False, "skinny"),
    "skinny32_bf16": (BF16, 384, 32, None, None, False, "skinny"),
    "skinny32_f16": (F16, 384, 32, None, None, False, "skinny"),
    "skinny16_bf16": (BF16, 384, 16, None, None, False, "skinny"),
    "skinny16_f32": (F32, 384, 16, None, None, False, "skinny"),          # the engine's fp32 router weight (E = 16)
    "skinny32_f32": (F32, 384, 32, None, None, False, "skinny"),
}
SPLITS = [1, 2, 3, 5, 7]
GROUPED_KERNELS = ["staged_f16", "dma_f16", "dma_f32", "big_f16", "dma_bf16", "big_bf16"]
GROUPED_SPLITS = [None, 1, 4]
GROUPED_COUNTS = [0, 700, 0, 45, 129, 0]


def plain_kernel(kern, splits):
    """the kernel of a plain call of KERNELS[kern] cut into `splits` parts.  The streaming kernel writes slabs only: with one
    part ops.wgrad_tn takes direct mode, and the call steps down to the 128 x 128 kernel of the default m3_wgrad_set_dma
    rule - LDS-DMA for fp32, register-staged for these small 16-bit weights"""
    dtype, stated = KERNELS[kern][0], KERNELS[kern][6]
    if stated == "skinny" and splits == 1:
        return "dma" if dtype == F32 else "staged"
    return stated


def scaled_kernel(kern):
    """the kernel of the grouped call with a per-row factor (gathered dC rows scaled by the gate score): the 256 x 256
    kernel has the factor for fp16 only, the 128-wide LDS-DMA kernel for fp16 and fp32 - a bf16 call steps down to the
    register-staged kernel from either"""
    dtype, stated = KERNELS[kern][0], KERNELS[kern][6]
    return "staged" if dtype == BF16 else stated


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("kern", list(KERNELS))
def test_wgrad_kernels_and_slab_splits(ops, kern, splits):
    """splits = 1 is direct mode for the 128 / 256 tiles (the kernel adds into dW itself, no slabs); 2..7 slab mode"""
    dtype, N, K, dma, big, want_db, kernel = KERNELS[kern]
    M = 333
    with knobs(ops, dma, big):
        if kern.startswith("skinny"):
            assert ops.wgrad_skinny(N, K)
        if kern.startswith("big"):
            assert ops.wgrad_tile(N, K, dtype) == (256, 256)
        kernel = plain_kernel(kern, splits)
        w = run(ops, dtype, M, N, K, kernel=kernel, splits=splits, want_db=want_db, tag=f"{kern}/{splits}")
        w = max(w, run(ops, dtype, M, N, K, kernel=kernel, splits=splits, want_db=want_db, beta=1, tag=f"{kern}/{splits}/beta1"))
    assert w < 1


@pytest.mark.parametrize("splits", GROUPED_SPLITS)
@pytest.mark.parametrize("kern", GROUPED_KERNELS)
def test_wgrad_grouped_balanced_and_direct(ops, kern, splits):
    """grouped: an empty first / middle / last expert and one hot one (balanced units give it more workgroups), slack rows
    past group_offsets[G]; rows gathered (a_row_idx / 2) and dC read through the combine's slot map (c_row_idx / k = 2) scaled
    by the gate score.  bf16 rows with a per-row factor are the one call both LDS-DMA kernels must refuse (the 256 x 256
    kernel has the factor for fp16 only, the 128-wide one for fp16 and fp32): it has to land on the register-staged kernel,
    and run() asserts that it does; the fp16 and fp32 calls with a factor stay on the LDS-DMA kernel they name"""
    dtype, N, K, dma, big, _, kernel = KERNELS[kern]
    counts = GROUPED_COUNTS
    G, M = len(counts), sum(counts) + 19
    g = torch.Generator().manual_seed(5)
    c_idx = torch.randperm(2 * M, generator=g)[:M].to(torch.int32).cuda()
    c_scale = (torch.rand(2 * M, generator=g) + 0.5).cuda()
    a_idx = torch.randint(0, 2 * M, (M,), generator=g, dtype=torch.int32).cuda()
    with knobs(ops, dma, big):
        w = run(ops, dtype, M, N, K, kernel=scaled_kernel(kern), G=G, counts=counts, splits=splits, c_idx=c_idx, c_div=2,
                c_scale=c_scale, a_idx=a_idx, a_div=2, tag=f"grouped/{kern}/{splits}")
        w = max(w, run(ops, dtype, M, N, K, kernel=kernel, G=G, counts=counts, splits=splits, beta=1, a_idx=a_idx, a_div=2,
                       tag=f"grouped/{kern}/{splits}/beta1"))
    assert w < 1


def many_groups_counts(G):
    g = torch.Generator().manual_seed(G)
    counts = torch.randint(0, 50, (G,), generator=g).tolist()
    counts[0] = counts[G // 2] = counts[-1] = 0
    counts[3] = 200
    return counts, sum(counts) + 7


@pytest.mark.parametrize("G", [65, 96])
def test_wgrad_more_than_64_groups(ops, G):
    """G > 64: no balanced units (every group in `splits` parts) and the scalar group walk of the kernels"""
    counts, M = many_groups_counts(G)
    for kern in ("staged_f16", "dma_f16"):
        dtype, N, K, dma, big, _, kernel = KERNELS[kern]
        with knobs(ops, dma, big):
            for sp in (1, 2):
                assert run(ops, dtype, M, 128, 64, kernel=kernel, G=G, counts=counts, splits=sp, tag=f"G{G}/{kern}/{sp}") < 1


# Every template instance of the three tile families (wgrad_staged.hip: WgStaged, wgrad_dma.hip: WgDma, WgBig): gathered dC rows
# (gc), gathered A rows (ga), per-row factor on gathered dC rows (sc) by dtype, on a grouped call with balanced units
FAMILIES = {"staged": ("staged_f16", "staged_bf16", "staged_f32"), "dma": ("dma_f16", "dma_bf16", "dma_f32"), "big": ("big_f16", "big_bf16")}


def has_instance(kernel, dtype, gc, ga, sc):
    """the instances the families state (the `instance()` members of the three structs)"""
    if not sc:
        return kernel != "big" or dtype != F32
    if not gc:
        return False
    return {"staged": True, "dma": dtype != BF16, "big": dtype == F16}[kernel]


INSTANCES = [(kernel, kern, gc, ga, sc) for kernel, kerns in FAMILIES.items() for kern in kerns
             for gc in (0, 1) for ga in (0, 1) for sc in (0, 1) if has_instance(kernel, KERNELS[kern][0], gc, ga, sc)]


def instance_case(kern, gc, ga, sc):
    dtype, N, K, dma, big = KERNELS[kern][:5]
    M = sum(GROUPED_COUNTS) + 19
    return (dtype, M, N, K), dict(G=len(GROUPED_COUNTS), grouped=True, splits=4, gc=bool(gc), c_div=2 if gc else 1, sc=bool(sc),
                                  ga=bool(ga), a_div=2 if ga else 1)


def _gathers(M, gc, ga, sc, c_div, a_div, seed=5):
    g = torch.Generator().manual_seed(seed)
    c_idx = torch.randperm(c_div * M, generator=g)[:M].to(torch.int32).cuda() if gc else None
    c_scale = (torch.rand(c_div * M, generator=g) + 0.5).cuda() if sc else None
    a_idx = torch.randint(0, a_div * M, (M,), generator=g, dtype=torch.int32).cuda() if ga else None
    return c_idx, c_scale, a_idx


@pytest.mark.parametrize("kernel,kern,gc,ga,sc", INSTANCES)
def test_wgrad_every_instance(ops, kernel, kern, gc, ga, sc):
    dtype, N, K, dma, big = KERNELS[kern][:5]
    (_, M, _, _), kw = instance_case(kern, gc, ga, sc)
    c_idx, c_scale, a_idx = _gathers(M, gc, ga, sc, kw["c_div"], kw["a_div"])
    with knobs(ops, dma, big):
        assert run(ops, dtype, M, N, K, kernel=kernel, G=kw["G"], counts=GROUPED_COUNTS, splits=4, c_idx=c_idx, c_div=kw["c_div"],
                   c_scale=c_scale, a_idx=a_idx, a_div=kw["a_div"], tag=f"instance/{kern}/{gc}{ga}{sc}") < 1


# The weight gradients as the engine launches them (tests/test_engine_launch_census_gpu.py), under the library's default
# m3_wgrad_set_dma / m3_wgrad_set_big rules: N and K whole tiles; the expert FC2 reads d y through the slot map with divisor
# k = 4, scaled by the gate score, and plain A rows; the expert FC1 gathers its A rows with divisor 4; the dense weights
# are plain with the bias column sums; the router's weight at E = 64 is a K tail without a bias.  splits 1 is direct mode,
# 4 balanced units (grouped) or slabs (dense).  A bf16 expert FC2 on a 256 x 256 shape steps down to the register-staged kernel
ENGINE_SHAPES = {"f32": (F32, 256, 128, "dma"), "f16": (F16, 256, 128, "staged"), "bf16": (BF16, 256, 128, "staged"),
                 "f16_big": (F16, 256, 512, "big"), "bf16_big": (BF16, 256, 512, "big")}
ENGINE_FORMS = {
    "fc2": dict(grouped=True, gc=True, c_div=4, sc=True),
    "fc1": dict(grouped=True, ga=True, a_div=4),
    "dense": dict(),
    "gate64": dict(want_db=False, K=64),
}
ENGINE = [(sh, form, sp) for sh in ENGINE_SHAPES for form in ENGINE_FORMS for sp in (1, 4) if not (sh.endswith("big") and form == "gate64")]


def engine_case(sh, form, sp):
    """(stated kernel, plan_args positional, keyword) of an ENGINE entry"""
    dtype, N, K, kernel = ENGINE_SHAPES[sh]
    kw = dict(ENGINE_FORMS[form])
    K = kw.pop("K", K)
    if kernel == "big" and kw.get("sc") and dtype == BF16:
        kernel = "staged"
    grouped = kw.get("grouped", False)
    M = sum(GROUPED_COUNTS) + 19 if grouped else 333
    return kernel, (dtype, M, N, K), dict(G=len(GROUPED_COUNTS) if grouped else 1, splits=sp, **kw)


def engine_cases():
    for sh, form, sp in ENGINE:
        kernel, args, kw = engine_case(sh, form, sp)
        yield f"engine/{sh}/{form}/{sp}", None, None, kernel, args, kw
    for kernel, kern, gc, ga, sc in INSTANCES:
        args, kw = instance_case(kern, gc, ga, sc)
        yield f"instance/{kern}/{gc}{ga}{sc}", KERNELS[kern][3], KERNELS[kern][4], kernel, args, kw


@pytest.mark.parametrize("sh,form,sp", ENGINE)
def test_wgrad_as_the_engine_launches(ops, sh, form, sp):
    kernel, (dtype, M, N, K), kw = engine_case(sh, form, sp)
    grouped = kw.pop("grouped", False)
    gc, ga, sc = kw.pop("gc", False), kw.pop("ga", False), kw.pop("sc", False)
    c_div, a_div = kw.pop("c_div", 1), kw.pop("a_div", 1)
    c_idx, c_scale, a_idx = _gathers(M, gc, ga, sc, c_div, a_div, seed=6)
    assert run(ops, dtype, M, N, K, kernel=kernel, counts=GROUPED_COUNTS if grouped else None, c_idx=c_idx, c_div=c_div, c_scale=c_scale,
               a_idx=a_idx, a_div=a_div, tag=f"engine/{sh}/{form}/{sp}", **kw) < 1


def cases():
    """every run() call of this module's tables as (case id, wgrad_set_dma, wgrad_set_big, stated kernel, plan_args positional,
    keyword): what the CPU test pins and the engine census is compared with"""
    for kern, (dtype, N, K, dma, big, want_db, kernel) in KERNELS.items():
        for sp in SPLITS:
            yield f"{kern}/{sp}", dma, big, plain_kernel(kern, sp), (dtype, 333, N, K), dict(splits=sp, want_db=want_db)
    G, M = len(GROUPED_COUNTS), sum(GROUPED_COUNTS) + 19
    for kern in GROUPED_KERNELS:
        dtype, N, K, dma, big, _, kernel = KERNELS[kern]
        for sp in GROUPED_SPLITS:
            yield (f"grouped/{kern}/{sp}", dma, big, scaled_kernel(kern), (dtype, M, N, K),
                   dict(G=G, grouped=True, splits=sp, gc=True, c_div=2, sc=True, ga=True, a_div=2))
            yield f"grouped/{kern}/{sp}/beta1", dma, big, kernel, (dtype, M, N, K), dict(G=G, grouped=True, splits=sp, ga=True, a_div=2)
    for G in (65, 96):
        _, M = many_groups_counts(G)
        for kern in ("staged_f16", "dma_f16"):
            dtype, N, K, dma, big, _, kernel = KERNELS[kern]
            for sp in (1, 2):
                yield f"G{G}/{kern}/{sp}", dma, big, kernel, (dtype, M, 128, 64), dict(G=G, grouped=True, splits=sp)
    yield from engine_cases()


def case_signatures(ops):
    """{case id: signature} from dummy structs under each case's knobs.  Host only"""
    out = {}
    for cid, dma, big, kernel, args, kw in cases():
        with knobs(ops, dma, big):
            out[cid] = ls.wgrad_signature(ops, plan_args(ops, *args, **kw))
    return out


def test_wgrad_queue_ride_along(ops):
    """two queued calls: the first one's slab reduction runs in front of the second's launch, the second's at flush()"""
    dtype, N, K, M = F16, 384, 192, 333
    _, units = ops.wgrad_plan(M, 1, 3, False)
    need = units * N * (K + 1)                                   # the slabs of splits = 3, weights and bias
    q = ops.WgradQueue(4, "cuda")
    (w0, c0), (w1, c1) = kc.guarded_ws(need), kc.guarded_ws(need)
    q.ws = [w0, w1]
    outs = []
    for j in range(2):
        dC, A = rnd(M, N, dtype=dtype, seed=10 + j), rnd(M, K, dtype=dtype, seed=20 + j)
        dW, dWc = kc.guarded(N, K, F32)
        db, dbc = kc.guarded(1, N, F32)
        ops.wgrad_tn(dC, A, dW, db=db.view(N), splits=3, queue=q)
        outs.append((dC, A, dW, dWc, db, dbc))
    q.flush()
    torch.cuda.synchronize()
    c0(); c1()
    for j, (dC, A, dW, dWc, db, dbc) in enumerate(outs):
        dWc(); dbc()
        W, rdb, bW, bdb = reference(dC, A, N, K, 1, torch.zeros(M, dtype=torch.long, device="cuda"), M, 3, dtype)
        WORST[f"queue/{j}"] = max(kc.assert_within(dW, W[0], bW[0], what=f"dW[{j}]"),
                                  kc.assert_within(db.view(N), rdb[0], bdb[0], what=f"db[{j}]"))


def _raw_wgrad(ops, *, dC, A, M, N, K, G=1, off=None, splits, ws, bias_ws=None, chunk=0, units=0, dtype):
    a = ops.WgradArgs()
    a.dC, a.lddc = dC.data_ptr(), dC.stride(0)
    a.A, a.lda = A.data_ptr(), A.stride(0)
    a.a_row_div = a.c_row_div = 1
    a.M, a.N, a.K, a.G = M, N, K, G
    a.group_offsets = off.data_ptr() if off is not None else None
    a.splits, a.ws, a.dtype = splits, ws.data_ptr(), ops.dt_code(dtype)
    a.bias_ws = bias_ws.data_ptr() if bias_ws is not None else None
    a.chunk_rows, a.units = chunk, units
    ops.check(ops.lib().m3_wgrad_tn(byref(a), ops._stream()), "m3_wgrad_tn")


@pytest.mark.parametrize("dtype,dma", [(F16, 0), (F16, 2), (BF16, 0), (F32, 2)])
def test_wgrad_padded_strides_and_direct_reductions(ops, dtype, dma):
    """lddc > N and lda > K through the C ABI; the slab reductions called directly: m3_wgrad_reduce (weights, beta 0),
    m3_wgrad_bias_reduce (bias, beta 1 onto a prior), and for a balanced grouped call m3_wgrad_reduce_grouped"""
    es = torch.empty(0, dtype=dtype).element_size()
    N, K, M, sp = 136, 72, 301, 3
    pad = 16 // es
    dC = rnd(M, N + pad, dtype=dtype, seed=30)[:, :N]
    A = rnd(M, K + 2 * pad, dtype=dtype, seed=31)[:, :K]
    ws, wcheck = kc.guarded_ws(sp * N * K + sp * N)
    snap = kc.snapshot(dC=dC, A=A)
    with knobs(ops, dma, 0):
        _raw_wgrad(ops, dC=dC, A=A, M=M, N=N, K=K, splits=sp, ws=ws, bias_ws=ws[sp * N * K:], dtype=dtype)
        dW, dWc = kc.guarded(N, K, F32)
        db, dbc = kc.guarded(1, N, F32)
        prior = rnd(1, N, seed=32)
        db.copy_(prior)
        ops.check(ops.lib().m3_wgrad_reduce(ops._p(ws), sp, N * K, ops._p(dW), 0, None, 0, None, 0, ops._stream()), "reduce")
        ops.check(ops.lib().m3_wgrad_bias_reduce(ops._p(ws[sp * N * K:]), sp, N, ops._p(db), 1, ops._stream()), "bias_reduce")
        torch.cuda.synchronize()
    kc.unchanged(snap); wcheck(); dWc(); dbc()
    W, rdb, bW, bdb = reference(dC, A, N, K, 1, torch.zeros(M, dtype=torch.long, device="cuda"), M, sp, dtype)
    w = kc.assert_within(dW, W[0], bW[0], what="dW")
    rdb = rdb[0] + prior.double().view(N)
    w = max(w, kc.assert_within(db.view(N), rdb, bdb[0] + kc.SAFETY * kc.U32 * rdb.abs(), what="db"))
    # balanced grouped units reduced by m3_wgrad_reduce_grouped, beta 1 onto a prior
    counts = [0, 250, 31, 0]
    G = len(counts)
    off, grp, Mv = routing(G, counts)
    chunk, units = ops.wgrad_plan(M, G, 2, True)
    ws2, wcheck2 = kc.guarded_ws(units * N * K + units * N)
    with knobs(ops, dma, 0):
        _raw_wgrad(ops, dC=dC, A=A, M=M, N=N, K=K, G=G, off=off, splits=2, ws=ws2, bias_ws=ws2[units * N * K:], chunk=chunk,
                   units=units, dtype=dtype)
        dW2, dW2c = kc.guarded(G * N, K, F32)
        db2, db2c = kc.guarded(G, N, F32)
        pw, pb = rnd(G * N, K, seed=33), rnd(G, N, seed=34)
        dW2.copy_(pw); db2.copy_(pb)
        ops.check(ops.lib().m3_wgrad_reduce_grouped(ops._p(ws2), ops._p(off), G, chunk, N * K, ops._p(dW2), 1,
                                                    ops._p(ws2[units * N * K:]), N, ops._p(db2), 1, ops._stream()), "reduce_grouped")
        torch.cuda.synchronize()
    wcheck2(); dW2c(); db2c()
    W, rdb, bW, bdb = reference(dC, A, N, K, G, grp, Mv, units, dtype)
    W = W + pw.double().view(G, N, K); rdb = rdb + pb.double()
    w = max(w, kc.assert_within(dW2.view(G, N, K), W, bW + kc.SAFETY * kc.U32 * W.abs(), what="grouped dW"))
    w = max(w, kc.assert_within(db2, rdb, bdb + kc.SAFETY * kc.U32 * rdb.abs(), what="grouped db"))
    WORST[f"raw/{dtype}/{dma}"] = w


@pytest.mark.parametrize("dtype", [F16, BF16, F32])
@pytest.mark.parametrize("grouped", [False, True])
def test_colsum_guarded_workspace(ops, dtype, grouped):
    N, M = 136, 777
    counts = [0, 500, 3, 0, 200] if grouped else None
    G = len(counts) if grouped else 1
    off, grp, Mv = routing(G, counts) if grouped else (None, torch.zeros(M, dtype=torch.long, device="cuda"), M)
    c_idx = torch.randperm(M + 40, generator=torch.Generator().manual_seed(6))[:M].to(torch.int32).cuda()
    dC = rnd(M + 40, N, dtype=dtype, seed=40)
    need = int(ops.lib().m3_colsum_ws_elems(M, N, G))
    ws, wcheck = kc.guarded_ws(need)
    db, dbc = kc.guarded(G, N, F32)
    prior = rnd(G, N, seed=41)
    db.copy_(prior)
    snap = kc.snapshot(dC=dC, c_idx=c_idx)
    ops.check(ops.lib().m3_colsum(ops._p(dC), ops.dt_code(dtype), N, ops._p(c_idx), M, N, G, ops._p(off), ops._p(ws),
                                  ops._p(db), 1, ops._stream()), "m3_colsum")
    torch.cuda.synchronize()
    kc.unchanged(snap); wcheck(); dbc()
    L = dC.double()[c_idx.long()[:Mv]]
    ref = torch.stack([L[grp[:Mv] == g].sum(0) for g in range(G)]) + prior.double()
    aref = torch.stack([L[grp[:Mv] == g].abs().sum(0) for g in range(G)]) + prior.double().abs()
    WORST[f"colsum/{dtype}/{grouped}"] = kc.assert_within(db, ref, kc.sum_bound(aref, Mv + 2, ref, F32), what="db")
