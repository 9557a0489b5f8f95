"""GPU: the batched weight-gradient launch (m3_wgrad_multi, csrc/wgrad_multi.hip: several dense weights over the same rows in one
launch, one common number of row parts) against torch fp64 on the same rounded operands and against the same problems issued
one by one through ops.wgrad_tn: a block's four weights on rows that are no multiple of a step, partial and single tiles with
an empty trailing part, one problem, eight problems, the queue's ride-along reductions in every order of single and batched
calls, guards around every output and the workspace, bit-identical repeats, and the refused alias."""
import ctypes

import pytest
import torch

import kernel_contract as kc

pytestmark = pytest.mark.gpu
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}          # relative Frobenius, as tests/test_wgrad_dma.py
DTYPES = [torch.float16, torch.bfloat16]
F32 = torch.float32
BLOCK = [(384, 384), (1152, 384), (1536, 384), (384, 1536)]            # proj, qkv, fc1, fc2 of a ViT-S block
SMALL = [(136, 72), (8, 8), (128, 264)]                               # partial tiles, a single tile far from full


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    return _ops


def dev():
    return torch.device("cuda:0")


def rel(a, b):
    a = a.double().flatten().cpu(); b = b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rnd(*shape, seed=0, dtype=torch.float16):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype).to(dev())


def case_signatures(ops):
    """{case id: launch signature (launch_signature.wgrad_multi_signature)} of the batches the tests below launch, from dummy
    argument structs: what tests/test_engine_launch_census_gpu.py compares the engine's m3_wgrad_multi launches with"""
    import launch_signature as ls
    out = {}
    for dtype in DTYPES:
        for cid, shapes, bias in (("block", BLOCK, [True, True, False, True]), ("small", SMALL, [True] * len(SMALL))):
            a = ops.WgradMultiArgs()
            a.dtype, a.n = ops.dt_code(dtype), len(shapes)
            for j, (N, K) in enumerate(shapes):
                a.prob[j].N, a.prob[j].K, a.prob[j].db = N, K, ls.DUMMY if bias[j] else None
            out[f"{cid}/{dtype}"] = ls.wgrad_multi_signature(ops, a)
    return out


_CASES = {}


def case(M, shapes, dtype, seed=0):
    """operands of a batch and their fp64 results, made once per (M, shapes, dtype) and never written"""
    key = (M, tuple(shapes), dtype, seed)
    if key not in _CASES:
        ops_ = []
        for j, (N, K) in enumerate(shapes):
            dC, A = rnd(M, N, seed=seed + 10 * j + 1, dtype=dtype), rnd(M, K, seed=seed + 10 * j + 2, dtype=dtype)
            ops_.append((dC, A, dC.double().t() @ A.double(), dC.double().sum(0)))
        _CASES[key] = ops_
    return _CASES[key]


def outputs(shapes, bias, seed=90):
    """non-zero dW / db to accumulate onto (and their copies)"""
    base = [(rnd(N, K, seed=seed + j, dtype=F32), rnd(N, seed=seed + 50 + j, dtype=F32) if bias[j] else None) for j, (N, K) in enumerate(shapes)]
    return base, [(w.clone(), None if b is None else b.clone()) for w, b in base]


def check_batch(ops, M, shapes, dtype, bias, parts, queue=None):
    cs = case(M, shapes, dtype)
    base, out = outputs(shapes, bias)
    ops.wgrad_multi([(c[0], c[1], o[0], o[1], 1) for c, o in zip(cs, out)], M, parts=parts, queue=queue)
    if queue is not None:
        queue.flush()
    _, one = outputs(shapes, bias)
    for c, o in zip(cs, one):
        ops.wgrad_tn(c[0], c[1], o[0], beta=1, db=o[1])
    for j, (c, b, o, s) in enumerate(zip(cs, base, out, one)):
        assert rel(o[0] - b[0], c[2]) < TOL[dtype], (j, shapes[j])
        assert rel(o[0] - b[0], s[0] - b[0]) < TOL[dtype], (j, shapes[j])
        if bias[j]:
            assert rel(o[1] - b[1], c[3]) < TOL[dtype], (j, shapes[j])
            assert rel(o[1] - b[1], s[1] - b[1]) < TOL[dtype], (j, shapes[j])
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("parts", [0, 3])
def test_block_weights_on_591_rows(ops, dtype, parts):
    """M = 3 x 197: 18 steps of 32 rows and one of 15; bias on three of the four; beta = 1 onto non-zero dW / db"""
    M = 591
    p = ops.wgrad_multi_plan([(N, K, True) for N, K in BLOCK], M, dtype, parts)
    assert p.allowed and p.tiles == 108 and p.parts == (parts or 1) and p.workgroups == 108 * p.parts
    check_batch(ops, M, BLOCK, dtype, [True, True, False, True], parts)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shapes", [SMALL, SMALL[:1], SMALL[1:2]], ids=["three", "one", "one-8x8"])
@pytest.mark.parametrize("parts", [3, 4])
def test_partial_tiles_and_an_empty_part(ops, dtype, shapes, parts):
    """M = 65: three steps of 32 rows (the last holds one row) - with 4 parts the trailing part has no rows and must still
    leave a zero slab for the reduction; with 3 every part has one step"""
    check_batch(ops, 65, shapes, dtype, [True] * len(shapes), parts)


def test_eight_problems(ops):
    shapes = [(136, 72), (8, 8), (128, 264), (384, 384), (72, 136), (264, 128), (16, 392), (200, 200)]
    assert len(shapes) == 8
    check_batch(ops, 130, shapes, torch.float16, [j % 2 == 0 for j in range(8)], 2)
    with pytest.raises(AssertionError):
        ops.wgrad_multi_plan([(8, 8, False)] * 9, 130, torch.float16)


def test_two_runs_give_identical_bits(ops):
    """slabs summed in part order, no atomics: the result does not depend on what the workspace held or on scheduling"""
    M, dtype, bias = 591, torch.float16, [True] * 4
    cs = case(M, BLOCK, dtype)
    runs = []
    for fill in (0.0, float("nan")):
        _, out = outputs(BLOCK, bias)
        ws = torch.full((ops.wgrad_multi_ws_elems([(N, K, True) for N, K in BLOCK], M, dtype, 4),), fill, device=dev())
        ops.wgrad_multi([(c[0], c[1], o[0], o[1], 1) for c, o in zip(cs, out)], M, parts=4, ws=ws)
        runs.append(out)
    for a, b in zip(*runs):
        assert kc.same_bits(a[0], b[0]) and kc.same_bits(a[1], b[1])


def test_queue_chains_single_and_batched_calls(ops):
    """multi -> multi, single -> multi, multi -> single, flush: every reduction rides in front of the next launch, the two
    workspaces of the queue in turn; against the same calls without a queue (same parts: same bits)"""
    M, dtype = 130, torch.float16
    A_sh, B_sh = [(136, 72), (8, 8)], [(128, 264), (72, 136), (264, 128)]
    cA, cB = case(M, A_sh, dtype, seed=300), case(M, B_sh, dtype, seed=400)
    (dCs, As, _, _), = case(M, [(200, 200)], dtype, seed=500)
    need = max(ops.wgrad_multi_ws_elems([(N, K, True) for N, K in sh], M, dtype, 2) for sh in (A_sh, B_sh))
    need = max(need, ops.wgrad_launch_plan(M, 200, 200, 1, dtype, grouped=False, splits=2).ws_elems)

    def run(queue):
        res = []

        def multi(cs, shapes, seed):
            _, out = outputs(shapes, [True] * len(shapes), seed=seed)
            ops.wgrad_multi([(c[0], c[1], o[0], o[1], 1) for c, o in zip(cs, out)], M, parts=2, queue=queue)
            res.extend(out)

        def single(seed):
            _, out = outputs([(200, 200)], [True], seed=seed)
            ops.wgrad_tn(dCs, As, out[0][0], beta=1, db=out[0][1], splits=2, queue=queue)
            res.extend(out)
        multi(cA, A_sh, 600); multi(cB, B_sh, 610)          # multi -> multi
        single(620); multi(cA, A_sh, 630)                   # single -> multi
        single(640)                                         # multi -> single
        if queue is not None:
            assert queue.pending is not None
            queue.flush()
            assert queue.pending is None
        return res
    want = run(None)
    got = run(ops.WgradQueue(need, dev()))
    assert len(want) == len(got) == 9
    for j, (a, b) in enumerate(zip(got, want)):
        assert kc.same_bits(a[0], b[0]) and kc.same_bits(a[1], b[1]), j


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_stray_writes(ops, dtype):
    """dW, db and an exactly sized workspace between guards; the operands keep their bits"""
    M, shapes, parts = 65, SMALL, 4
    cs = case(M, shapes, dtype)
    need = ops.wgrad_multi_ws_elems([(N, K, True) for N, K in shapes], M, dtype, parts)
    assert need == parts * sum(N * (K + 1) for N, K in shapes)
    ws, wcheck = kc.guarded_ws(need)
    outs, checks = [], [wcheck]
    for N, K in shapes:
        dW, c1 = kc.guarded(N, K, F32)
        db, c2 = kc.guarded(1, N, F32)
        outs.append((dW, db)); checks += [c1, c2]
    snap = kc.snapshot(**{f"dC{j}": c[0] for j, c in enumerate(cs)}, **{f"A{j}": c[1] for j, c in enumerate(cs)})
    ops.wgrad_multi([(c[0], c[1], o[0], o[1].view(-1), 0) for c, o in zip(cs, outs)], M, parts=parts, ws=ws)
    torch.cuda.synchronize()
    for c in checks:
        c()
    kc.unchanged(snap)
    for c, o in zip(cs, outs):
        assert rel(o[0], c[2]) < TOL[dtype] and rel(o[1], c[3]) < TOL[dtype]


def test_prev_reduction_into_this_launchs_dW_is_refused(ops):
    """the library refuses a prev reduction that writes a dW (or db) of the launch it would ride on; ops.WgradQueue never
    builds one - it runs such a reduction first"""
    from m3vit_amd import _lib
    M, dtype = 65, torch.float16
    (dC, A, _, _), = case(M, SMALL[:1], dtype)
    N, K = SMALL[0]
    dW, db = torch.zeros(N, K, device=dev()), torch.zeros(N, device=dev())
    other = torch.zeros(N, K, device=dev())
    slabs = torch.zeros(N * K, device=dev())
    ws = torch.zeros(ops.wgrad_multi_ws_elems([(N, K, True)], M, dtype, 1), device=dev())

    def call(prev_dW, prev_db):
        a = _lib.WgradMultiArgs()
        a.M = M; a.dtype = ops.dt_code(dtype); a.n = 1; a.parts = 1; a.ws = ws.data_ptr()
        q = a.prob[0]
        q.dC = dC.data_ptr(); q.lddc = N; q.A = A.data_ptr(); q.lda = K; q.N = N; q.K = K
        q.dW = dW.data_ptr(); q.db = db.data_ptr(); q.beta = 1; q.beta_db = 1
        prev = (_lib.WgradReduceDesc * 1)()
        prev[0].ws = slabs.data_ptr(); prev[0].splits = 1; prev[0].elems = N * K; prev[0].G = 1
        prev[0].dW = prev_dW.data_ptr(); prev[0].beta = 1
        if prev_db is not None:
            bslab = torch.zeros(N, device=dev())
            prev[0].bias_ws = bslab.data_ptr(); prev[0].bias_elems = N; prev[0].db = prev_db.data_ptr(); prev[0].beta_db = 1
        out = (_lib.WgradReduceDesc * 1)()
        a.prev = ctypes.cast(prev, ctypes.POINTER(_lib.WgradReduceDesc)); a.n_prev = 1
        a.reduce_out = ctypes.cast(out, ctypes.POINTER(_lib.WgradReduceDesc))
        rc = _lib.lib().m3_wgrad_multi(ctypes.byref(a), None)
        torch.cuda.synchronize()
        return rc
    assert call(other, None) == 0
    assert call(dW, None) != 0
    assert call(other, db) != 0
    # through the queue the same sequence is legal: the pending reduction into dW runs before the launch
    q = ops.WgradQueue(max(ws.numel(), 2 * N * (K + 1)), dev())
    ops.wgrad_tn(dC, A, dW, beta=0, db=db, splits=2, queue=q)
    assert q.pending is not None
    ops.wgrad_multi([(dC, A, dW, db, 1)], M, parts=1, queue=q)
    q.flush()
    ref = 2 * (dC.double().t() @ A.double())
    assert rel(dW, ref) < TOL[dtype]
