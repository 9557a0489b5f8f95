"""CPU: the checks of tests/kernel_contract.py have teeth.  A plain torch stand-in for a GEMM kernel (fp16 operands, fp32
arithmetic, + bias, GELU, one rounding to fp16 on the store) passes every check; each injected defect - the stray writes,
the wrong values confined to a few elements and the stale workspace read the GPU contract tests guard against - is caught,
and at least one of them passes the suite's older relative-L2 check, which is why the elementwise one exists."""
import pytest
import torch

import kernel_contract as kc

M, N, K, LD = 1000, 384, 384, 392
DEV = "cpu"


def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / 2 ** 0.5))


def gelu_grad64(x):
    return 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * torch.pi) ** 0.5


def rel(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def operands():
    g = torch.Generator().manual_seed(0)
    A = torch.randn(M, K, generator=g).half()
    B = (torch.randn(N, K, generator=g) * 0.05).half()
    bias = torch.randn(N, generator=g) * 0.1
    lin = A.double() @ B.double().t() + bias.double()
    ref = gelu64(lin)
    bound = kc.gemm_bound(A.double(), B.double(), ref, torch.float16, gain=gelu_grad64(lin).abs(),
                          extra=kc.U32 * lin.abs() + kc.gelu_eval_extra(lin))
    return A, B, bias, ref, bound


def kernel(A, B, bias, C, defect=None, c_row_idx=None, ws=None):
    """the stand-in: C[crow(m)] = fp16(GELU(A B^T + bias)) in fp32; `defect` injects one fault"""
    Kd = A.shape[1]
    acc = A.float() @ B.float().t()
    if defect == "k_slice":                                   # the last 8-wide K slice dropped for the first row tile
        acc[:128] -= A[:128, Kd - 8:].float() @ B[:, Kd - 8:].float().t()
    lin = acc + bias
    if defect == "bias_vec":                                  # bias lost from one 4-column vector of one row
        lin[517, 100:104] -= bias[100:104]
    if ws is not None:                                        # the per-column sum of the result goes through a workspace
        ws.copy_(lin.sum(0)[: ws.numel()])
        n = ws.numel() + (1 if defect == "ws_overread" else 0)
        lin[0, :n] += 0 * torch.as_strided(ws, (n,), (1,))
    out = torch.nn.functional.gelu(lin).half()
    rows = torch.arange(A.shape[0]) if c_row_idx is None else c_row_idx.clone()
    if defect == "scatter":                                   # one row lands on a destination it does not own
        rows[7] = C.shape[0] - 1
    C[rows] = out
    full = torch.as_strided(C, (C.shape[0] + 1, C.stride(0)), (C.stride(0), 1))
    if defect == "row_past_m":
        full[C.shape[0], 0] = 1.0
    if defect == "ld_pad":
        full[3, C.shape[1]] = 1.0


def run(operands, defect=None, scatter=False, ws=False):
    """returns (passes elementwise + guards, passes rel < 1e-3)"""
    A, B, bias, ref, bound = operands
    rows = M + 24 if scatter else M
    C, check = kc.guarded(rows, N, torch.float16, ld=LD, device=DEV)
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(1))[:M] if scatter else None
    W, wcheck = kc.guarded_ws(N - 8, device=DEV) if ws else (None, None)
    snap = kc.snapshot(A=A, B=B, bias=bias)
    kernel(A, B, bias, C, defect, perm, W)
    kc.unchanged(snap)
    got = C[perm] if scatter else C
    ok_rel = rel(got, ref) < 1e-3
    try:
        keep = None
        if scatter:
            mask = torch.ones(rows, dtype=torch.bool); mask[perm] = False
            keep = mask.nonzero().flatten()
        check(keep_rows=keep)
        if wcheck:
            wcheck()
        kc.assert_within(got, ref, bound)
    except AssertionError:
        return False, ok_rel
    return True, ok_rel


def test_the_clean_kernel_passes_every_check(operands):
    for kw in ({}, {"scatter": True}, {"ws": True}):
        assert run(operands, **kw) == (True, True), kw
    A, B, bias, ref, bound = operands
    C, _ = kc.guarded(M, N, torch.float16, ld=LD, device=DEV)
    kernel(A, B, bias, C)
    worst = kc.assert_within(C, ref, bound)
    assert 1e-2 < worst < 1, f"the bound is not tight enough to mean anything: worst err/bound {worst}"


@pytest.mark.parametrize("defect,kw", [("row_past_m", {}), ("ld_pad", {}), ("bias_vec", {}), ("k_slice", {}),
                                       ("scatter", {"scatter": True}), ("ws_overread", {"ws": True})])
def test_each_injected_defect_is_caught(operands, defect, kw):
    ok, _ = run(operands, defect, **kw)
    assert not ok, f"defect {defect} went unnoticed"


def test_relative_l2_alone_misses_defects_the_contract_catches(operands):
    missed = [d for d in ("row_past_m", "ld_pad", "bias_vec") if run(operands, d)[1]]
    assert "bias_vec" in missed and len(missed) == 3, missed


def test_guard_reports_the_first_bad_element():
    C, check = kc.guarded(5, 12, torch.float32, ld=16, device=DEV)
    C.fill_(0)
    check()
    torch.as_strided(C, (5, 16), (16, 1))[2, 13] = 0
    with pytest.raises(AssertionError, match=r"row 2, col 13.*row padding"):
        check()
    C2, check2 = kc.guarded(3, 4, torch.int32, device=DEV)
    C2[0] = 1
    with pytest.raises(AssertionError, match="does not own"):
        check2(keep_rows=[0])
    check2(keep_rows=[1, 2])
    assert C2.data_ptr() % kc.ALIGN == 0


def test_sentinels_are_nans_torch_does_not_produce():
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        s = kc.sentinel_like(torch.empty(1, dtype=dt))
        assert bool(torch.isnan(s).all())
        assert not kc.same_bits(s, torch.full((1,), float("nan"), dtype=dt))
        assert kc.same_bits(s, s.clone())


def test_int64_sentinel_is_a_word_no_index_or_count_takes():
    s = kc.sentinel_like(torch.empty(3, dtype=torch.int64))
    assert kc.same_bits(s, s.clone()) and int(s[0]) > 2 ** 62
    C, check = kc.guarded(4, 3, torch.int64, ld=5, device=DEV)
    C.fill_(0)
    check()
    torch.as_strided(C, (4, 5), (5, 1))[1, 4] = 7
    with pytest.raises(AssertionError, match=r"row 1, col 4.*row padding"):
        check()


# ----------------------------------------------------------------------------------------------------- the gate stand-in
# A plain torch restatement of m3_gate_fwd / m3_gate_bwd_logits (the pinned fma chain emulated in fp64: every product of
# two fp32 values is exact there and each step rounds to fp32, as fmaf does - up to a double rounding no input here hits),
# passing every check of kernel_contract.check_gate_fwd / gate_bwd_reference; each injected defect is one the GPU
# contract tests of the router must catch.
GT, GD, GE, GK = 300, 32, 12, 3


def gate_standin(x, w, k, bias, noise, std, out, T_alloc=None, defect=None):
    """writes out[...] (guarded views) like the kernel"""
    T, D = x.shape
    E = w.shape[1]
    acc = (bias.double() if bias is not None else torch.zeros(E, dtype=torch.float64)).float().expand(T, E).clone()
    for d in range(D):
        acc = (x[:, d:d + 1].double() * w[d].double() + acc.double()).float()
    clean = acc
    noisy = clean + noise * torch.tensor(std, dtype=torch.float32) if (noise is not None and std != 0) else clean
    m = noisy.max(1, keepdim=True).values
    q = torch.exp(noisy - m)
    s = (q[:, :-1] if defect == "pad_denominator" else q).sum(1, keepdim=True)
    p = q / s
    kp = min(k + 1, E)
    order = torch.sort(noisy.flip(1) if defect == "ties_high" else noisy, dim=1, descending=True, stable=True).indices
    if defect == "ties_high":
        order = E - 1 - order
    sel = order[:, :kp]
    out["idx"].copy_(sel[:, :k])
    out["idx32"].copy_(sel[:, :k].int())
    out["score"].copy_(p.gather(1, sel[:, :k]))
    out["top_logits"].copy_(p.gather(1, sel))
    if kp > k:
        out["idx_next"].copy_(sel[:, k].int())
    gates = torch.zeros(T, E).scatter(1, sel[:, :k], p.gather(1, sel[:, :k]))
    out["clean"].copy_(clean); out["noisy"].copy_(noisy); out["gates"].copy_(gates)
    if defect == "dense_past_T":
        g = out["gates"]
        torch.as_strided(g, (T + 1, E), (E, 1))[T] = 0.0
    nblk = out["part_load"].shape[0]
    selm = torch.zeros(T, E, dtype=torch.long).scatter(1, sel[:, :k], 1)
    out["part_importance"].copy_(kc._blocks(gates.double(), nblk).float())
    out["part_load"].copy_(kc._blocks(selm if defect == "load_counts_selected" else (gates > 0).long(), nblk).int())
    out["part_count"].copy_(kc._blocks(selm, nblk).int())
    if out.get("part_load_prob") is not None:
        thr_in, thr_out = p.gather(1, sel[:, k:k + 1]), p.gather(1, sel[:, k - 1:k])
        z = (clean - torch.where(noisy > thr_in, thr_in, thr_out)) * (1.0 / torch.tensor(std, dtype=torch.float32))
        out["part_load_prob"].copy_(kc._blocks((0.5 * torch.erfc(-z * 0.70710678)).double(), nblk).float())


def gate_bwd_standin(noisy, clean, top, idx, idx_next, k, d_score, d_top, d_imp, d_lp, bs, std, out, out_act, defect=None):
    T, E = noisy.shape
    m = noisy.max(1, keepdim=True).values
    q = torch.exp(noisy - m)
    p = q * (1.0 / q.sum(1, keepdim=True))
    g = torch.zeros(T, E)
    dthr_in = torch.zeros(T); dthr_out = torch.zeros(T)
    if d_lp is not None:
        is_in = noisy > top[:, k:k + 1]
        z = (clean - torch.where(is_in, top[:, k:k + 1], top[:, k - 1:k])) * (1.0 / torch.tensor(std, dtype=torch.float32))
        g = d_lp * bs * (0.3989422804014327 * torch.exp(-0.5 * z * z)) * (1.0 / torch.tensor(std, dtype=torch.float32))
        dthr_in = -(g * is_in).sum(1); dthr_out = -(g * ~is_in).sum(1)
    dp = torch.zeros(T, E)
    v = d_score.clone() + (d_top[:, :k] if d_top is not None else 0) + (d_imp[idx] * bs if d_imp is not None else 0)
    v[:, k - 1] += dthr_out
    dp.scatter_add_(1, idx, v)
    if k < E:
        vn = (d_top[:, k] if d_top is not None else 0) + (0 if defect == "drop_d_thr_in" else dthr_in)
        dp.scatter_add_(1, idx_next.long().unsqueeze(1), torch.as_tensor(vn).expand(T).unsqueeze(1).float())
    dl = p * (dp - (dp * p).sum(1, keepdim=True)) + g
    out.copy_(dl)
    if out_act is not None:
        if defect == "act_truncated":
            out_act.copy_((dl.view(torch.int32) & ~0xFFFF).view(torch.float32).bfloat16())
        else:
            out_act.copy_(dl.bfloat16())


@pytest.fixture(scope="module")
def gate_inputs():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(GT, GD, generator=g)
    w = torch.randn(GD, GE, generator=g) * 0.3
    w[:, 7] = w[:, 2]                                  # exact ties: experts 2 and 7 always share a logit
    bias = torch.randn(GE, generator=g) * 0.2
    bias[7] = bias[2]
    bias[0:2] = -200.0                                 # two experts whose probabilities underflow to 0: with k = E - 1 one
                                                       # of them is selected all the same
    noise = torch.randn(GT, GE, generator=g)
    return x, w, bias, noise


def run_gate(gate_inputs, defect=None, k=GK, noisy=True):
    """(all checks pass, rel-L2 of the dense gates < 1e-4)"""
    x, w, bias, noise = gate_inputs
    std = 0.05 if noisy else 0.0
    nblk = -(-GT // 64)
    kp = min(k + 1, GE)
    out, checks = {}, []
    for name, (r, c, dt) in {"idx": (GT, k, torch.int64), "idx32": (GT, k, torch.int32), "score": (GT, k, torch.float32),
                             "top_logits": (GT, kp, torch.float32), "idx_next": (GT, 1, torch.int32),
                             "clean": (GT, GE, torch.float32), "noisy": (GT, GE, torch.float32),
                             "gates": (GT, GE, torch.float32), "part_importance": (nblk, GE, torch.float32),
                             "part_load": (nblk, GE, torch.int32), "part_count": (nblk, GE, torch.int32),
                             "part_load_prob": (nblk, GE, torch.float32)}.items():
        v, chk = kc.guarded(r, c, dt, device=DEV)
        out[name] = v.view(GT) if name == "idx_next" else v
        checks.append((name, chk))
    if not noisy:
        out["part_load_prob"] = None
    snap = kc.snapshot(x=x, w=w, bias=bias, noise=noise)
    gate_standin(x, w, k, bias, noise if noisy else None, std, out, defect=defect)
    kc.unchanged(snap)
    from oracle import c_oracle
    c = c_oracle.gate_fwd(x.numpy(), w.numpy(), k, bias=bias.numpy(), noise=noise.numpy() if noisy else None, std=std)
    ref_g = torch.softmax(torch.tensor(c["noisy"]).double(), 1)
    ref_g = torch.zeros_like(ref_g).scatter(1, torch.tensor(c["idx"]), ref_g.gather(1, torch.tensor(c["idx"])))
    ok_rel = rel(out["gates"], ref_g) < 1e-4
    try:
        for name, chk in checks:
            chk(what=name)
        assert torch.equal(out["idx"], torch.tensor(c["idx"])), "idx differs from the C oracle"
        assert kc.same_bits(out["clean"], torch.tensor(c["clean"])), "clean differs from the C oracle"
        worst, near = kc.check_gate_fwd(out, x, w, k, bias=bias, noise=noise if noisy else None, std=std)
    except AssertionError:
        return False, ok_rel
    return True, ok_rel


def run_gate_bwd(gate_inputs, defect=None, k=GK):
    x, w, bias, noise = gate_inputs
    std = 0.05
    out, chk = {}, None
    o = {n: torch.empty(0) for n in ()}
    T, E, kp = GT, GE, min(k + 1, GE)
    fo = dict(idx=torch.empty(T, k, dtype=torch.int64), idx32=torch.empty(T, k, dtype=torch.int32),
              score=torch.empty(T, k), top_logits=torch.empty(T, kp), idx_next=torch.empty(T, dtype=torch.int32),
              clean=torch.empty(T, E), noisy=torch.empty(T, E), gates=torch.empty(T, E),
              part_importance=torch.empty(5, E), part_load=torch.empty(5, E, dtype=torch.int32),
              part_count=torch.empty(5, E, dtype=torch.int32), part_load_prob=torch.empty(5, E))
    gate_standin(x, w, k, bias, noise, std, fo)
    g = torch.Generator().manual_seed(9)
    d_score, d_top = torch.randn(T, k, generator=g), torch.randn(T, kp, generator=g)
    d_imp, d_lp = torch.randn(E, generator=g) * 1e-2, torch.randn(E, generator=g)
    bs = 0.5
    dl, check = kc.guarded(T, E, torch.float32, device=DEV)
    act, acheck = kc.guarded(T, E, torch.bfloat16, device=DEV)
    gate_bwd_standin(fo["noisy"], fo["clean"], fo["top_logits"], fo["idx"], fo["idx_next"], k, d_score, d_top, d_imp, d_lp,
                     bs, std, dl, act, defect=defect)
    ref, bound = kc.gate_bwd_reference(fo["noisy"], fo["idx"], k, clean=fo["clean"], top_logits=fo["top_logits"],
                                       idx_next=fo["idx_next"], d_score=d_score, d_top=d_top, d_importance=d_imp,
                                       d_load_prob=d_lp, balance_scale=bs, noise_std=std)
    ok_rel = rel(dl, ref) < 1e-4
    try:
        check(); acheck()
        worst = kc.assert_within(dl, ref, bound, "d_logits")
        assert kc.same_bits(act, dl.to(torch.bfloat16)), "d_logits_act is not d_logits rounded to nearest even"
    except AssertionError:
        return False, ok_rel, None
    return True, ok_rel, worst


def test_the_clean_gate_standin_passes_every_check(gate_inputs):
    assert run_gate(gate_inputs) == (True, True)
    assert run_gate(gate_inputs, noisy=False) == (True, True)
    assert run_gate(gate_inputs, k=GE - 1)[0]
    ok, ok_rel, worst = run_gate_bwd(gate_inputs)
    assert ok and ok_rel, (ok, ok_rel)
    assert 1e-3 < worst < 1, f"the backward bound is not tight enough to mean anything: worst err/bound {worst}"


def test_the_gate_fixture_has_the_edges_the_defects_need(gate_inputs):
    x, w, bias, noise = gate_inputs
    from oracle import c_oracle
    c = c_oracle.gate_fwd(x.numpy(), w.numpy(), GE - 1, bias=bias.numpy())
    assert (c["score"] == 0).all(1).sum() == 0 and (c["score"] == 0).any(), "a selected probability must underflow"
    idx = torch.tensor(c["idx"])
    assert bool(((idx == 2) | (idx == 7)).any())      # the tied pair is selected


@pytest.mark.parametrize("defect,kw", [("ties_high", {"noisy": False}), ("pad_denominator", {}), ("dense_past_T", {}),
                                       ("load_counts_selected", {"k": GE - 1})])
def test_each_injected_gate_defect_is_caught(gate_inputs, defect, kw):
    ok, _ = run_gate(gate_inputs, defect, **kw)
    assert not ok, f"defect {defect} went unnoticed"


@pytest.mark.parametrize("defect", ["drop_d_thr_in", "act_truncated"])
def test_each_injected_gate_backward_defect_is_caught(gate_inputs, defect):
    ok, _, _ = run_gate_bwd(gate_inputs, defect)
    assert not ok, f"defect {defect} went unnoticed"


def test_relative_l2_alone_misses_gate_defects_the_contract_catches(gate_inputs):
    missed = [d for d in ("dense_past_T", "load_counts_selected") if run_gate(gate_inputs, d, k=GE - 1)[1]]
    missed += [d for d in ("act_truncated",) if run_gate_bwd(gate_inputs, d)[1]]
    assert "dense_past_T" in missed and "act_truncated" in missed, missed


# ----------------------------------------------------------------------------------------------------- far operands
def test_far_rows_places_row_r_at_r_times_the_stride():
    """far_rows on a small stride (CPU, a few KB): the allocation is exactly the span of the rows rounded up to 16 bytes, row r
    starts r * ld_bytes behind row 0, windows of the same rows share the allocation, copy_ touches the rows' own bytes only,
    and check_outside finds a write that lands between two rows - as a store whose offset wrapped at 32 bits would"""
    rows, cols, ld_b, cb = 7, 24, 400 * 16, 64
    for dt in (torch.float16, torch.float32):
        es = torch.empty(0, dtype=dt).element_size()
        v, far = kc.far_rows(rows, cols, ld_b, dt, col_byte=cb, device=DEV)
        assert far.buf.numel() == -(-((rows - 1) * ld_b + cb + cols * es) // 16) * 16
        assert tuple(v.shape) == (rows, cols) and v.stride() == (ld_b // es, 1)
        assert v.data_ptr() - far.buf.data_ptr() == cb and v.data_ptr() % 16 == 0
        for r in range(rows):
            assert v[r].data_ptr() - v.data_ptr() == r * ld_b
        w = far.view(8, dt)                                          # a second window of the same rows, in front of the first
        assert w.data_ptr() == far.buf.data_ptr() and w[rows - 1].data_ptr() - w.data_ptr() == (rows - 1) * ld_b
        with pytest.raises(AssertionError, match="past the allocation"):
            far.view(cols + 8, dt, col_byte=cb)
        far.fill(dt)
        assert kc.same_bits(v.contiguous(), kc.sentinel_like(v))
        far.check_outside([], dt)
        vals = torch.randn(rows, cols).to(dt)
        v.copy_(vals)
        assert kc.same_bits(v.contiguous(), vals)
        far.check_outside([(cb, cols * es)], dt)                        # only the rows' own bytes changed
        with pytest.raises(AssertionError, match="row 0"):
            far.check_outside([(cb, (cols - 4) * es)], dt)              # the window's last columns count as outside
        far.buf[3 * ld_b + cb + cols * es] = 0                          # one byte behind row 3
        for chunk in (1 << 28, ld_b, 2 * ld_b):                         # whole, one row and two rows per chunk
            with pytest.raises(AssertionError, match=rf"row 3 at byte {cb + cols * es}"):
                far.check_outside([(cb, cols * es)], dt, chunk_bytes=chunk)


def test_reach_stride_is_the_last_16_byte_step_under_the_reach():
    assert kc.reach_stride(300) == 14_268_992
    for rows in (1, 3, 100, 300, 333, 1000, 11000, 2 ** 20):
        ld = kc.reach_stride(rows)
        assert ld % 16 == 0 and (rows + 1) * ld < 2 ** 32 <= (rows + 1) * (ld + 16)
    ld = kc.reach_stride(300)
    assert 150 * ld < 2 ** 31 < 151 * ld and 299 * ld + 2 * 1024 < 2 ** 32       # rows 151 .. 299 start above 2^31
    assert kc.reach_stride(9, reach=1 << 12) == 400


# ------------------------------------------------------------------- Inf / NaN helpers: torch stand-ins for a wrong kernel
NAN, INF = float("nan"), float("inf")


def test_nonfinite_agrees_passes_what_torch_gives_and_counts_the_classes():
    x = torch.tensor([[NAN, INF, -INF, 1.5], [0.25, -2.0, 3.0, 7e4]])
    n = kc.nonfinite_agrees(torch.relu(x), torch.relu(x.double()), torch.float32, bound64=0.0)
    assert n == {"nonfinite": 2, "finite": 6}
    # an overflowing store: 1e5 in fp16 is Inf; a finite reference in (1/2, 2) x max is the CASE's fault and says so
    n = kc.nonfinite_agrees(torch.tensor([1.4e5, -1.4e5, 1.0]).half(), torch.tensor([1.4e5, -1.4e5, 1.0]).double(), torch.float16)
    assert n == {"nonfinite": 2, "finite": 1}
    with pytest.raises(AssertionError, match=r"ill-posed.*first at \(1,\)"):
        kc.nonfinite_agrees(torch.tensor([1.0, 7e4]).half(), torch.tensor([1.0, 7e4]).double(), torch.float16)
    with pytest.raises(AssertionError, match=r"first at \(0, 1\).*must be -inf"):           # the wrong sign of Inf
        kc.nonfinite_agrees(torch.tensor([[0.0, INF]]), torch.tensor([[0.0, -INF]]).double(), torch.float32)
    with pytest.raises(AssertionError, match=r"first at \(2,\).*must be finite"):          # a NaN torch does not have
        kc.nonfinite_agrees(torch.tensor([0.0, 1.0, NAN]), torch.tensor([0.0, 1.0, 2.0]).double(), torch.float32)
    with pytest.raises(AssertionError, match=r"exceed their bound; first at \(1,\)"):
        kc.nonfinite_agrees(torch.tensor([NAN, 1.5]), torch.tensor([NAN, 1.0]).double(), torch.float32, bound64=0.25)


def test_a_relu_written_as_where_x_gt_0_is_caught_at_the_nan():
    x = torch.randn(5, 8, generator=torch.Generator().manual_seed(0))
    x[3, 2], x[1, 1], x[4, 7] = NAN, INF, -INF
    ref = torch.nn.functional.relu(x.double())
    kc.nonfinite_agrees(torch.nn.functional.relu(x), ref, torch.float32, bound64=0.0)
    wrong = torch.where(x > 0, x, torch.zeros_like(x))
    assert torch.equal(wrong[x == x], torch.relu(x)[x == x])                      # bit-identical on everything but the NaN
    with pytest.raises(AssertionError, match=r"relu: 1 of 40 elements.*first at \(3, 2\): got 0\.0, ref nan: must be NaN"):
        kc.nonfinite_agrees(wrong, ref, torch.float32, what="relu")


def test_a_tail_mask_written_as_a_product_with_0_is_caught_at_the_leaked_element():
    """rows 0..5 are the call's, rows 6..7 the padding of its last tile: the sum over the tile's rows masks the padding"""
    g = torch.Generator().manual_seed(1)
    tile = torch.randn(8, 4, generator=g)
    valid = (torch.arange(8) < 6).unsqueeze(1)
    right = lambda t: torch.where(valid, t, torch.zeros_like(t)).sum(0, keepdim=True)        # noqa: E731
    wrong = lambda t: (t * valid.float()).sum(0, keepdim=True)                               # noqa: E731
    poisoned = tile.clone()
    poisoned[7, 2] = NAN                                                                     # next door, not the call's
    assert kc.same_bits(right(tile), wrong(tile))                                            # invisible with finite data
    depends = torch.zeros(1, 4, dtype=torch.bool)                                            # nothing depends on row 7
    assert kc.independent_same_bits(right(tile), right(poisoned), depends) == 4
    with pytest.raises(AssertionError, match=r"tile sum: 1 element\(s\).*first at \(0, 2\).*poisoned run nan"):
        kc.independent_same_bits(wrong(tile), wrong(poisoned), depends, what="tile sum")


def test_an_fp16_store_that_clamps_to_65504_is_caught():
    x = torch.tensor([[1.0, -3.0, 2e5], [-2e5, 2.0, INF]])            # 2e5 >= 2 x 65504: out of the (1/2, 2) x max band
    ref = x.double()
    kc.nonfinite_agrees(x.half(), ref, torch.float16, bound64=kc.store(torch.float16, ref))
    wrong = x.clamp(-65504.0, 65504.0).half()
    with pytest.raises(AssertionError, match=r"cast: 3 of 6 elements.*first at \(0, 2\): got 65504\.0, ref 200000\.0: must be inf"):
        kc.nonfinite_agrees(wrong, ref, torch.float16, what="cast")


def test_a_grouped_sum_that_reads_the_next_groups_row_with_weight_0_is_caught():
    """groups of 3, 0 and 2 rows; group g's column sums.  The wrong one walks a tile of 4 rows from the group's first and
    weighs the rows past its end with 0; poison sits in the first row of the group after the ragged one"""
    g = torch.Generator().manual_seed(2)
    rows = torch.randn(5, 4, generator=g)
    off = [0, 3, 3, 5]

    def right(r):
        return torch.stack([r[off[i]:off[i + 1]].sum(0) for i in range(3)])

    def wrong(r):
        padded = torch.cat((r, torch.zeros(4, 4)))
        return torch.stack([(padded[off[i]:off[i] + 4] * (torch.arange(4) < off[i + 1] - off[i]).float().unsqueeze(1)).sum(0)
                            for i in range(3)])

    poisoned = rows.clone()
    poisoned[3, 1] = INF                                                                     # first row of group 2
    assert torch.allclose(right(rows), wrong(rows))
    depends = torch.zeros(3, 4, dtype=torch.bool)
    depends[2, 1] = True                                                                     # column 1 of group 2, nothing else
    assert kc.independent_same_bits(right(rows), right(poisoned), depends) == 11
    kc.nonfinite_agrees(right(poisoned), right(poisoned.double()), torch.float32)
    with pytest.raises(AssertionError, match=r"group sums: 2 element\(s\).*first at \(0, 1\): clean run .* poisoned run nan"):
        kc.independent_same_bits(wrong(rows), wrong(poisoned), depends, what="group sums")
    with pytest.raises(AssertionError, match=r"first at \(0, 1\): got nan, ref .*: must be finite"):
        kc.nonfinite_agrees(wrong(poisoned), right(poisoned.double()), torch.float32)
