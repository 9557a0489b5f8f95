"""GPU: the routing statistics (m3_moe_stats and everything above it).

Kernel contract, in the style of test_contract_rowops.py: record and workspace in guarded buffers, inputs bit-unchanged, row
strides larger than D, all three activation dtypes, two launches bit-identical, and every value against the definitions
below evaluated in float64 ON THE TENSORS THE KERNEL READ (the stored fp32 score / clean / gates / load and the rounded
h / y), so only the kernel's own fp32 arithmetic is charged.  Then end to end: `latest_moe_stats` of a small fused backbone
(eager first call, hipGraph replays, activation checkpointing), fused against per-op, task order, and the flag being off.

Definitions (per MoE block; p = gates [T,E], c = clean [T,E], h [T,D], m[t] = sum_j score[t,j] y[t k + j], load [E]):
  gate_entropy_sum   sum_t sum_e -p ln(max(p, 1e-12))          top1_prob_sum  sum_t max_e p[t,e]
  gate_token_count   T                                          expert_load_hist[e]  #{t : p[t,e] > 0}
  clean_logit_std    mean_t sqrt(mean_e (c - mean_e c)^2)       moe_out_norm_ratio   |m|_2 / (|h|_2 + 1e-12)
  expert_load_cv     var_pop(load) / (mean(load)^2 + 1e-10), 0 for E <= 1

Error bounds (u = 2^-24, all multiplied by kernel_contract.SAFETY; nothing here is tuned to what the kernel gives):
  * a sum of n fp32 terms in any order: kc.sum_bound(sum |terms|, n, ref, float32) = SAFETY (n u sum|terms| + u |ref|);
  * entropy terms: ln is within 3 ulp = 6 u (the OpenCL bound the device math library is built to), the product one more
    rounding, max() and the sign are exact: 8 u |term| per term on top of the sum;
  * m = fma chain over k products: dm <= k u sum_j |s_j y_j|; its square moves by 2 |m| dm + dm^2;
  * a row's population std: the mean of E values is off by dmu <= (E + 1) u mean|c|; every centred value by dmu + u |d|;
    the terms linear in dmu cancel in sum_e d^2 (sum_e d = 0), leaving dS <= (E + 4) u S + E dmu^2; var = S / E one more
    rounding; sqrt: d sqrt(a) <= min(da / (2 sqrt a), sqrt(da)) + u sqrt(a);
  * a quotient a / b: d <= da / b + (a / b) db / b + u a / b - first-order propagation, in `_div`;
  * load as float: counts below 2^24 convert exactly; the CV follows kc.cv2_bound's derivation with the population variance.
expert_load_hist and gate_token_count are integers and must be exact."""
import math

import pytest
import torch

import kernel_contract as kc

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
U = kc.U32
WORST = {}
FLOAT_KEYS = ("gate_entropy_sum", "top1_prob_sum", "clean_logit_std", "moe_out_norm_ratio", "expert_load_cv")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    yield _ops
    if WORST:
        print("\nmoe_stats worst err/bound:", max(WORST.values()), max(WORST, key=WORST.get))


# ------------------------------------------------------------------------------------------- float64 oracle and bounds
def _sqrt(a, da):
    """sqrt(a) and its error for an error da in a (a >= 0), plus the rounding of the root itself"""
    r = math.sqrt(a)
    d = math.sqrt(da) if r == 0.0 else min(da / (2 * r), math.sqrt(da))
    return r, d + U * r


def _div(a, da, b, db):
    q = a / b
    return q, da / abs(b) + abs(q) * db / abs(b) + U * abs(q)


def _cv_pop(v64):
    """(cv, bound) of var_pop(v) / (mean(v)^2 + 1e-10) evaluated in fp32 on the fp32 values v"""
    E = v64.numel()
    if E <= 1:
        return 0.0, 0.0
    mean = float(v64.mean())
    dm = (E + 1) * U * float(v64.abs().mean())
    S = float(((v64 - mean) ** 2).sum())
    dS = (E + 4) * U * S + E * dm * dm
    var, dvar = S / E, dS / E + U * S / E
    den = mean * mean + 1e-10
    dden = 2 * abs(mean) * dm + 3 * U * den
    return _div(var, dvar, den, dden)


def oracle(score, clean, gates, h, y, load):
    """-> (values, bounds): dicts over the record's fields, float64 on the tensors as stored"""
    T, k = score.shape
    E = gates.shape[1]
    D = h.shape[1]
    S = kc.SAFETY
    p, c, s = gates.double(), clean.double(), score.double()
    val, bnd = {}, {}
    terms = -(p * p.clamp_min(1e-12).log())
    ent = float(terms.sum())
    val["gate_entropy_sum"] = ent
    bnd["gate_entropy_sum"] = float(kc.sum_bound(terms.abs().sum(), T * E, terms.sum(), F32)) + S * 8 * U * float(terms.abs().sum())
    top = p.max(dim=1).values if T else p.new_zeros(0)
    val["top1_prob_sum"] = float(top.sum())
    bnd["top1_prob_sum"] = float(kc.sum_bound(top.sum(), T, top.sum(), F32))
    val["gate_token_count"] = T
    val["expert_load_hist"] = [int(v) for v in (gates > 0).sum(0).tolist()]
    # clean logit spread
    if T:
        mu = c.mean(1, keepdim=True)
        dmu = (E + 1) * U * c.abs().mean(1)
        d = c - mu
        Sq = (d * d).sum(1)
        dS = (E + 4) * U * Sq + E * dmu * dmu
        var, dvar = Sq / E, dS / E + U * Sq / E
        std = var.sqrt()
        dstd = torch.where(std > 0, torch.minimum(dvar / (2 * std.clamp_min(1e-300)), dvar.sqrt()), dvar.sqrt()) + U * std
        tot = float(std.sum())
        dtot = T * U * tot + float(dstd.sum())
        val["clean_logit_std"], b = _div(tot, dtot, float(T), 0.0)
        bnd["clean_logit_std"] = S * b
    else:
        val["clean_logit_std"], bnd["clean_logit_std"] = 0.0, 0.0
    # |m|^2 and |h|^2
    y3 = y.double().reshape(T, k, D)
    m = (s.unsqueeze(-1) * y3).sum(1)
    a = (s.abs().unsqueeze(-1) * y3.abs()).sum(1)
    dm = k * U * a
    msq = float((m * m).sum())
    dmsq = T * D * U * msq + float((2 * m.abs() * dm + dm * dm).sum()) + U * msq
    h64 = h.double()
    hsq = float((h64 * h64).sum())
    dhsq = T * D * U * hsq + U * hsq
    val["m_sumsq"], bnd["m_sumsq"] = msq, S * dmsq
    val["h_sumsq"], bnd["h_sumsq"] = hsq, S * dhsq
    rm, drm = _sqrt(msq, dmsq)
    rh, drh = _sqrt(hsq, dhsq)
    den = rh + 1e-12
    val["moe_out_norm_ratio"], b = _div(rm, drm, den, drh + 2 * U * den)
    bnd["moe_out_norm_ratio"] = S * b
    v = load.float().double()                    # the kernel's (float) conversion of a count: exact below 2^24
    assert load.dtype == F32 or int(load.max()) < 2 ** 24
    val["expert_load_cv"], b = _cv_pop(v)
    bnd["expert_load_cv"] = S * b
    return val, bnd


def check_block(got, val, bnd, tag):
    """a parsed block dict (or the raw record's extra fields) against the oracle; returns the worst err / bound"""
    assert got["gate_token_count"] == val["gate_token_count"], tag
    assert got["expert_load_hist"] == val["expert_load_hist"], tag
    worst = 0.0
    for key in FLOAT_KEYS + tuple(k_ for k_ in ("m_sumsq", "h_sumsq") if k_ in got):
        print(f"{tag} {key}: got {got[key]!r} ref {val[key]!r} bound {bnd[key]:.3e}")
        w = kc.assert_within(torch.tensor(got[key], dtype=torch.float64), torch.tensor(val[key], dtype=torch.float64),
                             torch.tensor(bnd[key], dtype=torch.float64), what=f"{tag} {key}")
        worst = max(worst, w)
    return worst


# ------------------------------------------------------------------------------------------------------ kernel contract
def strided(rows, D, ld, dtype, seed, scale=1.0):
    """[rows, D] view with row stride ld > D of a larger allocation (the padding holds other values)"""
    g = torch.Generator().manual_seed(seed)
    base = (torch.randn(rows, ld, generator=g) * scale).to(dtype).cuda()
    return base, base[:, :D]


def gate_like(T, E, k, seed, logits=None):
    """score / clean / gates as the gate kernel leaves them: fp32 softmax of noisy logits, top-k, scatter"""
    g = torch.Generator().manual_seed(seed)
    clean = torch.randn(T, E, generator=g) * 1.5 if logits is None else logits
    noisy = clean + 0.3 * torch.randn(T, E, generator=g) if logits is None else logits
    p = torch.softmax(noisy.float(), dim=1)
    score, idx = p.topk(k, dim=1)
    gates = torch.zeros(T, E).scatter_(1, idx, score)
    return score.contiguous().cuda(), clean.float().contiguous().cuda(), gates.contiguous().cuda(), idx


def run_kernel(ops, score, clean, gates, h, y, load, tag):
    from m3vit_amd import moe_stats as ms
    T, E = gates.shape
    words = ms.record_words(E)
    rec, rcheck = kc.guarded(1, words, torch.int32)
    ws, wcheck = kc.guarded_ws(ops.moe_stats_ws_elems(T, E))
    snap = kc.snapshot(score=score, clean=clean, gates=gates, h=h, y=y, load=load)
    ops.moe_stats(score, clean, gates, h, y, load, rec.view(words), ws=ws)
    torch.cuda.synchronize()
    kc.unchanged(snap)
    rcheck(what="record"); wcheck()
    first = rec.clone()
    ws.view(torch.int32).fill_(0x7FA5A5A5)                       # the second launch starts from a sentinel workspace again
    ops.moe_stats(score, clean, gates, h, y, load, rec.view(words), ws=ws)
    torch.cuda.synchronize()
    assert kc.same_bits(first, rec), f"{tag}: two launches on the same inputs differ"
    rcheck(what="record"); wcheck()
    w = rec.view(words).cpu().tolist()
    got = ms.parse_record(w, E)
    f = torch.tensor(w[:ms.HDR], dtype=torch.int32).view(F32).tolist()
    got["m_sumsq"], got["h_sumsq"] = f[ms.M_SUMSQ], f[ms.H_SUMSQ]
    return got


SHAPES = [(25216, 16, 4, 384), (64 * 394 - 1, 16, 4, 384), (1, 16, 4, 384), (4099, 64, 2, 768), (777, 6, 6, 64),
          (1030, 8, 8, 128), (515, 4, 1, 1024)]


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
@pytest.mark.parametrize("T,E,k,D", SHAPES)
def test_moe_stats_contract(ops, dtype, T, E, k, D):
    """the configs[1] shape (T = 64 * 394), one row less (the waves of the grid get unequal row counts), one row, E = 64 / k = 2 at
    ViT-B width (two 16-byte vectors per lane in f16, three in f32), k = E (run-time and unrolled k), k = 1 at D = 1024;
    the load as the float (noisy) form on even seeds and as int64 counts on odd ones"""
    seed = T + E + k
    score, clean, gates, _ = gate_like(T, E, k, seed)
    _, h = strided(T, D, D + 8 * (1 + seed % 3), dtype, seed + 1)
    _, y = strided(T * k, D, D + 16, dtype, seed + 2, scale=0.7)
    if seed % 2 == 0:
        load = (torch.rand(E, generator=torch.Generator().manual_seed(seed)) * T).float().cuda()
    else:
        load = (gates > 0).sum(0)
    tag = f"{dtype}/{T}/{E}/{k}/{D}"
    got = run_kernel(ops, score, clean, gates, h, y, load, tag)
    val, bnd = oracle(score, clean, gates, h, y, load)
    WORST[tag] = check_block(got, val, bnd, tag)


def test_one_expert_load_cv_is_zero(ops):
    """E = 1: the reference reports expert_load_cv = 0.0 when the load vector has one entry"""
    T, D = 70, 64
    score, clean, gates, _ = gate_like(T, 1, 1, 5)
    _, h = strided(T, D, D + 8, F16, 1)
    _, y = strided(T, D, D + 8, F16, 2)
    got = run_kernel(ops, score, clean, gates, h, y, torch.tensor([float(T)]).cuda(), "E1")
    assert got["expert_load_cv"] == 0.0 and got["expert_load_hist"] == [T] and got["clean_logit_std"] == 0.0
    assert got["gate_entropy_sum"] == 0.0 and got["top1_prob_sum"] == float(T)


@pytest.mark.parametrize("big", [110.0, 200.0])
def test_selected_probability_that_underflowed_does_not_count(ops, big):
    """one logit of `big` against zeros: in fp32 the softmax is exactly [1, 0, 0, ...], so three of the four selected
    experts of every token hold a probability of exactly 0 - the histogram follows p > 0 (one expert per token), not the
    routing counts (four per token)"""
    T, E, k, D = 300, 16, 4, 128
    hot = torch.arange(T) % 5                                   # experts 0..4 take turns; 5..15 never have p > 0
    logits = torch.zeros(T, E)
    logits[torch.arange(T), hot] = big
    p_cpu = torch.softmax(logits.float(), dim=1)                # verified on the CPU, in fp32, before relying on it
    top = p_cpu.topk(k, dim=1).values
    assert torch.equal(top, torch.tensor([1.0, 0.0, 0.0, 0.0]).expand(T, k))
    assert (p_cpu > 0).sum(0).tolist() == [60] * 5 + [0] * 11
    score, clean, gates, idx = gate_like(T, E, k, 0, logits=logits)
    counts = torch.bincount(idx.flatten(), minlength=E)
    assert int(counts.sum()) == T * k
    _, h = strided(T, D, D + 8, F16, 3)
    _, y = strided(T * k, D, D + 8, F16, 4)
    got = run_kernel(ops, score, clean, gates, h, y, counts.cuda(), f"underflow/{big}")
    assert got["expert_load_hist"] == [60] * 5 + [0] * 11
    assert got["expert_load_hist"] != counts.tolist()
    val, bnd = oracle(score, clean, gates, h, y, counts.cuda())
    assert val["gate_entropy_sum"] == 0.0 and got["gate_entropy_sum"] == 0.0
    check_block(got, val, bnd, f"underflow/{big}")


def test_wrapper_rejects_what_the_kernel_cannot_read(ops):
    from m3vit_amd._lib import M3Error
    T, E, k, D = 8, 4, 2, 64
    score, clean, gates, _ = gate_like(T, E, k, 1)
    _, h = strided(T, D, D + 8, F16, 1)
    _, y = strided(T * k, D, D + 8, F16, 2)
    load = (gates > 0).sum(0)
    rec = torch.zeros(8 + E, dtype=torch.int32, device="cuda")
    with pytest.raises(M3Error):
        ops.moe_stats(score, clean, gates, h, y.float(), load, rec)                     # two activation dtypes
    with pytest.raises(M3Error):
        ops.moe_stats(score, clean, gates, h, y, load.int(), rec)                       # load neither f32 nor i64
    with pytest.raises(M3Error):
        ops.moe_stats(score, clean, gates, h, y, load, rec[:8])                         # record too small
    with pytest.raises(M3Error):
        ops.moe_stats(score, clean, gates, h, y, load, rec, ws=torch.empty(3, device="cuda"))
    _, h_odd = strided(T, D, D + 4, F16, 1)                                             # rows not 16-byte multiples
    with pytest.raises(M3Error):
        ops.moe_stats(score, clean, gates, h_odd, y, load, rec)


# ----------------------------------------------------------------------------------------------------------- end to end
KW = dict(img_size=(32, 48), embed_dim=64, depth=4, num_heads=2, moe_top_k=2, gate_dim=66, multi_gate=True)
MOE = (1, 3)


def _model(std=1.0, E=8, fused="auto", act_dtype=F32, seed=9, drop_path=0.3, **model_kw):
    from m3vit_amd.vit import VisionTransformerMoE
    from oracle import ref_torch as R
    kw = dict(KW, moe_experts=E)
    cfg = R.BackboneCfg(mlp_ratio=4.0, moe_mlp_ratio=1.0, vmoe_noisy_std=std, **kw)
    P = R.init_backbone_params(cfg, seed=seed)
    m = VisionTransformerMoE(mlp_ratio=4.0, moe_mlp_ratio=1, vmoe_noisy_std=std, fused=fused, act_dtype=act_dtype,
                             drop_path_rate=drop_path, **kw, **model_kw).cuda()
    m.load_state_dict(P)
    m.train()
    return m, cfg


def _engine_oracle(eng, i):
    """the oracle on the executor's own buffers of block i (what its m3_moe_stats launch read)"""
    a = eng.act[i]
    g = a["gate"]
    load = g["load_prob"] if g["load_prob"] is not None else g["load"]
    return oracle(g["score"], g["clean"], g["gates"], a["h2"], a["y"], load)


def _aggregate_bounds(vals, bnds, positions):
    """the backbone dict of the oracle's block values and the bounds carried through the fold: quotients by the exact token
    count and plain means (the host's float64 arithmetic adds nothing at this scale)"""
    from m3vit_amd import moe_stats as ms
    blocks = [dict(v, expert_hidden_dim=64, active_vs_dense_flops_ratio=0.5) for v in vals]
    ref = ms.aggregate(blocks, positions)
    tokens = sum(v["gate_token_count"] for v in vals)
    n = len(vals)
    b = {"gate_entropy": sum(x["gate_entropy_sum"] for x in bnds) / tokens,
         "top1_prob_mean": sum(x["top1_prob_sum"] for x in bnds) / tokens}
    for key in ("expert_load_cv", "clean_logit_std", "moe_out_norm_ratio"):
        b[key] = sum(x[key] for x in bnds) / n
    return ref, b


def _check_latest(model, tag, blocks=MOE):
    """latest_moe_stats and the blocks' last_moe_analysis against the oracle on the buffers of the context that ran the
    most recent call.  Returns the backbone dict."""
    torch.cuda.synchronize()
    fb = model._fused
    eng = fb.stats_slot.eng
    vals, bnds = [], []
    for i in blocks:
        val, bnd = _engine_oracle(eng, i)
        got = model.blocks[i].last_moe_analysis
        assert got["expert_hidden_dim"] == 64 and got["active_vs_dense_flops_ratio"] == 0.5
        WORST[f"{tag}/block{i}"] = check_block(got, val, bnd, f"{tag}/block{i}")
        vals.append(val); bnds.append(bnd)
    stats = model.latest_moe_stats
    if tuple(blocks) == MOE:
        ref, b = _aggregate_bounds(vals, bnds, eng.B * (eng.N - 1))
        assert stats["moe_blocks"] == 2 and stats["total_positions"] == ref["total_positions"]
        an, ra = stats["analysis"], ref["analysis"]
        assert an["expert_load_hist"] == ra["expert_load_hist"] and an["dead_expert_ratio"] == ra["dead_expert_ratio"]
        assert an["expert_hidden_dim"] == 64.0 and an["active_vs_dense_flops_ratio"] == 0.5
        for key, bound in b.items():
            kc.assert_within(torch.tensor(an[key], dtype=torch.float64), torch.tensor(ra[key], dtype=torch.float64),
                             torch.tensor(bound, dtype=torch.float64), what=f"{tag} analysis.{key}")
    for i, blk in enumerate(model.blocks):
        if not blk.moe:
            assert blk.last_moe_analysis is None
    return stats


@pytest.mark.parametrize("act_dtype", [F16, F32])
def test_fused_backbone_latest_moe_stats(act_dtype):
    """depth 4, two MoE blocks, multi-gate, two tasks, DropPath and the noisy gate on: three joint steps with new images -
    the eager first call, the hipGraph capture and a replay - each call checked against the float64 oracle on the
    executor's own gates / clean / h2 / y / load of that call.  A record frozen at capture would fail the third step."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    m, cfg = _model(act_dtype=act_dtype, moe_stats=True)
    B = 3
    seen = []
    for step in range(3):
        img = torch.randn(B, 3, 32, 48, generator=torch.Generator().manual_seed(50 + step)).cuda()
        m.zero_grad(set_to_none=True)
        loss = 0.0
        for task in (0, 1):
            tok, cv = m(img, task_id=task)
            assert m.fused_fallback_reason is None
            stats = _check_latest(m, f"e2e/{act_dtype}/step{step}/task{task}")
            assert m._fused.stats_slot.eng.task_id == task
            loss = loss + tok.square().mean() + 0.01 * cv
        loss.backward()
        m._stats_cache = None                                    # (read the records again, not the cached dict)
        assert m.latest_moe_stats == stats                       # still the last call's (task 1) after the backward
        seen.append(stats)
    fb = m._fused
    assert fb.slots[0].graphs_f and fb.slots[1].graphs_f, "steps 2.. must have run as hipGraphs"
    assert seen[0] != seen[1] and seen[1] != seen[2], "new images must give new statistics"


def test_fused_backbone_checkpointing_counts_once():
    """use_checkpointing=True: backward re-runs every block's forward.  The recompute must not launch the statistics again:
    the records are overwritten with a marker between forward and backward and must still hold it afterwards.  The MoE
    blocks share their activation buffers in this mode, so the last MoE block is checked after the forward and the first
    one after the backward (whose recompute left that block's values, bit for bit the forward's, in the buffers) - on the
    eager first step, the capture and a replay."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import moe_stats as ms
    m, cfg = _model(act_dtype=F16, moe_stats=True, use_checkpointing=True)
    B = 3
    for step in range(3):
        img = torch.randn(B, 3, 32, 48, generator=torch.Generator().manual_seed(70 + step)).cuda()
        m.zero_grad(set_to_none=True)
        tok, cv = m(img, task_id=1)
        assert m.fused_fallback_reason is None
        eng = m._fused.stats_slot.eng
        assert eng.checkpoint
        if step == 0:        # (eager: from the capture on, the engine's gate tensors are those of the backward's recompute)
            _check_latest(m, f"ckpt/step{step}/fwd", blocks=(3,))
        first = m.blocks[1].last_moe_analysis
        cv_fwd = float(cv.detach())
        eng.stats_rec.fill_(0x5A5A5A5A)
        (tok.square().mean() + 0.01 * cv).backward()
        torch.cuda.synchronize()
        assert bool((eng.stats_rec == 0x5A5A5A5A).all()), "the checkpoint recompute launched m3_moe_stats again"
        assert float(cv.detach()) == cv_fwd
        val, bnd = _engine_oracle(eng, 1)
        check_block(first, val, bnd, f"ckpt/step{step}/block1")


def test_fused_and_per_op_paths_agree():
    """Same weights and images, no noise and no DropPath (the two paths draw them separately), fp32: both paths run the
    same forward kernels on the same values, so the tensors the two statistics launches read are the same and each result
    lies within its own bound of the one float64 value - the two differ by at most the sum of both bounds (twice the bound
    evaluated on the executor's buffers).  Histograms and token counts are exact."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    a, cfg = _model(std=0.0, drop_path=0.0, moe_stats=True)
    b, _ = _model(std=0.0, drop_path=0.0, moe_stats=True, fused=False)
    img = torch.randn(4, 3, 32, 48, generator=torch.Generator().manual_seed(3)).cuda()
    for task in (0, 1):
        a(img, task_id=task)
        b(img, task_id=task)
        assert a.fused_fallback_reason is None and b._fused is None
        sa = _check_latest(a, f"agree/task{task}")
        sb = b.latest_moe_stats
        eng = a._fused.stats_slot.eng
        bnds = []
        for i in MOE:
            val, bnd = _engine_oracle(eng, i)
            ga, gb = a.blocks[i].last_moe_analysis, b.blocks[i].last_moe_analysis
            assert ga["expert_load_hist"] == gb["expert_load_hist"] and ga["gate_token_count"] == gb["gate_token_count"]
            assert ga["expert_hidden_dim"] == gb["expert_hidden_dim"]
            for key in FLOAT_KEYS:
                print(f"agree/task{task}/block{i} {key}: fused {ga[key]!r} per-op {gb[key]!r} bound {2 * bnd[key]:.3e}")
                assert abs(ga[key] - gb[key]) <= 2 * bnd[key], (i, key, ga[key], gb[key], bnd[key])
            bnds.append(bnd)
        assert sa["moe_blocks"] == sb["moe_blocks"] and sa["total_positions"] == sb["total_positions"]
        assert sa["analysis"]["expert_load_hist"] == sb["analysis"]["expert_load_hist"]
        assert sa["analysis"]["dead_expert_ratio"] == sb["analysis"]["dead_expert_ratio"]
        assert set(sa["analysis"]) == set(sb["analysis"])
    # the per-op path also reports under autograd, and a backward leaves the statistics alone
    tok, cv = b(img, task_id=0)
    before = b.latest_moe_stats
    (tok.square().mean() + 0.01 * cv).backward()
    assert b.latest_moe_stats == before


def test_task_order_and_prefetched_passes():
    """forward(x, 0) then forward(x, 1): the statistics are task 1's, before and after backward().  From the second step on
    the executor starts task 1's pass ahead, inside the call for task 0 - the statistics read between the two calls must
    still be task 0's.  An evaluation pass in between reports itself and does not disturb the pending training calls."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    m, cfg = _model(std=0.0, drop_path=0.0, moe_stats=True)
    single = {}
    img = torch.randn(3, 3, 32, 48, generator=torch.Generator().manual_seed(8)).cuda()
    with torch.no_grad():
        for task in (0, 1):
            m(img, task_id=task)
            single[task] = m.latest_moe_stats
    assert single[0] != single[1], "the two gates must route differently for this test to mean anything"
    for step in range(3):
        m.zero_grad(set_to_none=True)
        tok0, cv0 = m(img, task_id=0)
        assert m.latest_moe_stats == single[0], step
        assert m._fused.stats_slot.eng.task_id == 0
        tok1, cv1 = m(img, task_id=1)
        assert m.latest_moe_stats == single[1], step
        (tok0.square().mean() + tok1.square().mean() + 0.01 * (cv0 + cv1)).backward()
        m._stats_cache = None                                    # (read the records again, not the cached dict)
        assert m.latest_moe_stats == single[1], step
        assert m._fused.stats_slot.eng.task_id == 1
    assert m._fused.prefetch_hits > 0, "task 1's pass should have been started ahead of its call"
    m.zero_grad(set_to_none=True)
    tok0, cv0 = m(img, task_id=0)
    with torch.no_grad():
        m(img, task_id=1)
    assert m.latest_moe_stats == single[1]
    tok0.square().mean().backward()
    m._stats_cache = None
    assert m.latest_moe_stats == single[1]


def test_logger_hook_is_called_in_training_only():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    m, cfg = _model(std=0.0, drop_path=0.0, moe_stats=True)

    class Logger:
        def __init__(self):
            self.seen = []

        def log_moe_stats(self, stats):
            self.seen.append(stats)

    log = Logger()
    img = torch.randn(2, 3, 32, 48).cuda()
    m(img, task_id=0)
    assert log.seen == []                       # no hook installed
    m.wandb_logger = lambda: None
    m(img, task_id=0)                           # a hook that returns no logger
    m.wandb_logger = lambda: log
    m(img, task_id=1)
    assert len(log.seen) == 1 and log.seen[0] == m.latest_moe_stats and log.seen[0]["moe_blocks"] == 2
    m.eval()
    with torch.no_grad():
        m(img, task_id=1)
    assert len(log.seen) == 1


def test_flag_off_allocates_nothing_and_changes_nothing():
    """a moe_stats=False engine has no record and no workspace, and a moe_stats=True engine computes bit-identical tokens,
    balance loss and gradients: the statistic only reads"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd.engine import BackboneEngine
    from oracle import ref_torch as R
    cfg = R.BackboneCfg(mlp_ratio=4.0, moe_mlp_ratio=1.0, vmoe_noisy_std=1.0, moe_experts=8, **KW)
    P = R.init_backbone_params(cfg, seed=4)
    B = 3
    g = torch.Generator().manual_seed(1)
    img = torch.randn(B, 3, 32, 48, generator=g).cuda()
    dtok = (torch.randn(B, cfg.num_tokens, 64, generator=g) * 0.1).cuda()
    noises = {i: torch.randn(B * cfg.num_tokens, 8, generator=g).cuda() for i in MOE}
    ps = {i: tuple((torch.floor(0.7 + torch.rand(B, generator=g)) / 0.7).cuda() for _ in range(2)) for i in (1, 2, 3)}
    out = {}
    for flag in (False, True):
        eng = BackboneEngine(cfg, P, batch=B, dtype=F16, moe_stats=flag)
        assert (eng.stats_rec is None) == (not flag) and (eng.ws_stats is None) == (not flag)
        if not flag:
            assert eng.moe_stats() is None
        eng.zero_grad()
        tok, cv = eng.forward(img, 1, noises=noises, path_scales=ps)
        tok = tok.clone()
        eng.backward(dtok, cv_weight=0.01)
        torch.cuda.synchronize()
        out[flag] = (tok, cv.clone(), eng.flat_grads.clone())
        if flag:
            blocks, total = eng.moe_stats()
            assert sorted(blocks) == list(MOE) and total["moe_blocks"] == 2
            for i in MOE:
                val, bnd = _engine_oracle(eng, i)
                check_block(blocks[i], val, bnd, f"engine/block{i}")
    for x, y in zip(out[False], out[True]):
        assert kc.same_bits(x, y)
