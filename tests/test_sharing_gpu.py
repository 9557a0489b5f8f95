"""GPU: the token sharing stage (csrc/share.hip, m3vit_amd/sharing.py) against the float64 restatement of sharing_cases.py,
on generated inputs and on the reference's own results (tests/golden/g14_sharing.npz).

Exact: shared_bits, shared_flat_idx, count, every statistic (the builder keeps every score 4 error bounds away from the
threshold, so no position is excluded).  Within derived bounds (sharing_cases.g_bound / forward_bounds / backward_bounds,
SAFETY = 2, nothing tuned per test): G, shared_x, d x_t, d w_gate, d task_emb.  Bitwise: pass-through rows, the rows a task
shares (they are shared_x's own bits), run-to-run parameter gradients, graph replay against eager.  Every output of the C
entry points lies in a guarded allocation (kernel_contract.guarded / guarded_ws), every input keeps its bits.

The compaction scan takes sharing_cases.SCAN_WIDTH = 1024 positions per step: (B, N) = (6, 197) is 1182 positions, two steps
with a carry between them."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sharing_cases as SC                                                                        # noqa: E402
from kernel_contract import U32, assert_within, guarded, guarded_ws, same_bits, snapshot, store, unchanged  # noqa: E402

pytestmark = pytest.mark.gpu
F64 = torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_sharing.npz")
_CACHE = {}


def inputs(c):
    """the case's inputs and float64 reference, built once and shared by the tests (never modified)"""
    k = SC.case_id(c)
    if k not in _CACHE:
        _CACHE[k] = SC.make_inputs(c)
    return _CACHE[k]


def dev(t):
    return None if t is None else t.cuda()


def _ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _rows(ts):
    from m3vit_amd import _lib
    r = _lib.ShareRows()
    for i, t in enumerate(ts):
        if t is not None:
            r.p[i] = t.data_ptr()
    return r


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw_stage_fwd(c, I, xs, w, emb, noise):
    """m3_share_stage_fwd through the C ABI with every output in a guarded allocation; returns the outputs and the checks"""
    from m3vit_amd import _lib, ops
    T, P, D, Dg = c["T"], c["B"] * c["N"], c["D"], c["Dg"]
    dt = SC.DTYPES[c["dtype"]]
    ys, checks = [], []
    for _ in range(T):
        v, ck = guarded(P, D, dt)
        ys.append(v); checks.append(ck)
    sx, ck = guarded(P, D, dt); checks.append(ck)
    bits, ck = guarded(P, 1, torch.int64); checks.append(ck)
    g, ck = guarded(T, P, torch.float32); checks.append(ck)
    soft, ck = guarded(T, P, torch.float32)
    if c["hard"]:
        checks.append(ck)
    xr, yr = _rows(xs), _rows(ys)
    _lib.check(_lib.lib().m3_share_stage_fwd(ctypes.byref(xr), ops.dt_code(dt), T, P, D, _ptr(w), _ptr(emb), Dg, _ptr(noise),
                                             c["tau"], int(c["hard"]), c["gamma"], c["eps"], ctypes.byref(yr), _ptr(sx),
                                             _ptr(bits), _ptr(g), _ptr(soft if c["hard"] else None), _stream()), "stage_fwd")
    torch.cuda.synchronize()
    return dict(ys=ys, sx=sx, bits=bits.view(-1), g=g, soft=soft if c["hard"] else None), checks


def raw_compact(bits, T, prev):
    from m3vit_amd import _lib
    P = bits.numel()
    idx, c1 = guarded(P, 1, torch.int32)
    count, c2 = guarded(1, 1, torch.int32)
    stats, c3 = guarded(_lib.M3_SHARE_STAT_WORDS, 1, torch.int64)
    stats.zero_()
    _lib.check(_lib.lib().m3_share_compact(_ptr(bits), _ptr(prev), P, T, _ptr(idx), _ptr(count), _ptr(stats), _stream()), "compact")
    torch.cuda.synchronize()
    for ck in (c1, c2, c3):
        ck()
    return idx.view(-1), count.view(-1), stats.view(-1)


def check_stats(stats, idx, count, ref, T, P):
    from m3vit_amd import _lib as L
    s = ref["stats"]
    w = stats.tolist()
    assert w[L.M3_SHARE_STAT_POSITIONS] == s["shared_positions"] == int(count[0]) == w[L.M3_SHARE_STAT_S]
    assert w[L.M3_SHARE_STAT_TASKTOKENS] == s["shared_tasktoken_count"]
    assert (w[L.M3_SHARE_STAT_PARTIAL], w[L.M3_SHARE_STAT_PARTIAL_TOTAL]) == (s["partial_split_count"], s["partial_split_total"])
    assert (w[L.M3_SHARE_STAT_FLIPS], w[L.M3_SHARE_STAT_FLIP_TOTAL]) == (s["shared_bits_flip_count"], s["shared_bits_flip_total"])
    assert w[L.M3_SHARE_STAT_S_T:L.M3_SHARE_STAT_S_T + T] == s["S_t"] and not any(w[L.M3_SHARE_STAT_S_T + T:])
    K = s["shared_positions"]
    assert torch.equal(idx[:K].cpu().long(), ref["flat_idx"]) and bool((idx[K:] == -1).all()) and idx.numel() == P


def check_forward(c, I, o):
    ref, dt = I["ref"], SC.DTYPES[c["dtype"]]
    T, P = c["T"], c["B"] * c["N"]
    assert torch.equal(o["bits"].cpu(), ref["bits"]), "shared_bits"
    gb, sxb, _ = SC.forward_bounds(ref, I["x64"], I["gb"], dt, c["eps"])
    if c["hard"]:
        assert torch.equal(o["g"].cpu().double(), ref["G"].round()), "hard G is the one-hot"
        assert_within(o["soft"], ref["soft"], gb, "soft")
    else:
        assert_within(o["g"], ref["G"], gb, "G")
    assert_within(o["sx"], ref["shared_x"], sxb, "shared_x")
    assert not bool(o["sx"][(o["bits"] == 0)].count_nonzero()), "shared_x rows of unshared positions are zero"
    for t in range(T):
        m = ref["M"][t].cuda()
        assert same_bits(o["ys"][t][~m], I["xs"][t].cuda()[~m]), f"y[{t}]: a row that is not shared keeps x's bits"
        assert same_bits(o["ys"][t][m], o["sx"][m]), f"y[{t}]: a shared row is shared_x's row"


@pytest.mark.parametrize("c", SC.stage_cases() + SC.degenerate_cases(), ids=SC.case_id)
def test_stage_forward(c):
    I = inputs(c)
    T, P = c["T"], c["B"] * c["N"]
    xs = [dev(I["xs"][t]) for t in range(T)]
    w, emb, noise, prev = dev(I["w_gate"]), dev(I["task_emb"]), dev(I["noise"]), dev(I["prev"])
    snap = snapshot(w=w, emb=emb, noise=noise, prev=prev, **{f"x{t}": x for t, x in enumerate(xs)})
    o, checks = raw_stage_fwd(c, I, xs, w, emb, noise)
    for ck in checks:
        ck()
    check_forward(c, I, o)
    idx, count, stats = raw_compact(o["bits"], T, prev)
    check_stats(stats, idx, count, I["ref"], T, P)
    unchanged(snap)
    if c["pattern"] == "none":
        assert int(count[0]) == 0 and bool((idx == -1).all()) and not bool(o["sx"].count_nonzero())
        assert all(same_bits(o["ys"][t], xs[t]) for t in range(T))
    if c["pattern"] == "all":
        assert int(count[0]) == P and bool((o["bits"] == (1 << T) - 1).all())
    if c["pattern"] == "one":
        assert int(count[0]) == 0 and not bool(o["bits"].any())
    if c["pattern"] == "two_of_three":
        assert stats.tolist()[2] == P == int(count[0])


def _bwd_setup(c, with_g=True):
    I = inputs(c)
    dt = SC.DTYPES[c["dtype"]]
    cy, cs, cg = SC.functional(c)
    cy, cs, cg = cy.to(dt), cs.to(dt), (cg.float() if with_g else None)      # as the kernel reads them
    return I, dt, cy, cs, cg


def _reference_grads(c, I, cy, cs, cg):
    xs = I["x64"].clone().requires_grad_(True)
    w = I["w64"].clone().requires_grad_(True)
    emb = None if I["e64"] is None else I["e64"].clone().requires_grad_(True)
    r = SC.stage(xs, w, emb, I["n64"], c["tau"], c["hard"], c["gamma"], c["eps"])
    f = (cy.double() * r["y"]).sum() + (cs.double() * r["shared_x"]).sum()
    if cg is not None:
        f = f + (cg.double() * r["G"]).sum()
    f.backward()
    return xs.grad, w.grad, None if emb is None else emb.grad


def raw_stage_bwd(c, I, dt, fwd, xs, w, emb, dys, dsx, dg):
    from m3vit_amd import _lib, ops
    T, P, D, Dg = c["T"], c["B"] * c["N"], c["D"], c["Dg"]
    dxs, checks = [], []
    for _ in range(T):
        v, ck = guarded(P, D, dt)
        dxs.append(v); checks.append(ck)
    ws, ck = guarded_ws(ops.share_bwd_ws_elems(P, T, D, Dg)); checks.append(ck)
    dw, ck = guarded(D + Dg, 2, torch.float32); checks.append(ck)
    demb = None
    if Dg:
        demb, ck = guarded(T, Dg, torch.float32); checks.append(ck)
    xr, dyr, dxr = _rows(xs), _rows(dys), _rows(dxs)
    _lib.check(_lib.lib().m3_share_stage_bwd(ctypes.byref(xr), ops.dt_code(dt), T, P, D, _ptr(w), _ptr(emb), Dg, c["tau"], c["eps"],
                                             _ptr(fwd["bits"]), _ptr(fwd["g"]), _ptr(fwd["soft"]), _ptr(fwd["sx"]), ctypes.byref(dyr),
                                             _ptr(dsx), _ptr(dg), ctypes.byref(dxr), _ptr(ws), _ptr(dw), _ptr(demb), _stream()),
               "stage_bwd")
    torch.cuda.synchronize()
    for ck in checks:
        ck()
    return dxs, dw, demb


def _contig(o):
    """the forward's guarded outputs as plain contiguous tensors (what the backward reads)"""
    return dict(bits=o["bits"].contiguous(), g=o["g"].contiguous(), soft=None if o["soft"] is None else o["soft"].contiguous(),
                sx=o["sx"].contiguous())


@pytest.mark.parametrize("c", SC.stage_cases() + SC.degenerate_cases(), ids=SC.case_id)
def test_stage_backward(c):
    """d x_t, d w_gate, d task_emb against float64 autograd of the restatement (hard mode: the straight-through gradient);
    the parameter gradients bit-identical across two runs"""
    I, dt, cy, cs, cg = _bwd_setup(c)
    T, P, D = c["T"], c["B"] * c["N"], c["D"]
    xs = [dev(I["xs"][t]) for t in range(T)]
    w, emb, noise = dev(I["w_gate"]), dev(I["task_emb"]), dev(I["noise"])
    o, _ = raw_stage_fwd(c, I, xs, w, emb, noise)
    fwd = _contig(o)
    dys, dsx, dg = [dev(cy[t]).contiguous() for t in range(T)], dev(cs), dev(cg)
    snap = snapshot(w=w, emb=emb, dsx=dsx, dg=dg, **{f"x{t}": x for t, x in enumerate(xs)}, **{f"dy{t}": x for t, x in enumerate(dys)},
                    **{k: v for k, v in fwd.items() if v is not None})
    dxs, dw, demb = raw_stage_bwd(c, I, dt, fwd, xs, w, emb, dys, dsx, dg)
    unchanged(snap)
    rx, rw, remb = _reference_grads(c, I, cy, cs, cg)
    _, sxb, dW = SC.forward_bounds(I["ref"], I["x64"], I["gb"], dt, c["eps"])
    bx, bw, bemb = SC.backward_bounds(I, c, dt, cy.double(), cs.double(), cg.double(), sxb, dW, rx)
    assert_within(torch.stack(dxs), rx, bx, "d x")
    assert_within(dw, rw, bw + U32 * rw.abs(), "d w_gate")
    if demb is not None:
        assert_within(demb, remb, bemb + U32 * remb.abs(), "d task_emb")
    dxs2, dw2, demb2 = raw_stage_bwd(c, I, dt, fwd, xs, w, emb, dys, dsx, dg)
    assert same_bits(dw2.contiguous(), dw.contiguous()) and (demb is None or same_bits(demb2.contiguous(), demb.contiguous()))
    assert all(same_bits(a.contiguous(), b.contiguous()) for a, b in zip(dxs, dxs2))


@pytest.mark.parametrize("c", [SC.stage_cases()[5], SC.stage_cases()[6], SC.degenerate_cases()[2]], ids=SC.case_id)
def test_backward_pass_through_rows_and_null_gradients(c):
    """without a gradient on G a row that is not shared passes its gradient through bitwise; d shared_x = NULL and a NULL d y
    entry agree with zero tensors"""
    I, dt, cy, cs, _ = _bwd_setup(c, with_g=False)
    T = c["T"]
    xs = [dev(I["xs"][t]) for t in range(T)]
    w, emb, noise = dev(I["w_gate"]), dev(I["task_emb"]), dev(I["noise"])
    o, _ = raw_stage_fwd(c, I, xs, w, emb, noise)
    fwd = _contig(o)
    dys = [dev(cy[t]).contiguous() for t in range(T)]
    dxs, dw, demb = raw_stage_bwd(c, I, dt, fwd, xs, w, emb, dys, dev(cs), None)
    for t in range(T):
        m = I["ref"]["M"][t].cuda()
        assert same_bits(dxs[t][~m], dys[t][~m]), f"d x[{t}]: rows that are not shared"
    zero_sx = torch.zeros_like(fwd["sx"])
    a = raw_stage_bwd(c, I, dt, fwd, xs, w, emb, dys, None, None)
    b = raw_stage_bwd(c, I, dt, fwd, xs, w, emb, dys, zero_sx, torch.zeros_like(fwd["g"]))
    assert all(same_bits(p.contiguous(), q.contiguous()) for p, q in zip(a[0], b[0])) and same_bits(a[1].contiguous(), b[1].contiguous())
    a = raw_stage_bwd(c, I, dt, fwd, xs, w, emb, [None] + dys[1:], None, None)
    b = raw_stage_bwd(c, I, dt, fwd, xs, w, emb, [torch.zeros_like(dys[0])] + dys[1:], None, None)
    assert all(same_bits(p.contiguous(), q.contiguous()) for p, q in zip(a[0], b[0])) and same_bits(a[1].contiguous(), b[1].contiguous())


@pytest.mark.parametrize("c", SC.stage_cases()[1:12:2] + SC.stage_cases()[-3:], ids=SC.case_id)
def test_predictor_alone_gives_the_stage_s_bits(c):
    """ShareabilityPredictor.forward on each task tensor: the same G, bit for bit, as the stage wrote for that row; and its
    backward against float64 autograd of the restatement's predictor"""
    from m3vit_amd.sharing import ShareabilityPredictor
    I = inputs(c)
    T, B, N, D, Dg = c["T"], c["B"], c["N"], c["D"], c["Dg"]
    xs = [dev(I["xs"][t]) for t in range(T)]
    w, emb, noise = dev(I["w_gate"]), dev(I["task_emb"]), dev(I["noise"])
    o, _ = raw_stage_fwd(c, I, xs, w, emb, noise)
    pred = ShareabilityPredictor(D, Dg, temperature=c["tau"], hard=c["hard"]).cuda()
    with torch.no_grad():
        pred.w_gate.copy_(w)
    pred.train()
    t = T - 1
    x = xs[t].view(B, N, D).clone().requires_grad_(True)
    e = None if emb is None else emb[t].clone().requires_grad_(True)
    g = pred(x, e, noise=noise[t])
    assert g.shape == (B, N) and same_bits(g.detach().reshape(-1), o["g"][t].contiguous())
    cg = SC.functional(c)[2][t].float()
    (g.reshape(-1) * cg.cuda()).sum().backward()
    x64 = I["x64"][t].clone().requires_grad_(True)
    w64 = I["w64"].clone().requires_grad_(True)
    e64 = None if e is None else I["e64"][t].clone().requires_grad_(True)
    G, soft = SC.predictor(x64, w64, e64, I["n64"][t], c["tau"], c["hard"])
    (G * cg.double()).sum().backward()
    # the stage's bounds with nothing shared: M = 0, so only the dl1 terms remain
    gb = I["gb"][t]
    s = soft.detach() * (1 - soft.detach()) / c["tau"]
    dl1 = cg.double() * s
    dl1_err = cg.double().abs() * ((1 - 2 * soft.detach()).abs() * gb + gb * gb) / c["tau"] + 4 * U32 * dl1.abs()
    wd = (w64[:D, 1] - w64[:D, 0]).detach().abs()
    dt = SC.DTYPES[c["dtype"]]
    assert_within(x.grad.reshape(-1, D), x64.grad, SC.SAFETY * (dl1_err.unsqueeze(-1) * wd + 2 * U32 * x64.grad.abs() + store(dt, x64.grad)), "d x")
    P = B * N
    ax = x64.detach().abs()
    rows = [(dl1_err.unsqueeze(-1) * ax).sum(0) + (P + 2) * U32 * (dl1.abs().unsqueeze(-1) * ax).sum(0)]
    R_err = dl1_err.sum() + (P + 2) * U32 * dl1.abs().sum()
    if e is not None:
        rows.append(e64.detach().abs() * R_err + 2 * U32 * (e64.detach() * dl1.sum()).abs())
        wde = (w64[D:, 1] - w64[D:, 0]).detach()
        assert_within(e.grad, e64.grad, SC.SAFETY * (R_err * wde.abs() + 2 * U32 * e64.grad.abs()), "d task_emb")
    assert_within(pred.w_gate.grad, w64.grad, SC.SAFETY * torch.cat(rows).unsqueeze(-1).expand(-1, 2) + U32 * w64.grad.abs(), "d w_gate")
    pred.eval()                                                       # eval: hard whatever self.hard says
    ge = pred(xs[t].view(B, N, D), None if emb is None else emb[t], noise=noise[t])
    assert bool(((ge == 0) | (ge == 1)).all()) and torch.equal(ge.reshape(-1).cpu().double(), I["ref"]["soft"][t].round())


def test_predictor_task_embedding_forms_agree():
    """[E], [B, E] and [B, N, E] task embeddings with the same values give the same scores within the bound (the first runs
    in the kernel, the others add their logits from a torch product), and all three carry gradient to the embedding"""
    from m3vit_amd.sharing import ShareabilityPredictor
    c = SC.stage_cases()[1]
    I = inputs(c)
    B, N, D, Dg = c["B"], c["N"], c["D"], c["Dg"]
    pred = ShareabilityPredictor(D, Dg, temperature=c["tau"]).cuda().train()
    with torch.no_grad():
        pred.w_gate.copy_(dev(I["w_gate"]))
    x, noise = dev(I["xs"][0]).view(B, N, D), dev(I["noise"][0])
    e1 = dev(I["task_emb"][0]).clone().requires_grad_(True)
    e2 = e1.detach().expand(B, Dg).clone().requires_grad_(True)
    e3 = e1.detach().expand(B, N, Dg).clone().requires_grad_(True)
    g1, g2, g3 = pred(x, e1, noise=noise), pred(x, e2, noise=noise), pred(x, e3, noise=noise)
    ref, gb = I["ref"]["G"][0].view(B, N), I["gb"][0].view(B, N)
    for g in (g1, g2, g3):
        assert_within(g, ref, gb, "G")
    for g, e in ((g1, e1), (g2, e2), (g3, e3)):
        g.sum().backward()
    torch.testing.assert_close(e2.grad.sum(0), e1.grad, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(e3.grad.sum((0, 1)), e1.grad, rtol=1e-4, atol=1e-6)


# --------------------------------------------------------------------------------------------------------- aggregation
def _agg_cases():
    return [c for c in SC.stage_cases() if c["T"] in (2, 5)]


@pytest.mark.parametrize("need_kind", ["mixed", "none", "all"])
@pytest.mark.parametrize("c", _agg_cases(), ids=SC.case_id)
def test_aggregation(c, need_kind):
    """m3_share_aggregate_fwd / _bwd through the C ABI (guarded outputs) against the restatement; agg_needed all false is a
    bitwise identity.  Bounds: an fp32 sum of at most T terms, the fp32 reciprocal of count + eps and the product:
    (T + 3) u32 sum |terms| / count, then the store."""
    from m3vit_amd import _lib, ops
    I = inputs(c)
    T, P, D = c["T"], c["B"] * c["N"], c["D"]
    dt = SC.DTYPES[c["dtype"]]
    gen = torch.Generator().manual_seed(5)
    masks = torch.rand(T, P, generator=gen) < 0.6
    need = {"mixed": (masks.sum(0) >= 2) & (torch.rand(P, generator=gen) < 0.8), "none": torch.zeros(P, dtype=torch.bool),
            "all": torch.ones(P, dtype=torch.bool)}[need_kind]
    bits = torch.zeros(P, dtype=torch.int64)
    for t in range(T):
        bits |= masks[t].to(torch.int64) << t
    xs = [dev(I["xs"][t]) for t in range(T)]
    mb, nd = bits.cuda(), need.cuda()
    snap = snapshot(mb=mb, nd=nd, **{f"x{t}": x for t, x in enumerate(xs)})

    def run(fn, ins, extra, want_agg):
        outs, checks = [], []
        for _ in range(T):
            v, ck = guarded(P, D, dt)
            outs.append(v); checks.append(ck)
        agg = None
        if want_agg:
            agg, ck = guarded(P, D, dt); checks.append(ck)
        ir, orr = _rows(ins), _rows(outs)
        if fn == "fwd":
            rc = _lib.lib().m3_share_aggregate_fwd(ctypes.byref(ir), ops.dt_code(dt), T, P, D, _ptr(mb), _ptr(nd), 1e-6,
                                                   ctypes.byref(orr), _ptr(agg), _stream())
        else:
            rc = _lib.lib().m3_share_aggregate_bwd(ctypes.byref(ir), ops.dt_code(dt), T, P, D, _ptr(mb), _ptr(nd), 1e-6,
                                                   _ptr(extra), ctypes.byref(orr), _stream())
        _lib.check(rc, fn)
        torch.cuda.synchronize()
        for ck in checks:
            ck()
        return outs, agg

    ys, agg = run("fwd", xs, None, True)
    x64 = I["x64"].clone().requires_grad_(True)
    ry, ragg = SC.aggregate(x64, masks, need)
    v = (masks & need.unsqueeze(0))
    cnt = v.sum(0).clamp(min=1).double().unsqueeze(-1)
    ab = SC.SAFETY * ((T + 3) * U32 * (v.unsqueeze(-1) * I["x64"].abs()).sum(0) / cnt + store(dt, ragg.detach()))
    assert_within(agg, ragg.detach(), ab, "agg")
    for t in range(T):
        m = v[t].cuda()
        assert same_bits(ys[t][~m], xs[t][~m]) and same_bits(ys[t][m], agg[m])
    if need_kind == "none":
        assert all(same_bits(ys[t], xs[t]) for t in range(T)) and not bool(agg.count_nonzero())
    cy, cs, _ = SC.functional(c)
    cy, cs = cy.to(dt), cs.to(dt)
    ((cy.double() * ry).sum() + (cs.double() * ragg).sum()).backward()
    dys, dagg = [dev(cy[t]).contiguous() for t in range(T)], dev(cs)
    dxs, _ = run("bwd", dys, dagg, False)
    terms = cs.double().abs() + (v.unsqueeze(-1) * cy.double().abs()).sum(0)
    bb = SC.SAFETY * (v.unsqueeze(-1) * ((T + 4) * U32 * terms / cnt).unsqueeze(0) + store(dt, x64.grad))
    assert_within(torch.stack(dxs), x64.grad, bb, "d x")
    for t in range(T):
        m = v[t].cuda()
        assert same_bits(dxs[t][~m], dys[t][~m])
    unchanged(snap)


def test_aggregation_modules_match_the_golden():
    """Aggregation / AggregationStage with the reference's list-of-bool-masks signature, values and gradients against the
    reference's own results; no device synchronisation in either call"""
    from m3vit_amd.sharing import Aggregation, AggregationStage
    g = np.load(GOLDEN)
    for c in SC.golden_cases():
        k = SC.case_id(c)
        T, B, N, D = c["T"], c["B"], c["N"], c["D"]
        xs = torch.from_numpy(g[f"{k}/xs"]).cuda().requires_grad_(True)
        masks = [m.view(B, N) for m in torch.from_numpy(g[f"{k}/agg_masks"]).cuda()]
        need = torch.from_numpy(g[f"{k}/agg_need"]).cuda().view(B, N)
        outs = {t: xs[t].view(B, N, D) for t in range(T)}
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            agg = Aggregation()(outs, masks, need)
            outs2 = AggregationStage(Aggregation(), T)(dict(outs), masks, need)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        y = torch.stack([outs2[t].reshape(B * N, D) for t in range(T)])
        torch.testing.assert_close(agg.reshape(B * N, D).double().cpu(), torch.from_numpy(g[f"{k}/agg"]), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(y.double().cpu(), torch.from_numpy(g[f"{k}/agg_y"]), rtol=1e-5, atol=1e-6)
        cy, cs, _ = SC.functional(c)
        ((cy.float().cuda() * y).sum() + (cs.float().cuda() * agg.reshape(B * N, D)).sum()).backward()
        torch.testing.assert_close(xs.grad.double().cpu(), torch.from_numpy(g[f"{k}/agg_d_xs"]), rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------------------- modules, golden, drop-ins
def _golden_stage(g, c, requires_grad=False):
    from m3vit_amd.sharing import ShareabilityPredictor, SharingStage
    k = SC.case_id(c)
    T, B, N, D, Dg = c["T"], c["B"], c["N"], c["D"], c["Dg"]
    pred = ShareabilityPredictor(D, Dg, temperature=c["tau"], hard=c["hard"]).cuda().train()
    with torch.no_grad():
        pred.w_gate.copy_(torch.from_numpy(g[f"{k}/w_gate"]))
    xs = torch.from_numpy(g[f"{k}/xs"]).cuda().requires_grad_(requires_grad)
    emb = torch.from_numpy(g[f"{k}/task_emb"]).cuda().requires_grad_(requires_grad) if Dg else None
    noise = torch.from_numpy(g[f"{k}/noise"]).float().cuda().view(T, B, N, 2)
    prev = torch.from_numpy(g[f"{k}/prev"]).cuda().view(B, N) if c["prev"] else None
    return SharingStage(pred, T), pred, xs, emb, noise, prev


@pytest.mark.parametrize("c", SC.golden_cases(), ids=SC.case_id)
def test_sharing_stage_on_the_golden(c):
    """SharingStage forward + backward on the reference's inputs against the reference's own outputs and gradients; no
    device synchronisation in the forward or the backward; aux() and compact() give the reference's values"""
    g = np.load(GOLDEN)
    k = SC.case_id(c)
    T, B, N, D, Dg = c["T"], c["B"], c["N"], c["D"], c["Dg"]
    P = B * N
    stage, pred, xs, emb, noise, prev = _golden_stage(g, c, requires_grad=True)
    outs = {t: xs[t].view(B, N, D) for t in range(T)}
    cy, cs, cg = (v.float().cuda() for v in SC.functional(c))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs2, shared = stage(outs, prev, emb, gamma=c["gamma"], noise=noise)
        y = torch.stack([outs2[t].reshape(P, D) for t in range(T)])
        ((cy * y).sum() + (cs * shared.x).sum() + (cg * shared.g.reshape(T, P)).sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert shared.bits.dtype == torch.int64 and shared.bits.shape == (B, N) and shared.flat_idx.dtype == torch.int32
    assert shared.x.shape == (P, D) and shared.g.shape == (T, B, N) and shared.count.dtype == torch.int32
    assert torch.equal(shared.bits.reshape(-1).cpu(), torch.from_numpy(g[f"{k}/bits"]))
    # the noise was stored in float64 and is read in float32 here: tolerances of the float32 pipeline, not the kernel contract
    tol = dict(rtol=2e-4, atol=2e-5)
    G = torch.from_numpy(g[f"{k}/G"])
    torch.testing.assert_close(shared.g.reshape(T, P).double().cpu(), G.round() if c["hard"] else G, **tol)
    torch.testing.assert_close(y.detach().double().cpu(), torch.from_numpy(g[f"{k}/y"]), **tol)
    sx, idx = shared.compact()
    K = g[f"{k}/flat_idx"].size
    if K == 0:
        assert sx is None and idx is None
    else:
        assert idx.dtype == torch.int64 and torch.equal(idx.cpu(), torch.from_numpy(g[f"{k}/flat_idx"])) and sx.shape == (K, D)
        torch.testing.assert_close(sx.detach().double().cpu(), torch.from_numpy(g[f"{k}/shared_x"]), **tol)
    a = shared.aux()
    assert [a["stats"]["shared_positions"], a["stats"]["shared_tasktoken_count"], a["analysis"]["partial_split_count"],
            a["analysis"]["partial_split_total"], a["analysis"]["shared_bits_flip_count"],
            a["analysis"]["shared_bits_flip_total"]] == g[f"{k}/stats"].tolist()
    gt = dict(rtol=2e-3, atol=2e-4)
    torch.testing.assert_close(xs.grad.double().cpu(), torch.from_numpy(g[f"{k}/d_xs"]), **gt)
    torch.testing.assert_close(pred.w_gate.grad.double().cpu(), torch.from_numpy(g[f"{k}/d_w_gate"]), **gt)
    if Dg:
        torch.testing.assert_close(emb.grad.double().cpu(), torch.from_numpy(g[f"{k}/d_task_emb"]), **gt)
    assert float(shared.regularization(0.01)) == float(g[f"{k}/loss"])


@pytest.mark.parametrize("c", SC.golden_cases(), ids=SC.case_id)
def test_regularisation_loss(c):
    """equal to the golden; zero when nothing is shared; no device synchronisation in the call"""
    from m3vit_amd.sharing import SharingRegularizationLoss
    g = np.load(GOLDEN)
    k = SC.case_id(c)
    bits = torch.from_numpy(g[f"{k}/bits"]).cuda().view(c["B"], c["N"])
    crit = SharingRegularizationLoss(0.01)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = crit(bits, c["T"])
        zero = crit(torch.zeros_like(bits), c["T"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert loss.dtype == torch.float32 and float(loss) == float(g[f"{k}/loss"]) and float(zero) == 0.0
    assert float(SharingRegularizationLoss(0.0)(bits, c["T"])) == 0.0
    if c["pattern"] == "pairs":
        assert float(loss) > 0.0


@pytest.mark.parametrize("c", SC.golden_cases(), ids=SC.case_id)
def test_drop_in_functions(c):
    """transition_stage / apply_shared_broadcast: the reference's shapes, types and values on the golden inputs, the Nones
    when nothing is shared"""
    from m3vit_amd.sharing import apply_shared_broadcast, transition_stage
    g = np.load(GOLDEN)
    k = SC.case_id(c)
    T, B, N, D = c["T"], c["B"], c["N"], c["D"]
    P = B * N
    xs = torch.from_numpy(g[f"{k}/xs"]).double().cuda()
    outs = {t: xs[t].view(B, N, D) for t in range(T)}
    g_shared = {t: torch.from_numpy(g[f"{k}/G"])[t].cuda().view(B, N) for t in range(T)}
    prev = torch.from_numpy(g[f"{k}/prev"]).cuda().view(B, N) if c["prev"] else None
    bits, sx, idx, aux = transition_stage(outs, prev, g_shared, gamma=c["gamma"], eps=c["eps"])
    assert bits.dtype == torch.int64 and bits.shape == (B, N) and torch.equal(bits.reshape(-1).cpu(), torch.from_numpy(g[f"{k}/bits"]))
    K = g[f"{k}/flat_idx"].size
    if K == 0:
        assert sx is None and idx is None
        assert apply_shared_broadcast(outs, bits, None) is outs
    else:
        assert idx.dtype == torch.int64 and torch.equal(idx.cpu(), torch.from_numpy(g[f"{k}/flat_idx"]))
        assert sx.shape == (K, D) and sx.dtype == xs.dtype
        torch.testing.assert_close(sx.cpu(), torch.from_numpy(g[f"{k}/shared_x"]), rtol=1e-12, atol=1e-14)
        for form in (idx, None):
            o2 = apply_shared_broadcast(dict(outs), bits, sx, form)
            y = torch.stack([o2[t].reshape(P, D) for t in range(T)])
            torch.testing.assert_close(y.cpu(), torch.from_numpy(g[f"{k}/y"]), rtol=1e-12, atol=1e-14)
    assert isinstance(aux["stats"]["shared_positions"], int) and aux["cv_loss"].shape == ()
    assert [aux["stats"]["shared_positions"], aux["stats"]["shared_tasktoken_count"], aux["analysis"]["partial_split_count"],
            aux["analysis"]["partial_split_total"], aux["analysis"]["shared_bits_flip_count"],
            aux["analysis"]["shared_bits_flip_total"]] == g[f"{k}/stats"].tolist()


@pytest.mark.parametrize("c", [SC.stage_cases()[10], SC.stage_cases()[7]], ids=SC.case_id)
def test_sharing_stage_is_graph_capturable(c):
    """SharingStage forward + backward under torch.cuda.graph: replayed with new inputs copied into the captured buffers it
    matches an eager run bitwise"""
    from m3vit_amd import ops
    from m3vit_amd.sharing import ShareabilityPredictor, SharingStage
    I = inputs(c)
    T, B, N, D, Dg = c["T"], c["B"], c["N"], c["D"], c["Dg"]
    dt = SC.DTYPES[c["dtype"]]
    pred = ShareabilityPredictor(D, Dg, temperature=c["tau"], hard=c["hard"]).cuda().train()
    with torch.no_grad():
        pred.w_gate.copy_(dev(I["w_gate"]))
    stage = SharingStage(pred, T)
    cy, cs, cg = SC.functional(c)
    cy, cs, cg = cy.to(dt).cuda(), cs.to(dt).cuda(), cg.float().cuda()
    emb0 = dev(I["task_emb"])

    def step(xs, emb, noise, prev):
        pred.w_gate.grad = None
        outs, shared = stage({t: xs[t] for t in range(T)}, prev, emb, gamma=c["gamma"], noise=noise)
        f = sum((cy[t].view(B, N, D) * outs[t]).sum() for t in range(T)) + (cs * shared.x).sum() + (cg * shared.g.reshape(T, -1)).sum()
        grads = torch.autograd.grad(f, list(xs) + [pred.w_gate] + ([emb] if emb is not None else []))
        return [outs[t] for t in range(T)] + [shared.x, shared.bits, shared.flat_idx, shared.count, shared.g, shared.stats] + list(grads)

    def fresh(seed):
        J = SC.make_inputs(c, seed=seed)
        return ([dev(J["xs"][t]).view(B, N, D) for t in range(T)], dev(J["noise"]).view(T, B, N, 2),
                dev(J["prev"]).view(B, N) if c["prev"] else None)

    xs_a, noise_a, prev_a = fresh(0)
    sx = [x.clone().requires_grad_(True) for x in xs_a]
    semb = None if emb0 is None else emb0.clone().requires_grad_(True)
    snoise, sprev = noise_a.clone(), None if prev_a is None else prev_a.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                    # warm-up on the side stream, as torch's capture recipe asks
        step(sx, semb, snoise, sprev)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with ops.graph_capture(graph):
        captured = step(sx, semb, snoise, sprev)
    xs_b, noise_b, prev_b = fresh(3)
    with torch.no_grad():
        for s, x in zip(sx, xs_b):
            s.copy_(x)
        snoise.copy_(noise_b)
        if sprev is not None:
            sprev.copy_(prev_b)
    graph.replay()
    torch.cuda.synchronize()
    ex = [x.clone().requires_grad_(True) for x in xs_b]
    eemb = None if emb0 is None else emb0.clone().requires_grad_(True)
    eager = step(ex, eemb, noise_b, prev_b)
    assert len(eager) == len(captured)
    for i, (a, b) in enumerate(zip(captured, eager)):
        assert same_bits(a.contiguous(), b.contiguous()), f"output {i} of the replay differs from the eager run"
    assert not torch.equal(eager[T + 1], step([x.clone().requires_grad_(True) for x in xs_a], eemb, noise_a, prev_a)[T + 1]), \
        "the two input sets route alike: the replay would prove nothing"


def test_module_limits_on_the_device():
    """D outside the stated limit and mismatched task tensors are refused with a message, nothing is launched"""
    from m3vit_amd._lib import M3Error
    from m3vit_amd.sharing import ShareabilityPredictor, SharingStage
    pred = ShareabilityPredictor(1032).cuda()
    x = {t: torch.randn(1, 4, 1032, device="cuda") for t in range(2)}
    with pytest.raises(M3Error, match="D=1032"):
        SharingStage(pred, 2)(x)
    pred = ShareabilityPredictor(16).cuda()
    x = {0: torch.randn(1, 4, 16, device="cuda"), 1: torch.randn(1, 4, 16, device="cuda", dtype=torch.float16)}
    with pytest.raises(M3Error, match="one dtype"):
        SharingStage(pred, 2)(x)
