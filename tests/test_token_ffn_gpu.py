"""GPU: the token blocks' FFN sublayer (csrc/token_ffn.hip, m3vit_amd.sharing.TokenFFNStage) against the float64 restatement
of token_ffn_cases.py, on generated inputs and on the reference's own results (tests/golden/g15_token_ffn.npz).

Exact: the work list (rows, slot_of, offsets, tile starts, count against the CPU enumeration), pass-through rows, the rows the
broadcast writes (one value, the same bits for every task), the zero gradients of overwritten rows and of unshared
representatives, run-to-run bits, graph replay against eager.  Within derived bounds (token_ffn_cases, SAFETY = 2, nothing
tuned per test): each row pass against float64 on the values it read.  Within the project's parity bounds (relative L2:
2e-5 fp32, 1e-3 fp16, 8e-3 bf16): the whole stage, forward and every gradient.  Every output of the C entry points lies in a
guarded allocation pre-filled with the sentinel; the compact buffers the row passes read carry NaN at and past row R."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import token_ffn_cases as TC                                                                          # noqa: E402
from kernel_contract import assert_within, guarded, guarded_ws, same_bits, snapshot, store, unchanged   # noqa: E402

pytestmark = pytest.mark.gpu
F64 = torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_token_ffn.npz")
PARAMS = ("gamma", "beta", "w1", "b1", "w2", "b2")
_CACHE = {}


def inputs(c):
    """the case's inputs, built once and shared by the tests (never modified)"""
    k = TC.case_id(c)
    if k not in _CACHE:
        _CACHE[k] = TC.make_inputs(c)
    return _CACHE[k]


def dev(t):
    return None if t is None else t.cuda()


def _ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _rows(ts):
    from m3vit_amd import _lib
    r = _lib.ShareRows()
    for i, t in enumerate(ts):
        r.p[i] = t.data_ptr()
    return r


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel(a, b):
    """as tests/test_engine.py defines it"""
    a = a.detach().double().cpu().flatten(); b = b.detach().double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def dims(c):
    return c["T"], c["B"] * c["N"], c["C"], TC.rows_ub(c["B"] * c["N"], c["T"], c["mode"]), TC.DTYPES[c["dtype"]]


def device_list(c, I):
    """the enumerated work list on the device in the kernels' layouts; rows past R hold 0 (a valid entry that must not be used)"""
    T, P, C, M_ub, dt = dims(c)
    w = I["wl"]
    rows = torch.zeros(max(M_ub, 1), dtype=torch.int32)
    rows[:w["R"]] = w["rows"].int()
    return rows.cuda(), w["slot_of"].int().contiguous().cuda(), torch.tensor([w["R"]], dtype=torch.int32).cuda()


def nan_tail(t, R):
    t[R:] = float("nan")
    return t


def scales(c, kind, gen):
    """DropPath factors: None, or per sample [B] / per position [P] values of {0, 1 / keep} with at least one 0 each"""
    if kind == "none":
        return None, None
    B, P = c["B"], c["B"] * c["N"]
    ps = torch.floor(0.75 + torch.rand(B, generator=gen)) / 0.75
    sps = torch.floor(0.75 + torch.rand(P, generator=gen)) / 0.75
    ps[int(torch.randint(0, B, (1,), generator=gen))] = 0.0
    sps[int(torch.randint(0, P, (1,), generator=gen))] = 0.0
    return ps, sps


ALL_CASES = TC.stage_cases() + TC.degenerate_cases()


# ------------------------------------------------------------------------------------------------------------ work list
@pytest.mark.parametrize("c", ALL_CASES, ids=TC.case_id)
def test_worklist_is_exact(c):
    """rows, slot_of, offsets, tile starts and count equal the CPU enumeration; entries of rows at and past R, the guards and
    the workspace's guard keep their bits; a degenerate pattern has the row count it was built for"""
    from m3vit_amd import _lib
    I = inputs(c)
    T, P, C, M_ub, dt = dims(c)
    w = I["wl"]
    bits = dev(I["bits"])
    snap = snapshot(bits=bits)
    rows, c1 = guarded(M_ub, 1, torch.int32)
    slot_of, c2 = guarded(T + 1, P, torch.int32)
    offsets, c3 = guarded(2, 1, torch.int32)
    tiles, c4 = guarded(2, 1, torch.int32)
    count, c5 = guarded(1, 1, torch.int32)
    ws, c6 = guarded_ws(int(_lib.lib().m3_token_ffn_list_ws_elems(P, T)), torch.int32)
    _lib.check(_lib.lib().m3_token_ffn_worklist(_ptr(bits), P, T, _lib.CONSTANTS["M3_TOKEN_FFN_" + c["mode"].upper()], _ptr(rows),
                                                _ptr(slot_of), _ptr(offsets), _ptr(tiles), _ptr(count), _ptr(ws), _stream()), "worklist")
    torch.cuda.synchronize()
    R = w["R"]
    c1(keep_rows=list(range(R, M_ub)), what="rows")
    for ck in (c2, c3, c4, c5, c6):
        ck()
    assert int(count[0, 0]) == R <= M_ub
    if TC.expected_rows(c) is not None:
        assert R == TC.expected_rows(c)
    assert rows.view(-1)[:R].cpu().long().tolist() == w["rows"].tolist()
    assert torch.equal(slot_of.cpu().long(), w["slot_of"])
    assert offsets.view(-1).tolist() == w["offsets"] and tiles.view(-1).tolist() == w["tile_starts"]
    unchanged(snap)


def test_worklist_limits():
    """T outside 2 .. 8 and an unknown mode are refused before anything is launched"""
    from m3vit_amd import _lib, ops
    bits = torch.zeros(8, dtype=torch.int64, device="cuda")
    for T in (1, 9):
        with pytest.raises(_lib.M3Error):
            ops.token_ffn_worklist(bits, T, "all")
    with pytest.raises(_lib.M3Error, match="neither"):
        ops.token_ffn_worklist(bits, 2, "private")


# ------------------------------------------------------------------------------------------------------ LayerNorm-gather
@pytest.mark.parametrize("c", ALL_CASES, ids=TC.case_id)
def test_ln_gather_forward(c):
    from m3vit_amd import _lib, ops
    I = inputs(c)
    T, P, C, M_ub, dt = dims(c)
    R = I["wl"]["R"]
    xs, sx = [dev(I["xs"][t]) for t in range(T)], dev(I["sx"])
    rows, _, count = device_list(c, I)
    gamma, beta = dev(I["params"]["gamma"]), dev(I["params"]["beta"])
    snap = snapshot(sx=sx, rows=rows, gamma=gamma, beta=beta, **{f"x{t}": x for t, x in enumerate(xs)})
    h, c1 = guarded(M_ub, C, dt)
    mean, c2 = guarded(M_ub, 1, torch.float32)
    rstd, c3 = guarded(M_ub, 1, torch.float32)
    xr = _rows(xs)
    _lib.check(_lib.lib().m3_token_ffn_ln_fwd(ctypes.byref(xr), _ptr(sx), ops.dt_code(dt), T, P, C, _ptr(rows), _ptr(count), M_ub,
                                              _ptr(gamma), _ptr(beta), TC.LN_EPS, _ptr(h), _ptr(mean), _ptr(rstd), _stream()), "ln_fwd")
    torch.cuda.synchronize()
    keep = list(range(R, M_ub))
    c1(keep_rows=keep, what="h"); c2(keep_rows=keep, what="mean"); c3(keep_rows=keep, what="rstd")
    unchanged(snap)
    if R == 0:
        return
    src = TC.source_rows(I["x64"], I["sx64"], I["wl"]["rows"], P)
    p = I["p64"]
    ref = TC.layernorm(src, p["gamma"], p["beta"])
    hb, mb, rb = TC.ln_gather_bounds(src, p["gamma"], p["beta"], ref, dt)
    assert_within(h[:R], ref, hb, "h")
    assert_within(mean.view(-1)[:R], src.mean(-1), mb, "mean")
    assert_within(rstd.view(-1)[:R], 1.0 / (src.var(-1, unbiased=False) + TC.LN_EPS).sqrt(), rb, "rstd")


# ------------------------------------------------------------------------------------------------------- scatter forward
@pytest.mark.parametrize("c", ALL_CASES, ids=TC.case_id)
def test_scatter_forward(c):
    """every y_t row by the formulas from a given compact f whose rows at and past R are NaN: outputs finite, listed rows within
    one fma and the store, pass-through rows x's own bits, broadcast rows one value for every task"""
    from m3vit_amd import _lib, ops
    I = inputs(c)
    T, P, C, M_ub, dt = dims(c)
    w = I["wl"]
    R = w["R"]
    gen = torch.Generator().manual_seed(11)
    f = nan_tail(torch.randn(M_ub, C, generator=gen).to(dt), R)
    ps, sps = scales(c, "none" if (c["T"] + c["N"]) % 2 else "drop", gen)
    xs, sx, fd, bits = [dev(I["xs"][t]) for t in range(T)], dev(I["sx"]), dev(f), dev(I["bits"])
    _, slot_of, _ = device_list(c, I)
    psd, spsd = dev(ps), dev(sps)
    snap = snapshot(sx=sx, f=fd, bits=bits, slot_of=slot_of, ps=psd, sps=spsd, **{f"x{t}": x for t, x in enumerate(xs)})
    ys, checks = [], []
    for _ in range(T):
        v, ck = guarded(P, C, dt)
        ys.append(v); checks.append(ck)
    xr, yr = _rows(xs), _rows(ys)
    _lib.check(_lib.lib().m3_token_ffn_scatter_fwd(ctypes.byref(xr), _ptr(sx), _ptr(fd), ops.dt_code(dt), T, P, c["N"], C,
                                                   ops.TOKEN_FFN_MODES[c["mode"]], _ptr(slot_of), _ptr(bits), _ptr(psd), _ptr(spsd),
                                                   ctypes.byref(yr), _stream()), "scatter_fwd")
    torch.cuda.synchronize()
    for ck in checks:
        ck()
    unchanged(snap)
    f64 = f.double()
    so = w["slot_of"]
    a_p = torch.ones(P, dtype=F64) if ps is None else ps.double().repeat_interleave(c["N"])
    a_s = torch.ones(P, dtype=F64) if sps is None else sps.double()
    M = TC.bit_masks(I["bits"], T)
    shared_out = I["sx64"] + a_s.unsqueeze(-1) * torch.nan_to_num(f64[so[T].clamp_min(0)])
    for t in range(T):
        y = ys[t].cpu()
        assert bool(torch.isfinite(y).all()), f"y[{t}] depends on a row past R"
        listed = so[t] >= 0
        own = I["x64"][t] + a_p.unsqueeze(-1) * torch.nan_to_num(f64[so[t].clamp_min(0)])
        ref = torch.where(M[t].unsqueeze(-1), shared_out, torch.where(listed.unsqueeze(-1), own, I["x64"][t]))
        assert_within(y, ref, TC.scatter_fwd_bound(ref, dt), f"y[{t}]")
        through = ~M[t] & ~listed
        assert same_bits(y[through], I["xs"][t][through]), f"y[{t}]: a row that is neither shared nor listed keeps x's bits"
    for t in range(T):
        for s in range(t + 1, T):
            both = (M[t] & M[s]).cuda()
            assert same_bits(ys[t][both], ys[s][both]), "tasks that share a position hold the same bits"


# ------------------------------------------------------------------------------------------------------- backward gather
@pytest.mark.parametrize("c", ALL_CASES, ids=TC.case_id)
def test_gather_backward(c):
    from m3vit_amd import _lib, ops
    I = inputs(c)
    T, P, C, M_ub, dt = dims(c)
    w = I["wl"]
    R = w["R"]
    gen = torch.Generator().manual_seed(12)
    dy = torch.randn(T, P, C, generator=gen).to(dt)
    ps, sps = scales(c, "drop" if (c["T"] + c["N"]) % 2 else "none", gen)
    dys, bits, psd, spsd = [dev(dy[t]) for t in range(T)], dev(I["bits"]), dev(ps), dev(sps)
    rows, _, count = device_list(c, I)
    snap = snapshot(bits=bits, rows=rows, ps=psd, sps=spsd, **{f"dy{t}": x for t, x in enumerate(dys)})
    df, ck = guarded(M_ub, C, dt)
    dyr = _rows(dys)
    _lib.check(_lib.lib().m3_token_ffn_gather_bwd(ctypes.byref(dyr), ops.dt_code(dt), T, P, c["N"], C, _ptr(rows), _ptr(count), M_ub,
                                                  _ptr(bits), _ptr(psd), _ptr(spsd), _ptr(df), _stream()), "gather_bwd")
    torch.cuda.synchronize()
    ck(keep_rows=list(range(R, M_ub)), what="df")
    unchanged(snap)
    if R == 0:
        return
    seg, pos = w["rows"] // P, w["rows"] % P
    a_p = torch.ones(P, dtype=F64) if ps is None else ps.double().repeat_interleave(c["N"])
    a_s = torch.ones(P, dtype=F64) if sps is None else sps.double()
    d64 = dy.double()
    M = TC.bit_masks(I["bits"], T).double()
    shared_sum, shared_abs = (M.unsqueeze(-1) * d64).sum(0), (M.unsqueeze(-1) * d64.abs()).sum(0)
    priv = seg < T
    segc = seg.clamp_max(T - 1)
    fac = torch.where(priv, a_p[pos], a_s[pos]).unsqueeze(-1)
    ref = fac * torch.where(priv.unsqueeze(-1), d64[segc, pos], shared_sum[pos])
    terms = fac.abs() * torch.where(priv.unsqueeze(-1), d64[segc, pos].abs(), shared_abs[pos])
    n = torch.where(priv, torch.ones_like(seg), M.sum(0).long()[pos]).double()
    assert_within(df[:R], ref, TC.gather_bwd_bound(ref, terms, n, dt), "df")


# ------------------------------------------------------------------------------------------------ position pass backward
@pytest.mark.parametrize("c", ALL_CASES, ids=TC.case_id)
def test_scatter_backward(c):
    """d x_t, d shared_x, d gamma, d beta from given d h / mean / rstd buffers whose rows at and past R are NaN: outputs finite;
    overwritten rows and unshared representatives exact zeros; pass-through rows d y's own bits"""
    from m3vit_amd import _lib, ops
    I = inputs(c)
    T, P, C, M_ub, dt = dims(c)
    w = I["wl"]
    R = w["R"]
    gen = torch.Generator().manual_seed(13)
    dy = torch.randn(T, P, C, generator=gen).to(dt)
    dh = nan_tail(torch.randn(M_ub, C, generator=gen).to(dt), R)
    src = TC.source_rows(I["x64"], I["sx64"], w["rows"], P)
    mu = src.mean(-1)
    var = ((src - mu.unsqueeze(-1)) ** 2).mean(-1)
    mean = nan_tail(torch.cat((mu, torch.zeros(M_ub - R, dtype=F64))).float(), R)
    rstd = nan_tail(torch.cat((1.0 / (var + TC.LN_EPS).sqrt(), torch.zeros(M_ub - R, dtype=F64))).float(), R)
    xs, sx, dys = [dev(I["xs"][t]) for t in range(T)], dev(I["sx"]), [dev(dy[t]) for t in range(T)]
    dhd, md, rd, bits, gamma = dev(dh), dev(mean), dev(rstd), dev(I["bits"]), dev(I["params"]["gamma"])
    _, slot_of, _ = device_list(c, I)
    snap = snapshot(sx=sx, dh=dhd, mean=md, rstd=rd, bits=bits, gamma=gamma, slot_of=slot_of,
                    **{f"x{t}": x for t, x in enumerate(xs)}, **{f"dy{t}": x for t, x in enumerate(dys)})
    dxs, checks = [], []
    for _ in range(T):
        v, ck = guarded(P, C, dt)
        dxs.append(v); checks.append(ck)
    dsx, ck = guarded(P, C, dt); checks.append(ck)
    dg, ck = guarded(1, C, torch.float32); checks.append(ck)
    db, ck = guarded(1, C, torch.float32); checks.append(ck)
    ws, ck = guarded_ws(ops.token_ffn_bwd_ws_elems(P, C)); checks.append(ck)
    xr, dyr, dxr = _rows(xs), _rows(dys), _rows(dxs)
    _lib.check(_lib.lib().m3_token_ffn_scatter_bwd(ctypes.byref(xr), _ptr(sx), ctypes.byref(dyr), _ptr(dhd), _ptr(md), _ptr(rd),
                                                   ops.dt_code(dt), T, P, C, ops.TOKEN_FFN_MODES[c["mode"]], _ptr(slot_of), _ptr(bits),
                                                   _ptr(gamma), ctypes.byref(dxr), _ptr(dsx), _ptr(ws), _ptr(dg), _ptr(db), _stream()),
               "scatter_bwd")
    torch.cuda.synchronize()
    for ck in checks:
        ck()
    unchanged(snap)
    so, M = w["slot_of"], TC.bit_masks(I["bits"], T)
    d64, g64 = dy.double(), I["p64"]["gamma"]
    ln, eln, tg, etg = TC.ln_bwd_terms(src, dh[:R].double(), g64, mean[:R].double(), rstd[:R].double())
    for t in range(T):
        out = dxs[t].cpu()
        assert bool(torch.isfinite(out).all()), f"dx[{t}] depends on a row past R"
        listed = so[t] >= 0
        assert not bool(out[M[t]].count_nonzero()), f"dx[{t}]: a row the broadcast overwrote has an exactly zero gradient"
        through = ~M[t] & ~listed
        assert same_bits(out[through], dy[t][through]), f"dx[{t}]: a pass-through row keeps d y's bits"
        if bool(listed.any()):
            s = so[t][listed]
            ref = d64[t][listed] + ln[s]
            bound = TC.SAFETY * (eln[s] + TC.U32 * (d64[t][listed].abs() + ln[s].abs()) + store(dt, ref))
            assert_within(out[listed], ref, bound, f"dx[{t}]")
    out = dsx.cpu()
    shared = so[T] >= 0
    assert bool(torch.isfinite(out).all()) and not bool(out[~shared].count_nonzero()), "d shared_x is exactly zero where bits == 0"
    if bool(shared.any()):
        s = so[T][shared]
        Md = M.double()[:, shared].unsqueeze(-1)
        gsum, gabs = (Md * d64[:, shared]).sum(0), (Md * d64[:, shared].abs()).sum(0)
        ref = gsum + ln[s]
        bound = TC.SAFETY * (eln[s] + (T + 1) * TC.U32 * (gabs + ln[s].abs()) + store(dt, ref))
        assert_within(out[shared], ref, bound, "d shared_x")
    dh64 = dh[:R].double()
    assert_within(dg.view(-1), tg.sum(0), TC.column_sum_bound(tg, etg, tg.sum(0)), "d gamma")
    assert_within(db.view(-1), dh64.sum(0), TC.column_sum_bound(dh64, torch.zeros_like(dh64), dh64.sum(0)), "d beta")


# ---------------------------------------------------------------------------------------------------------- whole stage
def make_stage(c, params, training=False, drop_path=0.0):
    from m3vit_amd.sharing import TokenFFNStage
    from m3vit_amd.vit import Mlp
    norm2, mlp = torch.nn.LayerNorm(c["C"], eps=TC.LN_EPS), Mlp(c["C"], c["H"])
    with torch.no_grad():
        for dst, name in ((norm2.weight, "gamma"), (norm2.bias, "beta"), (mlp.fc1.weight, "w1"), (mlp.fc1.bias, "b1"),
                          (mlp.fc2.weight, "w2"), (mlp.fc2.bias, "b2")):
            dst.copy_(params[name])
    st = TokenFFNStage(norm2, mlp, c["T"], mode=c["mode"], drop_path=drop_path).cuda()
    return st.train(training)


def stage_params(st):
    return [st.norm2.weight, st.norm2.bias, st.ffn.fc1.weight, st.ffn.fc1.bias, st.ffn.fc2.weight, st.ffn.fc2.bias]


def run_stage(c, st, xs, sx, bits, cy, ps=None, sps=None):
    """forward + backward of the module on device tensors: (ys [T] of [B, N, C], d xs, d sx, d params); cy: the incoming
    gradients [T, P, C] in the activation dtype"""
    from m3vit_amd.sharing import SharedTokens
    T, B, N, C = c["T"], c["B"], c["N"], c["C"]
    xl = [x.detach().clone().view(B, N, C).requires_grad_(True) for x in xs]
    sxl = sx.detach().clone().requires_grad_(True)
    shared = None if bits is None else SharedTokens(bits.view(B, N), sxl, None, None, None, None, T)
    out = st({t: xl[t] for t in range(T)}, shared, ps, sps)
    assert isinstance(out, dict) and sorted(out) == list(range(T))
    ys = [out[t] for t in range(T)]
    leaves = xl + ([sxl] if bits is not None else []) + stage_params(st)
    grads = list(torch.autograd.grad(ys, leaves, [cy[t].view(B, N, C) for t in range(T)], allow_unused=True))
    d_sx = grads.pop(T) if bits is not None else None
    return ys, grads[:T], d_sx, grads[T:]


def check_stage(c, I, ys, dxs, d_sx, dps, ref, what=""):
    T, P, C = c["T"], c["B"] * c["N"], c["C"]
    tol = TC.REL_BOUND[c["dtype"]]
    M = TC.bit_masks(I["bits"], T)
    figures = {}
    for t in range(T):
        figures[f"y[{t}]"] = rel(ys[t].reshape(P, C), ref["y"][t])
        figures[f"dx[{t}]"] = rel(dxs[t].reshape(P, C), ref["d_xs"][t])
        assert not bool(dxs[t].reshape(P, C).cpu()[M[t]].count_nonzero()), f"{what}dx[{t}] is exactly zero where the broadcast overwrote the row"
    if d_sx is not None:
        figures["d_sx"] = rel(d_sx, ref["d_sx"])
        assert not bool(d_sx.cpu()[I["bits"] == 0].count_nonzero()), f"{what}d shared_x is exactly zero where bits == 0"
    for name, g in zip(PARAMS, dps):
        figures["d_" + name] = rel(g, ref["d_" + name])
    print(f"{what}{TC.case_id(c)}: " + " ".join(f"{k}={v:.2e}" for k, v in figures.items()))
    bad = {k: v for k, v in figures.items() if not v <= tol}
    assert not bad, f"{what}relative error above {tol}: {bad}"


@pytest.mark.parametrize("c", ALL_CASES, ids=TC.case_id)
def test_stage_forward_and_backward(c):
    """the module against float64 on the rounded inputs, forward and every gradient, under the project's parity bounds; no
    device synchronisation in the forward or the backward"""
    I = inputs(c)
    T, P, C, M_ub, dt = dims(c)
    st = make_stage(c, I["params"])
    cy = TC.functional(c).to(dt)
    xs, sx, bits, cyd = [dev(I["xs"][t]) for t in range(T)], dev(I["sx"]), dev(I["bits"]), dev(cy)
    run_stage(c, st, xs, sx, bits, cyd)                                  # (first call: code objects load, torch allocates)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ys, dxs, d_sx, dps = run_stage(c, st, xs, sx, bits, cyd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ref = TC.reference(c, I, cy=cy.double())
    check_stage(c, I, ys, dxs, d_sx, dps, ref)
    R = I["wl"]["R"]
    if R == 0:                                                          # a grouped launch whose only group is empty
        for t in range(T):
            assert same_bits(ys[t].reshape(P, C), xs[t]), "nothing listed: y_t is x_t"
        for name, g in zip(PARAMS, dps):
            assert not bool(g.count_nonzero()), f"nothing listed: d {name} is zero"


def test_no_shared_tokens_is_the_all_zero_word():
    """shared=None (the reference's shared_bits=None): every row private, the same bits as an all-zero bits tensor"""
    c = TC.case(3, (1, 65), (192, 384), "f16", "all", "none")
    I = inputs(c)
    T, P, C, M_ub, dt = dims(c)
    st = make_stage(c, I["params"])
    cyd = dev(TC.functional(c).to(dt))
    xs, sx = [dev(I["xs"][t]) for t in range(T)], dev(I["sx"])
    a = run_stage(c, st, xs, sx, None, cyd)
    b = run_stage(c, st, xs, sx, dev(I["bits"]), cyd)
    for u, v in zip(a[0] + a[1] + a[3], b[0] + b[1] + b[3]):
        assert same_bits(u, v)
    lst = st([x.view(1, 65, C) for x in xs])
    assert isinstance(lst, list) and same_bits(lst[0], a[0][0])


@pytest.mark.parametrize("key", [TC.case_id(c) for c in TC.golden_cases()] + [TC.case_id(TC.golden_train_case()) + "/train"])
def test_stage_on_the_golden(key):
    """the HIP path in f32 on the reference's inputs against the reference's own outputs and gradients (the training case with
    its recorded drop-path draws handed over as factors)"""
    z = np.load(GOLDEN)
    c = TC.golden_train_case() if key.endswith("/train") else next(c for c in TC.golden_cases() if TC.case_id(c) == key)
    g = lambda n: torch.from_numpy(z[f"{key}/{n}"])                                   # noqa: E731
    T, P, C = c["T"], c["B"] * c["N"], c["C"]
    train = key.endswith("/train")
    st = make_stage(c, {n: g(n) for n in PARAMS}, training=train, drop_path=0.25 if train else 0.0)
    ps = dev(g("path_scale").float()) if train else None
    sps = dev(g("shared_path_scale").float()) if train else None
    xs, sx, bits = [dev(g("xs")[t]) for t in range(T)], dev(g("sx")), dev(g("bits"))
    ys, dxs, d_sx, dps = run_stage(c, st, xs, sx, bits, dev(TC.functional(c).float()), ps, sps)
    I = dict(bits=g("bits"))
    ref = {"y": g("y"), "d_xs": g("d_xs"), "d_sx": g("d_sx"), **{"d_" + n: g("d_" + n) for n in PARAMS}}
    check_stage(c, I, ys, dxs, d_sx, dps, ref, what="golden ")


@pytest.mark.parametrize("c", [TC.stage_cases()[16], TC.stage_cases()[11], TC.degenerate_cases()[3]], ids=TC.case_id)
def test_two_runs_give_the_same_bits(c):
    I = inputs(c)
    T, P, C, M_ub, dt = dims(c)
    st = make_stage(c, I["params"])
    cyd = dev(TC.functional(c).to(dt))
    gen = torch.Generator().manual_seed(3)
    ps, sps = scales(c, "drop", gen)
    xs, sx, bits = [dev(I["xs"][t]) for t in range(T)], dev(I["sx"]), dev(I["bits"])
    a = run_stage(c, st, xs, sx, bits, cyd, dev(ps), dev(sps))
    junk = torch.randn(1 << 22, device="cuda")                          # other allocations in between: the workspaces move
    b = run_stage(c, st, xs, sx, bits, cyd, dev(ps), dev(sps))
    del junk
    for i, (u, v) in enumerate(zip(a[0] + a[1] + [a[2]] + a[3], b[0] + b[1] + [b[2]] + b[3])):
        assert same_bits(u, v), f"tensor {i} differs between two runs on the same inputs"


@pytest.mark.parametrize("mode", TC.MODES)
def test_explicit_drop_path_factors(mode):
    """per-sample and per-position factors, zeros among them, against the restatement; in training with drop_path > 0 and no
    factors the module draws them itself: every row is then x, or x plus F / keep"""
    from m3vit_amd.sharing import SharedTokens
    c = TC.case(3, (2, 197), (192, 384), "f16", mode, "mixed")
    I = inputs(c)
    T, P, C, M_ub, dt = dims(c)
    gen = torch.Generator().manual_seed(21)
    ps, sps = scales(c, "drop", gen)
    st = make_stage(c, I["params"], training=True, drop_path=0.25)
    cy = TC.functional(c).to(dt)
    xs, sx, bits = [dev(I["xs"][t]) for t in range(T)], dev(I["sx"]), dev(I["bits"])
    ys, dxs, d_sx, dps = run_stage(c, st, xs, sx, bits, dev(cy), dev(ps), dev(sps).view(c["B"], c["N"]))
    ref = TC.reference(c, I, ps.double(), sps.double(), cy=cy.double())
    check_stage(c, I, ys, dxs, d_sx, dps, ref, what="drop ")
    # drawn on the device: y - x is 0 or F / keep, per sample for private rows
    torch.manual_seed(5)
    out = st({t: xs[t].view(c["B"], c["N"], C) for t in range(T)}, SharedTokens(bits.view(c["B"], c["N"]), sx, None, None, None, None, T))
    full = TC.stage(I["x64"], I["bits"], I["sx64"], I["p64"], mode, c["N"])
    M = TC.bit_masks(I["bits"], T)
    dropped = kept = 0
    for t in range(T):
        y = out[t].reshape(P, C).double().cpu()
        base = torch.where(M[t].unsqueeze(-1), I["sx64"], I["x64"][t])
        ffn = (full[t] - base) / 0.75
        e0, e1 = (y - base).norm(dim=-1), (y - base - ffn).norm(dim=-1)
        scale = ffn.norm(dim=-1) + 1e-30
        is0, is1 = e0 <= 4e-3 * scale + 1e-6, e1 <= 4e-3 * scale
        active = M[t] | (mode == "all")
        assert bool((is0 | is1)[active].all()), "a row is neither dropped nor kept"
        dropped += int((is0 & ~is1)[active].sum()); kept += int((is1 & ~is0)[active].sum())
        if mode == "all":                                               # one factor per sample for the private rows
            for b in range(c["B"]):
                pr = (~M[t])[b * c["N"]:(b + 1) * c["N"]]
                k = (is1 & ~is0)[b * c["N"]:(b + 1) * c["N"]][pr]
                assert bool(k.all()) or not bool(k.any())
    assert dropped > 0 and kept > 0


def test_graph_capture_replays_other_row_counts():
    """forward + backward captured once at (2, 197), T = 3, f16; replayed after new x, shared_x and bits were copied into the
    static tensors, for three patterns with different R (40 % shared, none, all): each replay equals the eager run bit for bit"""
    from m3vit_amd import ops
    from m3vit_amd.sharing import SharedTokens
    T, B, N, C = 3, 2, 197, 192
    cases = [TC.case(T, (B, N), (C, 384), "f16", "all", pat) for pat in ("mixed", "none", "all")]
    Is = [TC.make_inputs(c, seed=40 + i) for i, c in enumerate(cases)]
    assert len({I["wl"]["R"] for I in Is}) == 3
    c, dt = cases[0], torch.float16
    st = make_stage(c, Is[0]["params"])
    cyd = dev(TC.functional(c).to(dt))
    prm = stage_params(st)

    def step(xl, sxl, bits):
        out = st({t: xl[t] for t in range(T)}, SharedTokens(bits.view(B, N), sxl, None, None, None, None, T))
        ys = [out[t] for t in range(T)]
        grads = torch.autograd.grad(ys, xl + [sxl] + prm, [cyd[t].view(B, N, C) for t in range(T)])
        return ys + list(grads)

    def fresh(I):
        return [dev(I["xs"][t]).view(B, N, C).requires_grad_(True) for t in range(T)], dev(I["sx"]).requires_grad_(True), dev(I["bits"])

    sxs, ssx, sbits = fresh(Is[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                    # warm-up on the side stream, as torch's capture recipe asks
        step(sxs, ssx, sbits)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with ops.graph_capture(graph):
        captured = step(sxs, ssx, sbits)
    for I in (Is[1], Is[2], Is[0]):
        xl, sxl, bits = fresh(I)
        with torch.no_grad():
            for s, x in zip(sxs, xl):
                s.copy_(x)
            ssx.copy_(sxl)
            sbits.copy_(bits)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(xl, sxl, bits)
        for i, (a, b) in enumerate(zip(captured, eager)):
            assert same_bits(a.contiguous(), b.contiguous()), f"R = {I['wl']['R']}: output {i} of the replay differs from the eager run"


def test_chained_with_the_sharing_stage():
    """the outs / SharedTokens of a SharingStage call fed straight in: forward and the gradients that reach the sharing stage's
    inputs and predictor against float64 autograd of the two restatements composed"""
    import sharing_cases as SC
    from m3vit_amd.sharing import ShareabilityPredictor, SharingStage
    sc = SC.case(3, (2, 197), 192, 0, "f16", False, False)
    J = SC.make_inputs(sc)
    c = TC.case(3, (2, 197), (192, 384), "f16", "all", "chained")
    T, B, N, C, dt = 3, 2, 197, 192, torch.float16
    P = B * N
    params = TC.make_params(C, 384, torch.Generator().manual_seed(77))
    st = make_stage(c, params)
    pred = ShareabilityPredictor(C, 0, temperature=sc["tau"], hard=False).cuda().train()
    with torch.no_grad():
        pred.w_gate.copy_(dev(J["w_gate"]))
    sharing = SharingStage(pred, T)
    cy = TC.functional(c).to(dt)
    xl = [dev(J["xs"][t]).view(B, N, C).requires_grad_(True) for t in range(T)]
    outs, shared = sharing({t: xl[t] for t in range(T)}, None, None, gamma=sc["gamma"], noise=dev(J["noise"]).view(T, B, N, 2))
    out = st(outs, shared)
    ys = [out[t] for t in range(T)]
    grads = torch.autograd.grad(ys, xl + [pred.w_gate] + stage_params(st), [dev(cy)[t].view(B, N, C) for t in range(T)])
    assert torch.equal(shared.bits.reshape(-1).cpu(), J["ref"]["bits"])

    x64 = J["x64"].clone().requires_grad_(True)
    w64 = J["w64"].clone().requires_grad_(True)
    p64 = {k: (v.double().requires_grad_(True) if torch.is_tensor(v) else v) for k, v in params.items()}
    r = SC.stage(x64, w64, None, J["n64"], sc["tau"], False, sc["gamma"], sc["eps"], None, with_stats=False)
    y64 = TC.stage(r["y"], r["bits"], r["shared_x"], p64, "all", N)
    (cy.double() * y64).sum().backward()
    tol = TC.REL_BOUND["f16"]
    figures = {f"y[{t}]": rel(ys[t].reshape(P, C), y64[t]) for t in range(T)}
    figures.update({f"dx[{t}]": rel(grads[t].reshape(P, C), x64.grad[t]) for t in range(T)})
    figures.update({"d_" + n: rel(g, p64[n].grad) for n, g in zip(PARAMS, grads[T + 1:])})
    # (the predictor's own gradient is the sharing stage's business, held to its derived bounds in test_sharing_gpu.py: printed)
    print("chained: " + " ".join(f"{k}={v:.2e}" for k, v in figures.items()) + f" (d_w_gate={rel(grads[T], w64.grad):.2e})")
    bad = {k: v for k, v in figures.items() if not v <= tol}
    assert not bad, f"relative error above {tol}: {bad}"


def test_module_limits_on_the_device():
    """mismatched shared tokens and a width the Mlp does not take are refused with a message, nothing is launched"""
    from m3vit_amd._lib import M3Error
    from m3vit_amd.sharing import SharedTokens
    c = TC.case(2, (1, 4), (16, 32), "f32", "all", "none")
    st = make_stage(c, TC.make_params(16, 32, torch.Generator().manual_seed(1)))
    x = {t: torch.randn(1, 4, 16, device="cuda") for t in range(2)}
    bits = torch.zeros(1, 4, dtype=torch.int64, device="cuda")
    with pytest.raises(M3Error, match="do not go with"):
        st(x, SharedTokens(bits, torch.zeros(4, 16, device="cuda", dtype=torch.float16), None, None, None, None, 2))
    with pytest.raises(M3Error, match="do not go with"):
        st(x, SharedTokens(bits[:, :3], torch.zeros(4, 16, device="cuda"), None, None, None, None, 2))
    with pytest.raises(M3Error, match="width"):
        st({t: torch.randn(1, 4, 24, device="cuda") for t in range(2)})
    with pytest.raises(M3Error, match="path_scale"):
        st(x, None, torch.ones(3, device="cuda"))
    y = st(x, SharedTokens(bits, torch.zeros(4, 16, device="cuda"), None, None, None, None, 2))
    assert y[0].shape == (1, 4, 16) and bool(torch.isfinite(y[0]).all())
