"""GPU contract tests of route.hip through the C ABI with guarded outputs: m3_route_build (one and several scan rounds,
E up to 256, counts64 present and NULL, a workspace of exactly m3_route_ws_elems ints under two fills), m3_route_assign on
blk_base / offsets from m3_balance_route, and the exchange plans m3_ep_plan / m3_ep_plan_fixed (what lies past the valid
rows, the overflow flag at cap and cap - 1, W and W * E_loc at their limits).  Every result is exact: the C oracle and
m3vit_amd.ep.ExchangePlan are the references."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import kernel_contract as kc

pytestmark = pytest.mark.gpu
I32, I64 = torch.int32, torch.int64


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    return _ops


def _p(t):
    return None if t is None else c_void_p(t.data_ptr())


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _ids(n, E, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, E, (n,), generator=g)
    if E > 2:
        idx[idx == 1] = 0                              # an empty expert
    return idx.to(I32)


def route_build(ops, idx, E, want64, fill=None):
    n = idx.numel()
    out = {"counts": kc.guarded(1, E, I32), "offsets": kc.guarded(1, E + 1, I32), "pos": kc.guarded(1, n, I32),
           "row_of_slot": kc.guarded(1, n, I32), "tile_starts": kc.guarded(1, E + 1, I32), "counts64": kc.guarded(1, E, I64)}
    ws, wcheck = kc.guarded_ws(int(ops.lib().m3_route_ws_elems(n, E)), I32)
    if fill is not None:
        ws.fill_(fill)
    v = {k: o[0] for k, o in out.items()}
    snap = kc.snapshot(idx=idx)
    ops._lib.check(ops.lib().m3_route_build(_p(idx), n, E, _p(v["counts"]), _p(v["offsets"]), _p(v["pos"]),
                                            _p(v["row_of_slot"]), _p(v["tile_starts"]),
                                            _p(v["counts64"]) if want64 else None, _p(ws), _stream()), "m3_route_build")
    torch.cuda.synchronize()
    kc.unchanged(snap)
    wcheck()
    for k, (_, chk) in out.items():
        chk(keep_rows=[0] if (k == "counts64" and not want64) else None, what=k)
    return {k: t[0].clone() for k, t in v.items()}


def assert_route_matches_oracle(r, idx, E, want64=True):
    from oracle import c_oracle
    cc, co, cp, cr = c_oracle.route_build(idx.cpu().numpy(), E)
    assert np.array_equal(r["counts"].cpu().numpy(), cc)
    if want64:
        assert np.array_equal(r["counts64"].cpu().numpy(), cc)
    assert np.array_equal(r["offsets"].cpu().numpy(), co)
    assert np.array_equal(r["pos"].cpu().numpy(), cp)
    assert np.array_equal(r["row_of_slot"].cpu().numpy(), cr)
    if "tile_starts" in r:
        assert np.array_equal(r["tile_starts"].cpu().numpy(), np.concatenate([[0], np.cumsum((cc + 127) // 128)]))


@pytest.mark.parametrize("E", [1, 3, 64, 65, 255, 256])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 65 * 1024 + 1, 100864])
def test_route_build(ops, n, E):
    idx = _ids(n, E, seed=n + E).cuda()
    want64 = (n + E) % 2 == 0
    r = route_build(ops, idx, E, want64)
    assert_route_matches_oracle(r, idx, E, want64)
    r2 = route_build(ops, idx, E, True, fill=-7)            # another workspace fill: the same bits
    for k in ("counts", "offsets", "pos", "row_of_slot", "tile_starts"):
        assert torch.equal(r[k], r2[k]), k


@pytest.mark.parametrize("k", [1, 2, 4, 8, 16])
def test_route_assign_from_the_balance_scan(ops, k):
    E = 16
    for T in (1, 64, 65, 1000, 1601):
        n = T * k
        g = torch.Generator().manual_seed(T * k)
        idx = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]) if k <= E else None
        idx = idx.to(I32).contiguous()
        nblk = ops.lib().m3_gate_num_blocks(T)
        pc = torch.zeros(nblk, E, dtype=torch.int64)
        pc.index_put_((torch.arange(T).repeat_interleave(k) // 64, idx.flatten().long()), torch.ones(n, dtype=torch.int64),
                      accumulate=True)
        pc = pc.to(I32).cuda()
        pi = torch.zeros(nblk, E, device="cuda"); pl = torch.zeros(nblk, E, dtype=I32, device="cuda")
        small = torch.empty(5, E, device="cuda"); load = torch.empty(E, dtype=I64, device="cuda")
        bb = torch.empty(nblk, E, dtype=I32, device="cuda"); meta = torch.empty(3 * E + 2, dtype=I32, device="cuda")
        ops._lib.check(ops.lib().m3_balance_route(_p(pi), _p(pl), None, nblk, E, _p(small[0]), _p(load), None, _p(small[1]),
                                                  None, _p(small[2]), None, _p(pc), _p(bb), _p(meta[:E]),
                                                  _p(meta[E:2 * E + 1]), _p(meta[2 * E + 1:]), None, _stream()),
                       "m3_balance_route")
        pos, pcheck = kc.guarded(1, n, I32)
        ros, rcheck = kc.guarded(1, n, I32)
        idx_d = idx.cuda()
        snap = kc.snapshot(idx=idx_d, bb=bb, meta=meta)
        ops._lib.check(ops.lib().m3_route_assign(_p(idx_d), n, E, k, _p(bb), _p(meta[E:2 * E + 1]), _p(pos), _p(ros),
                                                 _stream()), "m3_route_assign")
        torch.cuda.synchronize()
        kc.unchanged(snap); pcheck(what="pos"); rcheck(what="row_of_slot")
        assert_route_matches_oracle({"counts": meta[:E], "offsets": meta[E:2 * E + 1], "pos": pos[0], "row_of_slot": ros[0]},
                                    idx, E, want64=False)
    # k must divide 16 and n must be a whole number of tokens: loud rejections, nothing written
    pos, pcheck = kc.guarded(1, 48, I32)
    for kk, nn in ((3, 48), (k, 16 * k + 1) if k > 1 else (5, 50)):
        with pytest.raises(ops._lib.M3Error):
            ops._lib.check(ops.lib().m3_route_assign(_p(idx_d), nn, E, kk, _p(bb), _p(meta[E:]), _p(pos), _p(pos),
                                                     _stream()), "m3_route_assign")
    torch.cuda.synchronize()
    pcheck(keep_rows=[0])


# ------------------------------------------------------------------------------------------------- exchange plans
def _counts(W, e_loc, hi, seed):
    g = torch.Generator().manual_seed(seed)
    send = torch.randint(0, hi, (W * e_loc,), generator=g)
    recv = torch.randint(0, hi, (W * e_loc,), generator=g)
    if W * e_loc > 2:
        send[1] = 0; recv[2] = 0
    return send, recv


@pytest.mark.parametrize("W,e_loc,hi", [(1, 4, 40), (3, 5, 17), (8, 2, 3000), (64, 64, 6), (4096, 1, 5), (16, 256, 3)])
def test_ep_plan(ops, W, e_loc, hi):
    from m3vit_amd.ep import ExchangePlan
    send, recv = _counts(W, e_loc, hi, seed=W * e_loc)
    hp = ExchangePlan(send.tolist(), recv.tolist(), W, e_loc)
    cap = hp.n_recv + 300                                        # a buffer larger than the rows received
    sd, rd = send.cuda(), recv.cuda()
    splits, scheck = kc.guarded(1, 2 * W, I64)
    rg, gcheck = kc.guarded(cap, 1, I32)
    offs, ocheck = kc.guarded(1, e_loc + 1, I32)
    ts, tcheck = kc.guarded(1, e_loc + 1, I32)
    snap = kc.snapshot(sd=sd, rd=rd)
    ops._lib.check(ops.lib().m3_ep_plan(_p(sd), _p(rd), W, e_loc, _p(splits), _p(rg), cap, _p(offs), _p(ts), _stream()),
                   "m3_ep_plan")
    torch.cuda.synchronize()
    kc.unchanged(snap)
    scheck(what="splits"); ocheck(what="offsets"); tcheck(what="tile_starts")
    gcheck(keep_rows=list(range(hp.n_recv, cap)), what="regroup (rows past n_recv stay untouched)")
    assert splits[0].tolist() == hp.in_splits + hp.out_splits
    assert rg[:hp.n_recv, 0].tolist() == hp.regroup
    fc = torch.tensor(hp.fwd_expert_count)
    assert offs[0].tolist() == [0] + torch.cumsum(fc, 0).tolist()
    assert ts[0].tolist() == [0] + torch.cumsum((fc + 127) // 128, 0).tolist()


def fixed_reference(send, recv, W, e_loc, cap, ros, pos):
    """host statement of m3_ep_plan_fixed (the header's promises): regroup of the kept rows in (e, src) order as positions
    in the padded received buffer, offsets / tile_starts of the kept rows, pad_idx / unpad_idx, overflow"""
    rv = recv.view(W, e_loc).tolist()
    kept = [[0] * e_loc for _ in range(W)]
    start = [[0] * e_loc for _ in range(W)]
    for s in range(W):
        before = 0
        for e in range(e_loc):
            lo, hi = min(before, cap), min(before + rv[s][e], cap)
            kept[s][e] = hi - lo
            start[s][e] = s * cap + lo
            before += rv[s][e]
    regroup, fc = [], []
    for e in range(e_loc):
        c = 0
        for s in range(W):
            regroup.extend(range(start[s][e], start[s][e] + kept[s][e]))
            c += kept[s][e]
        fc.append(c)
    sv = send.view(W, e_loc).sum(1).tolist()
    send_off = [0]
    for d in range(W):
        send_off.append(send_off[-1] + sv[d])
    n = pos.numel()
    pad = []
    for d in range(W):
        nd = sv[d]
        for j in range(cap):
            slot = send_off[d] + (min(j, nd - 1) if nd > 0 else 0)
            slot = min(slot, n - 1) if n > 0 else 0
            pad.append(int(ros[slot]) if n > 0 else 0)
    unpad = []
    for i in range(n):
        sl = int(pos[i])
        d = 0
        while d + 1 < W and send_off[d + 1] <= sl:
            d += 1
        unpad.append(d * cap + min(sl - send_off[d], cap - 1))
    over = any(v > cap for v in sv) or any(sum(r) > cap for r in rv)
    return regroup, fc, pad, unpad, over


@pytest.mark.parametrize("W,e_loc,n_tok", [(1, 4, 300), (4, 3, 500), (8, 8, 2000), (64, 2, 3000), (64, 64, 4096)])
def test_ep_plan_fixed(ops, W, e_loc, n_tok):
    E = W * e_loc
    idx = _ids(n_tok, E, seed=E).long()
    # this rank's routing (what m3_route_build writes, stated on the host: E_tot = W * E_loc may exceed its 256 experts)
    ros = torch.sort(idx, stable=True).indices
    posh = torch.empty_like(ros)
    posh[ros] = torch.arange(n_tok)
    r = type("R", (), {})()
    r.row_of_slot, r.pos = ros.to(I32).cuda(), posh.to(I32).cuda()
    send = torch.bincount(idx, minlength=E)
    recv = _counts(W, e_loc, 40, seed=W)[1]
    mx = max(max(send.view(W, e_loc).sum(1).tolist()), max(recv.view(W, e_loc).sum(1).tolist()))
    for cap, preset, want in ((mx, 0, 0), (mx - 1, 0, 1), (mx + 5, 1, 1)):
        if cap < 1:
            continue
        sd, rd = send.cuda(), recv.cuda()
        out = {"splits": kc.guarded(1, 2 * W, I64), "regroup": kc.guarded(W * cap, 1, I32),
               "offsets": kc.guarded(1, e_loc + 1, I32), "tile_starts": kc.guarded(1, e_loc + 1, I32),
               "pad_idx": kc.guarded(1, W * cap, I32), "unpad_idx": kc.guarded(1, n_tok, I32),
               "overflow": kc.guarded(1, 1, I32)}
        v = {k: o[0] for k, o in out.items()}
        v["overflow"].fill_(preset)
        snap = kc.snapshot(sd=sd, rd=rd, ros=r.row_of_slot, pos=r.pos)
        ops._lib.check(ops.lib().m3_ep_plan_fixed(_p(sd), _p(rd), W, e_loc, cap, _p(r.row_of_slot), _p(r.pos), n_tok,
                                                  _p(v["splits"]), _p(v["regroup"]), _p(v["offsets"]), _p(v["tile_starts"]),
                                                  _p(v["pad_idx"]), _p(v["unpad_idx"]), _p(v["overflow"]), _stream()),
                       "m3_ep_plan_fixed")
        torch.cuda.synchronize()
        kc.unchanged(snap)
        regroup, fc, pad, unpad, over = fixed_reference(send, recv, W, e_loc, cap, r.row_of_slot.cpu(), r.pos.cpu())
        nv = len(regroup)
        for k, (_, chk) in out.items():
            chk(keep_rows=list(range(nv, W * cap)) if k == "regroup" else None, what=k)
        assert int(v["overflow"]) == want and bool(over) == (cap < mx), (cap, mx)
        assert v["regroup"][:nv, 0].tolist() == regroup
        assert v["offsets"][0].tolist() == [0] + torch.cumsum(torch.tensor(fc), 0).tolist()
        assert v["tile_starts"][0].tolist() == [0] + torch.cumsum((torch.tensor(fc) + 127) // 128, 0).tolist()
        assert v["pad_idx"][0].tolist() == pad
        assert v["unpad_idx"][0].tolist() == unpad
        from m3vit_amd.ep import ExchangePlan
        hp = ExchangePlan(send.tolist(), recv.tolist(), W, e_loc)
        assert v["splits"][0].tolist() == hp.in_splits + hp.out_splits
        if cap >= mx:                       # nothing dropped: the exact plan, rows moved to their padded positions
            rs = [0]
            for s in range(W):
                rs.append(rs[-1] + hp.out_splits[s])
            moved = []
            for q in hp.regroup:
                s = max(i for i in range(W) if rs[i] <= q)
                moved.append(s * cap + q - rs[s])
            assert moved == regroup
