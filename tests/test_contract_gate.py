"""GPU contract tests of the router kernels of gate.hip, called through the C ABI with guarded outputs: m3_gate_fwd at all
60 instantiations (dtype x EPAD x exact / padded E x NS row-length fast path), m3_balance_loss / m3_balance_route /
m3_gate_reduce on synthetic partials (every branch of the reduction loop), m3_gate_bwd_logits at every EPAD with each
upstream gradient on and off, and m3_gate_bwd_params (the dw4 and fallback dW kernels, the dx kernel, the rejections).
Values are checked elementwise against fp64 under the bounds of kernel_contract (derivations there); expert indices
and clean logits bit for bit against the C oracle; inputs keep their bits."""
from ctypes import byref, c_void_p

import pytest
import torch

import kernel_contract as kc

pytestmark = pytest.mark.gpu
F32, F16, BF16, I32, I64 = torch.float32, torch.float16, torch.bfloat16, torch.int32, torch.int64
WORST = {}
NEAR = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    yield _ops
    if WORST:
        print("\ngate worst err/bound:", max(WORST.values()), max(WORST, key=WORST.get))
    if NEAR:
        print("gate top-k near-ties:", sum(NEAR.values()), "of", len(NEAR), "calls")


def _p(t):
    """the device pointer of t; an empty slice (nblk = 0) passes its allocation's (torch reports NULL for it)"""
    if t is None:
        return None
    return c_void_p(t.data_ptr() if t.numel() else t.untyped_storage().data_ptr())


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# ------------------------------------------------------------------------------------------------------ m3_gate_fwd
DT_CODE = {F32: 0, F16: 1, BF16: 2}
EPADS = {4: 4, 8: 8, 16: 16, 32: 32, 64: 64}
PADDED = {4: 3, 8: 5, 16: 12, 32: 24, 64: 48}
TS = [1, 63, 64, 65, 1000, 25216]


def _instances():
    """(dtype, EPAD, exact, NS, D): every template instance of gate_fwd_kernel"""
    out = []
    for dt in (F32, F16, BF16):
        es = 4 if dt == F32 else 2
        small = 16 // es                                   # the smallest legal D (one 16-byte chunk)
        odd = 36 if dt == F32 else 200                      # NS = 0 with a row that is not a multiple of 128 B
        for ep in EPADS:
            out.append((dt, ep, True, 6, 768 // es))
            out.append((dt, ep, True, 12, 1536 // es))
            out.append((dt, ep, True, 0, odd if ep in (4, 16, 64) else small))
            out.append((dt, ep, False, 0, small if ep in (4, 16, 64) else odd))
    return out


INSTANCES = _instances()
IDS = [f"{str(dt)[6:]}-epad{ep}-{'exact' if ex else 'padded'}-ns{ns}" for dt, ep, ex, ns, _ in INSTANCES]


def gate_call(ops, x, w, k, *, bias=None, noise=None, std=0.0, ldx=None, optional=True, T=None):
    """one m3_gate_fwd through the C ABI; every output (present or NULL) guarded.  Returns (outputs dict, checks)."""
    T = x.shape[0] if T is None else T
    D, E = w.shape
    kp = min(k + 1, E)
    nblk = ops.lib().m3_gate_num_blocks(T)
    prob = noise is not None and std != 0.0 and k < E and optional
    shapes = {"idx": (T, k, I64), "idx32": (T, k, I32), "idx_next": (T, 1, I32), "score": (T, k, F32),
              "top_logits": (T, kp, F32), "clean": (T, E, F32), "noisy": (T, E, F32), "gates": (T, E, F32),
              "part_importance": (nblk, E, F32), "part_load": (nblk, E, I32), "part_load_prob": (nblk, E, F32),
              "part_count": (nblk, E, I32)}
    passed = {"idx", "score", "top_logits", "part_importance", "part_load"}
    if optional:
        passed |= {"idx32", "clean", "noisy", "gates", "part_count"} | ({"idx_next"} if kp > k else set())
        if prob:
            passed.add("part_load_prob")
    bufs, checks = {}, {}
    for n, (r, c, dt) in shapes.items():
        bufs[n], checks[n] = kc.guarded(max(r, 1), c, dt)      # (T = 0: one row the call must not touch, a real pointer)
    a = ops._lib.GateFwdArgs(_p(x), DT_CODE[x.dtype], T, D, x.stride(0) if ldx is None else ldx, _p(w), E, _p(bias),
                             _p(noise), float(std), k, *[_p(bufs[n]) if n in passed else None for n in
                                                         ("idx", "idx32", "idx_next", "score", "top_logits", "clean",
                                                          "noisy", "gates", "part_importance", "part_load",
                                                          "part_load_prob", "part_count")])
    snap = kc.snapshot(x=x, w=w, bias=bias, noise=noise)
    ops._lib.check(ops.lib().m3_gate_fwd(byref(a), _stream()), "m3_gate_fwd")
    torch.cuda.synchronize()
    kc.unchanged(snap)
    for n, chk in checks.items():
        chk(keep_rows=None if (n in passed and T > 0) else list(range(max(shapes[n][0], 1))), what=n)
    o = {n: (bufs[n][:T].reshape(T) if n == "idx_next" else bufs[n][:shapes[n][0]]) if n in passed else None for n in shapes}
    return o


def run_gate(ops, dtype, D, E, k, T, *, seed, pad=0, bias=False, noise=False, optional=True, tag=""):
    from oracle import c_oracle
    es = 4 if dtype == F32 else 2
    ldx = D + pad
    xb = torch.zeros(T, ldx, dtype=dtype)
    xb[:, :D] = rnd(T, D, seed=seed).to(dtype)
    xb = xb.cuda()
    x = xb[:, :D]
    assert (ldx * es) % 16 == 0
    w = rnd(D, E, scale=0.3 / D ** 0.5 * 4, seed=seed + 1).cuda()
    b = rnd(E, scale=0.5, seed=seed + 2).cuda() if bias else None
    nz = rnd(T, E, seed=seed + 3).cuda() if noise else None
    std = 1.0 / E if noise else 0.0
    o = gate_call(ops, x, w, k, bias=b, noise=nz, std=std, ldx=ldx, optional=optional)
    c = c_oracle.gate_fwd(x.float().cpu().contiguous().numpy(), w.cpu().numpy(), k,
                          bias=None if b is None else b.cpu().numpy(), noise=None if nz is None else nz.cpu().numpy(),
                          std=std)
    assert torch.equal(o["idx"].cpu(), torch.from_numpy(c["idx"])), "idx differs from the C oracle"
    if o["clean"] is not None:
        assert kc.same_bits(o["clean"].cpu(), torch.from_numpy(c["clean"])), "clean differs from the C oracle"
    worst, near = kc.check_gate_fwd(o, x, w, k, bias=b, noise=nz, std=std)
    assert near <= max(2, T * k // 20), f"{near} near-ties in {T * k} selections"
    WORST[tag] = worst
    NEAR[tag] = near
    return worst


def _legal_ks(E):
    return sorted({k for k in (1, 2, 4, 8, E - 1, E) if 1 <= k <= min(8, E)})


@pytest.mark.parametrize("inst", range(len(INSTANCES)), ids=IDS)
def test_gate_fwd_every_instance(ops, inst):
    """two calls per instance: all optional outputs present, then all NULL; k, T, the row pad, the bias and the noise cycle
    pairwise over the instances"""
    dtype, ep, exact, ns, D = INSTANCES[inst]
    E = ep if exact else PADDED[ep]
    ks = _legal_ks(E)
    es = 4 if dtype == F32 else 2
    for j in range(2):
        k = ks[(inst + j) % len(ks)]
        T = TS[(inst + 3 * j) % len(TS)]
        if T == 25216 and D * E > 384 * 16:
            T = 4097
        pad = (32 // es) if (inst + j) % 2 == 0 else 0
        w = run_gate(ops, dtype, D, E, k, T, seed=100 * inst + j, pad=pad, bias=(inst // 2 + j) % 2 == 0,
                     noise=(inst // 3 + j) % 2 == 0, optional=j == 0, tag=f"{IDS[inst]}/{j}")
        assert w < 1


def test_gate_fwd_zero_tokens_write_nothing(ops):
    x = torch.zeros(1, 64, device="cuda")
    w = rnd(64, 16, seed=1).cuda()
    gate_call(ops, x, w, 4, T=0)          # every guard (and the empty views) keeps the sentinel


@pytest.mark.parametrize("E,k", [(16, 8), (64, 8), (12, 8)])
def test_gate_fwd_underflowing_selected_probability(ops, E, k):
    """a bias spread that underflows the softmax tail: a selected expert with probability exactly 0 is counted by
    part_count (routing) and not by part_load (gates > 0)"""
    T, D = 300, 64
    x = rnd(T, D, seed=E).cuda()
    w = rnd(D, E, scale=0.05, seed=E + 1).cuda()
    bias = torch.linspace(0.0, 110.0 * (E - 1), E).cuda()
    o = gate_call(ops, x, w, k, bias=bias)
    worst, _ = kc.check_gate_fwd(o, x, w, k, bias=bias)
    assert int(o["part_load"].sum()) < int(o["part_count"].sum()) == T * k, "the underflow case must occur"
    WORST[f"underflow/{E}/{k}"] = worst


# --------------------------------------------------------------------------------------- the balance reduction
def balance_case(E, nblk, seed, prob=True):
    g = torch.Generator().manual_seed(seed)
    nb = max(nblk, 1)
    pi = (torch.rand(nb, E, generator=g) * 128 / max(E, 1)).cuda()
    pl = torch.randint(0, 65, (nb, E), generator=g).to(I32).cuda()
    pp = (torch.rand(nb, E, generator=g) * 64).cuda() if prob else None
    pc = torch.randint(0, 65, (nb, E), generator=g).to(I32).cuda()
    return pi[:nblk], pl[:nblk], (pp[:nblk] if prob else None), pc[:nblk]


def _nblks(E):
    RL = 1024 // E
    return sorted({0, 1, 3 * RL, 3 * RL + 1, 4 * RL + 5, 394, 1600 + 7 * E})


def balance_call(ops, E, pi, pl, pp, pc=None, loss_acc0=0.25):
    nblk = pi.shape[0]
    outs = {n: kc.guarded(1, E, dt) for n, dt in (("importance", F32), ("load", I64), ("load_prob", F32),
                                                   ("d_importance", F32), ("d_load_prob", F32))}
    loss, lcheck = kc.guarded(1, 1, F32)
    acc, acheck = kc.guarded(1, 1, F32)
    acc.fill_(loss_acc0)
    snap = kc.snapshot(pi=pi, pl=pl, pp=pp, pc=pc)
    v = {n: o[0] for n, o in outs.items()}
    if pc is None:
        rc = ops.lib().m3_balance_loss(_p(pi), _p(pl), _p(pp), nblk, E, _p(v["importance"]), _p(v["load"]),
                                       _p(v["load_prob"]), _p(loss), _p(acc), _p(v["d_importance"]), _p(v["d_load_prob"]),
                                       _stream())
        route = None
    else:
        route = {n: kc.guarded(r, c, I32) for n, (r, c) in (("blk_base", (nblk, E)), ("counts", (1, E)),
                                                          ("offsets", (1, E + 1)), ("tile_starts", (1, E + 1)))}
        route["counts64"] = kc.guarded(1, E, I64)
        r = {n: o[0] for n, o in route.items()}
        rc = ops.lib().m3_balance_route(_p(pi), _p(pl), _p(pp), nblk, E, _p(v["importance"]), _p(v["load"]),
                                        _p(v["load_prob"]), _p(loss), _p(acc), _p(v["d_importance"]),
                                        _p(v["d_load_prob"]), _p(pc), _p(r["blk_base"]), _p(r["counts"]), _p(r["offsets"]),
                                        _p(r["tile_starts"]), _p(r["counts64"]), _stream())
    ops._lib.check(rc, "balance")
    torch.cuda.synchronize()
    kc.unchanged(snap)
    for n, (_, chk) in outs.items():
        chk(what=n)
    lcheck(what="loss"); acheck(what="loss_acc")
    if route:
        for n, (_, chk) in route.items():
            chk(what=n)
        route = {n: o[0].clone() for n, o in route.items()}
    return {n: t.clone() for n, t in v.items()}, loss.clone(), acc.clone(), route


@pytest.mark.parametrize("E", [1, 2, 5, 16, 48, 64])
def test_balance_reduction_loss_and_route(ops, E):
    for nblk in _nblks(E):
        for prob in (True, False):
            pi, pl, pp, pc = balance_case(E, nblk, seed=nblk * 7 + E, prob=prob)
            use_route = nblk >= 1 and prob
            v, loss, acc, route = balance_call(ops, E, pi, pl, pp, pc if use_route else None)
            tag = f"balance/E{E}/nblk{nblk}/{'prob' if prob else 'count'}"
            # the sums: importance / load_prob under sum_bound, load exactly
            pi64, pp64 = pi.double().sum(0), (pp.double().sum(0) if prob else None)
            w = kc.assert_within(v["importance"][0], pi64, kc.sum_bound(pi.double().abs().sum(0), max(nblk, 1), pi64, F32),
                                 "importance")
            assert torch.equal(v["load"][0], pl.long().sum(0)), "load"
            if prob:
                w = max(w, kc.assert_within(v["load_prob"][0], pp64,
                                            kc.sum_bound(pp.double().abs().sum(0), max(nblk, 1), pp64, F32), "load_prob"))
            # the loss and its gradients on the kernel's own reduced vectors
            vi = v["importance"][0].double().cpu()
            vl = (v["load_prob"][0] if prob else v["load"][0]).double().cpu()
            cvi, gi = kc.cv2_reference(vi)
            cvl, gl = kc.cv2_reference(vl)
            bci, bgi = kc.cv2_bound(vi)
            bcl, bgl = kc.cv2_bound(vl)
            ref = cvi + cvl
            if E == 1:
                assert float(loss) == 0.0 and float(v["d_importance"].abs().max()) == 0.0
            w = max(w, kc.assert_within(loss.view(()), ref, bci + bcl + kc.SAFETY * kc.U32 * ref.abs(), "cv_loss"))
            w = max(w, kc.assert_within(v["d_importance"][0], gi, bgi, "d_importance"))
            if prob:
                w = max(w, kc.assert_within(v["d_load_prob"][0], gl, bgl, "d_load_prob"))
            else:
                assert float(v["d_load_prob"].abs().max()) == 0.0 and not bool(v["d_load_prob"].isnan().any()), \
                    "d_load_prob must be zeros without part_load_prob"
            assert kc.same_bits(acc.view(()), torch.tensor(0.25, device="cuda") + loss.view(())), "loss_acc != fl(before + loss)"
            if use_route:
                cnt = pc.long()
                base = torch.cumsum(cnt, 0) - cnt
                tot = cnt.sum(0)
                offs = torch.cat((tot.new_zeros(1), torch.cumsum(tot, 0)))
                ts = torch.cat((tot.new_zeros(1), torch.cumsum((tot + 127) // 128, 0)))
                assert torch.equal(route["blk_base"].long(), base), "blk_base"
                assert torch.equal(route["counts"][0].long(), tot) and torch.equal(route["counts64"][0], tot), "counts"
                assert torch.equal(route["offsets"][0].long(), offs) and torch.equal(route["tile_starts"][0].long(), ts)
            # the whole launch again: the same bits
            v2, loss2, acc2, route2 = balance_call(ops, E, pi, pl, pp, pc if use_route else None)
            assert all(kc.same_bits(v[n], v2[n]) for n in v) and kc.same_bits(loss, loss2) and kc.same_bits(acc, acc2)
            if route:
                assert all(torch.equal(route[n], route2[n]) for n in route)
            WORST[tag] = w
            assert w < 1


@pytest.mark.parametrize("E", [1, 5, 64])
def test_gate_reduce(ops, E):
    for nblk in (0, 1, 394, 1600):
        pi, pl, _, _ = balance_case(E, nblk, seed=nblk + E, prob=False)
        imp, icheck = kc.guarded(1, E, F32)
        load, lcheck = kc.guarded(1, E, I64)
        ops._lib.check(ops.lib().m3_gate_reduce(_p(pi), _p(pl), nblk, E, _p(imp), _p(load), _stream()), "m3_gate_reduce")
        torch.cuda.synchronize()
        icheck(); lcheck()
        ref = pi.double().sum(0)
        WORST[f"reduce/{E}/{nblk}"] = kc.assert_within(imp[0], ref, kc.sum_bound(ref.abs(), max(nblk, 1), ref, F32))
        assert torch.equal(load[0], pl.long().sum(0))


# --------------------------------------------------------------------------------------------- m3_gate_bwd_logits
BWD_E = [2, 3, 4, 5, 8, 12, 16, 24, 32, 48, 64]
BWD_T = [1, 255, 257, 1000]
VARIANTS = ["all", "score", "top", "balance"]


def bwd_inputs(T, E, k, seed, std):
    """stored-forward stand-ins: noisy / clean logits, the selection on noisy (ties -> lowest index), fp32 top_logits"""
    g = torch.Generator().manual_seed(seed)
    clean = torch.randn(T, E, generator=g) * 2
    noise = torch.randn(T, E, generator=g)
    noisy = clean + noise * torch.tensor(std, dtype=F32)
    order = torch.sort(noisy, dim=1, descending=True, stable=True).indices
    kp = min(k + 1, E)
    p = torch.softmax(noisy, 1)
    return noisy.cuda(), clean.cuda(), order[:, :k].contiguous().cuda(), order[:, k].int().cuda() if kp > k else None, \
        p.gather(1, order[:, :kp]).contiguous().cuda()


def bwd_call(ops, noisy, idx, k, *, clean=None, top=None, idx_next=None, d_score=None, d_top=None, d_imp=None, d_lp=None,
             bs=1.0, bs_dev=None, std=0.0, act=None):
    T, E = noisy.shape
    dl, check = kc.guarded(T, E, F32)
    da, acheck = kc.guarded(T, E, act) if act is not None else (None, None)
    a = ops._lib.GateBwdArgs(_p(noisy), _p(clean), _p(top), _p(idx), _p(idx_next), _p(d_score), _p(d_top), _p(d_imp),
                             _p(d_lp), float(bs), float(std), T, E, k, _p(dl), _p(bs_dev), _p(da),
                             DT_CODE[act] if act is not None else 0)
    snap = kc.snapshot(noisy=noisy, clean=clean, top=top, idx=idx, idx_next=idx_next, d_score=d_score, d_top=d_top,
                       d_imp=d_imp, d_lp=d_lp, bs_dev=bs_dev)
    ops._lib.check(ops.lib().m3_gate_bwd_logits(byref(a), _stream()), "m3_gate_bwd_logits")
    torch.cuda.synchronize()
    kc.unchanged(snap)
    check(what="d_logits")
    if acheck:
        acheck(what="d_logits_act")
    return dl, da


@pytest.mark.parametrize("E", BWD_E)
def test_gate_bwd_logits_every_epad(ops, E):
    ks = sorted({k for k in (1, E - 1, E) if k >= 1})
    n = 0
    for k in ks:
        for T in BWD_T:
            var = VARIANTS[n % len(VARIANTS)]
            act = (F16, BF16, F32, None)[n % 4]
            n += 1
            std = 0.3
            noisy, clean, idx, nxt, top = bwd_inputs(T, E, k, seed=E * 1000 + k * 10 + T, std=std)
            g = torch.Generator().manual_seed(T + E + k)
            kp = top.shape[1]
            d_score = (torch.randn(T, k, generator=g).cuda() if var in ("all", "score") else None)
            d_top = (torch.randn(T, kp, generator=g).cuda() if var in ("all", "top") and (kp == k or nxt is not None) else None)
            d_imp = (torch.randn(E, generator=g).cuda() * 0.1 if var in ("all", "balance") else None)
            d_lp = (torch.randn(E, generator=g).cuda() if var in ("all", "balance") and k < E else None)
            kw = dict(clean=clean if d_lp is not None else None, top=top if d_lp is not None else None,
                      idx_next=nxt if (d_top is not None or d_lp is not None) else None,
                      d_score=d_score, d_top=d_top, d_imp=d_imp, d_lp=d_lp, std=std if d_lp is not None else 0.0)
            bs = 0.75
            dl, da = bwd_call(ops, noisy, idx, k, bs=bs, act=act, **kw)
            ref, bound = kc.gate_bwd_reference(noisy, idx, k, clean=kw["clean"], top_logits=kw["top"],
                                               idx_next=kw["idx_next"], d_score=d_score, d_top=d_top, d_importance=d_imp,
                                               d_load_prob=d_lp, balance_scale=bs, noise_std=kw["std"])
            tag = f"bwd/E{E}/k{k}/T{T}/{var}"
            WORST[tag] = kc.assert_within(dl, ref, bound, tag)
            assert WORST[tag] < 1
            if da is not None:
                assert kc.same_bits(da, dl.to(act)), "d_logits_act is not d_logits rounded to nearest even"
            if var == "balance":
                # a device-resident factor s: the same bits as balance_scale = fl32(bs * s) and no factor
                s = torch.tensor([1.6180339], dtype=F32, device="cuda")
                dl2, _ = bwd_call(ops, noisy, idx, k, bs=bs, bs_dev=s, **kw)
                dl3, _ = bwd_call(ops, noisy, idx, k, bs=float(torch.tensor(bs, dtype=F32) * s.cpu()[0]), **kw)
                assert kc.same_bits(dl2, dl3), "balance_scale_dev is not one fp32 product onto balance_scale"


# --------------------------------------------------------------------------------------------- m3_gate_bwd_params
def params_call(ops, x, D, E, T, w, dl, *, ldx, beta_dw=0, want_dx=True, lddx=None, beta_dx=0, prior=None, fill=None):
    nb = ops.lib().m3_gate_dw_blocks(T)
    part, pcheck = kc.guarded_ws(nb * D * E)
    if fill is not None:
        part.normal_(generator=None).mul_(fill)
    dW, wcheck = kc.guarded(D, E, F32)
    if beta_dw:
        dW.copy_(prior[0])
    lddx = D if lddx is None else lddx
    dx, xcheck = kc.guarded(T, D, F32, ld=lddx) if want_dx else (None, None)
    if want_dx and beta_dx:
        dx.copy_(prior[1])
    snap = kc.snapshot(x=x, w=w, dl=dl)
    ops._lib.check(ops.lib().m3_gate_bwd_params(_p(x), DT_CODE[x.dtype], T, D, ldx, _p(w), E, _p(dl), _p(part), _p(dW),
                                                beta_dw, _p(dx), lddx, beta_dx, _stream()), "m3_gate_bwd_params")
    torch.cuda.synchronize()
    kc.unchanged(snap)
    pcheck(); wcheck(what="d_w_gate")
    if want_dx:
        xcheck(what="dx")
    return dW.clone(), (dx.clone() if want_dx else None)


PARAM_CASES = [
    # dtype, D, E, ldx pad (elements), form
    (F16, 256, 16, 0, "dw4 rpn4"), (BF16, 768, 8, 0, "dw4 rpn2"), (F32, 512, 4, 2, "dw4 ldx 8B-aligned"),
    (F16, 1024, 2, 8, "dw4 rpn2 padded"),
    (F16, 256, 24, 0, "fallback E>16"), (F32, 100, 48, 0, "fallback ep64"), (BF16, 102, 16, 0, "fallback D%4"),
    (F16, 256, 16, 1, "fallback ldx breaks 8B"), (F32, 64, 64, 0, "fallback ep64 E64"), (F32, 130, 32, 0, "fallback ep32"),
    (BF16, 96, 12, 0, "dw4 ep16 padded E"), (F16, 48, 5, 0, "dw4 ep8 padded E"),
    # the remaining (dtype, padded E) pairs of both dW kernels: D = 132 takes the four-wide kernel, D = 130 (no multiple of 4)
    # the fallback
    (F32, 132, 16, 0, "dw4 f32 ep16"),
    (F16, 130, 8, 0, "fallback f16 ep8"), (F16, 130, 64, 0, "fallback f16 ep64"), (BF16, 130, 8, 0, "fallback bf16 ep8"),
    (BF16, 130, 32, 0, "fallback bf16 ep32"), (BF16, 130, 64, 0, "fallback bf16 ep64"), (F32, 130, 8, 0, "fallback f32 ep8"),
    (F32, 130, 16, 0, "fallback f32 ep16"),
]


@pytest.mark.parametrize("case", range(len(PARAM_CASES)), ids=[c[4] for c in PARAM_CASES])
def test_gate_bwd_params(ops, case):
    dtype, D, E, pad, form = PARAM_CASES[case]
    for T in (1, 63, 200, 1000):
        ldx = D + pad
        xb = rnd(T, ldx, seed=T + D).to(dtype).cuda()
        x = xb[:, :D]
        w = rnd(D, E, scale=0.1, seed=E).cuda()
        dl = rnd(T, E, scale=0.01, seed=T * 3).cuda()
        x64, dl64, w64 = x.double(), dl.double(), w.double()
        W64 = x64.t() @ dl64
        nb = ops.lib().m3_gate_dw_blocks(T)
        bW = kc.gemm_bound(None, None, W64, F32, K=T + nb + 2, absacc=x64.abs().t() @ dl64.abs())
        X64 = dl64 @ w64.t()
        bX = kc.gemm_bound(dl64, w64, X64, F32)
        lddx = D + 4
        # beta 0: the old dx (sentinel NaN) is not read
        dW, dx = params_call(ops, xb, D, E, T, w, dl, ldx=ldx, lddx=lddx)
        wst = kc.assert_within(dW, W64, bW, "dW")
        wst = max(wst, kc.assert_within(dx, X64, bX, "dx"))
        # bitwise repeat under a different workspace fill
        dW2, dx2 = params_call(ops, xb, D, E, T, w, dl, ldx=ldx, lddx=lddx, fill=1e3)
        assert kc.same_bits(dW, dW2) and kc.same_bits(dx, dx2), "dW / dx depend on the workspace's prior contents"
        # beta 1 onto priors
        prior = (rnd(D, E, seed=5).cuda(), rnd(T, D, seed=6).cuda())
        dW, dx = params_call(ops, xb, D, E, T, w, dl, ldx=ldx, lddx=lddx, beta_dw=1, beta_dx=1, prior=prior)
        R = W64 + prior[0].double()
        RX = X64 + prior[1].double()
        wst = max(wst, kc.assert_within(dW, R, bW + kc.SAFETY * kc.U32 * R.abs(), "dW beta 1"))
        wst = max(wst, kc.assert_within(dx, RX, bX + kc.SAFETY * kc.U32 * RX.abs(), "dx beta 1"))
        WORST[f"params/{form}/T{T}"] = wst
        assert wst < 1


@pytest.mark.parametrize("E", [2, 8, 12, 16, 24, 32, 48, 64])
def test_gate_bwd_params_dx_every_epad(ops, E):
    T, D = 130, 256
    x = rnd(T, D, seed=E).cuda()
    w = rnd(D, E, scale=0.1, seed=E + 1).cuda()
    dl = rnd(T, E, scale=0.01, seed=E + 2).cuda()
    nb = ops.lib().m3_gate_dw_blocks(T)
    dx, xcheck = kc.guarded(T, D, F32, ld=D + 12)
    snap = kc.snapshot(x=x, w=w, dl=dl)
    ops._lib.check(ops.lib().m3_gate_bwd_params(_p(x), 0, T, D, D, _p(w), E, _p(dl), None, None, 0, _p(dx), D + 12, 0,
                                                _stream()), "m3_gate_bwd_params")
    torch.cuda.synchronize()
    kc.unchanged(snap); xcheck(what="dx")
    X64 = dl.double() @ w.double().t()
    WORST[f"dx/E{E}"] = kc.assert_within(dx, X64, kc.gemm_bound(dl.double(), w.double(), X64, F32), "dx")
    assert WORST[f"dx/E{E}"] < 1


@pytest.mark.parametrize("D,E,want_dx", [(1025, 8, False), (1024, 17, True), (512, 33, True)])
def test_gate_bwd_params_rejects_before_any_launch(ops, D, E, want_dx):
    """D > 1024, and D * E * 4 > 64 KiB for the dx kernel: M3Error, and d_w_gate / dx keep their sentinel"""
    T = 70
    x = rnd(T, D, seed=1).cuda()
    w = rnd(D, E, seed=2).cuda()
    dl = rnd(T, E, seed=3).cuda()
    nb = ops.lib().m3_gate_dw_blocks(T)
    part, pcheck = kc.guarded_ws(nb * D * E)
    dW, wcheck = kc.guarded(D, E, F32)
    dx, xcheck = kc.guarded(T, D, F32) if want_dx else (None, None)
    with pytest.raises(ops._lib.M3Error):
        ops._lib.check(ops.lib().m3_gate_bwd_params(_p(x), 0, T, D, D, _p(w), E, _p(dl), _p(part), _p(dW), 0, _p(dx), D, 0,
                                                    _stream()), "m3_gate_bwd_params")
    torch.cuda.synchronize()
    wcheck(keep_rows=list(range(D)), what="d_w_gate")
    if want_dx:
        xcheck(keep_rows=list(range(T)), what="dx")
    assert kc.same_bits(part, kc.sentinel_like(part)), "part_dw was written by a rejected call"
