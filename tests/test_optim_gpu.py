"""GPU: the fused optimizer step (csrc/optim.hip through ops.OptimPlan and m3vit_amd.optim) against torch.optim in float64.

Inputs, references and bounds are tests/optim_cases.py's (tests/test_optim_cpu.py shows that torch's own fp32 optimizers keep
the same bounds on the same inputs).  Every case uses the smallest shapes at which its mechanism can go wrong; all tensors
of a case together stay under 1 M elements - but optim_cases.MANY_CHUNKS_INPUTS, whose one 1.2 M-element tensor gives the
norm's finalize launch more partials than it has threads."""
import pytest
import torch

import kernel_contract as kc
import optim_cases as oc

pytestmark = pytest.mark.gpu
F32 = torch.float32
WORST = {}
# Where a clipped |g| is near eps the update lr g / (|g| + eps) is proportional to the clip coefficient, so it inherits the
# relative error of the norm on top of the optimizer's bound.  The kernels' norm: 16 fused multiply-adds per thread, 6 shuffle
# levels and 3 adds per 4096-element chunk in fp32 (25 roundings deep), the chunks in double; the square root halves it; then
# the products with inv_scale, the quotient and sum of the clip coefficient and their product (4 roundings): (25 / 2 + 4) u.
NORM_REL = (25 / 2 + 4) * oc.U32
FUSED = {"adamw": "FusedAdamW", "adamw_nodecay": "FusedAdamW", "adam": "FusedAdam", "sgd": "FusedSGD", "sgd_nesterov": "FusedSGD"}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    yield _ops
    if WORST:
        print("\nfused optimizer worst err / bound:", {k: round(v, 3) for k, v in WORST.items()})


def _fused_cls(kind):
    from m3vit_amd import optim
    return getattr(optim, FUSED[kind])


def _hyper_row(ops, cls, kw):
    if cls is torch.optim.SGD:
        return ops.optim_hyper_row(kw["lr"], kw["momentum"], weight_decay=kw["weight_decay"], nesterov=kw["nesterov"])
    return ops.optim_hyper_row(kw["lr"], 0.9, 0.999, 1e-8, kw["weight_decay"], decoupled=cls is torch.optim.AdamW)


def _plan_run(ops, name, layout):
    """the steps of case `name` through ops.OptimPlan on guarded buffers.  layout "flat": the gradients are views of ONE flat
    buffer packed without padding (element offsets 1, 2, 3 mod 4 -> the scalar path; the aligned ones the 16-byte path);
    "aligned": every gradient in an allocation of its own (all 16-byte paths).  m and v lie in flat buffers with every offset
    rounded up to 4 elements, as m3vit_amd.optim lays them out.  Returns the records of every step."""
    cls, group_kw, group_of, clip, lr_change, _ = oc.case(name)
    params, grads = oc.inputs_of(name)
    sgd = cls is torch.optim.SGD
    kind = "sgd" if sgd else ("adamw" if cls is torch.optim.AdamW else "adam")
    checks, ps = [], []
    for p in params:
        t, c = kc.guarded_ws(p.numel())
        t.copy_(p.cuda())
        ps.append(t); checks.append(c)
    offs, o = [], 0
    for p in params:
        offs.append(o)
        o += (p.numel() + 3) & ~3
    mflat, c = kc.guarded_ws(o); checks.append(c)
    mflat.zero_()
    vflat = None
    if not sgd:
        vflat, c = kc.guarded_ws(o); checks.append(c)
        vflat.zero_()
    ms = [mflat[a:a + p.numel()] for a, p in zip(offs, params)]
    vs = [vflat[a:a + p.numel()] if vflat is not None else None for a, p in zip(offs, params)]
    if layout == "flat":
        gflat, c = kc.guarded_ws(sum(p.numel() for p in params)); checks.append(c)
        gs, a = [], 0
        for p in params:
            gs.append(gflat[a:a + p.numel()])
            a += p.numel()
        assert {g.data_ptr() % 16 for g in gs} == {0, 4, 8, 12}
    else:
        gs = []
        for p in params:
            t, c = kc.guarded_ws(p.numel())
            gs.append(t); checks.append(c)
    plan = ops.OptimPlan([(p, g, m, v, gi) for p, g, m, v, gi in zip(ps, gs, ms, vs, group_of)], len(group_kw), kind)
    rows = [_hyper_row(ops, cls, kw) for kw in group_kw]
    out = []
    for s, step_grads in enumerate(grads):
        if lr_change is not None and lr_change[0] == s:
            kw = dict(group_kw[lr_change[1]], lr=lr_change[2])
            rows[lr_change[1]] = _hyper_row(ops, cls, kw)
        for g, src in zip(gs, step_grads):
            g.copy_(src)
        snap = kc.snapshot(**{f"g{i}": g for i, g in enumerate(gs)})
        plan.set_hyper(rows)
        plan.prepare(max_norm=clip or 0.0)
        plan.step()
        torch.cuda.synchronize()
        kc.unchanged(snap)                                         # the gradient buffer keeps its bits
        rec = {"p": [p.clone() for p in ps], "norm": plan.total_norm.clone()}
        keys = oc.STATE_KEYS[cls]
        rec[keys[0]] = [m.clone() for m in ms]
        if not sgd:
            rec[keys[1]] = [v.clone() for v in vs]
        out.append(rec)
    for c in checks:
        c(what=f"{name}/{layout}")                                 # nothing outside p, m, v was written (and g not at all)
    assert int(plan.step_count) == len(grads) and int(plan.skipped) == 0
    return out


# ------------------------------------------------------------------------------------------- 1. shapes and alignment
@pytest.mark.parametrize("layout", ["flat", "aligned"])
@pytest.mark.parametrize("name", ["adamw", "adam", "sgd", "sgd_nesterov"])
def test_shapes_and_alignment(ops, name, layout):
    cls, group_kw, group_of, _, _, lrs = oc.case(name)
    _, grads = oc.inputs_of(name)
    a = _plan_run(ops, name, layout)
    oc.check_run(a, oc.reference(name), grads, group_kw, group_of, cls, f"{name}/{layout}", lrs=lrs, worst=WORST)
    b = _plan_run(ops, name, layout)                               # a second run: the same bits
    for ra, rb in zip(a, b):
        for key in ("p",) + oc.STATE_KEYS[cls]:
            assert all(kc.same_bits(x, y) for x, y in zip(ra[key], rb[key])), f"{key} differs between two runs"


# -------------------------------------------------------------------------------------------------------- 2. groups
def test_groups_interleaved_in_descriptor_order(ops):
    cls, group_kw, group_of, _, _, lrs = oc.case("groups")
    assert group_of[:4] == [0, 1, 0, 1]
    a = _plan_run(ops, "groups", "flat")
    oc.check_run(a, oc.reference("groups"), oc.inputs_of("groups")[1], group_kw, group_of, cls, "groups/plan", lrs=lrs, worst=WORST)


def _optimizer_run(fused_cls, group_kw, group_of, params, grads, lr_change=None, before_step=None, **kw):
    """the same through the torch.optim.Optimizer front: parameters as nn.Parameters, gradients as .grad"""
    ps = [torch.nn.Parameter(p.cuda()) for p in params]
    groups = [dict(params=[p for p, g in zip(ps, group_of) if g == gi], **gkw) for gi, gkw in enumerate(group_kw)]
    opt = fused_cls(groups, **kw)
    out = []
    for s, step_grads in enumerate(grads):
        if lr_change is not None and lr_change[0] == s:
            opt.param_groups[lr_change[1]]["lr"] = lr_change[2]
        for p, g in zip(ps, step_grads):
            p.grad = g.cuda()
        if before_step is not None:
            before_step(opt, ps, s)
        opt.step()
        rec = {"p": [p.detach().clone() for p in ps]}
        for key in opt._state_keys:
            rec[key] = [opt.state[p][key].clone() for p in ps]
        out.append(rec)
    return out, opt, ps


def test_groups_and_lr_change_through_param_groups(ops):
    cls, group_kw, group_of, _, lr_change, lrs = oc.case("groups")
    params, grads = oc.inputs_of("groups")
    a, opt, _ = _optimizer_run(_fused_cls("adamw"), group_kw, group_of, params, grads, lr_change=lr_change)
    oc.check_run(a, oc.reference("groups"), grads, group_kw, group_of, cls, "groups/optimizer", lrs=lrs, worst=WORST)
    assert opt.param_groups[0]["lr"] == lr_change[2]
    # the change mattered: without it step 3 is outside the bound for group 0
    b, _, _ = _optimizer_run(_fused_cls("adamw"), group_kw, group_of, params, grads)
    with pytest.raises(AssertionError):
        oc.check_run(b, oc.reference("groups"), grads, group_kw, group_of, cls, "groups/unchanged lr", lrs=lrs)


# ------------------------------------------------------------------------------------------------ 3. clip and scale
def _bits_equal(a, b, keys):
    return all(kc.same_bits(x, y) for ra, rb in zip(a, b) for key in keys for x, y in zip(ra[key], rb[key]))


def test_max_grad_norm_above_the_norm_changes_no_bit(ops):
    cls, group_kw, group_of, *_ = oc.case("adamw")
    params, grads = oc.inputs_of("adamw")
    a, _, _ = _optimizer_run(_fused_cls("adamw"), group_kw, group_of, params, grads)
    b, opt, _ = _optimizer_run(_fused_cls("adamw"), group_kw, group_of, params, grads, max_grad_norm=1e6)
    assert _bits_equal(a, b, ("p", "exp_avg", "exp_avg_sq"))
    assert float(opt.last_grad_norm) < 1e6


def _norm_within(opt, last_grads, what, n64=None):
    """last_grad_norm after the last step, against the float64 norm n64 (default: of last_grads): sqrt of an fp32 sum of
    squares (chunks of 4096 terms, then double): d sqrt(S) = dS / (2 sqrt S)"""
    S = sum(float((g.double() ** 2).sum()) for g in last_grads)
    n64 = S ** 0.5 if n64 is None else n64
    assert abs(n64 - S ** 0.5) < 1e-9 * n64
    bound = float(kc.sum_bound(torch.tensor(S), 4096, torch.tensor(S), F32)) / (2 * n64) + 2 * oc.U32 * n64
    err = abs(float(opt.last_grad_norm) - n64)
    print(f"{what}: last_grad_norm {float(opt.last_grad_norm)!r} float64 {n64!r} err / bound {err / bound:.3g}")
    assert err <= bound


def test_clip_matches_clip_grad_norm_then_step(ops):
    cls, group_kw, group_of, clip, _, lrs = oc.case("clip")
    params, grads = oc.inputs_of("clip")
    ref = oc.reference("clip")
    a, opt, _ = _optimizer_run(_fused_cls("adamw"), group_kw, group_of, params, grads, max_grad_norm=clip)
    _norm_within(opt, grads[-1], "clip", float(ref[-1]["norm"]))
    oc.check_run(a, ref, grads, group_kw, group_of, cls, "clip", lrs=lrs, worst=WORST)
    # the norm alone over 303 chunks: more partials than the finalize launch has threads (optim_cases.MANY_CHUNKS_INPUTS)
    params, grads = oc.inputs(**oc.MANY_CHUNKS_INPUTS)
    _, opt, _ = _optimizer_run(_fused_cls("adamw"), group_kw, [0] * len(params), params, grads, max_grad_norm=clip)
    _norm_within(opt, grads[-1], "many chunks")


def test_grad_scale_power_of_two_changes_no_bit(ops):
    cls, group_kw, group_of, *_ = oc.case("adamw")
    params, grads = oc.inputs_of("adamw")
    a, _, _ = _optimizer_run(_fused_cls("adamw"), group_kw, group_of, params, grads, max_grad_norm=100.0)
    scale = torch.full((), 65536.0, device="cuda")
    none = torch.zeros((), device="cuda")

    def install(opt, ps, s):                                       # what torch.amp.GradScaler.step installs
        opt.grad_scale, opt.found_inf = scale, none
    b, opt, _ = _optimizer_run(_fused_cls("adamw"), group_kw, group_of, params, [[g * 65536.0 for g in gs] for gs in grads],
                               before_step=install, max_grad_norm=100.0)
    assert _bits_equal(a, b, ("p", "exp_avg", "exp_avg_sq"))


# ---------------------------------------------------------------------------------------------------------- 4. skip
@pytest.mark.parametrize("how", ["scaler", "own_check"])
@pytest.mark.parametrize("bad", ["inf_last", "nan_first"])
def test_skipped_step_keeps_every_bit_and_the_step_count(ops, how, bad):
    cls, group_kw, group_of, *_ = oc.case("adamw")
    params, grads = oc.inputs_of("adamw")
    ref = oc.reference("adamw")
    ps = [torch.nn.Parameter(p.cuda()) for p in params]
    mult = 4.0 if how == "scaler" else 1.0
    opt = _fused_cls("adamw")(ps, max_grad_norm=1e6 if how == "own_check" else None, **group_kw[0])
    scaler = torch.amp.GradScaler("cuda", init_scale=mult, growth_interval=1000) if how == "scaler" else None
    if scaler is not None:
        scaler.scale(torch.zeros((), device="cuda"))               # (creates the scale tensor, as the first backward would)

    def step(gs):
        for p, g in zip(ps, gs):
            p.grad = (g * mult).cuda()
        if scaler is not None:
            scaler.step(opt)
            scaler.update()
        else:
            opt.step()

    step(grads[0])
    poisoned = [g.clone() for g in grads[1]]
    if bad == "inf_last":
        poisoned[-1][-1] = float("inf")
    else:
        poisoned[0][0] = float("nan")
    state = {f"{k}{i}": opt.state[p][k] for i, p in enumerate(ps) for k in ("exp_avg", "exp_avg_sq")}
    snap = kc.snapshot(counter=opt._block[1:2], **{f"p{i}": p.data for i, p in enumerate(ps)}, **state)
    versions = [p._version for p in ps]
    step(poisoned)
    torch.cuda.synchronize()
    kc.unchanged(snap)                                             # p, m, v and the step counter keep their bits
    assert int(opt._plan.skipped) == 1 and int(opt._plan.step_count) == 1
    assert all(p._version > v for p, v in zip(ps, versions))       # the host cannot know: the versions move all the same
    if scaler is not None:
        assert scaler.get_scale() == mult / 2
        mult = mult / 2
    step(grads[1])                                                 # the next clean step is step 2, not 3
    assert int(opt._plan.skipped) == 0 and int(opt._plan.step_count) == 2
    got = [None, {"p": [p.detach() for p in ps], "exp_avg": [opt.state[p]["exp_avg"] for p in ps],
                  "exp_avg_sq": [opt.state[p]["exp_avg_sq"] for p in ps]}]
    for i in range(len(ps)):
        kc.assert_within(got[1]["p"][i], ref[1]["p"][i], oc.param_bound(ref[1]["p"][i], group_kw[0]["lr"], 2), f"p[{i}] after the skip")
        for key in ("exp_avg", "exp_avg_sq"):
            kc.assert_within(got[1][key][i], ref[1][key][i], oc.state_bound(ref[1][key][i], oc.gmax_of(grads, i, 1), 2),
                             f"{key}[{i}] after the skip")
    assert float(opt.state_dict()["state"][0]["step"]) == 2.0


# ------------------------------------------------------------------------------------------ 5. no host synchronisation
def test_step_does_not_synchronise_with_the_host(ops):
    cls, group_kw, group_of, *_ = oc.case("groups")
    params, grads = oc.inputs_of("groups")
    ps = [torch.nn.Parameter(p.cuda()) for p in params]
    groups = [dict(params=[p for p, g in zip(ps, group_of) if g == gi], **gkw) for gi, gkw in enumerate(group_kw)]
    opt = _fused_cls("adamw")(groups, max_grad_norm=1.0)
    dev_grads = [[g.cuda() for g in gs] for gs in grads]
    scale, none = torch.full((), 2.0, device="cuda"), torch.zeros((), device="cuda")
    for p, g in zip(ps, dev_grads[0]):
        p.grad = g
    opt.step()                                                     # builds the tables (that may synchronise)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for p, g in zip(ps, dev_grads[1]):
            p.grad.copy_(g)                                        # the same gradient tensors, as a training loop has them
        opt.step()
        opt.param_groups[0]["lr"] = 5e-4                           # an lr scheduler's write: one pinned, non-blocking copy
        opt.grad_scale, opt.found_inf = scale, none
        opt.step()
        norm = opt.last_grad_norm                                  # a view: no read
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert float(norm) > 0 and int(opt._plan.step_count) == 3


# ------------------------------------------------------------------------------------------ 6. checkpoint compatibility
@pytest.mark.parametrize("direction", ["torch_to_fused", "fused_to_torch"])
def test_state_dict_round_trip_with_torch_adamw(ops, direction):
    cls, group_kw, group_of, _, _, lrs = oc.case("adamw")
    params, grads = oc.inputs_of("adamw")
    ref = oc.reference("adamw")
    ps = [torch.nn.Parameter(p.cuda()) for p in params]
    first, second = ((torch.optim.AdamW, dict(foreach=False)), (_fused_cls("adamw"), {}))
    if direction == "fused_to_torch":
        first, second = second, first
    a = first[0](ps, **group_kw[0], **first[1])
    for s in range(2):
        for p, g in zip(ps, grads[s]):
            p.grad = g.cuda()
        a.step()
    b = second[0](ps, **group_kw[0], **second[1])
    b.load_state_dict(a.state_dict())
    for p, g in zip(ps, grads[2]):
        p.grad = g.cuda()
    b.step()
    sd = b.state_dict()
    assert all(float(st["step"]) == 3.0 for st in sd["state"].values())
    for i, p in enumerate(ps):
        WORST[f"{direction}/p"] = max(WORST.get(f"{direction}/p", 0.0), kc.assert_within(
            p, ref[2]["p"][i], oc.param_bound(ref[2]["p"][i], group_kw[0]["lr"], 3), f"{direction}: p[{i}]"))
        for key in ("exp_avg", "exp_avg_sq"):
            kc.assert_within(b.state[p][key], ref[2][key][i], oc.state_bound(ref[2][key][i], oc.gmax_of(grads, i, 2), 3),
                             f"{direction}: {key}[{i}]")


# ------------------------------------------------------------------------------------------------- 7. executor wiring
def _tiny_cfg():
    from oracle import ref_torch as R
    return R.BackboneCfg(img_size=(32, 48), embed_dim=64, depth=2, num_heads=2, mlp_ratio=4.0, moe_mlp_ratio=1.0,
                         moe_experts=4, moe_top_k=2, gate_dim=66, multi_gate=True)


def test_for_engine_refreshes_the_operand_copies(ops):
    from m3vit_amd.engine import BackboneEngine
    from m3vit_amd.optim import FusedAdamW
    from oracle import ref_torch as R
    cfg = _tiny_cfg()
    P = R.init_backbone_params(cfg, seed=5)
    g = torch.Generator().manual_seed(1)
    img = torch.randn(3, 3, 32, 48, generator=g).cuda()
    dtok = (torch.randn(3, cfg.num_tokens, 64, generator=g) * 0.1).cuda()
    eng = BackboneEngine(cfg, P, batch=3, dtype=torch.float16)
    assert sum(eng.is_moe) == 1
    opt = FusedAdamW.for_engine(eng, lr=1e-3, weight_decay=0.05, max_grad_norm=1.0)
    decay, plain = opt.param_groups
    assert decay["weight_decay"] == 0.05 and plain["weight_decay"] == 0.0
    named = {id(p): n for n, p in eng.params.items()}
    assert all(any(k in named[id(p)] for k in ("bias", "norm", "pos_embed", "cls_token", "w_gate")) for p in plain["params"])
    assert any(named[id(p)].endswith("attn.qkv.weight") for p in decay["params"])
    assert len(decay["params"]) + len(plain["params"]) == len(eng.params)
    opt.zero_grad()
    tok0, _ = eng.forward(img, 1)
    tok0 = tok0.clone()
    eng.backward(dtok, cv_weight=0.01)
    before = {n: p.clone() for n, p in eng.params.items()}
    g64 = {n: v.double().cpu() for n, v in eng.grads.items()}
    opt.step()
    torch.cuda.synchronize()
    # the update itself: AdamW step 1 in float64 from the executor's own gradients, clipped to norm 1
    norm = sum(float((v ** 2).sum()) for v in g64.values()) ** 0.5
    coef = min(1.0, 1.0 / (norm + 1e-6))
    for n, p in eng.params.items():
        wd = 0.0 if any(k in n for k in ("bias", "norm", "pos_embed", "cls_token", "w_gate")) else 0.05
        gc = g64[n] * coef
        m, v = 0.1 * gc, 0.001 * gc * gc
        want = before[n].double().cpu() * (1 - 1e-3 * wd) - (1e-3 / (1 - 0.9)) * m / ((v / (1 - 0.999)).sqrt() + 1e-8)
        extra = 1e-3 * NORM_REL                            # lr x the norm's relative error (NORM_REL above)
        kc.assert_within(p, want, oc.param_bound(want, 1e-3, 1) + extra, f"engine {n}")
    assert any(not kc.same_bits(before[n], p) for n, p in eng.params.items())
    for n in eng._linear_names():                                  # the operand copies are casts of the NEW masters
        w = eng.params[n + ".weight"]
        w2 = w.reshape(w.shape[0], -1) if n == "patch_embed.proj" else w
        assert kc.same_bits(eng.wc[n], w2.to(torch.float16)), n
        if n in eng.wt:
            assert kc.same_bits(eng.wt[n], w2.transpose(-1, -2).contiguous().to(torch.float16)), n
    for n, c in eng.wgate_c.items():
        assert kc.same_bits(c, eng.params[n].to(torch.float16)), n
    tok1, _ = eng.forward(img, 1)
    assert not kc.same_bits(tok1, tok0)
    eng2 = BackboneEngine(cfg, eng.state_dict(), batch=3, dtype=torch.float16)
    tok2, _ = eng2.forward(img, 1)
    assert kc.same_bits(tok1, tok2)


# ----------------------------------------------------------------------------------------------------- 8. module path
KW = dict(img_size=(32, 48), embed_dim=64, depth=2, num_heads=2, moe_top_k=2, gate_dim=66, multi_gate=True, moe_experts=4)


def _module(state=None, seed=9):
    from m3vit_amd.vit import VisionTransformerMoE
    from oracle import ref_torch as R
    cfg = R.BackboneCfg(mlp_ratio=4.0, moe_mlp_ratio=1.0, vmoe_noisy_std=0.0, **KW)
    m = VisionTransformerMoE(mlp_ratio=4.0, moe_mlp_ratio=1, vmoe_noisy_std=0.0, fused="auto", act_dtype=torch.float16, **KW).cuda()
    m.load_state_dict(state if state is not None else R.init_backbone_params(cfg, seed=seed))
    m.train()
    return m, cfg


def _joint_loss(m, img, dtok):
    return sum((tok * dtok).sum() + 0.01 * cv for tok, cv in (m(img, task_id=t) for t in (0, 1)))


def test_module_path_three_joint_steps(ops):
    from m3vit_amd.optim import FusedAdamW
    hyper = dict(lr=1e-3, weight_decay=0.05)
    a, cfg = _module()
    b, _ = _module()                                               # the same weights, trained with torch's AdamW
    oa = FusedAdamW(a.parameters(), **hyper)
    ob = torch.optim.AdamW(b.parameters(), foreach=False, **hyper)
    gen = torch.Generator().manual_seed(5)
    names = [n for n, _ in a.named_parameters()]
    p0 = [p.detach().cpu().clone() for p in a.parameters()]
    own = []
    for s in range(3):
        img = torch.randn(3, 3, 32, 48, generator=gen).cuda()
        dtok = (torch.randn(3, cfg.num_tokens, 64, generator=gen) * 0.1).cuda()
        with torch.no_grad():
            before, _ = a(img, task_id=0)
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad(set_to_none=True)
            _joint_loss(m, img, dtok).backward()
            assert m.fused_fallback_reason is None, m.fused_fallback_reason
        if s == 0:      # identical parameters, the same executor: the two runs' gradients differ by nothing
            assert all((x.grad is None and y.grad is None) or kc.same_bits(x.grad, y.grad) for x, y in zip(a.parameters(), b.parameters()))
        own.append([None if p.grad is None else p.grad.detach().cpu().clone() for p in a.parameters()])
        oa.step(); ob.step()
        with torch.no_grad():
            after, _ = a(img, task_id=0)
            fresh, _ = _module(state=a.state_dict())[0](img, task_id=0)
        assert not kc.same_bits(after, before)                     # the executor saw the step (p._version moved) ...
        assert kc.same_bits(after, fresh)                          # ... and runs on the new masters' operand copies
        if s == 0:      # from the same gradients: the fused step inside the bound of the float64 update, and torch's fp32
            ref, _ = oc.run_torch(torch.optim.AdamW, [hyper], p0, own, torch.float64)       # step no further from it than twice that
            for n, x, y, r in zip(names, a.parameters(), b.parameters(), ref[0]["p"]):
                kc.assert_within(x, r, oc.param_bound(r, hyper["lr"], 1), f"fused {n}")
                kc.assert_within(y, x.detach().double(), 2 * oc.param_bound(r, hyper["lr"], 1), f"torch against fused {n}")
    # from step 2 on the runs' fp16 gradients differ; the fused run against float64 updates of ITS OWN gradients
    ref, _ = oc.run_torch(torch.optim.AdamW, [hyper], p0, own, torch.float64)
    for n, x, r in zip(names, a.parameters(), ref[2]["p"]):
        WORST["module"] = max(WORST.get("module", 0.0), kc.assert_within(x, r, oc.param_bound(r, hyper["lr"], 3), f"module {n} after 3 steps"))


# --------------------------------------------------------------------------------------------------------- 9. AMP step
def _cls_model(state=None):
    from m3vit_amd.cls import MoEViTConfig, MoEViTForImageNet
    cfg = MoEViTConfig(img_size=32, embed_dim=64, depth=2, num_heads=2, num_classes=16, moe_experts=4, moe_top_k=2, gate_dim=64,
                       vmoe_noisy_std=0.0)
    torch.manual_seed(7)
    m = MoEViTForImageNet(cfg, act_dtype=torch.float16).cuda().train()
    if state is not None:
        m.load_state_dict(state)
    return m


def test_amp_train_step_with_the_fused_optimizer(ops):
    import torch.nn.functional as F
    from m3vit_amd.cls import amp_train_step
    from m3vit_amd.optim import FusedAdamW
    hyper = dict(lr=2e-3, weight_decay=0.05)
    a = _cls_model()
    b = _cls_model(state=a.state_dict())
    oa = FusedAdamW(a.parameters(), max_grad_norm=1.0, **hyper)
    ob = torch.optim.AdamW(b.parameters(), foreach=False, **hyper)
    sa, sb = (torch.amp.GradScaler("cuda", init_scale=1024.0) for _ in range(2))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(16, 3, 32, 32, generator=g).cuda()
    y = torch.randint(0, 16, (16,), generator=g).cuda()
    crit = lambda samples, logits, targets: F.cross_entropy(logits, targets)          # noqa: E731
    names = [n for n, _ in a.named_parameters()]
    p0 = [p.detach().cpu().clone() for p in a.parameters()]
    own = []
    extra = hyper["lr"] * NORM_REL                         # lr x the relative error of the kernels' norm
    # torch's own clip_grad_norm_ sums in an order that is not ours to know: worst case n u for 4096-term pieces
    extra_torch = hyper["lr"] * (4096 + 2) * oc.U32
    for s in range(2):
        la, _ = amp_train_step(a, crit, oa, sa, x, y, clip_grad=None)            # unscale, clip, skip and update: fused
        lb, _ = amp_train_step(b, crit, ob, sb, x, y, clip_grad=1.0)             # the torch-optimizer form
        assert sa.get_scale() == 1024.0 and sb.get_scale() == 1024.0
        own.append([None if p.grad is None else p.grad.detach().cpu() / 1024.0 for p in a.parameters()])
        if s == 0:
            assert la == lb
            ref, _ = oc.run_torch(torch.optim.AdamW, [hyper], p0, own, torch.float64, clip=1.0)
            print(f"gradient norm of step 1: {float(ref[0]['norm']):.4g} (max_grad_norm 1.0)")
            for n, pa, pb, r in zip(names, a.parameters(), b.parameters(), ref[0]["p"]):
                kc.assert_within(pa, r, oc.param_bound(r, hyper["lr"], 1) + extra, f"fused {n}")
                kc.assert_within(pb, pa.detach().double(), 2 * oc.param_bound(r, hyper["lr"], 1) + extra + extra_torch,
                                 f"torch against fused {n}")
    ref, _ = oc.run_torch(torch.optim.AdamW, [hyper], p0, own, torch.float64, clip=1.0)
    for n, pa, r in zip(names, a.parameters(), ref[1]["p"]):
        kc.assert_within(pa, r, oc.param_bound(r, hyper["lr"], 2) + 2 * extra, f"fused {n} after 2 steps")
    n64 = float(ref[1]["norm"])
    S = torch.tensor(n64 * n64)
    assert abs(float(oa.last_grad_norm) - n64) <= float(kc.sum_bound(S, 4096, S, F32)) / (2 * n64) + 2 * oc.U32 * n64
    # an absurd scale: fp16 gradients overflow, the step is skipped on the device and the scale halves
    before = [p.detach().clone() for p in a.parameters()]
    big = torch.amp.GradScaler("cuda", init_scale=2.0 ** 40)
    amp_train_step(a, crit, oa, big, x, y, clip_grad=None)
    assert big.get_scale() == 2.0 ** 39
    assert all(kc.same_bits(p.detach(), q) for p, q in zip(a.parameters(), before))
    assert int(oa._plan.step_count) == 2
    # clip_grad with a fused optimizer keeps working: unscale_ has run, grad_scale arrives as None
    oc_ = FusedAdamW(b.parameters(), **hyper)
    lc, _ = amp_train_step(b, crit, oc_, sb, x, y, clip_grad=1.0)
    assert lc == lc and int(oc_._plan.step_count) == 1
