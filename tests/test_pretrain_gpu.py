"""GPU: the pretraining recipe's kernels (csrc/pretrain.hip) and modules (m3vit_amd/pretrain.py) against the float64 closed
forms and the derived bounds of tests/pretrain_cases.py.  Outputs, workspaces and records are guarded allocations; inputs keep
their bits; a second run gives the same bits."""
import contextlib
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pretrain_cases as PC                                        # noqa: E402
from kernel_contract import assert_within, guarded, guarded_ws, same_bits, snapshot, unchanged   # noqa: E402

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def no_host_sync():
    """torch.cuda.set_sync_debug_mode("error") around a block: any .item(), bool() of a GPU tensor or blocking copy inside
    raises.  Where this torch build does not honour the mode (a probe .item() under it does not raise) only that claim is
    left out - the reason is printed - and the block runs all the same."""
    probe = torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if not honoured:
            torch.cuda.set_sync_debug_mode("default")
            print("sync-debug claim not checked: this torch build does not raise on a synchronising call under "
                  "set_sync_debug_mode('error')")
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


# ---------------------------------------------------------------------------------------------------------------- loss
def run_softce(x, target, smoothing, upstream=1.0):
    """one forward + backward through ops with every output guarded.  Returns dict(loss, grad, lse, record)."""
    from m3vit_amd import ops
    B, C = x.shape
    d2, d_check = guarded(B, C, x.dtype)
    l2, l_check = guarded(1, B, torch.float32)
    t2, t_check = guarded(1, B, torch.float32)
    r2, r_check = guarded(1, ops.LOSS_REC_WORDS, torch.int32)
    need = ops.softce_ws_elems(B)
    assert need == 2 * B
    ws, ws_check = guarded_ws(need)
    dense = target.dtype == torch.float32
    gout = torch.tensor([upstream], dtype=torch.float32, device="cuda")
    snap = snapshot(logits=x, target=target, grad_out=gout)
    record, lse, tsum = ops.loss_softce_fwd(x, target, smoothing, lse=l2.view(-1), tsum=t2.view(-1) if dense else None, ws=ws,
                                            record=r2.view(-1))
    ops.loss_softce_bwd(x, target, lse, tsum, record, gout, smoothing, dlogits=d2)
    torch.cuda.synchronize()
    for chk, what in ((d_check, "dlogits"), (l_check, "lse"), (r_check, "record"), (ws_check, "ws")):
        chk(what=what)
    if dense:
        t_check(what="tsum")
    else:
        t_check(keep_rows=[0], what="tsum (not written with labels)")
    unchanged(snap)
    return dict(loss=record[:1].view(torch.float32).clone(), grad=d2.clone(), lse=lse.clone(), record=record.clone(),
                n_bad=int(record[5]))


def check_softce(x32, target, smoothing, dtype, upstream=1.0, offset=0):
    """x32: float32 CPU logits; target: CPU dense float32 or int64 labels.  offset: elements the logits' storage is shifted
    by (rows then start off a 16-byte boundary).  Checks value, gradient, lse, guards, input bits and run-to-run bits."""
    B, C = x32.shape
    store_ = torch.empty(B * C + offset, dtype=dtype, device="cuda")
    x = store_[offset:].view(B, C)
    x.copy_(x32)
    tgt = target.cuda()
    x64 = x.double().cpu()
    kw = dict(target=target) if target.dtype == torch.float32 else dict(label=target, smoothing=smoothing)
    r = PC.softce_ref(x64, **kw)
    loss_b, grad_b = PC.softce_bounds(r, x64, dtype, smoothing=smoothing, upstream=upstream)
    out = run_softce(x, tgt, smoothing, upstream)
    assert_within(out["loss"], r["loss"].reshape(1), loss_b, "loss")
    assert_within(out["lse"], r["lse"], PC.SAFETY * PC.lse_bound(x64, r["lse"]), "lse")
    assert_within(out["grad"], r["grad"] * upstream, grad_b, "gradient")
    assert out["n_bad"] == r["n_bad"]
    again = run_softce(x, tgt, smoothing, upstream)
    for k in ("loss", "grad", "lse", "record"):
        assert same_bits(out[k], again[k]), f"{k}: a second run gave other bits"
    return out, r


def _target_for(form, B, C):
    if form == "dense":
        return PC.make_soft_target(B, C), 0.0
    return PC.make_labels(B, C), float(form.split("-")[1])


@pytest.mark.parametrize("dtype", PC.DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("form", ["dense", "label-0.0", "label-0.1"])
@pytest.mark.parametrize("B,C", PC.LOSS_SHAPES, ids=lambda v: str(v))
def test_softce_values_guards_and_same_bits(B, C, form, dtype):
    target, s = _target_for(form, B, C)
    check_softce(PC.make_logits(B, C), target, s, dtype)


@pytest.mark.parametrize("form", ["dense", "label-0.1"])
def test_softce_rows_off_a_16_byte_boundary(form):
    """C % 4 == 0 but the storage starts one element past an aligned address: the scalar path"""
    target, s = _target_for(form, 4, 1000)
    check_softce(PC.make_logits(4, 1000), target, s, torch.float32, offset=1)
    check_softce(PC.make_logits(4, 1000), target, s, torch.float16, offset=1)


@pytest.mark.parametrize("dtype", PC.DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("B,C", [(3, 5), (4, 1000)])
def test_softce_upstream_65536_through_the_device_pointer(B, C, dtype):
    """a GradScaler's scale arrives as a device scalar; 65536 / B stays inside the fp16 range at these shapes"""
    for form in ("dense", "label-0.1"):
        target, s = _target_for(form, B, C)
        check_softce(PC.make_logits(B, C, seed=1), target, s, dtype, upstream=65536.0)


@pytest.mark.parametrize("dtype", PC.DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_softce_zero_row_double_row_and_bad_labels(dtype):
    B, C = 4, 1000
    x = PC.make_logits(B, C, seed=2)
    t = PC.make_soft_target(B, C, seed=2)
    t[1] = 0.0                                                     # a row of all-zero targets: no loss, no gradient
    t[2] = t[2] * 2                                                # a row that sums to 2
    out, r = check_softce(x, t, 0.0, dtype)
    assert bool((out["grad"][1] == 0).all())
    y = torch.tensor([C, 3, -1, 0])
    for s in PC.SMOOTHINGS:
        out, r = check_softce(x, y, s, dtype)
        assert out["n_bad"] == 2 and math.isfinite(float(out["loss"]))


def test_softce_logits_of_6e4_in_fp16():
    B, C = 3, 65
    sign = torch.where(torch.rand(B, C, generator=PC._gen(5)) < 0.5, -1.0, 1.0)
    for target, s in (_target_for("dense", B, C), _target_for("label-0.1", B, C)):
        out, _ = check_softce(sign * 6e4, target, s, torch.float16)
        assert math.isfinite(float(out["loss"])) and bool(torch.isfinite(out["lse"]).all())


def test_softce_wrappers_refuse_bad_arguments():
    from m3vit_amd import _lib, ops
    x = torch.zeros(2, 4, device="cuda")
    for bad in (lambda: ops.loss_softce_fwd(x.cpu(), torch.zeros(2, dtype=torch.int64)),
                lambda: ops.loss_softce_fwd(x, torch.zeros(3, dtype=torch.int64, device="cuda")),
                lambda: ops.loss_softce_fwd(x, torch.zeros(2, 5, device="cuda")),
                lambda: ops.loss_softce_fwd(x.t(), torch.zeros(4, dtype=torch.int64, device="cuda")),
                lambda: ops.loss_softce_fwd(x, torch.zeros(2, dtype=torch.int64, device="cuda"), smoothing=1.5),
                lambda: ops.loss_softce_fwd(x, torch.zeros(2, dtype=torch.int64, device="cuda"), ws=torch.zeros(3, device="cuda")),
                lambda: ops.cls_eval_update(x, torch.zeros(2, 4, device="cuda")),
                lambda: ops.mix_batch(torch.zeros(3, 1, 2, 2, device="cuda"), torch.ones(3, device="cuda"),
                                      torch.zeros(3, 4, dtype=torch.int32, device="cuda")),
                lambda: ops.mix_target(torch.zeros(3, dtype=torch.int64, device="cuda"), torch.ones(3, device="cuda"), 4)):
        with pytest.raises(_lib.M3Error):
            bad()


# ----------------------------------------------------------------------------------------------------------------- mix
def _mix_params(B, H, W, shift=0):
    """per-sample lam and box that differ within every pair: the four boxes and the three lams dealt round-robin"""
    names = list(PC.boxes(H, W))
    box = torch.tensor([PC.boxes(H, W)[names[(i + shift) % 4]] for i in range(B)], dtype=torch.int32)
    lam = torch.tensor([PC.MIX_LAMS[(i + shift) % 3] for i in range(B)], dtype=torch.float32)
    return lam, box


@pytest.mark.parametrize("chw", PC.MIX_CHW, ids=str)
@pytest.mark.parametrize("B", PC.MIX_B)
def test_mix_batch_in_place_and_out_of_place(B, chw):
    from m3vit_amd import ops
    C, H, W = chw
    x = torch.randn(B, C, H, W, generator=PC._gen(B * 100 + H))
    N = C * H * W
    for shift in range(4):                                         # every sample meets every box and lam
        lam, box = _mix_params(B, H, W, shift)
        if shift == 3:
            box[:] = 0                                             # Mixup alone, lam 0 / 0.3 / 1 differing within pairs
        ref, blended = PC.mix_ref(x.double(), lam.double(), box)
        copied = ~blended
        lam_d, box_d = lam.cuda(), box.cuda()
        for dtype in PC.DTYPES:
            o2, o_check = guarded(B, N, dtype)
            out = o2.view(B, C, H, W)
            if dtype == torch.float32:
                out.copy_(x)                                       # in place inside the guarded allocation
                src = out
            else:
                src = x.cuda()
            snap = snapshot(lam=lam_d, box=box_d, **({} if src is out else {"x": src}))
            got = ops.mix_batch(src, lam_d, box_d, out=out)
            torch.cuda.synchronize()
            o_check(what=f"mixed batch {dtype}")
            unchanged(snap)
            assert got.data_ptr() == out.data_ptr()
            assert_within(out, ref, PC.mix_bound(x.double(), lam.double(), ref, blended, dtype), f"mix {dtype}")
            want = ref.to(dtype)                                   # CutMix pixels and lam 0 / 1 samples: bit-exact copies
            assert same_bits(out.cpu()[copied], want[copied]), f"{dtype}: a copied element is not bit-exact"
            if dtype == torch.float32:
                first = out.clone()
                out.copy_(x)
                ops.mix_batch(out, lam_d, box_d)
                assert same_bits(first, out), "a second run gave other bits"


def test_mix_batch_copies_keep_special_bits_and_odd_batch_raises():
    from m3vit_amd import _lib, ops
    x = torch.randn(2, 1, 4, 4)
    x[0, 0, 0, 0], x[1, 0, 0, 1], x[1, 0, 3, 3] = -0.0, float("inf"), float("nan")
    lam = torch.tensor([1.0, 0.0]).cuda()
    box = torch.zeros(2, 4, dtype=torch.int32).cuda()
    out = ops.mix_batch(x.cuda(), lam, box).cpu()
    assert same_bits(out[0], x[0]) and same_bits(out[1], x[0]), "lam 1 keeps the sample, lam 0 takes the partner, bit for bit"
    with pytest.raises(_lib.M3Error):
        ops.mix_batch(torch.zeros(3, 1, 4, 4, device="cuda"), torch.ones(3, device="cuda"),
                      torch.zeros(3, 4, dtype=torch.int32, device="cuda"))
    from m3vit_amd.pretrain import Mixup
    with pytest.raises(ValueError):
        Mixup(num_classes=4)(torch.zeros(3, 1, 4, 4, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda"))


@pytest.mark.parametrize("C", PC.TARGET_C)
@pytest.mark.parametrize("B", PC.MIX_B)
def test_mix_target(B, C):
    from m3vit_amd import ops
    y = PC.make_labels(B, C)
    y[0] = C                                                       # one label outside [0, C): the floor only, counted
    lam = torch.tensor([PC.MIX_LAMS[i % 3] for i in range(B)], dtype=torch.float32)
    t2, t_check = guarded(B, C, torch.float32)
    n2, n_check = guarded(1, 1, torch.int32)
    yd, ld = y.cuda(), lam.cuda()
    snap = snapshot(label=yd, lam=ld)
    out, n_bad = ops.mix_target(yd, ld, C, 0.1, out=t2, n_bad=n2.view(-1))
    torch.cuda.synchronize()
    t_check(what="soft target"); n_check(what="n_bad")
    unchanged(snap)
    ref = PC.target_ref(y, y.flip(0), lam.double(), C, 0.1, torch.float64)
    bound = PC.target_bound(y, y.flip(0), lam.double(), C, 0.1)
    assert_within(out, ref, bound, "soft target")
    assert int(n_bad) == 1
    rows = torch.ones(B, dtype=torch.float64)
    hit = (lam.double() * (y == C)) + ((1 - lam.double()) * (y.flip(0) == C))       # the weight of the label that hit nothing
    assert_within(out.double().sum(1), rows - 0.9 * hit, bound.sum(1), "row sums")
    first = out.clone()
    ops.mix_target(yd, ld, C, 0.1, out=t2, n_bad=n2.view(-1))
    assert same_bits(first, t2)


# ---------------------------------------------------------------------------------------------------------- evaluation
def test_cls_eval_two_updates_accumulate_without_a_host_read():
    from m3vit_amd.pretrain import ClsEvalMeter
    m = ClsEvalMeter()
    want, bound = [0.0] * 4, 0.0
    batches = []
    for i, (B, C, dtype) in enumerate(((6, 1000, torch.float16), (1030, 1000, torch.float32))):
        x = PC.make_logits(B, C, seed=10 + i).to(dtype).cuda()
        y = PC.make_labels(B, C, seed=10 + i)
        r = PC.eval_ref(x.double().cpu(), y)
        want = [a + b for a, b in zip(want, r["state"])]
        bound += PC.eval_loss_bound(r, x.double().cpu())
        batches.append((x, y.cuda()))
    m.update(*batches[0])                                          # a warm-up of the allocator outside the checked region
    m.reset()
    torch.cuda.synchronize()
    with no_host_sync():
        for x, y in batches:
            m.update(x, y)
    st = m.state.cpu()
    assert st.dtype == torch.float64 and st.shape == (4,)
    assert st[1:].tolist() == want[1:], "top-1 / top-5 / count against the float64 rank rule"
    assert abs(float(st[0]) - want[0]) <= bound
    assert m.bad_labels == 0
    res = m.get()
    assert res["acc1"] == 100.0 * want[1] / want[3] and res["acc5"] == 100.0 * want[2] / want[3]
    first = st.clone()
    m.reset()
    assert m.state.cpu().tolist() == [0.0] * 4
    for x, y in batches:
        m.update(x, y)
    assert same_bits(m.state.cpu(), first), "a second run gave other bits"


def test_cls_eval_constructed_rows_and_guards():
    from m3vit_amd import ops
    nan = float("nan")
    rows = [([1.0, 3.0, 3.0, 0.0, -1.0, -2.0, -3.0], 2),           # a tie at the target: the lower index wins, rank 1
            ([1.0, 3.0, 3.0, 0.0, -1.0, -2.0, -3.0], 1),           # ... and the lower index itself: rank 0
            ([1.0, nan, 5.0, nan, 0.0, 0.5, 0.2], 2),              # two NaNs beat a number: rank 2
            ([1.0, nan, 5.0, nan, 0.0, 0.5, 0.2], 3),              # the second NaN: rank 1
            ([1.0, nan, 5.0, nan, 0.0, 0.5, 0.2], 1),              # the first NaN: rank 0
            ([7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0], 5),              # rank 5: outside the top five
            ([7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0], 4),              # rank 4: inside
            ([7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0], 7)]              # a bad label: counted, never correct
    x = torch.tensor([r for r, _ in rows])
    y = torch.tensor([t for _, t in rows])
    for dtype in PC.DTYPES:
        xd = x.to(dtype).cuda()
        s2, s_check = guarded(1, ops.CLS_EVAL_WORDS, torch.int64)
        state = s2.view(-1)
        state.zero_()
        ws, ws_check = guarded_ws(ops.cls_eval_ws_elems(len(rows)), dtype=torch.int32)
        ops.cls_eval_update(xd, y.cuda(), ws=ws, state=state)
        torch.cuda.synchronize()
        s_check(what="state"); ws_check()
        st = state[:4].view(torch.float64).cpu().tolist()
        assert st[1:] == [2.0, 6.0, 8.0], (dtype, st)
        assert math.isnan(st[0]), "rows with a NaN logit have a NaN loss, as torch's cross_entropy"
        assert int(state[4]) == 1
    x3 = torch.tensor([[0.0, 2.0, 1.0], [0.0, 2.0, 1.0]]).cuda()    # C = 3 < 5: every valid label is a top-"5" hit
    st = ops.cls_eval_update(x3, torch.tensor([0, 1]).cuda())
    ref = PC.eval_ref(x3.double().cpu(), torch.tensor([0, 1]))
    got = st[:4].view(torch.float64).cpu().tolist()
    assert got[1:] == [1.0, 2.0, 2.0] == ref["state"][1:]
    assert abs(got[0] - ref["state"][0]) <= PC.eval_loss_bound(ref, x3.double().cpu())


# ----------------------------------------------------------------------------------------------------------------- EMA
@pytest.mark.parametrize("decay", PC.EMA_DECAYS)
def test_ema_update_sizes_offsets_and_three_steps(decay):
    """five tensors carved from one buffer at offsets that are no multiples of 4 (scalar path) and, a second time, at
    16-byte offsets (vector path), in one table"""
    from m3vit_amd import ops
    g = PC._gen(11)
    for rem in (1, 0):                                             # offsets = rem mod 4 elements: 1 is off every 16-byte boundary
        offs, o = [], rem
        for n in PC.EMA_SIZES:
            offs.append(o)
            o += n
            o += (rem - o) % 4
        total = o + 8
        assert all(v % 4 == rem for v in offs)
        ebuf, e_check = guarded_ws(total)
        e0 = torch.randn(total, generator=g)
        ebuf.copy_(e0)
        pbuf = torch.randn(total, generator=g).cuda()
        views = [(ebuf[a:a + n], pbuf[a:a + n]) for a, n in zip(offs, PC.EMA_SIZES)]
        owned = torch.zeros(total, dtype=torch.bool)
        for a, n in zip(offs, PC.EMA_SIZES):
            owned[a:a + n] = True
        table = ops.ema_table(views)
        assert table[1] == 5 and table[2] == sum(-(-n // 4096) for n in PC.EMA_SIZES)
        ref, bound = e0.double(), torch.zeros(total, dtype=torch.float64)
        p64 = pbuf.double().cpu()
        snap = snapshot(p=pbuf)
        for step in range(3):
            ops.ema_update(*table, decay)
            torch.cuda.synchronize()
            e_check(what="ema buffer")
            ref = torch.where(owned, PC.ema_ref(ref, p64, decay), ref)
            bound = torch.where(owned, PC.ema_bound_compound(bound, ref, p64, decay), bound)
            got = ebuf.cpu()
            assert same_bits(got[~owned], e0[~owned]), "elements between the tensors changed"
            assert_within(got, ref, bound, f"ema step {step}")
        unchanged(snap)
        if decay == 1.0:
            assert same_bits(ebuf.cpu(), e0), "decay 1 must leave the shadow bit-identical"
        if decay == 0.0:
            assert same_bits(ebuf.cpu()[owned], pbuf.cpu()[owned]), "decay 0 copies"


# ------------------------------------------------------------------------------------------------------- tiny model
# the head and its backward are m3_gemm_nt calls with num_classes as N, then as K: N % 4 == 0 and 16-byte rows of fp16
# (K % 8 == 0).  10 classes cannot run on this model; 16 is the next count that can.
NUM_CLASSES = 16


def _tiny(seed=7, act=torch.float16):
    from m3vit_amd.cls import MoEViTConfig, MoEViTForImageNet
    cfg = MoEViTConfig(img_size=32, patch_size=16, embed_dim=64, depth=2, num_heads=2, num_classes=NUM_CLASSES, moe_experts=4,
                       moe_top_k=2, gate_dim=64, vmoe_noisy_std=0.0)
    torch.manual_seed(seed)
    return MoEViTForImageNet(cfg, act_dtype=act).cuda().train()


def test_model_ema_keys_round_trip_and_applied():
    from m3vit_amd.pretrain import ModelEma
    model = _tiny()
    ema = ModelEma(model, decay=0.5)
    sd = model.state_dict()
    assert list(ema.state_dict()) == list(sd)
    assert not hasattr(ema, "module") and not hasattr(ema, "ema")
    assert all(v.data_ptr() != sd[k].data_ptr() for k, v in ema.state_dict().items() if v.numel())
    x = torch.randn(4, 3, 32, 32, generator=PC._gen(3)).cuda()
    model.eval()
    with torch.no_grad():
        base = model(x)["logits"].clone()
        for p in model.parameters():                               # the model moves on, the EMA follows half way
            p.add_(0.05 * torch.randn(p.shape, generator=PC._gen(p.numel())).cuda())
        ema.update(model)
        moved = model(x)["logits"].clone()
        assert not same_bits(base, moved)
        saved = {k: v.clone() for k, v in ema.state_dict().items()}
        with ema.applied(model):
            inside = model(x)["logits"].clone()
        after = model(x)["logits"].clone()
    assert not same_bits(inside, moved), "the EMA weights did not reach the executor (version counters)"
    assert same_bits(after, moved), "the original weights were not restored bit for bit"
    # round trip: into a second EMA, which then applies the same weights
    other = ModelEma(model, decay=0.5)
    other.load_state_dict({k: v.cpu() for k, v in saved.items()})
    assert all(same_bits(a, b) for a, b in zip(other.state_dict().values(), saved.values()))
    with torch.no_grad(), other.applied(model):
        assert same_bits(model(x)["logits"], inside)
    with pytest.raises(KeyError):
        other.load_state_dict({})


def test_pretrain_step_ema_overflow_and_no_host_sync():
    from m3vit_amd.optim import FusedAdamW
    from m3vit_amd.pretrain import ClsEvalMeter, Mixup, ModelEma, build_criterion, pretrain_step
    from types import SimpleNamespace as NS
    model = _tiny()
    opt = FusedAdamW(model.parameters(), lr=1e-2, weight_decay=0.05, max_grad_norm=1.0)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    crit = build_criterion(NS(mixup=0.8, cutmix=1.0, cutmix_minmax=None, smoothing=0.1, distillation_type="none",
                              distillation_alpha=0.5, distillation_tau=1.0))
    decay = 0.9
    ema = ModelEma(model, decay=decay)
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=NUM_CLASSES, mode="elem")
    lam = np.array([0.3, 1.0, 0.75, 0.6], dtype=np.float32)
    box = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [8, 24, 8, 24], [0, 0, 0, 0]], dtype=np.int32)
    mix.draw = lambda B, H, W: (lam, box)                          # the parameters pinned
    g = PC._gen(21)
    names = list(model.state_dict())
    fl = [k for k, v in model.state_dict().items() if v.dtype == torch.float32]
    ref = {k: v.double().cpu() for k, v in ema.state_dict().items() if k in fl}
    bound = {k: torch.zeros_like(v) for k, v in ref.items()}
    before = {k: v.clone() for k, v in model.state_dict().items()}
    for step in range(2):
        x = torch.randn(4, 3, 32, 32, generator=g).cuda()
        y = torch.randint(0, NUM_CLASSES, (4,), generator=g).cuda()
        loss, cv = pretrain_step(model, crit, opt, scaler, x, y, mixup_fn=mix, model_ema=ema, moe_cv_weight=0.01, clip_grad=1.0)
        assert loss.is_cuda and cv.is_cuda and math.isfinite(float(loss)) and math.isfinite(float(cv))
        now = model.state_dict()
        for k in fl:
            p64 = now[k].double().cpu()
            ref[k] = PC.ema_ref(ref[k], p64, decay)
            bound[k] = PC.ema_bound_compound(bound[k], ref[k], p64, decay)
    assert any(not same_bits(before[k], model.state_dict()[k]) for k in fl), "two steps changed no parameter"
    shadow = ema.state_dict()
    assert list(shadow) == names
    for k in fl:
        assert_within(shadow[k], ref[k], bound[k], f"ema of {k}")
    assert math.isfinite(crit.last_stats["loss_base"]) and crit.last_stats["loss_distill"] == 0.0

    # a forced overflow: at a scale of 2^40 the fp16 gradients are Inf, the step is skipped, the parameters keep their bits
    held = {k: v.clone() for k, v in model.state_dict().items()}
    hot = torch.amp.GradScaler("cuda", init_scale=2.0 ** 40)
    x = torch.randn(4, 3, 32, 32, generator=g).cuda()
    y = torch.randint(0, NUM_CLASSES, (4,), generator=g).cuda()
    pretrain_step(model, crit, opt, hot, x, y, mixup_fn=mix, model_ema=None, clip_grad=1.0)
    assert all(same_bits(held[k], v) for k, v in model.state_dict().items()), "an overflow step changed the parameters"

    # the new pieces read nothing back: mix, criterion forward + backward on a leaf, the meter, the EMA (all warmed up above)
    x = torch.randn(4, 3, 32, 32, generator=g).cuda()
    y = torch.randint(0, NUM_CLASSES, (4,), generator=g).cuda()
    logits = torch.randn(4, NUM_CLASSES, generator=g).cuda().requires_grad_(True)
    meter = ClsEvalMeter()
    meter.update(logits, y)
    mix(x.clone(), y)
    torch.cuda.synchronize()
    with no_host_sync():
        xm, soft = mix(x, y)
        crit(xm, logits, soft).backward()
        meter.update(logits, y)
        ema.update(model)
    torch.cuda.synchronize()
    assert logits.grad is not None and bool(torch.isfinite(logits.grad).all())
    assert mix.last_bad_labels == 0 and crit.base_criterion.last_bad_labels == 0
    assert float(meter.state[3]) == 8.0
