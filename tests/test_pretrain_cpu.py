"""CPU: the pretraining recipe's closed forms and bounds (tests/pretrain_cases.py) and the host halves of m3vit_amd.pretrain.

Torch's own fp32 evaluation of every closed form must stay inside the bounds the kernels are held to, against the float64
evaluation of the same inputs: a bound that torch's fp32 breaks is wrong.  Then Mixup.draw (the host random stream), the row
sums of the soft target, the dense form against the label-pair formula, and ClsEvalMeter's arithmetic."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pretrain_cases as PC                                        # noqa: E402
from kernel_contract import assert_within                          # noqa: E402

from m3vit_amd import pretrain                                     # noqa: E402


def _pair_labels(B, C, seed=0):
    y = PC.make_labels(B, C, seed)
    return y, y.flip(0)


@pytest.mark.parametrize("B,C", PC.LOSS_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("form", ["dense", "label-0", "label-0.1"])
def test_fp32_softce_inside_the_bounds(B, C, form):
    x = PC.make_logits(B, C)
    if form == "dense":
        kw = dict(target=PC.make_soft_target(B, C))
        s = 0.0
    else:
        s = float(form.split("-")[1])
        kw = dict(label=PC.make_labels(B, C), smoothing=s)
    r64 = PC.softce_ref(x.double(), **kw)
    r32 = PC.softce_ref(x, **kw)
    loss_b, grad_b = PC.softce_bounds(r64, x.double(), torch.float32, smoothing=s)
    assert_within(r32["loss"], r64["loss"], loss_b, "loss")
    assert_within(r32["grad"], r64["grad"], grad_b, "gradient")
    assert_within(r32["lse"], r64["lse"], PC.SAFETY * PC.lse_bound(x.double(), r64["lse"]), "lse")


def test_fp32_softce_odd_targets_and_bad_labels():
    """a row of zeros, a row that sums to 2, labels C and -1: finite, inside the bounds, two bad labels"""
    B, C = 4, 10
    x = PC.make_logits(B, C, seed=2)
    t = PC.make_soft_target(B, C, seed=2)
    t[1] = 0.0
    t[2] = t[2] * 2
    r64, r32 = PC.softce_ref(x.double(), target=t), PC.softce_ref(x, target=t)
    loss_b, grad_b = PC.softce_bounds(r64, x.double(), torch.float32)
    assert_within(r32["loss"], r64["loss"], loss_b)
    assert_within(r32["grad"], r64["grad"], grad_b)
    assert bool((r64["grad"][1] == 0).all()) and abs(float(r64["S"][2]) - 2.0) < 1e-6
    y = torch.tensor([C, 3, -1, 0])
    for s in PC.SMOOTHINGS:
        r64, r32 = PC.softce_ref(x.double(), label=y, smoothing=s), PC.softce_ref(x, label=y, smoothing=s)
        assert r64["n_bad"] == 2 and torch.isfinite(r64["loss"])
        loss_b, grad_b = PC.softce_bounds(r64, x.double(), torch.float32, smoothing=s)
        assert_within(r32["loss"], r64["loss"], loss_b)
        assert_within(r32["grad"], r64["grad"], grad_b)


@pytest.mark.parametrize("chw", PC.MIX_CHW, ids=str)
@pytest.mark.parametrize("B", PC.MIX_B)
def test_fp32_mix_and_target_inside_the_bounds(B, chw):
    C, H, W = chw
    x = torch.randn(B, C, H, W, generator=PC._gen(B * 100 + H))
    names = list(PC.boxes(H, W))
    box = torch.tensor([PC.boxes(H, W)[names[i % 4]] for i in range(B)], dtype=torch.int32)
    lam = torch.tensor([PC.MIX_LAMS[i % 3] for i in range(B)], dtype=torch.float32)
    ref, blended = PC.mix_ref(x.double(), lam.double(), box)
    out32, _ = PC.mix_ref(x, lam, box)
    assert_within(out32, ref, PC.mix_bound(x.double(), lam.double(), ref, blended, torch.float32), "mix")
    assert torch.equal(out32[~blended].double(), ref[~blended]), "copied elements are exact"
    for nc in PC.TARGET_C:
        y, yp = _pair_labels(B, nc)
        t64 = PC.target_ref(y, yp, lam.double(), nc, 0.1, torch.float64)
        t32 = PC.target_ref(y, yp, lam, nc, 0.1, torch.float32)
        b = PC.target_bound(y, yp, lam.double(), nc, 0.1)
        assert_within(t32, t64, b, "soft target")
        assert_within(t32.double().sum(1), torch.ones(B, dtype=torch.float64), b.sum(1), "soft target row sums")


@pytest.mark.parametrize("B,C", [(4, 10), (6, 1000)])
def test_dense_form_equals_the_label_pair_formula(B, C):
    x = PC.make_logits(B, C, seed=4).double()
    y, yp = _pair_labels(B, C, seed=4)
    lam = torch.rand(B, generator=PC._gen(9)).double()
    t = PC.target_ref(y, yp, lam, C, 0.1, torch.float64)
    dense = PC.softce_ref(x, target=t)["loss"]
    pair = PC.label_pair_loss(x, y, yp, lam, 0.1)
    assert abs(float(dense - pair)) <= 1e-12 * (1 + abs(float(pair)))


def test_rank_rule_on_constructed_rows():
    nan = float("nan")
    x = torch.tensor([[1.0, 3.0, 3.0, 0.0],        # a tie at the target (index 2): the lower index 1 wins -> rank 1
                      [1.0, nan, 5.0, nan],        # target 2 is a number: both NaNs beat it -> rank 2
                      [1.0, nan, 5.0, nan],        # target 3 is the second NaN: the first beats it -> rank 1
                      [1.0, nan, 5.0, nan]],       # target 1 is the first NaN: nothing beats it -> rank 0
                     dtype=torch.float64)
    y = torch.tensor([2, 2, 3, 1])
    assert PC.rank_ref(x, y).tolist() == [1, 2, 1, 0]
    r = PC.eval_ref(torch.tensor([[0.0, 2.0, 1.0]], dtype=torch.float64), torch.tensor([0]))     # C = 3 < 5: the last rank, 2, is still < min(5, C)
    assert r["state"][1:] == [0.0, 1.0, 1.0]
    r = PC.eval_ref(torch.tensor([[0.0, 2.0, 1.0]], dtype=torch.float64), torch.tensor([3]))     # a bad label
    assert r["n_bad"] == 1 and r["state"][1:] == [0.0, 0.0, 1.0]


@pytest.mark.parametrize("decay", PC.EMA_DECAYS)
def test_fp32_ema_inside_the_bound(decay):
    g = PC._gen(5)
    e, p = torch.randn(4097, generator=g), torch.randn(4097, generator=g)
    e64, e32, bound = e.double(), e.clone(), torch.zeros(4097, dtype=torch.float64)
    for _ in range(3):
        e64 = PC.ema_ref(e64, p.double(), decay)
        e32 = PC.ema_ref(e32, p, decay)
        bound = PC.ema_bound_compound(bound, e64, p.double(), decay)
        assert_within(e32, e64, bound, "ema")
    if decay == 1.0:
        assert torch.equal(e32, e)
    if decay == 0.0:
        assert torch.equal(e32, p)


# ------------------------------------------------------------------------------------------------------ Mixup.draw
@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
def test_draw_boxes_lam_and_pairing(mode):
    np.random.seed(0)
    H, W, B = 32, 40, 8
    m = pretrain.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode=mode, num_classes=10)
    cut = mixed = 0
    for _ in range(50):
        lam, box = m.draw(B, H, W)
        assert lam.dtype == np.float32 and lam.shape == (B,) and box.dtype == np.int32 and box.shape == (B, 4)
        assert ((0 <= lam) & (lam <= 1)).all()
        yl, yh, xl, xh = box.T
        assert ((0 <= yl) & (yl <= yh) & (yh <= H) & (0 <= xl) & (xl <= xh) & (xh <= W)).all()
        area = (yh - yl) * (xh - xl)
        nz = area > 0
        assert np.array_equal(lam[nz], (1.0 - area[nz] / float(H * W)).astype(np.float32)), "correct_lam: 1 - area / (H W)"
        cut += int(nz.sum())
        mixed += int((~nz & (lam < 1)).sum())
        if mode == "batch":
            assert (lam == lam[0]).all() and (box == box[0]).all()
        if mode == "pair":
            assert np.array_equal(lam, lam[::-1]) and np.array_equal(box, box[::-1])
    assert cut > 0 and mixed > 0, "both kinds are drawn when both alphas are positive"


def test_draw_prob_zero_modes_and_refusals():
    np.random.seed(1)
    for mode in ("batch", "pair", "elem"):
        lam, box = pretrain.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.0, mode=mode).draw(6, 8, 8)
        assert (lam == 1).all() and (box == 0).all()
    lam, box = pretrain.Mixup(mixup_alpha=0.0, cutmix_alpha=1.0, correct_lam=False).draw(4, 16, 16)
    assert (lam <= 1).all()
    lam, box = pretrain.Mixup(mixup_alpha=1.0, cutmix_alpha=0.0).draw(4, 16, 16)
    assert (box == 0).all(), "Mixup alone draws no box"
    with pytest.raises(ValueError):
        pretrain.Mixup().draw(3, 8, 8)
    with pytest.raises(NotImplementedError):
        pretrain.Mixup(cutmix_minmax=(0.2, 0.8))
    with pytest.raises(NotImplementedError):
        pretrain.DistillationLoss(pretrain.CrossEntropy(), None, "soft", 0.5, 1.0)
    with pytest.raises(NotImplementedError):
        pretrain.ModelEma(torch.nn.Linear(2, 2), device="cpu")


def test_build_criterion_picks_the_reference_classes():
    from types import SimpleNamespace as NS
    base = dict(cutmix_minmax=None, distillation_type="none", distillation_alpha=0.5, distillation_tau=1.0)
    c = pretrain.build_criterion(NS(mixup=0.8, cutmix=1.0, smoothing=0.1, **base))
    assert isinstance(c, pretrain.DistillationLoss) and type(c.base_criterion) is pretrain.SoftTargetCrossEntropy
    c = pretrain.build_criterion(NS(mixup=0.0, cutmix=0.0, smoothing=0.1, **base))
    assert type(c.base_criterion) is pretrain.LabelSmoothingCrossEntropy and c.base_criterion.smoothing == 0.1
    c = pretrain.build_criterion(NS(mixup=0.0, cutmix=0.0, smoothing=0.0, **base))
    assert type(c.base_criterion) is pretrain.CrossEntropy


def test_cls_eval_meter_arithmetic():
    assert pretrain.ClsEvalMeter.result([12.5, 30.0, 45.0, 50.0]) == {"loss": 0.25, "acc1": 60.0, "acc5": 90.0}
    assert pretrain.ClsEvalMeter.result([0.0, 0.0, 0.0, 0.0]) == {"loss": 0.0, "acc1": 0.0, "acc5": 0.0}
