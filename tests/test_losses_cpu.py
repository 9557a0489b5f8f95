"""CPU: the dense-prediction losses' reference, bounds and public surface (no kernel runs without a GPU).

* the plain-torch restatement of tests/loss_cases.py reproduces tests/golden/g12_losses.npz - recorded from the reference's own
  classes by tests/gen_golden_losses.py - in float64, value and gradient, and the MultiTaskLoss module of m3vit_amd.losses
  reproduces every recorded dictionary when it is given the restated losses;
* torch's own fp32 evaluation of the restatement stays inside the bounds the kernels are held to, on every input the GPU
  tests use: the bounds are attainable before a GPU is involved;
* names, constructor signatures, the get_loss table, and the errors of the public surface.
"""
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_cases as LC                                           # noqa: E402
from kernel_contract import assert_within                         # noqa: E402

G12 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_losses.npz")


@pytest.fixture(scope="module")
def g12():
    return np.load(G12)


def _close(a, b, what):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert torch.equal(torch.isnan(a), torch.isnan(b)), f"{what}: NaN pattern differs"
    a, b = a.nan_to_num(0.0), b.nan_to_num(0.0)
    scale = b.abs().max().clamp_min(1e-300) if b.numel() else 1.0
    err = float((a - b).abs().max() / scale) if b.numel() else 0.0
    assert err <= 1e-12, f"{what}: relative error {err:.3e}"


@pytest.mark.parametrize("case", LC.fixture_cases(), ids=LC.case_id)
def test_restatement_reproduces_the_reference(g12, case):
    kind, C, size, extra = case
    k = LC.case_id(case)
    pred, label = torch.from_numpy(g12[f"{k}/pred"]), torch.from_numpy(g12[f"{k}/label"])
    mine, lab = LC.make_inputs(kind, C, size)
    assert torch.equal(mine, pred) and torch.equal(lab, label), "the input makers no longer produce the recorded inputs"
    r = LC.reference(kind, pred.double(), label, extra)
    _close(r["loss"], g12[f"{k}/loss"], f"{k} loss")
    _close(r["grad"], g12[f"{k}/grad"], f"{k} gradient")


def test_restatement_nan_and_zero_rules():
    """no valid pixel / element: CE and L1 give NaN (0 / 0) with a zero gradient, the normals loss 0 - what the reference's
    classes give in float64 (checked when the fixture was generated: see the all-ignored human_parts of mt/plain5)"""
    for name, kind, pred, label, extra, _, expect in LC.edge_cases():
        if expect not in ("nan", "zero"):
            continue
        r = LC.reference(kind, pred.double(), label, extra)
        assert (math.isnan(float(r["loss"])) if expect == "nan" else float(r["loss"]) == 0.0), name
        assert not bool(r["grad"].abs().any()), name


def _criterion(name, loss_of):
    from m3vit_amd import losses
    tasks, _, multi_level, tam, _ = LC.SCHEMES[name]
    ft = torch.nn.ModuleDict({t: loss_of(t) for t in tasks})
    return losses.MultiTaskLoss(list(tasks), ft, {t: LC.TASK_WEIGHT[t] for t in tasks}, multi_level, {"model_kwargs": {"tam": tam}})


@pytest.mark.parametrize("name", list(LC.SCHEMES))
def test_multitask_scheme_reproduces_the_reference(g12, name):
    """m3vit_amd.losses.MultiTaskLoss over the restated losses, float64 on the CPU: keys, every entry, total and gradients"""
    crit = _criterion(name, lambda t: LC.RefLoss(*LC.TASK_KIND[t]))
    single = LC.SCHEMES[name][4]
    pred, gt = LC.scheme_inputs(name)
    for key, v in pred.items():
        assert np.array_equal(v.numpy(), g12[f"mt/{name}/pred/{key}"])
    xs = {key: v.double().requires_grad_(True) for key, v in pred.items()}
    out = crit(xs, {t: v.double() for t, v in gt.items()}, single_task=single)
    want = {k.split("/")[-1] for k in g12.files if k.startswith(f"mt/{name}/out/")}
    assert set(out) == want
    for key in want:
        _close(out[key].detach(), g12[f"mt/{name}/out/{key}"], f"{name} {key}")
    out["total"].backward()
    for key, x in xs.items():
        _close(torch.zeros_like(x) if x.grad is None else x.grad, g12[f"mt/{name}/grad/{key}"], f"{name} d {key}")


def _fp32_within(kind, pred, label, extra, dtype, what):
    """torch's fp32 evaluation of the restatement on the dtype-rounded inputs against the float64 one, inside the kernels' bounds"""
    x = pred.to(dtype)
    x64 = x.double()
    r = LC.reference(kind, x64, label, extra)
    f = LC.reference(kind, x.float(), label, extra)
    for up in LC.UPSTREAMS:
        if not LC.upstream_fits(r, dtype, up):
            continue
        lb, gb = LC.bounds(kind, r, x64, dtype, extra, upstream=up)
        if math.isnan(float(r["loss"])):
            assert math.isnan(float(f["loss"])), what
        else:
            assert_within(f["loss"], r["loss"], lb, f"{what} loss")
        assert_within((f["grad"] * up).to(dtype), r["grad"] * up, gb, f"{what} gradient x{up}")


@pytest.mark.parametrize("dtype", LC.DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("case", [c for c in LC.cases() if c[2] != LC.GRID_CAP], ids=LC.case_id)
def test_fp32_evaluation_is_inside_the_kernel_bounds(case, dtype):
    kind, C, size, extra = case
    pred, label = LC.make_inputs(kind, C, size)
    _fp32_within(kind, pred, label, extra, dtype, LC.case_id(case))


def test_fp32_evaluation_is_inside_the_kernel_bounds_grid_cap_and_edges():
    pred, label = LC.make_inputs("ce", 40, LC.GRID_CAP)
    _fp32_within("ce", pred, label, None, torch.float32, "grid cap")
    for case in LC.multi_pass_cases():
        pred, label = LC.make_inputs(*case[:3])
        _fp32_within(case[0], pred, label, case[3], torch.float32, LC.case_id(case))
    for C in LC.GROUP_CLASSES:
        for dtype in LC.DTYPES:
            pred, label = LC.make_inputs("ce", C, (3, 17, 33))
            _fp32_within("ce", pred, label, None, dtype, f"groups C{C} {dtype}")
    for name, kind, pred, label, extra, dtypes, expect in LC.edge_cases():
        for dtype in dtypes:
            _fp32_within(kind, pred, label, extra, dtype, f"{name} {dtype}")


def test_bad_labels_are_ignored_and_counted_by_the_restatement():
    for name, kind, pred, label, extra, _, expect in LC.edge_cases():
        if not isinstance(expect, tuple):
            continue
        r = LC.reference(kind, pred.double(), label, extra)
        assert r["n_bad"] == expect[1], name
        _, valid, bad = LC.class_of(label, pred.shape[1])
        clean = label.clone()
        clean[bad.unsqueeze(1)] = LC.IGNORE
        c = LC.reference(kind, pred.double(), clean, extra)
        assert float(c["loss"]) == float(r["loss"]) and torch.equal(c["grad"], r["grad"]) and c["n_bad"] == 0


# ---------------------------------------------------------------------------------------------------- the public surface
def test_names_signatures_and_the_get_loss_table():
    import m3vit_amd
    from m3vit_amd import losses

    def params(cls):
        return [(p.name, p.default) for p in list(inspect.signature(cls.__init__).parameters.values())[1:]]
    E = inspect.Parameter.empty
    assert params(losses.SoftMaxwithLoss) == []
    assert params(losses.BalancedCrossEntropyLoss) == [("size_average", True), ("batch_average", True), ("pos_weight", None)]
    assert params(losses.DepthLoss) == [("loss", "l1")]
    assert params(losses.NormalsLoss) == [("size_average", True), ("normalize", False), ("norm", 1)]
    assert params(losses.SingleTaskLoss) == [("loss_ft", E), ("task", E)]
    assert params(losses.MultiTaskLoss) == [("tasks", E), ("loss_ft", E), ("loss_weights", E), ("multi_level", False), ("p", None)]
    assert [p for p in inspect.signature(losses.MultiTaskLoss.forward).parameters] == ["self", "pred", "gt", "single_task"]
    assert [p for p in inspect.signature(losses.BalancedCrossEntropyLoss.forward).parameters] == ["self", "output", "label", "void_pixels"]
    for n in losses.__all__:
        assert getattr(m3vit_amd, n) is getattr(losses, n)
    p = {"edge_w": 0.95, "normloss": 1, "depthloss": "l1"}
    table = {"edge": (losses.BalancedCrossEntropyLoss, {"pos_weight": 0.95}), "sal": (losses.BalancedCrossEntropyLoss, {"pos_weight": None}),
             "semseg": (losses.SoftMaxwithLoss, {}), "human_parts": (losses.SoftMaxwithLoss, {}),
             "normals": (losses.NormalsLoss, {"norm": 1}), "depth": (losses.DepthLoss, {})}
    for task, (cls, attrs) in table.items():
        m = losses.get_loss(p, task)
        assert type(m) is cls and all(getattr(m, k) == v for k, v in attrs.items()), task
    assert losses.get_loss(dict(p, normloss=2), "normals").norm == 2
    with pytest.raises(NotImplementedError):
        losses.get_loss(p, "flow")
    with pytest.raises(NotImplementedError):
        losses.DepthLoss("l2")
    with pytest.raises(NotImplementedError):
        losses.NormalsLoss(normalize=True, norm=3)


def test_constructors_do_not_print_and_multi_level_divides_the_weights(capsys):
    from m3vit_amd import losses
    ft = torch.nn.ModuleDict({"semseg": losses.SoftMaxwithLoss(), "normals": losses.NormalsLoss(normalize=True, norm=2)})
    w = {"semseg": 1.0, "normals": 10.0}
    m = losses.MultiTaskLoss(["semseg", "normals"], ft, w, multi_level=True)
    assert capsys.readouterr().out == ""
    assert m.loss_weights == {"semseg": 0.25, "normals": 2.5} and m.tam is False
    assert losses.MultiTaskLoss(["semseg", "normals"], ft, dict(w), p={"model_kwargs": {"tam": True}}).tam is True


def test_cpu_tensors_and_void_pixels_raise():
    from m3vit_amd import losses, ops
    from m3vit_amd._lib import M3Error
    x, y = torch.randn(1, 3, 4, 4), torch.zeros(1, 1, 4, 4)
    for m, lab in ((losses.SoftMaxwithLoss(), y), (losses.DepthLoss(), torch.zeros(1, 3, 4, 4)),
                   (losses.NormalsLoss(normalize=True), torch.zeros(1, 3, 4, 4)),
                   (losses.BalancedCrossEntropyLoss(), torch.zeros(1, 3, 4, 4))):
        with pytest.raises(M3Error):
            m(x, lab)
    with pytest.raises(NotImplementedError):
        losses.BalancedCrossEntropyLoss()(x, torch.zeros(1, 3, 4, 4), void_pixels=torch.zeros(1, 3, 4, 4))
    for fn in (ops.loss_ce_fwd, ops.loss_l1_fwd, ops.loss_normals_fwd, ops.loss_bce_fwd):
        with pytest.raises(M3Error):
            fn(x, y)
    assert ops.loss_ws_elems(1) == 4 and ops.loss_ws_elems(10 ** 9) == 4 * 1024 and ops.loss_ws_elems(257) == 8
