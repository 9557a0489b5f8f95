"""CPU: the task meters' float64 restatement (tests/meter_cases.py) against the reference's own numbers in
tests/golden/g13_meters.npz, torch's fp32 evaluation of the same formulas inside the bounds the kernels are held to, and the
host side of m3vit_amd.meters: constructor tables, refused arguments, no CPU path."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meter_cases as MC                                          # noqa: E402

G13 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_meters.npz")
REL = 1e-12


@pytest.fixture(scope="module")
def g13():
    return np.load(G13)


def close(a, b, rel=REL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((np.abs(a - b) <= rel * np.abs(b) + 1e-300).all())


def restated(g13, key, upto, dtype=torch.float64):
    """the restatement accumulated over updates 0 .. upto of a recorded case (with the bounds of the float sums)"""
    _, task, db, C, size = next(f for f in MC.FIXTURES if f[0] == key)
    kind = MC.TASK_KIND[task]
    acc, last = MC.Accumulated(kind), None
    for u in range(upto + 1):
        pred, label = torch.from_numpy(g13[f"{key}/pred{u}"]), torch.from_numpy(g13[f"{key}/label{u}"])
        ncls = MC.N_CLASSES[db] if task == "semseg" else 7
        r64 = MC.reference(kind, pred.double(), label, ncls)
        last = r64 if dtype == torch.float64 else MC.reference(kind, pred.to(dtype), label, ncls)
        acc.add(last, MC.bounds(kind, r64, pred.double()))
    return kind, acc, last


@pytest.mark.parametrize("u", [0, 1])
@pytest.mark.parametrize("key", [f[0] for f in MC.FIXTURES])
def test_restatement_reproduces_the_reference(g13, key, u):
    """counts exact, sums and scores to 1e-12 relative; the edge meter's reference runs its loss in fp32, so its two numbers
    are held to the fp32 bound of that loss instead (the reference's own error)"""
    kind, acc, last = restated(g13, key, u)
    a = lambda name: g13[f"{key}/acc{u}/{name}"]                   # noqa: E731
    if kind == "iou":
        assert all(np.array_equal(acc.ints[i], a(n)) for i, n in enumerate(("tp", "fp", "fn")))
        if key.endswith("-ties"):
            assert acc.ints[0][2] + acc.ints[1][2] > 0 and acc.ints[0][5] + acc.ints[1][5] == 0      # channel 2 wins, 5 never
    elif kind == "depth":
        assert acc.ints[0] == a("n_valid") and close(acc.sums, [a("total_rmses"), a("total_log_rmses")])
    elif kind == "normals":
        assert acc.ints[3] == a("n") and list(acc.ints[:3] * 100) == [a("11.25"), a("22.5"), a("30")]
        assert close(acc.sums, [a("mean"), a("rmse")])
    elif kind == "sal":
        got = last["per_image"].numpy()
        assert close(got[0], a("jaccards")) and close(got[1], a("prec")) and close(got[2], a("rec"))
    else:
        assert acc.ints[0] == a("n") and abs(acc.sums[0] - a("loss")) <= acc.bounds[0]
    want = {k.split("/")[-1]: g13[k] for k in g13.files if k.startswith(f"{key}/score{u}/")}
    got = MC.score(kind, acc.ints, acc.sums)
    assert set(got) == set(want)
    for k, v in want.items():
        if kind == "edge":
            assert abs(got[k] - float(v)) <= acc.bounds[0] / acc.ints[0]
        else:
            assert close(got[k], v), (k, got[k], v)


@pytest.mark.parametrize("case", [c for c in MC.cases() if c[0] != "iou"], ids=MC.case_id)
def test_fp32_evaluation_stays_within_the_kernel_bounds(case):
    """torch's own fp32 evaluation of the restated formulas against the float64 one, inside the bounds the GPU test uses -
    and not far inside: the bounds are within a few thousand fp32 roundings of the sums, not vacuous"""
    kind, C, size = case
    pred, label = MC.settle(kind, *MC.make_inputs(kind, C, size))
    r64, r32 = MC.reference(kind, pred.double(), label), MC.reference(kind, pred, label)
    a64, a32 = MC.Accumulated(kind).add(r64, MC.bounds(kind, r64, pred.double())), MC.Accumulated(kind).add(r32)
    assert np.array_equal(a64.ints, a32.ints)
    err = np.abs(a64.sums - a32.sums)
    print(MC.case_id(case), "err / bound", (err / np.maximum(a64.bounds, 1e-300)).max() if err.size else 0.0)
    assert bool((err <= a64.bounds).all()), (err, a64.bounds)
    if kind != "sal":
        mag = {"depth": ("sum_sq", "sum_log_sq"), "normals": ("sum_angle", "sum_sq"), "edge": ("sum",)}[kind]
        mag = [abs(float(r64[k])) for k in mag]
        assert all(b <= 1e-3 * float(m) + 1e-6 for b, m in zip(a64.bounds, mag))


@pytest.mark.parametrize("C", MC.IOU_CLASSES)
def test_iou_restatement_is_the_class_loop(C):
    """tp + fn = the label histogram, tp + fp = the prediction histogram over the valid pixels - what the kernel accumulates"""
    pred, label = MC.make_inputs("iou", C, (3, 17, 33))
    r = MC.iou_ref(pred.double(), label, C)
    lab, valid = MC.class_of(label)
    am = pred.argmax(1)
    assert all(r["tp"][i] + r["fn"][i] == int(((lab == i) & valid).sum()) and r["tp"][i] + r["fp"][i] == int(((am == i) & valid).sum())
               for i in range(C))


def test_constructor_tables_and_refused_arguments():
    from m3vit_amd import _lib, meters
    assert [meters.SemsegMeter(d).n_classes for d in ("PASCALContext", "NYUD", "CityScapes")] == [21, 40, 7]
    assert len(meters.SemsegMeter("PASCALContext").cat_names) == 21 and len(meters.SemsegMeter("NYUD").cat_names) == 40
    assert meters.HumanPartsMeter("PASCALContext").n_classes == 7
    with pytest.raises(NotImplementedError):
        meters.SemsegMeter("ADE20K")
    with pytest.raises(AssertionError):
        meters.HumanPartsMeter("NYUD")
    with pytest.raises(NotImplementedError):
        meters.get_single_task_meter({}, "NYUD", "flow")
    with pytest.raises(ValueError):
        meters.get_output(torch.zeros(1, 1, 2, 2), "flow")
    assert np.array_equal(meters.SaliencyMeter().mask_thres, np.linspace(0.2, 0.9, 15))

    class P(dict):
        pass
    p = P(train_db_name="NYUD", edge_w=0.95)
    p.TASKS = P()
    p.TASKS.NAMES = ["semseg", "depth", "normals", "edge", "sal"]
    pm = meters.PerformanceMeter(p)
    assert [type(pm.meters[t]).__name__ for t in pm.tasks] == ["SemsegMeter", "DepthMeter", "NormalsMeter", "EdgeMeter", "SaliencyMeter"]
    assert pm.meters["edge"].pos_weight == 0.95 and pm.meters["semseg"].n_classes == 40
    pm2 = meters.PerformanceMeter(["semseg", "human_parts"], "PASCALContext")
    assert pm2.database == "PASCALContext" and pm2.meters["semseg"].n_classes == 21
    pm3 = meters.PerformanceMeter({"train_db_name": "NYUD", "TASKS": {"NAMES": ["depth"]}})
    assert list(pm3.meters) == ["depth"]
    # no update yet: the reference's division by zero becomes NaN, the IoU's max(.., 1e-8) denominator gives 0
    sc = pm.get_score(verbose=False)
    assert sc["semseg"]["mIoU"] == 0.0 and all(np.isnan(sc[t][k]) for t, k in (("depth", "rmse"), ("normals", "mean"), ("edge", "loss")))
    assert isinstance(_lib.M3Error("x"), Exception)


@pytest.mark.parametrize("task", ["semseg", "human_parts", "depth", "normals", "sal", "edge"])
def test_cpu_tensors_and_post_processed_predictions_are_refused(task):
    """no eager fallback: a CPU tensor raises before anything else is looked at (so this runs without a GPU); so does the wrapper
    around one"""
    from m3vit_amd import _lib, meters
    m = meters.get_single_task_meter({"edge_w": 0.95}, "PASCALContext", task)
    kind = MC.TASK_KIND[task]
    pred, label = MC.make_inputs(kind, 7 if kind == "iou" else MC.KIND_C[kind], (2, 3, 7))
    for x in (pred, meters.get_output(pred, task)):
        with pytest.raises(_lib.M3Error, match="GPU"):
            m.update(x, label)
    with pytest.raises(_lib.M3Error):
        m.update(meters.get_output(pred, "depth" if task != "depth" else "sal"), label)
    with pytest.raises(_lib.M3Error):
        meters.AverageMeter("loss").update(torch.tensor(1.0))
    with pytest.raises(_lib.M3Error):
        meters.AverageMeter("loss").update(1.0)


def test_calculate_multi_task_performance(g13):
    from m3vit_amd import meters
    ev, st = json.loads(str(g13["mtl/eval"])), json.loads(str(g13["mtl/single"]))
    assert close(meters.calculate_multi_task_performance(ev, st), g13["mtl/value"])
    two = {k: ev[k] for k in ("semseg", "depth")}
    assert close(meters.calculate_multi_task_performance(two, {k: st[k] for k in two}),
                 ((0.41 - 0.40) / 0.40 - (0.62 - 0.60) / 0.60) / 2)
    with pytest.raises(AssertionError):
        meters.calculate_multi_task_performance(ev, two)
    with pytest.raises(NotImplementedError):
        meters.calculate_multi_task_performance({"flow": {}}, {"flow": {}})
