"""GPU: the task-metric kernels (csrc/meter.hip) through ops and the meter classes of m3vit_amd.meters.

Every count is compared exactly and every float sum inside the bounds derived in tests/meter_cases.py (the ones
test_meters_cpu.py holds torch's fp32 evaluation to), against the float64 restatement on the dtype-rounded inputs and directly
against the reference's own numbers in tests/golden/g13_meters.npz.  The state and the partials workspace are guarded
allocations, the workspace starts poisoned; pred and label keep their bits."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_cases as LC                                           # noqa: E402
import meter_cases as MC                                          # noqa: E402
from kernel_contract import guarded, guarded_ws, same_bits, snapshot, unchanged   # noqa: E402

pytestmark = pytest.mark.gpu
G13 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_meters.npz")
_dt = lambda d: str(d).split(".")[-1]                             # noqa: E731
_sz = lambda s: "x".join(map(str, s))                             # noqa: E731


@pytest.fixture(scope="module")
def g13():
    return np.load(G13)


def place(pred, dtype, layout, odd=False):
    """pred (CPU float32 NCHW) on the GPU in `dtype` and `layout`; odd: its storage starts one element into an allocation, so
    no pointer of it is 16-byte aligned and every kernel takes its scalar path"""
    x = LC.as_layout(pred.to(dtype), layout).cuda()
    if odd:
        buf = torch.empty(x.numel() + 1, dtype=dtype, device="cuda")
        v = torch.as_strided(buf, x.shape, x.stride(), 1)
        v.copy_(x)
        assert v.data_ptr() % 16 != 0
        x = v
    return x


def inputs(kind, C, size, dtype, seed=0, **kw):
    """(pred as float32 holding `dtype`-representable values, label), settled on the rounded values"""
    pred, label = MC.make_inputs(kind, C, size, seed=seed, **kw)
    return MC.settle(kind, pred.to(dtype).float(), label)


class Meter:
    """one kernel family on a guarded, zeroed state; update() hands every call a freshly poisoned, guarded workspace"""

    def __init__(self, kind, n_classes=None):
        from m3vit_amd import _lib, meters, ops
        self.kind, self.ncls = kind, n_classes
        if kind == "edge":
            self.edge = meters.EdgeMeter(MC.EDGE_W)
            return
        self.code = {"iou": _lib.M3_METER_IOU, "depth": _lib.M3_METER_DEPTH, "normals": _lib.M3_METER_NORMALS, "sal": _lib.M3_METER_SAL}[kind]
        s2, self.s_check = guarded(1, ops.METER_WORDS[self.code], torch.int64)
        self.state = s2.view(-1)
        self.state.zero_()

    def update(self, x, label, label_dtype=None):
        from m3vit_amd import ops
        lab = label.cuda() if label_dtype is None else label.to(label_dtype).cuda()
        snap = snapshot(pred=x, label=lab)
        if self.kind == "edge":
            self.edge.update(x, lab)
        else:
            aux = {"iou": self.ncls, "sal": x.shape[0]}.get(self.kind, 0)
            need = ops.meter_ws_elems(self.code, x.numel(), aux)
            ws, ws_check = guarded_ws(need, torch.int32)
            if self.kind == "iou":
                ops.meter_iou_update(x, lab, self.ncls, ws=ws, state=self.state)
            else:
                getattr(ops, f"meter_{self.kind}_update")(x, lab, ws=ws, state=self.state)
            torch.cuda.synchronize()
            ws_check(); self.s_check(what="state")
        unchanged(snap)
        return self

    def bits(self):
        return (self.edge.state if self.kind == "edge" else self.state).clone()

    def read(self):
        """(ints, sums) in meter_cases.Accumulated's order"""
        from m3vit_amd import _lib as L
        if self.kind == "edge":
            s, n = self.edge.state.cpu().tolist()
            return np.array([int(n)]), np.array([s])
        w = self.state.cpu()
        i, f = w.numpy(), w.view(torch.float64).numpy()
        if self.kind == "iou":
            n = self.ncls
            tp, pr, lb = (i[o:o + L.M3_METER_IOU_BINS] for o in (L.M3_METER_IOU_TP, L.M3_METER_IOU_PRED, L.M3_METER_IOU_LABEL))
            assert not tp[n:].any() and not pr[n:].any() and not lb[n:].any(), "bins past n_classes were written"
            return np.stack([tp[:n], pr[:n] - tp[:n], lb[:n] - tp[:n]]), np.zeros(0)
        if self.kind == "depth":
            return i[L.M3_METER_DEPTH_N_VALID:L.M3_METER_DEPTH_N_VALID + 1].copy(), f[:2].copy()
        if self.kind == "normals":
            return i[L.M3_METER_NORMALS_N_11:L.M3_METER_NORMALS_N + 1].copy(), f[:2].copy()
        return i[L.M3_METER_SAL_N_IMAGES:L.M3_METER_SAL_N_IMAGES + 1].copy(), f[:45].copy()


def expect(kind, x, label, n_classes=None, acc=None):
    """the float64 restatement on x's own (rounded) values, added to acc"""
    x64 = x.double()
    r = MC.reference(kind, x64, label.cuda(), n_classes)
    return (acc or MC.Accumulated(kind)).add(r, MC.bounds(kind, r, x64))


def same_score(a, b):
    """two get_score dictionaries from the same accumulators: equal but for the last bit of a square root or a power"""
    return set(a) == set(b) and all(np.allclose(a[k], b[k], rtol=1e-14, atol=0, equal_nan=True) for k in a)


def agree(got, acc, what):
    ints, sums = got
    assert np.array_equal(ints, acc.ints), f"{what}: counts {ints.tolist()} != {acc.ints.tolist()}"
    err = np.abs(sums - acc.sums)
    ratio = float((err / np.maximum(acc.bounds, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: worst err / bound {ratio:.3g}")
    assert bool((err <= acc.bounds).all()) and bool(np.isfinite(sums).all()), f"{what}: sums {sums} ref {acc.sums} bound {acc.bounds}"


# -------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("dtype", MC.DTYPES, ids=_dt)
@pytest.mark.parametrize("layout", MC.LAYOUTS)
@pytest.mark.parametrize("case", MC.cases(), ids=MC.case_id)
def test_values_guards_and_same_bits(case, layout, dtype):
    kind, C, size = case
    pred, label = inputs(kind, C, size, dtype)
    x = place(pred, dtype, layout)
    a = Meter(kind, C).update(x, label)
    agree(a.read(), expect(kind, x, label, C), f"{MC.case_id(case)} {layout} {_dt(dtype)}")
    assert same_bits(a.bits(), Meter(kind, C).update(x, label).bits())            # two runs: the same bits
    if kind == "iou":                                                              # the label dtypes: the same counts
        for ld in (torch.int64, torch.uint8):
            assert same_bits(a.bits(), Meter(kind, C).update(x, label, label_dtype=ld).bits()), ld


@pytest.mark.parametrize("layout", MC.LAYOUTS)
@pytest.mark.parametrize("key", [f[0] for f in MC.FIXTURES])
def test_against_the_recorded_reference_directly(g13, key, layout):
    """the reference's own accumulators after one and two updates, no restatement in between, through the meter CLASSES and
    get_output's wrapper; get_score is the reference's arithmetic on the state (exact for the count-only meters)"""
    from m3vit_amd import meters
    _, task, db, C, size = next(f for f in MC.FIXTURES if f[0] == key)
    kind = MC.TASK_KIND[task]
    m = meters.get_single_task_meter({"edge_w": MC.EDGE_W}, db or "NYUD", task)
    bound = 0.0
    for u in (0, 1):
        pred, label = torch.from_numpy(g13[f"{key}/pred{u}"]), torch.from_numpy(g13[f"{key}/label{u}"])
        x = place(pred, torch.float32, layout)
        m.update(meters.get_output(x, task), label.cuda())
        a = lambda name: g13[f"{key}/acc{u}/{name}"]               # noqa: E731
        r = MC.reference(kind, x.double(), label.cuda(), getattr(m, "n_classes", None))
        bound = bound + MC.bounds(kind, r, x.double())
        sc = m.get_score(verbose=False)
        want = {k.split("/")[-1]: g13[k] for k in g13.files if k.startswith(f"{key}/score{u}/")}
        assert set(sc) == set(want)
        w = m.state.cpu()
        i, f = w.numpy(), (w if kind == "edge" else w.view(torch.float64)).numpy()
        if kind == "iou":
            tp, fp, fn = m.counts()
            assert np.array_equal(tp, a("tp")) and np.array_equal(fp, a("fp")) and np.array_equal(fn, a("fn"))
            assert sc["jaccards_all_categs"] == want["jaccards_all_categs"].tolist() and sc["mIoU"] == float(want["mIoU"])
        elif kind == "depth":
            assert i[2] == a("n_valid") and abs(f[0] - a("total_rmses")) <= bound[0] and abs(f[1] - a("total_log_rmses")) <= bound[1]
            assert same_score(sc, MC.score(kind, i[2:3], f[:2]))
            assert abs(sc["rmse"] - want["rmse"]) <= bound[0] / (2 * want["rmse"] * i[2]) * 1.01
        elif kind == "normals":
            assert i[5] == a("n") and [v * 100 for v in i[2:5]] == [a("11.25"), a("22.5"), a("30")]
            assert abs(f[0] - a("mean")) <= bound[0] and abs(f[1] - a("rmse")) <= bound[1]
            assert same_score(sc, MC.score(kind, i[2:6], f[:2])) and all(sc[k] == float(want[k]) for k in ("11.25", "22.5", "30"))
            assert abs(sc["mean"] - want["mean"]) <= bound[0] / i[5]
        elif kind == "sal":
            assert i[45] == 2 * (u + 1)
            for k, v in want.items():
                assert np.allclose(sc[k], v, rtol=1e-12, atol=0), k
        else:
            assert f[1] == a("n") and abs(f[0] - a("loss")) <= 2 * bound[0]        # the reference's own fp32 loss carries the bound once more
            assert abs(sc["loss"] - want["loss"]) <= 2 * bound[0] / f[1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=_dt)
@pytest.mark.parametrize("layout", MC.LAYOUTS)
@pytest.mark.parametrize("case", [("iou", 40, (2, 3, 7)), ("iou", 7, (1, 5, 65)), ("iou", 20, (3, 16, 33)), ("depth", 1, (3, 17, 33)),
                                  ("normals", 3, (3, 17, 33)), ("sal", 1, (3, 16, 33)), ("edge", 1, (3, 17, 33))], ids=MC.case_id)
def test_odd_storage_offset_takes_the_scalar_path(case, layout, dtype):
    kind, C, size = case
    pred, label = inputs(kind, C, size, dtype)
    x = place(pred, dtype, layout, odd=True)
    agree(Meter(kind, C).update(x, label).read(), expect(kind, x, label, C), f"odd {MC.case_id(case)} {layout} {_dt(dtype)}")


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd"])
@pytest.mark.parametrize("layout", MC.LAYOUTS)
@pytest.mark.parametrize("case", MC.multi_pass_cases(), ids=MC.case_id)
def test_more_than_one_pass_of_the_capped_grid(case, layout, odd):
    """every kernel's grid-stride loop goes round more than once, with a partial last pass (meter_cases.multi_pass_cases says
    which case is sized for which kernel).  fp32 pred: the loops are the same code for every dtype."""
    kind, C, size = case
    pred, label = inputs(kind, C, size, torch.float32)
    x = place(pred, torch.float32, layout, odd=odd)
    a = Meter(kind, C).update(x, label)
    agree(a.read(), expect(kind, x, label, C), f"multi-pass {MC.case_id(case)} {layout} odd={odd}")
    assert same_bits(a.bits(), Meter(kind, C).update(x, label).bits())


@pytest.mark.parametrize("dtype", MC.DTYPES, ids=_dt)
@pytest.mark.parametrize("size", [(2, 3, 7), (3, 17, 33)], ids=_sz)
@pytest.mark.parametrize("C", MC.GROUP_CLASSES)
def test_channels_last_group_sizes(C, size, dtype):
    """the 16-byte channels-last kernel with 1, 2, 4, 8, 32 and 64 lanes per pixel (16: C = 40 of the case table): each level of
    the group reduction, the DPP ones and the two shuffles - with int64 labels, on the vector path"""
    pred, label = inputs("iou", C, size, dtype)
    x = place(pred, dtype, "nhwc")
    agree(Meter("iou", C).update(x, label, label_dtype=torch.int64).read(), expect("iou", x, label, C), f"groups C{C} {size} {_dt(dtype)}")


@pytest.mark.parametrize("layout", MC.LAYOUTS)
@pytest.mark.parametrize("special", MC.special_iou_cases(), ids=lambda s: s[0])
def test_iou_labels_ties_and_nans(special, layout):
    name, pred, label, ncls, want = special
    for dtype in MC.DTYPES:
        for odd in (False, True):
            x = place(pred, dtype, layout, odd=odd)
            got = Meter("iou", ncls).update(x, label).read()
            agree(got, expect("iou", x, label, ncls), f"{name} {layout} {_dt(dtype)} odd={odd}")
            if want is not None:
                assert not got[0].any()
    if name == "ties-lowest-index":
        assert got[0][:2, 1].sum() > 0 and got[0][:2, 4].sum() == 0 and got[0][:2, 6].sum() == 0
    if name == "labels-that-are-no-class":                        # the four pixels count as fp of their predictions
        clean = label.clone()
        clean.view(-1)[[0, 9, 20, 33]] = MC.IGNORE
        ref = Meter("iou", ncls).update(x, clean).read()[0]
        assert (got[0][1] - ref[1]).sum() == 4 and np.array_equal(got[0][0], ref[0]) and np.array_equal(got[0][2], ref[2])


# ------------------------------------------------------------------------------------------- accumulation, reset, empties
@pytest.mark.parametrize("layout", MC.LAYOUTS)
@pytest.mark.parametrize("kind", MC.KINDS)
def test_updates_accumulate_an_empty_one_changes_nothing_and_reset_zeroes(kind, layout):
    """two and three updates of different shapes on one state against the summed restatement; an update whose every label is
    ignored in between leaves the bits as they were; the same sequence twice gives the same bits; reset() gives zeros"""
    from m3vit_amd import meters
    C = 21 if kind == "iou" else MC.KIND_C[kind]
    seq = [(2, 3, 7), (3, 17, 33), (1, 5, 65)]
    runs = []
    for _ in range(2):
        m, acc = Meter(kind, C), None
        for k, size in enumerate(seq):
            pred, label = inputs(kind, C, size, torch.float32, seed=40 + k)
            x = place(pred, torch.float32, layout)
            m.update(x, label)
            acc = expect(kind, x, label, C, acc)
            if k >= 1:
                agree(m.read(), acc, f"{kind} {layout} after {k + 1} updates")
            if k == 1 and kind in ("iou", "depth", "normals"):
                before = m.bits()
                m.update(x, torch.full_like(label, float(MC.IGNORE)))
                assert same_bits(before, m.bits()), "an all-ignored update changed the state"
        runs.append(m.bits())
    assert same_bits(*runs)
    task = {"iou": "semseg", "edge": "edge"}.get(kind, kind)
    cm = meters.get_single_task_meter({"edge_w": MC.EDGE_W}, "PASCALContext", task)
    cm.reset()                                                    # before any update: nothing to do
    cm.update(x, label.cuda())
    assert bool(cm.state.any())
    cm.reset()
    assert not bool(cm.state.any())
    cm.update(x, label.cuda()); cm.update(x, label.cuda()); cm.reset(); cm.update(x, label.cuda())
    if kind == "iou":
        agree((np.stack(cm.counts()), np.zeros(0)), expect(kind, x, label, 21), "after reset")


def test_score_of_nothing_valid_is_nan_as_the_reference_divides():
    from m3vit_amd import meters
    for task, keys in (("depth", ("rmse", "log_rmse")), ("normals", ("mean", "rmse", "11.25"))):
        kind = MC.TASK_KIND[task]
        pred, label = inputs(kind, MC.KIND_C[kind], (2, 3, 7), torch.float32)
        m = meters.get_single_task_meter({}, "NYUD", task)
        m.update(place(pred, torch.float32, "nchw"), torch.full_like(label, float(MC.IGNORE)).cuda())
        sc = m.get_score(verbose=False)
        assert all(math.isnan(sc[k]) for k in keys)


def test_saliency_runs_a_single_image_and_refused_inputs_raise():
    from m3vit_amd import _lib, meters
    pred, label = inputs("sal", 1, (1, 9, 11), torch.float32)
    m = meters.SaliencyMeter()
    m.update(place(pred, torch.float32, "nchw"), label.cuda())
    r = MC.sal_ref(pred.double(), label)
    sc = m.get_score(verbose=False)
    assert np.allclose(sc["mIoUs"], r["sums"][0].numpy(), rtol=1e-12, atol=0) and sc["mIoU"] == max(sc["mIoUs"])
    sem = meters.SemsegMeter("NYUD")
    x, lab = torch.randn(2, 40, 3, 7, device="cuda"), torch.zeros(2, 1, 3, 7, device="cuda")
    for bad in (x.argmax(1), x.permute(0, 2, 3, 1), x.argmax(1, keepdim=True)):            # the reference's post-processed forms
        with pytest.raises(_lib.M3Error, match="RAW"):
            sem.update(bad, lab)
    with pytest.raises(_lib.M3Error):
        meters.DepthMeter().update(torch.rand(2, 3, 7, 1, device="cuda"), torch.rand(2, 1, 3, 7, device="cuda"))
    with pytest.raises(_lib.M3Error):
        meters.NormalsMeter().update(x, lab)
    with pytest.raises(_lib.M3Error):
        sem.update(x, lab.double())
    with pytest.raises(_lib.M3Error):
        meters.DepthMeter().update(torch.rand(2, 1, 3, 7, device="cuda"), torch.ones(2, 1, 3, 7, dtype=torch.int64, device="cuda"))
    assert sem.state is None or not bool(sem.state.any())


def test_average_meter_accumulates_on_the_device():
    from m3vit_amd import meters
    am = meters.AverageMeter("Loss semseg", ":.4e")
    assert am.count == 0 and math.isnan(am.avg)
    vals = [torch.tensor(v, device="cuda") for v in (0.5, 2.0, 4.25)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for v in vals:
            am.update(v)
        am.update(vals[0].half(), n=2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert (am.sum, am.count, am.val, am.avg) == (7.75, 5.0, 0.5, 1.55)
    assert str(am) == "Loss semseg 5.0000e-01 (1.5500e+00)"
    am.reset()
    assert am.count == 0 and am.sum == 0


# -------------------------------------------------------------------------------------------------------- no host read
TASKS3 = ["semseg", "depth", "normals"]


def _three(size, seed, dtype=torch.float32, ignore_frac=0.2):
    out, gt = {}, {}
    for t, C in (("semseg", 40), ("depth", 1), ("normals", 3)):
        pred, label = inputs(MC.TASK_KIND[t], C, size, dtype, seed=seed, ignore_frac=ignore_frac)
        out[t], gt[t] = place(pred, dtype, "nhwc"), label.cuda()
    return out, gt


def _states(pm):
    return {t: pm.meters[t].state.clone() for t in pm.tasks}


def test_performance_meter_update_reads_nothing_back():
    """PerformanceMeter.update for (semseg, depth, normals), the reference's call line, under set_sync_debug_mode("error"): any
    .item(), masked_select or host copy inside would raise.  Where this torch build does not honour the mode (a probe .item()
    under it does not raise) only that claim is left out - the reason is printed - and the rest runs all the same."""
    from m3vit_amd import meters
    pm = meters.PerformanceMeter(TASKS3, "NYUD")
    out, gt = _three((3, 17, 33), 50)
    pm.update({t: meters.get_output(out[t], t) for t in TASKS3}, gt)      # warm-up: library load, the one-time allocations
    pm.reset()
    torch.cuda.synchronize()
    probe = torch.ones((), device="cuda")
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
        for _ in range(2):
            pm.update({t: meters.get_output(out[t], t) for t in TASKS3}, gt)
        pm.reset()
        pm.update({t: meters.get_output(out[t], t) for t in TASKS3}, gt)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for t, C in (("semseg", 40), ("depth", 1), ("normals", 3)):
        kind = MC.TASK_KIND[t]
        fresh = Meter(kind, C).update(out[t], gt[t])
        assert same_bits(pm.meters[t].state, fresh.bits()), t
    sc = pm.get_score(verbose=False)
    assert set(sc) == set(TASKS3) and 0 <= sc["semseg"]["mIoU"] <= 1 and sc["depth"]["rmse"] > 0 and 0 < sc["normals"]["mean"] < 180


def test_captured_graph_follows_the_labels_in_place():
    """the same three-task update captured in a graph and replayed after the labels - and the predictions - were overwritten in
    place: the state then holds the eager result of the first inputs plus that of the second, bit for bit as a fresh eager meter
    run over the same two updates - nothing of the capture-time call was baked in on the host"""
    from m3vit_amd import meters, ops
    size = (3, 17, 33)
    out, gt = _three(size, 60)
    pm = meters.PerformanceMeter(TASKS3, "NYUD")
    call = lambda: pm.update({t: meters.get_output(out[t], t) for t in TASKS3}, gt)   # noqa: E731
    call()                                                        # warm-up outside the capture
    pm.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.graph_capture(g):
        call()
    pm.reset()
    first = {t: (out[t].clone(), gt[t].clone()) for t in TASKS3}
    g.replay()
    out2, gt2 = _three(size, 61, ignore_frac=0.7)
    for t in TASKS3:
        out[t].copy_(out2[t]); gt[t].copy_(gt2[t])                # in place: the captured pointers stay
    g.replay()
    torch.cuda.synchronize()
    eager = meters.PerformanceMeter(TASKS3, "NYUD")
    eager.update({t: first[t][0] for t in TASKS3}, {t: first[t][1] for t in TASKS3})
    eager.update(out2, gt2)
    for t in TASKS3:
        assert same_bits(pm.meters[t].state, eager.meters[t].state), t
    acc = expect("iou", first["semseg"][0], first["semseg"][1].cpu(), 40)
    acc = expect("iou", out2["semseg"], gt2["semseg"].cpu(), 40, acc)
    agree((np.stack(pm.meters["semseg"].counts()), np.zeros(0)), acc, "replayed semseg")


def test_model_to_performance_meter_end_to_end():
    """MultiTaskModel (tiny backbone, two heads) -> get_output's wrapper -> PerformanceMeter, the reference's evaluation loop:
    the scores equal the reference arithmetic on the float64 restatement of the model's own outputs"""
    from m3vit_amd import meters
    from m3vit_amd.heads import MultiTaskModel, VisionTransformerUpHead
    from m3vit_amd.vit import VisionTransformerMoE
    torch.manual_seed(8)
    kw = dict(img_size=(32, 48), embed_dim=64, depth=2, num_heads=2, moe_experts=4, moe_top_k=2, gate_dim=66, multi_gate=True)
    bb = VisionTransformerMoE(mlp_ratio=4.0, moe_mlp_ratio=1, vmoe_noisy_std=0, **kw)
    tasks = ["semseg", "depth"]
    heads = torch.nn.ModuleDict({"semseg": VisionTransformerUpHead((32, 48), 16, 64, num_classes=40),
                                 "depth": VisionTransformerUpHead((32, 48), 16, 64, num_classes=1, num_conv=2, num_upsampe_layer=2)})
    m = MultiTaskModel(bb, heads, tasks, multi_gate=True).cuda().eval()
    _, sem = MC.make_inputs("iou", 40, (2, 32, 48), seed=11)
    _, dep = MC.make_inputs("depth", 1, (2, 32, 48), seed=11)
    gt = {"semseg": sem.cuda(), "depth": dep.cuda()}
    pm = meters.PerformanceMeter({"train_db_name": "NYUD", "TASKS": {"NAMES": tasks}})
    accs = {}
    with torch.no_grad():
        for seed in (1, 2):
            x = torch.randn(2, 3, 32, 48, device="cuda", generator=torch.Generator("cuda").manual_seed(seed))
            output = m(x)
            output = output[0] if isinstance(output, tuple) else output
            pm.update({t: meters.get_output(output[t], t) for t in tasks}, gt)
            for t in tasks:
                accs[t] = expect(MC.TASK_KIND[t], output[t], gt[t].cpu(), 40 if t == "semseg" else None, accs.get(t))
    sc = pm.get_score(verbose=False)
    assert same_score(sc["semseg"], MC.score("iou", accs["semseg"].ints, accs["semseg"].sums))
    want = MC.score("depth", accs["depth"].ints, accs["depth"].sums)
    n = accs["depth"].ints[0]
    assert abs(sc["depth"]["rmse"] - want["rmse"]) <= accs["depth"].bounds[0] / (2 * want["rmse"] * n) * 1.01
    assert abs(sc["depth"]["log_rmse"] - want["log_rmse"]) <= accs["depth"].bounds[1] / (2 * want["log_rmse"] * n) * 1.01
