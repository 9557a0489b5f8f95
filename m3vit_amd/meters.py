"""Drop-in task meters over the HIP metric kernels (csrc/meter.hip): the names and constructor signatures of the reference's
evaluation/evaluate_utils.py (PerformanceMeter, get_single_task_meter, calculate_multi_task_performance), its meter classes
(evaluation/eval_semseg.py, eval_human_parts.py, eval_depth.py, eval_normals.py, eval_sal.py, eval_edge.py) and
utils/utils.py (get_output, AverageMeter), so that the reference's call line

    performance_meter.update({t: get_output(output[t], t) for t in tasks}, targets)

runs unchanged - with no host read.  update() takes the RAW head output [B,C,H,W] (or what this module's get_output returns:
a wrapper around the raw tensor that computes nothing); argmax / clamp / normalise / sigmoid happen inside the kernels, which
ADD to a device-resident state (meter.state: int64 counts and double sums, layout in include/m3vit_hip.h).  Nothing is
synchronised or allocated per step, so update() can be captured in a graph.  get_score() makes ONE device-to-host copy per meter
and then does the reference's host arithmetic (the max(.., 1e-8) IoU denominator included), with the reference's keys.

Differences from the reference, all on purpose:
  * a plain tensor in the reference's post-processed form (an argmax map, an NHWC 0..255 copy) is refused with M3Error; CPU
    tensors raise M3Error: there is no eager fallback;
  * DepthMeter.reset() really resets (the reference's resets two attributes nothing uses);
  * NormalsMeter.update does not overwrite the caller's label tensor in place, and get_output's 0..255 round trip of the
    normals (fp32 rounding only) is not reproduced;
  * SaliencyMeter keeps running sums over the images, not the per-image arrays: all_jaccards / prec / rec are not returned;
    B = 1 works (the reference's squeeze() breaks it); counts are exact integers where numpy sums a float32 (the same below
    2^24 pixels per image);
  * an update whose every label is ignored leaves the state unchanged; get_score then divides as the reference does, a
    ZeroDivisionError becoming NaN;
  * AverageMeter.update takes a 0-dim device tensor and accumulates on the device; .val / .avg / .sum / .count read lazily.
Several processes: the states are ordinary device tensors of sums (the saliency ones too) - all_reduce(meter.state view) is the
caller's; see INTEGRATION.md.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, ops

__all__ = ["SemsegMeter", "HumanPartsMeter", "DepthMeter", "NormalsMeter", "SaliencyMeter", "EdgeMeter", "AverageMeter",
           "PerformanceMeter", "get_single_task_meter", "calculate_multi_task_performance", "get_output", "MeterInput"]

TASKS = ("semseg", "human_parts", "depth", "normals", "sal", "edge")

VOC_CATEGORY_NAMES = ["background", "aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow",
                      "diningtable", "dog", "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor"]
NYU_CATEGORY_NAMES = ["wall", "floor", "cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf", "picture",
                      "counter", "blinds", "desk", "shelves", "curtain", "dresser", "pillow", "mirror", "floor mat", "clothes",
                      "ceiling", "books", "refridgerator", "television", "paper", "towel", "shower curtain", "box", "whiteboard",
                      "person", "night stand", "toilet", "sink", "lamp", "bathtub", "bag", "otherstructure", "otherfurniture",
                      "otherprop"]
PART_CATEGORY_NAMES = ["background", "head", "torso", "uarm", "larm", "uleg", "lleg"]
# database -> (classes, background class in front, names); CityScapes: the reference's 7-class table
SEMSEG_TABLE = {"PASCALContext": (20, True, VOC_CATEGORY_NAMES), "NYUD": (40, False, NYU_CATEGORY_NAMES),
                "CityScapes": (7, False, NYU_CATEGORY_NAMES[:7])}


class MeterInput:
    """what get_output returns: the raw head output and its task, nothing computed"""
    __slots__ = ("raw", "task")

    def __init__(self, raw, task):
        self.raw, self.task = raw, task


def get_output(output, task):
    """utils/utils.py:60-79 for the meters of this module: detaches and wraps the raw [B,C,H,W] output; the task's transform
    runs inside the meter's kernel"""
    if task not in TASKS:
        raise ValueError("Select one of the valid tasks")
    if not isinstance(output, torch.Tensor):
        raise _lib.M3Error(f"get_output takes the head's output tensor, got {type(output).__name__}")
    return MeterInput(output.detach(), task)


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        return float("nan")


class _DeviceMeter:
    """the device-resident state of one meter, its workspace per pred shape, and the lazy host copy"""
    KIND = None
    TASKS = ()
    CHANNELS = None                                  # the C of pred this meter takes; None: any (class logits)

    def __init__(self):
        self._state = None
        self._ws = {}

    @property
    def state(self):
        """the accumulator (int64 words; .view(torch.float64) for the sums), None before the first update"""
        return self._state

    def reset(self):
        if self._state is not None:
            self._state.zero_()                      # a memset on the current stream

    def _raw(self, pred, gt):
        if isinstance(pred, MeterInput):
            if pred.task not in self.TASKS:
                raise _lib.M3Error(f"{type(self).__name__} was handed get_output(.., {pred.task!r})")
            pred = pred.raw
        if not isinstance(pred, torch.Tensor) or not isinstance(gt, torch.Tensor):
            raise _lib.M3Error(f"{type(self).__name__}.update takes tensors (pred: the raw head output or get_output's wrapper)")
        if not pred.is_cuda or not gt.is_cuda:
            raise _lib.M3Error(f"{type(self).__name__}.update: pred and gt must live on the GPU (no CPU path)")
        ok = (pred.dim() == 4 and gt.dim() == 4 and pred.dtype.is_floating_point and pred.shape[0] == gt.shape[0]
              and pred.shape[2:] == gt.shape[2:] and (self.CHANNELS is None or pred.shape[1] == self.CHANNELS))
        if not ok:
            raise _lib.M3Error(
                f"{type(self).__name__}.update takes the RAW head output [B, C, H, W] (floating point"
                f"{'' if self.CHANNELS is None else f', C = {self.CHANNELS}'}) next to gt {tuple(gt.shape)}, got {pred.dtype} "
                f"{tuple(pred.shape)}: the reference's post-processed form (argmax map, NHWC or 0..255 copy) is not read - "
                f"pass the head output itself or this module's get_output(output, task)")
        return pred

    def _bufs(self, pred, aux=0):
        if self._state is None:
            self._state = ops.meter_state(self.KIND, pred.device)
        key = (tuple(pred.shape), pred.device)
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = torch.empty(ops.meter_ws_elems(self.KIND, pred.numel(), aux), dtype=torch.int32, device=pred.device)
        return ws

    def _host(self):
        """(int64 words, the same words as float64) - ONE device-to-host copy"""
        w = torch.zeros(ops.METER_WORDS[self.KIND], dtype=torch.int64) if self._state is None else self._state.cpu()
        return w.numpy(), w.view(torch.float64).numpy()


class _ClassIoUMeter(_DeviceMeter):
    KIND = _lib.M3_METER_IOU
    TITLE = ""

    def __init__(self, n_classes, cat_names):
        super().__init__()
        self.n_classes = n_classes
        self.cat_names = cat_names

    @torch.no_grad()
    def update(self, pred, gt):
        pred = self._raw(pred, gt)
        ops.meter_iou_update(pred, gt, self.n_classes, ws=self._bufs(pred, self.n_classes), state=self._state)

    def counts(self):
        """(tp, fp, fn) as int64 arrays [n_classes] - one device-to-host copy"""
        w, _ = self._host()
        n = self.n_classes
        tp = w[_lib.M3_METER_IOU_TP:_lib.M3_METER_IOU_TP + n]
        return tp, w[_lib.M3_METER_IOU_PRED:_lib.M3_METER_IOU_PRED + n] - tp, w[_lib.M3_METER_IOU_LABEL:_lib.M3_METER_IOU_LABEL + n] - tp

    def get_score(self, verbose=True):
        tp, fp, fn = self.counts()
        jac = [float(tp[i]) / max(float(tp[i] + fp[i] + fn[i]), 1e-8) for i in range(self.n_classes)]
        eval_result = {"jaccards_all_categs": jac, "mIoU": np.mean(jac)}
        if verbose:
            print("\n{0:s} mIoU: {1:.4f}\n".format(self.TITLE, 100 * eval_result["mIoU"]))
            for name, v in zip(self.cat_names, jac):
                print("{0:<20s}{1:.4f}".format(name, 100 * v))
        return eval_result


class SemsegMeter(_ClassIoUMeter):
    """per-class tp / fp / fn of the argmax over the pixels with gt != 255 (eval_semseg.py:83-146)"""
    TASKS = ("semseg",)
    TITLE = "Semantic Segmentation"

    def __init__(self, database):
        if database not in SEMSEG_TABLE:
            raise NotImplementedError(f"SemsegMeter: no class table for database {database!r}")
        n, has_bg, names = SEMSEG_TABLE[database]
        super().__init__(n + int(has_bg), names)
        self.database = database


class HumanPartsMeter(_ClassIoUMeter):
    """the same counts over background + 6 parts (eval_human_parts.py:78-122)"""
    TASKS = ("human_parts",)
    TITLE = "Human Parts"

    def __init__(self, database):
        assert database == "PASCALContext"
        super().__init__(7, PART_CATEGORY_NAMES)
        self.database = database
        self.n_parts = 6


class DepthMeter(_DeviceMeter):
    """rmse and log-rmse over gt != 255 with pred clamped to >= 1e-9 (eval_depth.py:61-104)"""
    KIND = _lib.M3_METER_DEPTH
    TASKS = ("depth",)
    CHANNELS = 1

    @torch.no_grad()
    def update(self, pred, gt):
        pred = self._raw(pred, gt)
        ops.meter_depth_update(pred, gt, ws=self._bufs(pred), state=self._state)

    def get_score(self, verbose=True):
        w, f = self._host()
        n = float(w[_lib.M3_METER_DEPTH_N_VALID])
        eval_result = {"rmse": math.sqrt(_div(float(f[_lib.M3_METER_DEPTH_SUM_SQ]), n)),
                       "log_rmse": math.sqrt(_div(float(f[_lib.M3_METER_DEPTH_SUM_LOG_SQ]), n))}
        if verbose:
            print("Results for depth prediction")
            for k, v in eval_result.items():
                print("{0:<15s}{1:.4f}".format(k, v))
        return eval_result


class NormalsMeter(_DeviceMeter):
    """angular error in degrees over the pixels whose label is valid (eval_normals.py:68-115)"""
    KIND = _lib.M3_METER_NORMALS
    TASKS = ("normals",)
    CHANNELS = 3

    @torch.no_grad()
    def update(self, pred, gt):
        pred = self._raw(pred, gt)
        ops.meter_normals_update(pred, gt, ws=self._bufs(pred), state=self._state)

    def get_score(self, verbose=True):
        w, f = self._host()
        n = int(w[_lib.M3_METER_NORMALS_N])
        eval_result = {"mean": _div(float(f[_lib.M3_METER_NORMALS_SUM_ANGLE]), n),
                       "rmse": _div(float(f[_lib.M3_METER_NORMALS_SUM_SQ]), n) ** 0.5,
                       "11.25": _div(float(w[_lib.M3_METER_NORMALS_N_11]) * 100, n),
                       "22.5": _div(float(w[_lib.M3_METER_NORMALS_N_22]) * 100, n),
                       "30": _div(float(w[_lib.M3_METER_NORMALS_N_30]) * 100, n)}
        if verbose:
            print("Results for Surface Normal Estimation")
            for k, v in eval_result.items():
                print("{0:<15s}{1:.4f}".format(k, v))
        return eval_result


class SaliencyMeter(_DeviceMeter):
    """jaccard, precision and recall per image at 15 thresholds of sigmoid(pred), averaged over the images; the maximum over
    the thresholds (eval_sal.py:68-131)"""
    KIND = _lib.M3_METER_SAL
    TASKS = ("sal",)
    CHANNELS = 1

    def __init__(self):
        super().__init__()
        self.mask_thres = np.linspace(0.2, 0.9, _lib.M3_METER_SAL_THRESHOLDS)

    @torch.no_grad()
    def update(self, pred, gt):
        pred = self._raw(pred, gt)
        ops.meter_sal_update(pred, gt, ws=self._bufs(pred, pred.shape[0]), state=self._state)

    def get_score(self, verbose=True):
        w, f = self._host()
        nt = _lib.M3_METER_SAL_THRESHOLDS
        n = float(w[_lib.M3_METER_SAL_N_IMAGES])
        with np.errstate(divide="ignore", invalid="ignore"):
            miou, mprec, mrec = (f[o:o + nt] / n for o in (_lib.M3_METER_SAL_JACCARD, _lib.M3_METER_SAL_PREC, _lib.M3_METER_SAL_REC))
            fscore = 2 * mprec * mrec / (mprec + mrec + 1e-12)
        eval_result = {"mIoUs": miou.tolist(), "mPrec": mprec.tolist(), "mRec": mrec.tolist(), "F": fscore.tolist(),
                       "mIoU": float(np.max(miou)), "maxF": float(np.max(fscore))}
        if verbose:
            print("Results for Saliency Estimation")
            print("mIoU: {0:.3f}".format(100 * eval_result["mIoU"]))
            print("maxF: {0:.3f}".format(100 * eval_result["maxF"]))
        return eval_result


class EdgeMeter:
    """the balanced BCE of sigmoid(pred) FED IN AS A LOGIT, as the reference does (eval_edge.py:14-40: its update hands the
    probability to BalancedCrossEntropyLoss), weighted by the element count.  state: float64 [2] = (sum of numel * loss, sum of
    numel), added to on the device."""
    TASKS = ("edge",)
    CHANNELS = 1

    def __init__(self, pos_weight):
        self.pos_weight = pos_weight
        self._state = None
        self._bufs = {}

    @property
    def state(self):
        return self._state

    def reset(self):
        if self._state is not None:
            self._state.zero_()

    @torch.no_grad()
    def update(self, pred, gt):
        pred = _DeviceMeter._raw(self, pred, gt)
        if pred.shape[1] != 1 or gt.shape != pred.shape:
            raise _lib.M3Error(f"EdgeMeter.update takes pred and gt of shape [B, 1, H, W], got {tuple(pred.shape)} and {tuple(gt.shape)}")
        if self._state is None:
            self._state = torch.zeros(2, dtype=torch.float64, device=pred.device)
        key = (tuple(pred.shape), pred.dtype, pred.device)
        if key not in self._bufs:
            self._bufs[key] = (torch.empty(pred.shape, dtype=torch.float32, device=pred.device),
                               torch.empty(ops.loss_ws_elems(pred.numel()), dtype=torch.float32, device=pred.device),
                               torch.empty(ops.LOSS_REC_WORDS, dtype=torch.int32, device=pred.device))
        prob, ws, rec = self._bufs[key]
        prob.copy_(pred.contiguous())
        torch.sigmoid_(prob)
        ops.loss_bce_fwd(prob, gt.contiguous(), self.pos_weight, ws=ws, record=rec)
        numel = pred.numel()
        self._state[0:1].add_(rec[_lib.M3_LOSS_REC_VALUE:_lib.M3_LOSS_REC_VALUE + 1].view(torch.float32).double(), alpha=numel)
        self._state[1:2].add_(numel)

    def get_score(self, verbose=True):
        s, n = (0.0, 0.0) if self._state is None else self._state.cpu().tolist()
        eval_dict = {"loss": _div(s, n)}
        if verbose:
            print("\n Edge Detection Evaluation")
            print("Edge Detection Loss %.3f" % (eval_dict["loss"]))
        return eval_dict


class AverageMeter:
    """utils/utils.py:20-40 with the sum and the count on the device: update(value) takes a 0-dim GPU tensor (a loss) and reads
    nothing back; .val, .avg, .sum and .count copy the three words to the host when asked"""

    def __init__(self, name, fmt=":f"):
        self.name = name
        self.fmt = fmt
        self._state = None                           # float64 [3]: sum, count, last value

    def reset(self):
        if self._state is not None:
            self._state.zero_()

    @torch.no_grad()
    def update(self, val, n=1):
        if not isinstance(val, torch.Tensor) or not val.is_cuda or val.numel() != 1:
            raise _lib.M3Error("AverageMeter.update takes a 0-dim GPU tensor (no .item() on the way in)")
        if self._state is None:
            self._state = torch.zeros(3, dtype=torch.float64, device=val.device)
        v = val.detach().reshape(1).double()
        self._state[0:1].add_(v, alpha=n)
        self._state[1:2].add_(n)
        self._state[2:3].copy_(v)

    @property
    def state(self):
        return self._state

    def _host(self):
        return (0.0, 0.0, 0.0) if self._state is None else tuple(self._state.cpu().tolist())

    sum = property(lambda self: self._host()[0])
    count = property(lambda self: self._host()[1])
    val = property(lambda self: self._host()[2])

    @property
    def avg(self):
        s, c, _ = self._host()
        return _div(s, c)

    def __str__(self):
        s, c, v = self._host()
        fmtstr = "{name} {val" + self.fmt + "} ({avg" + self.fmt + "})"
        return fmtstr.format(name=self.name, val=v, avg=_div(s, c))


def get_single_task_meter(p, database, task):
    """the meter of one task (evaluate_utils.py:74-101); p is read only for p['edge_w']"""
    if task == "semseg":
        return SemsegMeter(database)
    if task == "human_parts":
        return HumanPartsMeter(database)
    if task == "normals":
        return NormalsMeter()
    if task == "sal":
        return SaliencyMeter()
    if task == "depth":
        return DepthMeter()
    if task == "edge":
        return EdgeMeter(pos_weight=p["edge_w"])
    raise NotImplementedError(f"no meter for task {task!r}")


class PerformanceMeter:
    """one meter per task (evaluate_utils.py:17-42).  PerformanceMeter(p) reads p['train_db_name'] and p.TASKS.NAMES (or
    p['TASKS']['NAMES']); PerformanceMeter(tasks, database, edge_w=None) takes them directly."""

    def __init__(self, p, database=None, edge_w=None):
        if database is None:
            self.database = p["train_db_name"]
            self.tasks = list(p.TASKS.NAMES if hasattr(p, "TASKS") else p["TASKS"]["NAMES"])
        else:
            self.database = database
            self.tasks = list(p)
            p = {"edge_w": edge_w}
        self.meters = {t: get_single_task_meter(p, self.database, t) for t in self.tasks}

    def reset(self):
        for t in self.tasks:
            self.meters[t].reset()

    def update(self, pred, gt):
        for t in (pred.keys() if len(pred.keys()) < len(self.tasks) else self.tasks):
            self.meters[t].update(pred[t], gt[t])

    def get_score(self, verbose=True):
        return {t: self.meters[t].get_score(verbose) for t in self.tasks}


# task -> (the key compared, +1 where higher is better)
_MTL_KEY = {"depth": ("rmse", -1), "semseg": ("mIoU", 1), "sal": ("mIoU", 1), "human_parts": ("mIoU", 1), "normals": ("mean", -1),
            "edge": ("odsF", 1)}


def calculate_multi_task_performance(eval_dict, single_task_dict):
    """the mean over the tasks of the signed relative difference to the single-task results (evaluate_utils.py:45-70)"""
    assert set(eval_dict.keys()) == set(single_task_dict.keys())
    total = 0.0
    for task in eval_dict:
        if task not in _MTL_KEY:
            raise NotImplementedError(task)
        key, sign = _MTL_KEY[task]
        total += sign * (eval_dict[task][key] - single_task_dict[task][key]) / single_task_dict[task][key]
    return total / len(eval_dict)
