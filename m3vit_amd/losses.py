"""Drop-in criterion modules over the HIP loss kernels (csrc/loss.hip): the names and constructor signatures of the
reference's losses/loss_functions.py and losses/loss_schemes.py:10-115, and get_loss with the task -> loss table of
utils/common_config.py:780-807.

Differences from the reference, all on purpose:
  * no host read anywhere in a forward or backward: no .item(), no masked_select, no `if torch.any(torch.isnan(..))`.  Where
    the reference replaces a NaN loss by 0 after a host-side test, torch.nan_to_num(.., nan=0.0) is applied unconditionally:
    the value is the same;
  * a class label that is neither 255 nor in [0, C) is ignored and counted (SoftMaxwithLoss.last_bad_labels, read lazily)
    where the reference hits a device assert;
  * BalancedCrossEntropyLoss takes no void_pixels (NotImplementedError) and only size_average=True; NormalsLoss only
    normalize=True, size_average=True; constructors do not print;
  * CPU tensors raise M3Error: there is no eager fallback.
PADNetLoss, JTRLLoss, MTINetLoss and BinaryCrossEntropyLoss serve models and setups this package does not have.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from .functional import BalancedBCEFn, MaskedL1Fn, NormalsLossFn, SoftmaxCrossEntropyFn

__all__ = ["SoftMaxwithLoss", "BalancedCrossEntropyLoss", "DepthLoss", "NormalsLoss", "SingleTaskLoss", "MultiTaskLoss",
           "get_loss"]


class _RecordLoss(nn.Module):
    """keeps the device-resident record of the last forward; the host copies it only when somebody asks"""

    def __init__(self):
        super().__init__()
        self._record = None

    def last_record(self):
        """the last forward's record as a list of (loss, coef, coef2, n_valid, n_aux, n_bad) - ONE device-to-host copy"""
        if self._record is None:
            return None
        w = self._record.cpu()
        f = w[:3].view(torch.float32)
        return (float(f[0]), float(f[1]), float(f[2]), int(w[_lib.M3_LOSS_REC_N_VALID]), int(w[_lib.M3_LOSS_REC_N_AUX]),
                int(w[_lib.M3_LOSS_REC_N_BAD]))


class SoftMaxwithLoss(_RecordLoss):
    """Pixel-wise softmax cross-entropy, mean over the pixels whose label is not 255 (loss_functions.py:16-33).
    out [B,C,H,W] (2 <= C <= 255), label [B,1,H,W] float32 / int64 / uint8."""

    def forward(self, out, label):
        assert not label.requires_grad
        loss, self._record = SoftmaxCrossEntropyFn.apply(out, label)
        return loss

    @property
    def last_bad_labels(self):
        """labels of the last forward that were neither 255 nor a class (ignored by the loss); reads the device when called"""
        r = self.last_record()
        return None if r is None else r[5]


class BalancedCrossEntropyLoss(_RecordLoss):
    """Balanced binary cross-entropy (loss_functions.py:36-84) with size_average=True."""

    def __init__(self, size_average=True, batch_average=True, pos_weight=None):
        super().__init__()
        if not size_average:
            raise NotImplementedError("BalancedCrossEntropyLoss: only size_average=True is built (what get_loss asks for)")
        self.size_average = size_average
        self.batch_average = batch_average
        self.pos_weight = pos_weight

    def forward(self, output, label, void_pixels=None):
        if void_pixels is not None:
            raise NotImplementedError("BalancedCrossEntropyLoss: void_pixels is not supported (no loss scheme passes it)")
        if output.size() != label.size():
            raise _lib.M3Error(f"output {tuple(output.shape)} and label {tuple(label.shape)} differ in shape")
        loss, self._record = BalancedBCEFn.apply(output, label, self.pos_weight)
        return loss


class DepthLoss(_RecordLoss):
    """L1 over the elements whose label is not 255 (loss_functions.py:126-140)."""

    def __init__(self, loss='l1'):
        super().__init__()
        if loss != 'l1':
            raise NotImplementedError('Loss {} currently not supported in DepthLoss'.format(loss))
        self.loss = loss

    def forward(self, out, label):
        loss, self._record = MaskedL1Fn.apply(out, label)
        return loss


class NormalsLoss(_RecordLoss):
    """L1 / L2 loss on normalised normals with ignore labels (loss_functions.py:143-197)."""

    def __init__(self, size_average=True, normalize=False, norm=1):
        super().__init__()
        if not (size_average and normalize):
            raise NotImplementedError("NormalsLoss: only normalize=True, size_average=True is built (what get_loss asks for)")
        if norm not in (1, 2):
            raise NotImplementedError
        self.size_average = size_average
        self.normalize = normalize
        self.norm = norm

    def forward(self, out, label, ignore_label=255):
        assert not label.requires_grad
        if ignore_label != 255:
            raise NotImplementedError("NormalsLoss: the ignore label is 255")
        loss, self._record = NormalsLossFn.apply(out, label, self.norm)
        return loss


def _no_nan(loss):
    return torch.nan_to_num(loss, nan=0.0)


class SingleTaskLoss(nn.Module):
    def __init__(self, loss_ft, task):
        super().__init__()
        self.loss_ft = loss_ft
        self.task = task

    def forward(self, pred, gt):
        out = {self.task: self.loss_ft(pred[self.task], gt[self.task])}
        out['total'] = out[self.task]
        return out


class MultiTaskLoss(nn.Module):
    """Fixed-weight sum of the task losses (loss_schemes.py:23-115): the plain branch (with single_task), the
    tam_level{0,1,2}_{task} branch MultiTaskModel produces, and the legacy tam_{task} branch.  Same keys, same total."""

    def __init__(self, tasks: list, loss_ft: nn.ModuleDict, loss_weights: dict, multi_level=False, p=None):
        super().__init__()
        assert set(tasks) == set(loss_ft.keys())
        assert set(tasks) == set(loss_weights.keys())
        self.tasks = tasks
        self.loss_ft = loss_ft
        self.loss_weights = loss_weights
        self.multi_level = multi_level
        if self.multi_level:                         # in place, as the reference: the caller's dictionary is divided
            for key in list(self.loss_weights):
                self.loss_weights[key] = self.loss_weights[key] / 4
        self.tam = bool(p['model_kwargs']['tam']) if (p is not None and 'model_kwargs' in p) else False

    def forward(self, pred, gt, single_task=None):
        if 'tam_%s' % (self.tasks[0]) in pred:
            total = 0.
            out = {}
            for prefix in ('tam_', ''):
                for task in self.tasks:
                    loss_ = self.loss_ft[task](pred[prefix + task], gt[task])
                    out[prefix + task] = loss_
                    total += self.loss_weights[task] * loss_
            out['total'] = total
            return out

        if self.tam:
            total = 0.
            out = {}
            for prefix in ('tam_level0_', 'tam_level1_', 'tam_level2_', ''):
                if prefix and prefix + self.tasks[0] not in pred:
                    continue
                for task in self.tasks:
                    loss_ = _no_nan(self.loss_ft[task](pred[prefix + task], gt[task]))
                    out[prefix + task] = loss_
                    total += self.loss_weights[task] * loss_
            out['total'] = total
            return out

        if single_task is None:
            out = {task: self.loss_ft[task](pred[task], gt[task]) for task in self.tasks}
            if 'human_parts' in out:
                out['human_parts'] = _no_nan(out['human_parts'])
            out['total'] = torch.sum(torch.stack([self.loss_weights[t] * out[t] for t in self.tasks]))
        else:
            out = {single_task: self.loss_ft[single_task](pred[single_task], gt[single_task])}
            out['total'] = self.loss_weights[single_task] * out[single_task]
        return out


def get_loss(p, task=None):
    """the loss of one task (utils/common_config.py:780-807)"""
    if task == 'edge':
        return BalancedCrossEntropyLoss(size_average=True, pos_weight=p['edge_w'])
    if task in ('semseg', 'human_parts'):
        return SoftMaxwithLoss()
    if task == 'normals':
        return NormalsLoss(normalize=True, size_average=True, norm=p['normloss'])
    if task == 'sal':
        return BalancedCrossEntropyLoss(size_average=True)
    if task == 'depth':
        return DepthLoss(p['depthloss'])
    raise NotImplementedError('Undefined Loss: Choose a task among edge, semseg, human_parts, sal, depth, or normals')
