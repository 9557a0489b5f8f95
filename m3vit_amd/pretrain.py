"""The recipe around an ImageNet pretraining step, on the device (csrc/pretrain.hip): Mixup / CutMix with label smoothing, the
soft-target / label-smoothing cross-entropy, the evaluation meter and the weight EMA, under the names and constructor
signatures pretrain/train.py uses (:461-471, 498, 536, 877-905), so that its call lines work with their imports swapped
(INTEGRATION.md section 3).  The reference takes these four pieces from `timm`; here they are restated from their published
formulas and checked against float64 closed forms (tests/pretrain_cases.py), not against `timm`.

Differences from the reference, all on purpose:
  * nothing reads the device in a step: no .item() for logging (DistillationLoss.last_stats holds device scalars that convert
    when read), no "loss is not finite" test (pretrain_step leaves it to the caller; the GradScaler's overflow skip still
    protects the weights), evaluation sums live in a device state (ClsEvalMeter);
  * a label outside [0, C) indexes nothing and is counted (last_bad_labels, read lazily) where torch hits a device assert;
  * ModelEma keeps fp32 shadow TENSORS keyed by state_dict() names, not a deep copy of the module: a MoEViTForImageNet carries
    executor contexts and captured graphs that must not be copied.  It has neither `.module` nor `.ema`, so
    pretrain/utils/checkpoint.py:20-39 falls back to its state_dict() / load_state_dict();
  * CPU tensors raise M3Error: there is no eager fallback.
Distillation (DistillationLoss 'soft' / 'hard', pretrain/models/losses.py:50-68) runs with a distilled model
(MoEViTConfig(distilled=True)) and a teacher module the caller supplies.
Not here: cutmix_minmax, RandomErasing, RandAugment, building a teacher, a CPU-resident EMA.
"""
from __future__ import annotations

import contextlib
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from .functional import DistillLossFn, SoftCrossEntropyFn

__all__ = ["Mixup", "SoftTargetCrossEntropy", "LabelSmoothingCrossEntropy", "CrossEntropy", "DistillationLoss",
           "build_criterion", "ClsEvalMeter", "ModelEma", "pretrain_step"]


# ------------------------------------------------------------------------------------------------------------ mixing
class Mixup:
    """Mixup / CutMix of a batch with its batch-reversed self, and the label-smoothed soft target of the same pairing
    (train.py:461-471; applied at train_one_epoch.py:32-33).  __call__(x, target) -> (x_mixed, soft_target [B, C]): x float32
    [B, C, H, W] on the GPU is mixed IN PLACE and returned (with out_dtype: a new tensor of that activation dtype, x untouched),
    target int64 [B].

    The parameters are drawn on the host with numpy.random in draw() - no device read - and reach the device in one
    non-blocking copy; tests pin or bypass draw().  Per batch (mode 'batch'), per sample ('elem') or per pair ('pair': sample
    B-1-i takes the parameters of sample i): with probability `prob` mix, else lam = 1; with both alphas positive CutMix is
    chosen with probability switch_prob; lam ~ Beta(alpha, alpha) of the chosen kind.  CutMix box: ratio = sqrt(1 - lam), size
    int(H ratio) x int(W ratio), centred at a uniform integer point of the image, every edge clipped to the image; with
    correct_lam, lam = 1 - box_area / (H W).  A CutMix draw whose box comes out empty exchanges no pixel and sets lam = 1.

    The host random stream was written from the description of timm.data.Mixup; it could not be compared with timm, which
    is not available here: the same seed need not give timm's draws.  cutmix_minmax is refused."""

    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch',
                 correct_lam=True, label_smoothing=0.1, num_classes=1000, out_dtype=None):
        if cutmix_minmax is not None:
            raise NotImplementedError("Mixup: cutmix_minmax is not supported")
        if mode not in ("batch", "pair", "elem"):
            raise ValueError(f"Mixup: mode must be 'batch', 'pair' or 'elem', got {mode!r}")
        if mixup_alpha < 0 or cutmix_alpha < 0 or not (mixup_alpha > 0 or cutmix_alpha > 0):
            raise ValueError("Mixup: one of mixup_alpha / cutmix_alpha must be positive, neither negative")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.mix_prob, self.switch_prob = float(prob), float(switch_prob)
        self.mode, self.correct_lam = mode, bool(correct_lam)
        self.label_smoothing, self.num_classes = float(label_smoothing), int(num_classes)
        self.out_dtype = out_dtype
        self.mixup_enabled = True
        self.last_bad = None

    def _draw_one(self, H, W):
        """(lam, yl, yh, xl, xh) of one decision"""
        if not self.mixup_enabled or not np.random.rand() < self.mix_prob:
            return 1.0, 0, 0, 0, 0
        cut = self.cutmix_alpha > 0 and (self.mixup_alpha <= 0 or np.random.rand() < self.switch_prob)
        a = self.cutmix_alpha if cut else self.mixup_alpha
        lam = float(np.random.beta(a, a))
        if not cut:
            return lam, 0, 0, 0, 0
        ratio = math.sqrt(1.0 - lam)
        ch, cw = int(H * ratio), int(W * ratio)
        cy, cx = int(np.random.randint(0, H)), int(np.random.randint(0, W))
        yl, yh = min(max(cy - ch // 2, 0), H), min(max(cy + ch // 2, 0), H)
        xl, xh = min(max(cx - cw // 2, 0), W), min(max(cx + cw // 2, 0), W)
        area = (yh - yl) * (xh - xl)
        if area == 0:
            return 1.0, 0, 0, 0, 0
        if self.correct_lam:
            lam = 1.0 - area / float(H * W)
        return lam, yl, yh, xl, xh

    def draw(self, B, H, W):
        """(lam float32 [B], box int32 [B, 4] = yl, yh, xl, xh) as numpy arrays; an empty box (all zeros) means Mixup"""
        if B < 2 or B % 2:
            raise ValueError(f"Mixup pairs sample i with B-1-i: the batch size must be even, got {B}")
        lam, box = np.ones(B, dtype=np.float32), np.zeros((B, 4), dtype=np.int32)
        if self.mode == "batch":
            d = self._draw_one(H, W)
            lam[:], box[:] = d[0], d[1:]
        elif self.mode == "pair":
            for i in range(B // 2):
                d = self._draw_one(H, W)
                lam[i] = lam[B - 1 - i] = d[0]
                box[i] = box[B - 1 - i] = d[1:]
        else:
            for i in range(B):
                d = self._draw_one(H, W)
                lam[i], box[i] = d[0], d[1:]
        return lam, box

    def __call__(self, x, target, out_dtype=None):
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise _lib.M3Error("Mixup: x must be a [B, C, H, W] tensor")
        B, _, H, W = x.shape
        lam, box = self.draw(B, H, W)
        # one pinned buffer, one non-blocking copy: lam's bits in front of the boxes
        host = torch.empty(5 * B, dtype=torch.int32).pin_memory()
        host[:B] = torch.from_numpy(np.ascontiguousarray(lam, dtype=np.float32)).view(torch.int32)
        host[B:] = torch.from_numpy(np.ascontiguousarray(box, dtype=np.int32)).reshape(-1)
        dev = host.to(x.device, non_blocking=True)
        lam_d, box_d = dev[:B].view(torch.float32), dev[B:]
        out = ops.mix_batch(x, lam_d, box_d, out_dtype=out_dtype or self.out_dtype)
        soft, self.last_bad = ops.mix_target(target, lam_d, self.num_classes, self.label_smoothing)
        return out, soft

    @property
    def last_bad_labels(self):
        """labels of the last call outside [0, num_classes); reads the device when called"""
        return None if self.last_bad is None else int(self.last_bad.item())


# --------------------------------------------------------------------------------------------------------- criteria
class _SoftCE(nn.Module):
    smoothing = 0.0

    def __init__(self):
        super().__init__()
        self._record = None

    def forward(self, x, target):
        loss, self._record = SoftCrossEntropyFn.apply(x, target, self.smoothing)
        return loss

    @property
    def last_bad_labels(self):
        """labels of the last forward outside [0, C) (hard labels only); reads the device when called"""
        return None if self._record is None else int(self._record[_lib.M3_LOSS_REC_N_BAD].item())


class SoftTargetCrossEntropy(_SoftCE):
    """mean over the batch of sum(-target * log_softmax(x)); x [B, C] fp32 / fp16 / bf16, target float32 [B, C]"""

    def forward(self, x, target):
        if target.dtype != torch.float32:
            raise _lib.M3Error(f"SoftTargetCrossEntropy takes a dense float32 target [B, C], got {target.dtype}")
        return super().forward(x, target)


class LabelSmoothingCrossEntropy(_SoftCE):
    """(1 - smoothing) * nll + smoothing * mean(-log_softmax(x)), mean over the batch; target int64 [B]"""

    def __init__(self, smoothing=0.1):
        super().__init__()
        if not 0.0 <= smoothing < 1.0:
            raise ValueError(f"smoothing must be in [0, 1), got {smoothing}")
        self.smoothing = float(smoothing)
        self.confidence = 1.0 - self.smoothing

    def forward(self, x, target):
        if target.dtype != torch.int64:
            raise _lib.M3Error(f"LabelSmoothingCrossEntropy takes int64 labels [B], got {target.dtype}")
        return super().forward(x, target)


class CrossEntropy(LabelSmoothingCrossEntropy):
    """nn.CrossEntropyLoss() over [B, C] logits and int64 labels (mean reduction, no class weights, no ignore_index)"""

    def __init__(self):
        super().__init__(smoothing=0.0)


class DistillationLoss(nn.Module):
    """pretrain/models/losses.py:8-74.  forward(inputs, outputs, labels): 'none' -> base_criterion(outputs, labels); 'soft' /
    'hard' -> base * (1 - alpha) + distill * alpha, where outputs is the (class logits, distillation logits) pair a distilled
    model returns in training, the teacher runs on `inputs` under no_grad and the teacher term is one kernel pair
    (m3_loss_distill_fwd / _bwd: KL at temperature tau scaled tau^2 / numel, or cross-entropy against the teacher's argmax).
    The teacher is any nn.Module that maps the inputs to [B, C] logits on the GPU (fp32, fp16 or bf16).
    last_stats keeps the reference's keys (loss_base, loss_distill, loss_no_cv); the losses in it are 0-dim DEVICE tensors
    that become floats when a reader converts them (float(v), a logger's .item()) - the reference calls .item() every step.
    'soft' / 'hard' without a teacher is refused here; the reference would fail at the first forward, on None(inputs)."""

    def __init__(self, base_criterion, teacher_model, distillation_type, alpha, tau):
        super().__init__()
        if distillation_type not in ("none", "soft", "hard"):
            raise ValueError(f"DistillationLoss: distillation_type must be 'none', 'soft' or 'hard', got {distillation_type!r}")
        if distillation_type != "none" and teacher_model is None:
            raise NotImplementedError(f"DistillationLoss: distillation_type {distillation_type!r} needs a teacher_model; "
                                      "building one (timm.create_model) is the caller's")
        self.base_criterion = base_criterion
        self.teacher_model = teacher_model
        self.distillation_type = distillation_type
        self.alpha = alpha
        self.tau = tau
        self.last_stats = {}

    def forward(self, inputs, outputs, labels):
        outputs_kd = None
        if isinstance(outputs, tuple):
            outputs, outputs_kd = outputs
        base_loss = self.base_criterion(outputs, labels)
        if self.distillation_type == "none":
            d = base_loss.detach()
            self.last_stats = {"loss_base": d, "loss_distill": 0.0, "loss_no_cv": d}
            return base_loss
        if outputs_kd is None:
            raise ValueError("Distillation is enabled but model did not return distillation logits. "
                             "Either disable distillation or add a distillation head.")
        with torch.no_grad():
            teacher_outputs = self.teacher_model(inputs)
        distill_loss, _ = DistillLossFn.apply(outputs_kd, teacher_outputs, self.distillation_type, float(self.tau))
        total = base_loss * (1 - self.alpha) + distill_loss * self.alpha
        self.last_stats = {"loss_base": base_loss.detach(), "loss_distill": distill_loss.detach(), "loss_no_cv": total.detach()}
        return total


def build_criterion(args, teacher_model=None):
    """pretrain/models/losses.py:77-91: SoftTargetCrossEntropy when mixing is on, else LabelSmoothingCrossEntropy, else plain
    cross-entropy - wrapped in DistillationLoss"""
    if args.mixup > 0.0 or args.cutmix > 0.0 or getattr(args, "cutmix_minmax", None) is not None:
        base = SoftTargetCrossEntropy()
    elif args.smoothing > 0.0:
        base = LabelSmoothingCrossEntropy(smoothing=args.smoothing)
    else:
        base = CrossEntropy()
    return DistillationLoss(base_criterion=base, teacher_model=teacher_model,
                            distillation_type=getattr(args, "distillation_type", "none"),
                            alpha=getattr(args, "distillation_alpha", 0.5), tau=getattr(args, "distillation_tau", 1.0))


# ------------------------------------------------------------------------------------------------------- evaluation
class ClsEvalMeter:
    """The sums of pretrain/engine/evaluate.py:29-55 in a device-resident state.  update(logits, target) adds one batch and
    reads nothing back; `state` is the float64 [4] tensor [loss_sum, correct1, correct5, count] evaluate.py:44-50 all-reduces
    (reduce it across ranks yourself, in place); get() makes ONE copy and returns {"loss", "acc1", "acc5"}."""

    def __init__(self, device="cuda"):
        self._words = ops.cls_eval_state(device)
        self._ws = None

    @property
    def state(self):
        return self._words[:4].view(torch.float64)

    @property
    def bad_labels(self):
        """labels outside [0, C) seen so far (counted, never correct); reads the device when called"""
        return int(self._words[_lib.M3_CLS_EVAL_N_BAD].item())

    def reset(self):
        self._words.zero_()

    @torch.no_grad()
    def update(self, logits, target):
        need = ops.cls_eval_ws_elems(logits.shape[0]) if logits.dim() == 2 else 0
        if self._ws is None or self._ws.numel() < need or self._ws.device != logits.device:
            self._ws = torch.empty(max(need, 1), dtype=torch.int32, device=logits.device)
        ops.cls_eval_update(logits.detach().contiguous(), target, ws=self._ws, state=self._words)

    def get(self):
        return self.result(self.state.cpu().tolist())

    @staticmethod
    def result(state):
        """evaluate.py:52-55 on [loss_sum, correct1, correct5, count]"""
        loss_sum, c1, c5, count = (float(v) for v in state)
        count = max(count, 1.0)
        return {"loss": loss_sum / count, "acc1": 100.0 * c1 / count, "acc5": 100.0 * c5 / count}


# -------------------------------------------------------------------------------------------------------------- EMA
class ModelEma:
    """Exponential moving average of a model's state_dict() entries (train.py:536; updated at train_one_epoch.py:62-63):
    ema = decay * ema + (1 - decay) * value for every float32 entry in ONE launch (m3_ema_update); every other entry
    (integer buffers, other float dtypes) is copied.  The shadows are float32 tensors keyed by state_dict() names - the
    module is never copied.  The descriptor table is rebuilt only when a source tensor's pointer changed."""

    def __init__(self, model, decay=0.9999, device=None):
        if device is not None and torch.device(device).type != "cuda":
            raise NotImplementedError("ModelEma: a CPU-resident EMA is not supported; the shadows live beside the model")
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"decay must be in [0, 1], got {decay}")
        self.decay = float(decay)
        self.device = None if device is None else torch.device(device)
        self.shadow = {}
        with torch.no_grad():
            for k, v in model.state_dict().items():
                if not v.is_cuda:
                    raise _lib.M3Error(f"ModelEma: {k} lives on {v.device}; move the model to the GPU first")
                self.shadow[k] = v.detach().to(self.device or v.device, copy=True).contiguous()
        self._src, self._src_of, self._sig, self._table = None, None, None, None

    def _sources(self, model):
        if self._src_of is not model:
            src = model.state_dict(keep_vars=True)          # the parameters / buffers themselves: their pointers are the signature
            if list(src) != list(self.shadow):
                raise KeyError("ModelEma: the model's state_dict() keys differ from the ones the EMA was built from")
            self._src, self._src_of, self._sig = list(src.values()), model, None
        return self._src

    @torch.no_grad()
    def update(self, model):
        src = self._sources(model)
        sig = [t.data_ptr() for t in src]
        if sig != self._sig:
            pairs, self._copied = [], []
            for (k, e), s in zip(self.shadow.items(), src):
                if e.dtype == torch.float32 and s.dtype == torch.float32 and s.is_contiguous() and s.numel() > 0:
                    pairs.append((e, s.detach()))
                else:
                    self._copied.append((e, s))
            self._pairs = pairs                              # keeps the tensors the table points at alive
            self._table = ops.ema_table(pairs) if pairs else None
            self._sig = sig
        if self._table is not None:
            ops.ema_update(*self._table, self.decay)
        for e, s in self._copied:
            e.copy_(s)

    def state_dict(self):
        return dict(self.shadow)

    def load_state_dict(self, state_dict, strict=True):
        missing = [k for k in self.shadow if k not in state_dict]
        extra = [k for k in state_dict if k not in self.shadow]
        if strict and (missing or extra):
            raise KeyError(f"ModelEma.load_state_dict: missing {missing[:5]}, unexpected {extra[:5]}")
        with torch.no_grad():
            for k, e in self.shadow.items():
                if k in state_dict:
                    e.copy_(state_dict[k])                   # in place: the descriptor table keeps pointing at the shadows

    @torch.no_grad()
    def copy_to(self, model):
        """the EMA values into the model's own tensors (device-side copies).  The in-place copies bump the parameters'
        version counters, which is how FusedBackbone learns that its operand copies are stale."""
        for e, s in zip(self.shadow.values(), self._sources(model)):
            s.copy_(e)

    @contextlib.contextmanager
    def applied(self, model):
        """`with ema.applied(model): evaluate(...)`: the EMA weights inside the block, the originals (bit for bit) after it"""
        src = self._sources(model)
        with torch.no_grad():
            saved = [s.detach().clone() for s in src]
        self.copy_to(model)
        try:
            yield model
        finally:
            with torch.no_grad():
                for s, o in zip(src, saved):
                    s.copy_(o)


# ------------------------------------------------------------------------------------------------------------- step
def pretrain_step(model, criterion, optimizer, scaler, samples, targets, mixup_fn=None, model_ema=None, moe_cv_weight=0.01,
                  clip_grad=None):
    """The body of pretrain/engine/train_one_epoch.py:32-63 without its host reads: mix, forward,
    criterion(samples, logits, targets), + moe_cv_weight * cv, scaler.scale(loss).backward(), scaler.step, scaler.update,
    model_ema.update.  Returns (loss, cv) as device tensors (cv None for a model without one).

    The reference's "loss is not finite: stop" test needs a host read and is the caller's (read the returned loss when you
    log); the GradScaler's overflow skip still keeps a non-finite step away from the weights.  Meant for
    FusedAdamW(max_grad_norm=clip_grad), which clips inside its step; with another optimizer and clip_grad set this falls back
    to scaler.unscale_ + clip_grad_norm_, as cls.amp_train_step does."""
    if mixup_fn is not None:
        samples, targets = mixup_fn(samples, targets)
    out = model(samples)
    logits = out["logits"] if isinstance(out, dict) else out
    cv_loss = out.get("cv_loss", None) if isinstance(out, dict) else None
    loss = criterion(samples, logits, targets)
    cv = None
    if cv_loss is not None:
        cv = cv_loss.mean() if torch.is_tensor(cv_loss) else torch.tensor(float(cv_loss), device=samples.device)
        loss = loss + moe_cv_weight * cv
    optimizer.zero_grad(set_to_none=True)
    scaler.scale(loss).backward()
    if clip_grad is not None and getattr(optimizer, "max_grad_norm", None) is None:
        scaler.unscale_(optimizer)
        torch.nn.utils.clip_grad_norm_(model.parameters(), clip_grad)
    scaler.step(optimizer)
    scaler.update()
    if model_ema is not None:
        model_ema.update(model)
    return loss.detach(), (cv.detach() if cv is not None else None)
