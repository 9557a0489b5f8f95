"""The transform chain in front of a multi-task training step, on the device (csrc/augment.hip): what get_transformations
(utils/common_config.py:583-632) composes from data/custom_transforms.py - RandomHorizontalFlip, ScaleNRotate, FixedResize,
AddIgnoreRegions, ToTensor, Normalize - for every map of a raw batch in ONE launch.  The raw batch (uint8 image, label maps at
native size, [B, H, W, C] as a collate of the numpy samples gives them) is copied to the device once; the random parameters are
drawn on the host and follow in one pinned buffer; nothing is read back.

cv2 is not available here, so - like m3vit_amd.pretrain - this is restated from the published formulas (cv2.getRotationMatrix2D,
the half-pixel-centre resize, the Keys cubic with a = -0.75) and checked against float64 closed forms and torch's grid_sample
(tests/augment_cases.py), not against cv2 output.

Differences from the reference, all on purpose:
  * flip, warp and resize are composed into ONE resampling (the reference resamples twice when the sizes differ);
  * cv2's 1/32-pixel coordinate quantisation and its fixed-point nearest rounding are not reproduced: coordinates are exact
    doubles, nearest ties follow floor(u + 0.5);
  * ToTensor's astype(np.uint8) wraps an out-of-range cubic overshoot; here the value is clamped to [0, 255] first;
  * the list form's random.randint(0, len(rots)) can index past the list in the reference; here it is a uniform choice;
  * the host random stream need not match the reference's;
  * the human-parts rule "no part anywhere in the sample => the whole map 255" (custom_transforms.py:258-262) needs a
    reduction over the sample and is NOT built: a human_parts map is a plain `label`;
  * samples of different native size (PASCALContext) go one call per sample (B = 1);
  * CPU tensors raise M3Error: there is no eager fallback.
"""
from __future__ import annotations

import math
import random

import numpy as np
import torch

from . import _lib, ops

__all__ = ["BatchAugment", "AugmentParams", "affine_params", "rotation_matrix", "rotation_matrix_inv"]

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)       # common_config.py:619-620
# utils/config.py:27-91 (FLAGVALS, used by the train AND the test transforms) and :165-179 (TRAIN.SCALE = TEST.SCALE)
_TASK_MAPS = {"semseg": ("label", "nearest"), "human_parts": ("label", "nearest"), "sal": ("label", "nearest"),
              "edge": ("label", "nearest"), "depth": ("depth", "nearest"), "normals": ("normals", "cubic")}
_DB = {"NYUD": dict(rots=[0], scales=[1.0, 1.2, 1.5], size=(480, 640)),
       "CityScapes": dict(rots=[0], scales=[1.0, 1.2, 1.5], size=(128, 256)),
       "PASCALContext": dict(rots=(-20, 20), scales=(.75, 1.25), size=(512, 512))}


def affine_params(rot, sc, flip, size, out_size):
    """(A float64 [B, 6], aux float32 [B, 4]) of per-sample rotations (degrees), scales and flips for sources of size
    (H, W) resampled to out_size (Ho, Wo).  A = F . M^-1 . R maps an output pixel to source coordinates:
      M = cv2.getRotationMatrix2D((W / 2, H / 2), rot, sc) = [alpha, beta, (1 - alpha) cx - beta cy; -beta, alpha,
          beta cx + (1 - alpha) cy], alpha = sc cos, beta = sc sin - warpAffine reads the source at M^-1 (x, y);
      R: xr = (x + 0.5) W / Wo - 0.5 (half-pixel centres), exactly the identity for equal sizes;
      F: x -> W - 1 - x when flipped (the flip comes first in the chain, so it is the last map towards the source).
    aux = sc, cos(rot), sin(rot), flip.  rot 0, sc 1, no flip gives exactly the identity matrix."""
    H, W = size
    Ho, Wo = out_size
    rot = np.atleast_1d(np.asarray(rot, dtype=np.float64))
    sc = np.atleast_1d(np.asarray(sc, dtype=np.float64))
    flip = np.atleast_1d(np.asarray(flip)).astype(bool)
    B = rot.shape[0]
    if sc.shape != (B,) or flip.shape != (B,):
        raise ValueError("rot, sc and flip must have one entry per sample")
    if not bool((sc > 0).all()):
        raise ValueError("scales must be positive")
    rad = rot * (math.pi / 180.0)
    cos, sin = np.cos(rad), np.sin(rad)
    A = np.empty((B, 6), dtype=np.float64)
    sx, sy = W / Wo, H / Ho
    R = np.array([[sx, 0.0, 0.5 * sx - 0.5], [0.0, sy, 0.5 * sy - 0.5], [0.0, 0.0, 1.0]])
    for i in range(B):
        F = np.array([[-1.0, 0.0, W - 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) if flip[i] else np.eye(3)
        A[i] = _matmul3(F, _matmul3(rotation_matrix_inv(size, rot[i], sc[i]), R))[:2].reshape(6)
    aux = np.stack([sc, cos, sin, flip.astype(np.float64)], axis=1).astype(np.float32)
    return A, aux


def rotation_matrix(size, rot, sc):
    """cv2.getRotationMatrix2D((W / 2, H / 2), rot, sc) as a 3 x 3 float64 matrix (rot in degrees)"""
    H, W = size
    rad = float(rot) * (math.pi / 180.0)
    alpha, beta = sc * math.cos(rad), sc * math.sin(rad)
    cx, cy = W / 2.0, H / 2.0
    return np.array([[alpha, beta, (1.0 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1.0 - alpha) * cy],
                     [0.0, 0.0, 1.0]])


def rotation_matrix_inv(size, rot, sc):
    """the inverse of rotation_matrix in closed form: the linear part [alpha, beta; -beta, alpha] / (alpha^2 + beta^2)
    transposed, applied to (p - t)"""
    M = rotation_matrix(size, rot, sc)
    alpha, beta, tx, ty = M[0, 0], M[0, 1], M[0, 2], M[1, 2]
    det = alpha * alpha + beta * beta
    ia, ib = alpha / det, beta / det
    return np.array([[ia, -ib, -(ia * tx - ib * ty)], [ib, ia, -(ib * tx + ia * ty)], [0.0, 0.0, 1.0]])


def _matmul3(a, b):
    """3 x 3 product with plain sums of rounded products (no BLAS, no fused multiply-add): identity factors stay exact"""
    out = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            out[i, j] = (a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]
    return out + 0.0                                                       # -0 -> +0


class AugmentParams:
    """The per-sample parameters of one BatchAugment call on the device: one buffer of 8 B doubles - `mats` float64 [B, 6] in
    front, `aux` float32 [B, 4] behind it.  copy_(other) overwrites it in place (a captured call then replays with them)."""

    def __init__(self, buf, B):
        self.buf, self.B = buf, B
        self.mats = buf[:6 * B].view(B, 6)
        self.aux = buf[6 * B:].view(torch.float32).view(B, 4)

    @staticmethod
    def host(A, aux):
        """the pinned host buffer of (A [B, 6] float64, aux [B, 4] float32)"""
        B = A.shape[0]
        host = torch.empty(8 * B, dtype=torch.float64).pin_memory()
        host[:6 * B] = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float64)).reshape(-1)
        host[6 * B:].view(torch.float32)[:] = torch.from_numpy(np.ascontiguousarray(aux, dtype=np.float32)).reshape(-1)
        return host

    def copy_(self, other):
        src = other.buf if isinstance(other, AugmentParams) else other
        self.buf.copy_(src, non_blocking=True)
        return self


class BatchAugment:
    """maps = {name: (kind, mode)}: kind 'image' / 'label' / 'depth' / 'normals', mode 'nearest' / 'linear' / 'cubic'.
    __call__(batch) takes a dict of CUDA tensors - every name of `maps` as [B, H, W, C] or [B, H, W] (uint8 or float32, all of
    one B, H, W) - and returns a dict with each map as [B, C, Ho, Wo] (image: image_dtype, normalised with mean / std; the rest
    float32, ignore regions marked 255), the form model(images), MultiTaskLoss and PerformanceMeter.update take.  Entries of
    the batch that are no map (meta, bbox, ...) pass through untouched.

    rots / scales: a tuple is a continuous range with the reference's centred formulas, rot = (hi - lo) r - (hi - lo) / 2 and
    sc = (hi - lo) r - (hi - lo) / 2 + 1 (custom_transforms.py:35-41); a list is a uniform choice.  A human_parts map is a
    plain 'label': the "all zero => all 255" rule of the reference is not applied (see the module docstring).

    The output buffers are kept and reused while the shapes repeat, so a captured call replays onto the same storage - and a
    caller that keeps a result across calls must copy it."""

    def __init__(self, maps, out_size=None, rots=(0, 0), scales=(1.0, 1.0), flip_prob=0.5, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                 border="zero", image_dtype=torch.float32, quantize=True):
        if not maps:
            raise ValueError("BatchAugment: no maps")
        if type(rots) is not type(scales) or not isinstance(rots, (tuple, list)):
            raise ValueError("BatchAugment: rots and scales must both be tuples (ranges) or both be lists (choices)")
        if isinstance(rots, tuple) and (len(rots) != 2 or len(scales) != 2):
            raise ValueError("BatchAugment: a range is (lo, hi)")
        if isinstance(rots, list) and (not rots or not scales):
            raise ValueError("BatchAugment: an empty choice list")
        for name, (kind, mode) in maps.items():
            if kind not in ops.AUG_KINDS or mode not in ops.AUG_MODES:
                raise ValueError(f"BatchAugment: map {name!r}: unknown kind / mode {kind!r} / {mode!r}")
        if border not in ops.AUG_BORDERS:
            raise ValueError(f"BatchAugment: border must be 'zero' or 'replicate', got {border!r}")
        if not 0.0 <= flip_prob <= 1.0:
            raise ValueError("BatchAugment: flip_prob outside [0, 1]")
        self.maps = {k: tuple(v) for k, v in maps.items()}
        self.out_size = None if out_size is None else (int(out_size[0]), int(out_size[1]))
        self.rots, self.scales, self.flip_prob = rots, scales, float(flip_prob)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.border, self.image_dtype, self.quantize = border, image_dtype, bool(quantize)
        self._out = {}

    @classmethod
    def from_config(cls, db_name, tasks, train=True, out_size=None, **kw):
        """The transforms get_transformations builds for a dataset and its task names: NYUD and CityScapes rots [0], scales
        [1.0, 1.2, 1.5]; PASCALContext (-20, 20) and (.75, 1.25); image and normals cubic, the rest nearest (FLAGVALS); the
        dataset's TRAIN.SCALE as out_size.  train=False: the test transforms - no flip, no warp, the same modes, the resize of
        cv2.resize (border 'replicate')."""
        if db_name not in _DB:
            raise ValueError(f"Invalid train db name {db_name!r}")
        db = _DB[db_name]
        maps = {"image": ("image", "cubic")}
        for t in tasks:
            if t not in _TASK_MAPS:
                raise ValueError(f"unknown task {t!r}")
            maps[t] = _TASK_MAPS[t]
        size = db["size"] if out_size is None else out_size
        if train:
            return cls(maps, out_size=size, rots=db["rots"], scales=db["scales"], flip_prob=0.5, border="zero", **kw)
        return cls(maps, out_size=size, rots=[0], scales=[1.0], flip_prob=0.0, border="replicate", **kw)

    # ------------------------------------------------------------------------------------------------ parameters
    def _sizes(self, size):
        return size, (self.out_size or size)

    def draw_values(self, B):
        """(rot degrees [B], sc [B], flip bool [B]) from the host generators `random` and `numpy.random`"""
        rot, sc = np.empty(B), np.empty(B)
        for i in range(B):
            if isinstance(self.rots, tuple):
                dr, ds = self.rots[1] - self.rots[0], self.scales[1] - self.scales[0]
                rot[i] = dr * np.random.random() - dr / 2
                sc[i] = ds * np.random.random() - ds / 2 + 1
            else:
                rot[i], sc[i] = random.choice(self.rots), random.choice(self.scales)
        flip = np.random.random(B) < self.flip_prob
        return rot, sc, flip

    def params_from(self, rot, sc, flip, size=None, device="cuda"):
        """AugmentParams of explicit per-sample rotations (degrees), scales and flips for sources of size (H, W); size=None:
        the sources already have out_size (NYUD, CityScapes)"""
        if size is None and self.out_size is None:
            raise ValueError("BatchAugment: without out_size the source size must be given")
        size, out = self._sizes(size or self.out_size)
        A, aux = affine_params(rot, sc, flip, size, out)
        host = AugmentParams.host(A, aux)
        return AugmentParams(host.to(device, non_blocking=True), A.shape[0])

    def draw(self, B, size=None, device="cuda"):
        """AugmentParams of B fresh draws: one pinned buffer, one non-blocking copy, no device read"""
        return self.params_from(*self.draw_values(B), size=size, device=device)

    # ------------------------------------------------------------------------------------------------------ call
    def __call__(self, batch, params=None):
        srcs, shape = [], None
        for name in self.maps:
            if name not in batch:
                raise _lib.M3Error(f"BatchAugment: the batch has no {name!r}")
            t = batch[name]
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise _lib.M3Error(f"BatchAugment: {name!r} must be a GPU tensor (no CPU path)")
            if t.dim() not in (3, 4):
                raise _lib.M3Error(f"BatchAugment: {name!r} must be [B, H, W, C] or [B, H, W], got {tuple(t.shape)}")
            if shape is None:
                shape = tuple(t.shape[:3])
            elif tuple(t.shape[:3]) != shape:
                raise _lib.M3Error(f"BatchAugment: {name!r} is {tuple(t.shape[:3])}, the other maps {shape}: one B, H, W per call")
            srcs.append(t)
        B, H, W = shape
        (_, _), (Ho, Wo) = self._sizes((H, W))
        dev = srcs[0].device
        if params is None:
            params = self.draw(B, (H, W), dev)
        if params.B != B:
            raise _lib.M3Error(f"BatchAugment: parameters of {params.B} samples for a batch of {B}")
        key = (B, Ho, Wo, dev, tuple((n, t.shape[3] if t.dim() == 4 else 1) for n, t in zip(self.maps, srcs)))
        outs = self._out.get(key)
        if outs is None:
            outs = [torch.empty(B, c, Ho, Wo, device=dev, dtype=self.image_dtype if self.maps[n][0] == "image" else torch.float32)
                    for n, c in key[4]]
            self._out = {key: outs}                                            # one shape at a time is kept
        table = []
        for (name, (kind, mode)), src, dst in zip(self.maps.items(), srcs, outs):
            img = kind == "image"
            table.append((src, dst, kind, mode, self.quantize and img, self.mean if img else None, self.std if img else None))
        ops.augment_batch(table, params.mats, params.aux, self.border)
        result = {k: v for k, v in batch.items() if k not in self.maps}
        result.update(zip(self.maps, outs))
        return result
