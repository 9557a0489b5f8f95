"""The task meters' reference, cases and error bounds, imported by test_meters_cpu.py / test_meters_gpu.py and
tests/gen_golden_meters.py (not a conftest: nothing here runs by itself).

* the meters restated in plain torch, one function per kernel, returning what the device state holds (and what the bound
  builders need).  They compute in the dtype of `pred` (float64: the reference; float32: torch's own fp32 evaluation, which
  test_meters_cpu.py holds to the bounds the kernels are held to):
    iou_ref      evaluation/eval_semseg.py:109-120, eval_human_parts.py:88-98 after utils/utils.py:67-68 (torch.max over C)
    depth_ref    evaluation/eval_depth.py:67-85
    normals_ref  evaluation/eval_normals.py:72-94 after utils/utils.py:64-65, without the 0..255 round trip
    sal_ref      evaluation/eval_sal.py:75-96 with evaluation/jaccard.py after utils/utils.py:70-71
    edge_ref     evaluation/eval_edge.py:20-27: the balanced BCE (loss_cases.bce_ref) of the PROBABILITY fed in as a logit
  and score(kind, state): the host arithmetic of the get_score methods.
* the case table, the seeded input makers, settle() - which moves an input off the conditions under which a count may
  legitimately differ between two precisions - and the error-bound builders (derivations next to each; U32 and SAFETY come from
  kernel_contract and are never tuned per test).
"""
import math

import numpy as np
import torch

import loss_cases as LC
from kernel_contract import SAFETY, U32

IGNORE = 255
SIZES = [(1, 1, 1), (2, 3, 7), (1, 5, 65), (3, 17, 33)]          # (B, H, W): one pixel; odd; a row that fills no vector; > 1 block
IOU_CLASSES = [2, 7, 21, 40, 150]
GROUP_CLASSES = [4, 8, 12, 20, 68, 152]                          # channels-last chunks of 1, 2, 3, 5, 17, 38: groups of 1 .. 64 lanes (16: C = 40)
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
LAYOUTS = ["nchw", "nhwc"]
KINDS = ["iou", "depth", "normals", "sal", "edge"]
KIND_C = {"depth": 1, "normals": 3, "sal": 1, "edge": 1}
EDGE_W = 0.95
THRESHOLDS = np.linspace(0.2, 0.9, 15).astype(np.float32).astype(np.float64)   # torch compares an fp32 tensor with the fp32 value
ANGLE_CUTS = (11.25, 22.5, 30.0)
ANGLE_MARGIN = 0.05              # degrees: acos near +-1 turns an fp32 rounding of the dot product into about 0.03 degrees
PROB_MARGIN = 1e-5


def cases():
    """(kind, C, (B, H, W)) of every value case"""
    out = [("iou", C, s) for C in IOU_CLASSES for s in SIZES]
    for kind in KINDS[1:]:
        out += [(kind, KIND_C[kind], s) for s in SIZES]
    return out


def multi_pass_cases():
    """Per kernel the smallest shape at which a grid capped at 1024 workgroups of 256 threads goes round its loop more than
    once on the scalar path (odd storage), ending on a partial pass:
      iou C2 (8,129,257)      265 224 pixels: iou_planar, one pixel per thread, 262 144 a pass (aligned storage: H * W is odd, the
                              scalar path as well)
      iou C40 (2,48,48)       4 608 pixels, 184 320 elements: iou_cl1 with 64 lanes per pixel takes 4 pixels per workgroup and pass;
                              the grid is held to the 720 workgroups the workspace is sized for: 2 880 pixels a pass
      iou C40 (2,192,176)     67 584 pixels: iou_cl4 (aligned storage) takes 16 steps of 4 pixels per workgroup: 65 536 a pass - the
                              prefetched pieces a pass hands to the next
      depth, edge (4,257,511) 525 308 elements: depth_kernel / flat_kernel, two pieces per thread: 524 288 a pass
      normals (8,129,257)     one pixel per thread: 262 144 a pass
      sal (64,91,91)          8 281 pixels per image on 1024 / 64 = 16 workgroups of two pieces: 8 192 a pass
    One case is here for the finalize launch instead (sums_finalize_kernel: 256 threads add the workgroups' partials, thread t
    those of workgroups t, t + 256, ...), which goes round more than once only above 256 workgroups and raggedly only off a
    multiple of 256 - every case above runs the full 1024:
      normals (3,159,161)     76 797 pixels, one per thread and 256 per workgroup: 300 workgroups, the last one partial, so
                              a second round of 44 partials (the <2, 4> instance).  The <2, 1> instance has its own in
                              depth (4,257,511) on aligned storage: 131 327 vectors of 4, 512 per workgroup, 257 workgroups."""
    return [("iou", 2, (8, 129, 257)), ("iou", 40, (2, 48, 48)), ("iou", 40, (2, 192, 176)), ("depth", 1, (4, 257, 511)),
            ("edge", 1, (4, 257, 511)), ("normals", 3, (8, 129, 257)), ("sal", 1, (64, 91, 91)), ("normals", 3, (3, 159, 161))]


def case_id(c):
    kind, C, (B, H, W) = c[:3]
    return f"{kind}-C{C}-{B}x{H}x{W}"


# the cases tests/golden/g13_meters.npz records from the reference's own classes: (key, task, database, C, size).  The
# reference's saliency class cannot run B = 1 and its squeezes are shape-fragile: B >= 2 and H, W >= 2 throughout.
FIXTURES = [("semseg-NYUD", "semseg", "NYUD", 40, (2, 3, 7)), ("semseg-PASCALContext", "semseg", "PASCALContext", 21, (2, 3, 7)),
            ("semseg-CityScapes", "semseg", "CityScapes", 7, (2, 5, 65)),
            ("semseg-CityScapes-C21", "semseg", "CityScapes", 21, (2, 3, 7)),      # predictions and labels >= n_classes = 7
            ("semseg-NYUD-ties", "semseg", "NYUD", 40, (2, 3, 7)),                 # the dedicated tie case
            ("human_parts", "human_parts", "PASCALContext", 7, (2, 3, 7)),
            ("depth-a", "depth", None, 1, (2, 3, 7)), ("depth-b", "depth", None, 1, (2, 5, 65)),
            ("normals-a", "normals", None, 3, (2, 3, 7)), ("normals-b", "normals", None, 3, (2, 5, 65)),
            ("sal-a", "sal", None, 1, (2, 3, 7)), ("sal-b", "sal", None, 1, (2, 5, 65)),
            ("edge-a", "edge", None, 1, (2, 3, 7)), ("edge-b", "edge", None, 1, (2, 5, 65))]
TASK_KIND = {"semseg": "iou", "human_parts": "iou", "depth": "depth", "normals": "normals", "sal": "sal", "edge": "edge"}
N_CLASSES = {"NYUD": 40, "PASCALContext": 21, "CityScapes": 7}


def fixture_inputs(key, update):
    """(pred float32 [B,C,H,W], label float32) of update 0 or 1 of a recorded case, settled for float32"""
    _, task, db, C, size = next(f for f in FIXTURES if f[0] == key)
    kind = TASK_KIND[task]
    pred, label = make_inputs(kind, C, size, seed=20 + update)
    if key.endswith("-ties"):
        pred[:, 2] += 4.0                                         # two equal logits in every pixel, often the maximum: the
        pred[:, 5] = pred[:, 2]                                   # lower index must win
    return settle(kind, pred, label)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_inputs(kind, C, size, seed=0, ignore_frac=0.2):
    """(pred float32 [B,C,H,W] NCHW on the CPU, label float32): logits ~ N(0, 3^2) with labels over [0, C); depths ~ U(-0.5, 9.5)
    (the negative ones are clamped) against labels ~ U(0.1, 10.1); normals ~ N(0, 1) per component with unit-length labels;
    saliency and edge logits ~ N(0, 2^2) with {0, 1} labels (saliency: a few 255, which count as set).  About ignore_frac of
    the labels are 255 (normals: per element, as the reference masks)."""
    B, H, W = size
    g = _gen(7000 + 1000 * seed + 17 * C + B * H * W + 131 * KINDS.index(kind))
    if kind == "iou":
        pred = torch.randn(B, C, H, W, generator=g) * 3
        label = torch.randint(0, C, (B, 1, H, W), generator=g).float()
        label[torch.rand(B, 1, H, W, generator=g) < ignore_frac] = IGNORE
    elif kind == "depth":
        pred = torch.rand(B, C, H, W, generator=g) * 10 - 0.5
        label = torch.rand(B, C, H, W, generator=g) * 10 + 0.1
        label[torch.rand(B, C, H, W, generator=g) < ignore_frac] = IGNORE
    elif kind == "normals":
        pred = torch.randn(B, C, H, W, generator=g)
        label = torch.randn(B, C, H, W, generator=g)
        label = label / label.norm(dim=1, keepdim=True).clamp_min(1e-3)
        label[torch.rand(B, C, H, W, generator=g) < ignore_frac] = IGNORE
    elif kind in ("sal", "edge"):
        pred = torch.randn(B, C, H, W, generator=g) * 2
        label = (torch.rand(B, C, H, W, generator=g) < 0.3).float()
        if kind == "sal":
            label[torch.rand(B, C, H, W, generator=g) < 0.05] = IGNORE
    else:
        raise ValueError(kind)
    return pred, label


def conditions_hold(kind, pred, label):
    """the conditions under which every integer count is the same in any precision (the fixture generator asserts them on the
    reference's inputs; settle() establishes them).  pred: the values the kernel reads (rounded to its dtype)."""
    x = pred.double()
    if kind == "normals":
        r = normals_ref(x, label.double())
        a = r["angle"][r["mask"]]                                 # the pixels that count
        return all(bool(((a - c).abs() > ANGLE_MARGIN).all()) for c in ANGLE_CUTS)
    if kind == "sal":
        p = torch.sigmoid(x).unsqueeze(-1)
        return bool(((p - torch.from_numpy(THRESHOLDS)).abs() > PROB_MARGIN).all())
    if kind == "depth":
        return bool((label[label != IGNORE] > 0).all())
    return True


def settle(kind, pred, label):
    """(pred, label) with the offending pixels moved away: a normals pixel whose float64 angle is within ANGLE_MARGIN of a cut
    has channel 0 of its label set to 255 (it no longer counts); a saliency logit whose probability is within PROB_MARGIN of
    a threshold becomes 3.0 (p = 0.953, exact in every dtype).  Call it on the dtype-ROUNDED pred."""
    pred, label = pred.clone(), label.clone()
    if kind == "normals":
        a = normals_ref(pred.double(), label.double())["angle"]
        near = torch.zeros_like(a, dtype=torch.bool)
        for c in ANGLE_CUTS:
            near |= (a - c).abs() <= ANGLE_MARGIN
        label[:, 0][near] = IGNORE
    elif kind == "sal":
        p = torch.sigmoid(pred.double()).unsqueeze(-1)
        near = ((p - torch.from_numpy(THRESHOLDS)).abs() <= PROB_MARGIN).any(-1)
        pred[near] = 3.0
    assert conditions_hold(kind, pred, label)
    return pred, label


# ------------------------------------------------------------------------------------------------------ the restatement
def class_of(label):
    """[B,H,W] float64 labels as the meters compare them (`gt == i`: equality, no truncation) and the mask gt != 255"""
    lab = label.reshape(label.shape[0], *label.shape[-2:]).double()
    return lab, lab != IGNORE


def iou_ref(pred, label, n_classes):
    am = torch.max(pred, dim=1)[1]                                # lowest index on ties; a NaN beats everything, the first NaN wins
    lab, valid = class_of(label.to(pred.device))
    tp, fp, fn = [], [], []
    for i in range(n_classes):
        g, p = lab == i, am == i
        tp.append(int((g & p & valid).sum())); fp.append(int((~g & p & valid).sum())); fn.append(int((g & ~p & valid).sum()))
    return dict(tp=np.array(tp), fp=np.array(fp), fn=np.array(fn))


def depth_ref(pred, label):
    label = label.to(pred.device, pred.dtype)
    valid = label != IGNORE
    p = torch.clamp(pred, min=1e-9)
    sq = torch.where(valid, (label - p) ** 2, torch.zeros_like(p))
    lq = torch.where(valid, (torch.log(label) - torch.log(p)) ** 2, torch.zeros_like(p))
    return dict(n=int(valid.sum()), sum_sq=sq.sum(), sum_log_sq=lq.sum(), sq=sq, lq=lq, p=p, valid=valid, label=label)


def normals_ref(pred, label):
    label = label.to(pred.device, pred.dtype)
    t = pred / pred.norm(p=2, dim=1, keepdim=True).clamp_min(1e-12)
    bad = label == IGNORE
    t0, g0 = torch.where(bad, torch.zeros_like(t), t), torch.where(bad, torch.zeros_like(label), label)
    dot = torch.clamp((t0 * g0).sum(1), min=-1, max=1)
    angle = (180 / math.pi) * torch.acos(dot)
    m = label[:, 0] != IGNORE
    a = torch.where(m, angle, torch.zeros_like(angle))
    return dict(n=int(m.sum()), sum_angle=a.sum(), sum_sq=(a * a).sum(), angle=angle, dot=dot, mask=m, t=t0, g=g0,
                counts=[int(((angle < c) & m).sum()) for c in ANGLE_CUTS])


def sal_ref(pred, label):
    """per image and threshold: counts (exact), then jaccard / precision / recall in double; sums over the images [3][15]"""
    B = pred.shape[0]
    p = torch.sigmoid(pred).reshape(B, -1, 1).double()
    y = (label.to(pred.device).reshape(B, -1, 1) != 0)
    m = p > torch.from_numpy(THRESHOLDS).to(pred.device)
    tp = (m & y).sum(1).double(); npred = m.sum(1).double(); ngt = y.sum(1).double()
    union = ngt + npred - tp
    jac = torch.where((ngt == 0) & (npred == 0), torch.ones_like(tp), tp / union.clamp_min(1))
    per_image = torch.stack([jac, tp / (npred + 1e-12), tp / (ngt + 1e-12)])          # [3][B][15]
    return dict(sums=per_image.sum(1), n_images=B, per_image=per_image, tp=tp, npred=npred, ngt=ngt)


def edge_ref(pred, label, pos_weight=EDGE_W):
    r = LC.bce_ref(torch.sigmoid(pred), label, pos_weight)
    return dict(sum=r["loss"] * pred.numel(), n=pred.numel(), bce=r)


def reference(kind, pred, label, n_classes=None):
    if kind == "iou":
        return iou_ref(pred, label, n_classes if n_classes is not None else pred.shape[1])
    return {"depth": depth_ref, "normals": normals_ref, "sal": sal_ref, "edge": edge_ref}[kind](pred, label)


class Accumulated:
    """the state a meter holds after a sequence of updates, from the restatement: counts as Python ints, sums and their bounds
    as float64.  add(kind, r, bound) after every update; fields by kind as read() of test_meters_gpu.py returns them."""

    def __init__(self, kind):
        self.kind, self.ints, self.sums, self.bounds = kind, None, None, None

    def add(self, r, b=None):
        k = self.kind
        ints = {"iou": lambda: np.stack([r["tp"], r["fp"], r["fn"]]), "depth": lambda: np.array([r["n"]]),
                "normals": lambda: np.array(r["counts"] + [r["n"]]), "sal": lambda: np.array([r["n_images"]]),
                "edge": lambda: np.array([r["n"]])}[k]()
        sums = {"iou": lambda: np.zeros(0), "depth": lambda: np.array([float(r["sum_sq"]), float(r["sum_log_sq"])]),
                "normals": lambda: np.array([float(r["sum_angle"]), float(r["sum_sq"])]),
                "sal": lambda: r["sums"].double().cpu().numpy().reshape(-1), "edge": lambda: np.array([float(r["sum"])])}[k]()
        b = np.zeros_like(sums) if b is None else np.asarray(b, dtype=np.float64)
        if self.ints is None:
            self.ints, self.sums, self.bounds = ints, sums, b
        else:
            self.ints, self.sums, self.bounds = self.ints + ints, self.sums + sums, self.bounds + b
        return self


def score(kind, ints, sums):
    """the get_score arithmetic of the reference's meters on accumulated values (Accumulated's fields)"""
    if kind == "iou":
        tp, fp, fn = ints
        jac = [float(tp[i]) / max(float(tp[i] + fp[i] + fn[i]), 1e-8) for i in range(len(tp))]
        return {"jaccards_all_categs": jac, "mIoU": float(np.mean(jac))}
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == "depth":
            n = np.float64(ints[0])
            return {"rmse": float(np.sqrt(sums[0] / n)), "log_rmse": float(np.sqrt(sums[1] / n))}
        if kind == "normals":
            n = np.float64(ints[3])
            return {"mean": float(sums[0] / n), "rmse": float((sums[1] / n) ** 0.5), "11.25": float(ints[0] * 100 / n),
                    "22.5": float(ints[1] * 100 / n), "30": float(ints[2] * 100 / n)}
        if kind == "sal":
            m = sums.reshape(3, 15) / np.float64(ints[0])
            F = 2 * m[1] * m[2] / (m[1] + m[2] + 1e-12)
            return {"mIoUs": m[0].tolist(), "mPrec": m[1].tolist(), "mRec": m[2].tolist(), "F": F.tolist(),
                    "mIoU": float(m[0].max()), "maxF": float(F.max())}
        return {"loss": float(sums[0] / np.float64(ints[0]))}


# --------------------------------------------------------------------------------------------------- error-bound builders
# Common form (kernel_contract): the reference is fp64 on the dtype-ROUNDED inputs, so only the kernel's own arithmetic is
# charged.  Counts are integers: exact, no bound.  The saliency sums are double quotients of exact counts added in double: 45
# values whose only error is the order of B double additions - B * 2^-53 relative, checked as 1e-12 relative.
#
# A float sum S of per-element terms: every term passes through at most K fp32 additions before the partials are added in
# double (loss_cases._depth: a thread adds at most 8 terms per pass over a grid of up to 1024 x 256 threads, then 6 shuffle
# levels and 3 additions over the four waves): |S - S_ref| <= sum_i e_i + K u32 sum_i |term_i|, e_i the error of term i.
SUM_REL = 1e-12


def _sum_bound(term_err, terms, n_elements):
    return SAFETY * float(term_err.sum() + LC._depth(n_elements) * U32 * terms.abs().sum())


def depth_bounds(r):
    """p = max(x, 1e-9f): exact but where it clamps (the fp32 constant is off by u32 of itself: relative u32 in p, absolute u32
    in log p).  d = g - p: u32 |d|, squared: 2 |d| u32 |d| + u32 d^2 = 3 u32 d^2 (+ 2 |d| u32 p where clamped).
    q = log g - log p: logf is good to 2 ulps (2 u32 |log g| + 2 u32 |log p|), the clamp's u32, the subtraction u32 |q|;
    squared: 2 |q| e_q + u32 q^2.  Returns (bound of sum_sq, bound of sum_log_sq)."""
    g, p, v = r["label"].double(), r["p"].double(), r["valid"]
    clamped = (p <= 1e-9).double()
    d = (g - p).abs()
    e_sq = (3 * U32 * d * d + 2 * d * U32 * p * clamped) * v
    lg, lp = torch.log(g.clamp_min(1e-300)), torch.log(p)
    q = (lg - lp).abs()
    e_q = 2 * U32 * (lg.abs() + lp.abs()) + U32 * clamped + U32 * q
    e_lq = (2 * q * e_q + U32 * q * q) * v
    n = g.numel()
    return np.array([_sum_bound(e_sq, r["sq"].double(), n), _sum_bound(e_lq, r["lq"].double(), n)])


def normals_bounds(r):
    """per pixel (C = 3): |x| = sqrt of two fmas and a product, then max(., 1e-12): (C / 2 + 1) u32 relative; t = x / |x|:
    e_t = (C / 2 + 2) u32 |t| <= (C + 4) u32 |t| (loss_cases' figure, kept); dot = fma chain over C: e_dot = sum_c |g_c| e_t_c
    + C u32 sum_c |t_c g_c|.  The angle is (180 / pi) acos(dot): an error e_dot in dot moves it by e_dot / sqrt(1 - dot^2)
    to first order - unbounded at |dot| = 1, where the first order says nothing.  acos is monotone, so the exact carry is used
    instead: max |acos(clamp(dot +- e_dot)) - acos(dot)|, which equals the first-order term away from +-1 and is
    sqrt(2 e_dot) at it.  acosf itself 4 ulps and the product with 180 / pi (the fp32 constant, the rounding): 6 u32 angle.
    angle^2: 2 angle e_a + u32 angle^2.  Returns (bound of sum_angle, bound of sum_sq)."""
    C = 3
    t, g, dot, a, m = r["t"].double(), r["g"].double(), r["dot"].double(), r["angle"].double(), r["mask"]
    e_t = (C + 4) * U32 * t.abs()
    e_dot = (g.abs() * e_t).sum(1) + C * U32 * (t * g).abs().sum(1)
    k = 180 / math.pi
    lo, hi = torch.acos((dot + e_dot).clamp(-1, 1)), torch.acos((dot - e_dot).clamp(-1, 1))
    e_a = (k * torch.maximum((hi - torch.acos(dot)).abs(), (lo - torch.acos(dot)).abs()) + 6 * U32 * a) * m
    e_sq = (2 * a * e_a + U32 * a * a) * m
    n = t.numel()
    am = a * m
    return np.array([_sum_bound(e_a, am, n), _sum_bound(e_sq, am * am, n)])


def edge_bounds(r, pred64):
    """numel x the balanced-BCE bound of loss_cases on the probability fed in as a logit, plus what the fp32 sigmoid in front
    leaves in that input: 4 u32 absolute per element (p <= 1), carried by |d loss / d input| = k |sigmoid(p) - y| <= k"""
    lb, _ = LC.bce_bounds(r["bce"], torch.sigmoid(pred64), torch.float32)
    return np.array([(float(lb) + SAFETY * 4 * U32 * float(r["bce"]["k"].abs().sum())) * pred64.numel()])


def bounds(kind, r, pred64):
    """bounds of the float sums of one update, in Accumulated's order (none for iou; saliency: relative, see SUM_REL)"""
    if kind == "depth":
        return depth_bounds(r)
    if kind == "normals":
        return normals_bounds(r)
    if kind == "edge":
        return edge_bounds(r, pred64)
    if kind == "sal":
        return SUM_REL * np.abs(r["sums"].double().cpu().numpy().reshape(-1)) + 1e-300
    return np.zeros(0)


# ------------------------------------------------------------------------------------------------------------ edge cases
def special_iou_cases():
    """(name, pred float32, label, n_classes, expected) - expected: None (the restatement), or a dict of exact counts"""
    out = []
    C, size = 7, (2, 3, 7)
    pred, label = make_inputs("iou", C, size, seed=3)
    lab = label.clone()
    lab.view(-1)[[0, 9, 20, 33]] = torch.tensor([300.0, -3.0, 2.5, 9.0])          # valid, but no class: fp for the prediction
    out.append(("labels-that-are-no-class", pred, lab, C, None))
    out.append(("labels-above-n_classes", pred, label, 4, None))                   # classes 4, 5, 6 match nothing
    out.append(("all-ignored", pred, torch.full_like(label, float(IGNORE)), C, dict(tp=0, fp=0, fn=0)))
    tie = pred.clone()
    tie[:, 4] = tie.amax(1) + 1.0
    tie[:, 1] = tie[:, 4]                                                          # two maxima: channel 1 must win over 4
    tie[:, 6] = tie[:, 4]
    out.append(("ties-lowest-index", tie, label, C, None))
    same = torch.zeros_like(pred)
    same[:, ::2] = -0.0                                                            # +0 and -0 compare equal: channel 0 everywhere
    out.append(("all-equal-signed-zeros", same, label, C, None))
    nan = pred.clone()
    nan[:, 3, 0, :] = float("nan")
    nan[:, 5, 0, ::2] = float("nan")                                               # the first NaN (channel 3) wins
    nan[:, 0, 1, 1] = float("inf")
    nan[:, 2, 2, :] = float("-inf")
    out.append(("nan-beats-everything", nan, label, C, None))
    return out
