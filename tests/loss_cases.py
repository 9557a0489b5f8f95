"""The dense-prediction losses' reference, cases and error bounds, imported by test_losses_cpu.py / test_losses_gpu.py and
tests/gen_golden_losses.py (not a conftest: nothing here runs by itself).

* the four formulas restated in plain torch, closed form for the value AND the gradient (no masked_select, no autograd: the
  reference's own autograd gives NaN-free zeros where a mean over nothing is differentiated, and so does the closed form):
    ce_ref       losses/loss_functions.py:16-33    LogSoftmax + NLLLoss(ignore_index=255), mean over label != 255
    l1_ref       losses/loss_functions.py:126-140  L1Loss over masked_select(label != 255)
    normals_ref  losses/loss_functions.py:143-197  Normalize (:143-151: x / (|x|_2 + 1e-12)), l1 / mse with reduction='sum' over
                                                   the elements with label != 255, / max(n_valid, 1e-6)
    bce_ref      losses/loss_functions.py:36-84    labels = label >= 0.5; w = n_neg / n_total or pos_weight; the stable
                                                   x (y - [x >= 0]) - log(1 + exp(x - 2 x [x >= 0])) form; / numel
  Each returns a dict: loss (0-dim), grad (d loss / d pred for upstream 1) and what the bound builders need.  They compute
  in the dtype of `pred` (float64: the reference; float32: torch's own fp32 evaluation, which test_losses_cpu.py holds to the
  bounds the kernels are held to).
* RefLoss: the same closed forms as a differentiable criterion (the end-to-end test trains a model against it in float64).
* the case table, the seeded input makers and the error-bound builders (derivations next to each; U32, u(), store(), SAFETY
  come from kernel_contract and are never tuned per test).
"""
import math

import torch

from kernel_contract import SAFETY, U32, store

IGNORE = 255
ETA32 = 2.0 ** -126               # a flushed / subnormal fp32 exp

# ------------------------------------------------------------------------------------------------------- the case table
SIZES = [(1, 1, 1), (2, 3, 7), (1, 5, 65), (3, 17, 33)]          # (B, H, W): one pixel; odd; a row that fills no vector; > 1 block
GRID_CAP = (2, 96, 160)                                          # with C = 40: the issue's case; wraps the channels-last scalar grids only
CE_CLASSES = [2, 7, 21, 40, 150]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
LAYOUTS = ["nchw", "nhwc"]


def cases():
    """(kind, C, (B, H, W), extra) of every value case; extra: norm for normals, pos_weight for bce"""
    out = [("ce", C, s, None) for C in CE_CLASSES for s in SIZES] + [("ce", 40, GRID_CAP, None)]
    out += [("l1", 1, s, None) for s in SIZES]
    out += [("normals", 3, s, norm) for s in SIZES for norm in (1, 2)]
    out += [("bce", 1, s, pw) for s in SIZES for pw in (None, 0.95)]
    return out


# Channels-last classes that are multiples of 4 (the 16-byte forward), by their C / 4 chunks of a pixel: 1, 2, 3, 5, 17 and 38
# chunks -> groups of 1, 2, 4, 8, 32 and 64 lanes (16 lanes: C = 40 of the case table): every level of the group reduction.
GROUP_CLASSES = [4, 8, 12, 20, 68, 152]


def multi_pass_cases():
    """Cases sized so that a grid of 1024 workgroups goes round its loop more than once and ends on a partial pass; B * C rows
    stay many and H * W small so that the guarded allocations stay small.  Which kernel each is for (aligned / odd storage):
      ce C40 (2,192,176)   67 584 pixels, 2.7 M elements.  channels-last: ce_fwd_cl4 takes 16 steps of 4 pixels per workgroup
                           and pass (65 536 pixels a pass), ce_bwd_cl 2048 elements x 4 (2.1 M a pass) / odd: ce_fwd_cl1, scalar
                           ce_bwd_cl.  (planar: one pass - the next case)
      ce C2 (32,128,260)   1 064 960 pixels, 2.1 M elements.  planar: ce_fwd_planar / ce_bwd_planar own 4 pixels (odd: 1) per
                           thread, 1 048 576 (262 144) pixels a pass
      l1, bce (64,128,258) 2 113 536 elements: flat_kernel, two pieces of 4 (odd: 1) elements per thread, 2 097 152 (524 288) a pass
      normals (8,129,257)  265 224 pixels: normals_kernel, one pixel per thread, 262 144 a pass
    These are larger than the 2 M elements of the other cases because a second pass cannot be had for less.
    (All of them run the full 1024 workgroups.  The finalize launch, whose 256 threads add the workgroups' partials t, t + 256,
    ..., has its ragged second round in cases(): ce C40 GRID_CAP, channels-last on aligned storage, is 7 680 steps of 4
    pixels, 16 per workgroup: 480 workgroups.)"""
    return [("ce", 40, (2, 192, 176), None), ("ce", 2, (32, 128, 260), None), ("l1", 1, (64, 128, 258), None),
            ("bce", 1, (64, 128, 258), None), ("normals", 3, (8, 129, 257), 1), ("normals", 3, (8, 129, 257), 2)]


def case_id(c):
    kind, C, (B, H, W), extra = c
    return f"{kind}-C{C}-{B}x{H}x{W}" + ("" if extra is None else f"-{extra}")


def fixture_cases():
    """the cases tests/golden/g12_losses.npz records (float64, from the reference's own classes): the two smallest sizes
    for every C, and the odd row for the single-channel losses - the file stays small"""
    out = [("ce", C, s, None) for C in CE_CLASSES[:4] for s in SIZES[:2]] + [("ce", 150, (1, 1, 1), None), ("ce", 150, (1, 2, 3), None)]
    for s in SIZES[:3]:
        out += [("l1", 1, s, None), ("normals", 3, s, 1), ("normals", 3, s, 2), ("bce", 1, s, None), ("bce", 1, s, 0.95)]
    return out


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_inputs(kind, C, size, seed=0, ignore_frac=0.2):
    """(pred float32 [B,C,H,W] NCHW on the CPU, label float32).  Values are kept to ranges the fp32 evaluation of the bounds was
    checked on (test_losses_cpu.py): logits ~ N(0, 3^2); depths ~ U(0, 10); normals ~ N(0, 1) per component with unit-length
    labels; edge logits ~ N(0, 2^2) with {0, 1} labels.  About ignore_frac of the labels are 255 (CE: pixels; L1, normals:
    elements, as the reference masks per element)."""
    B, H, W = size
    g = _gen(1000 * seed + 17 * C + B * H * W)
    if kind == "ce":
        pred = torch.randn(B, C, H, W, generator=g) * 3
        label = torch.randint(0, C, (B, 1, H, W), generator=g).float()
        label[torch.rand(B, 1, H, W, generator=g) < ignore_frac] = IGNORE
    elif kind == "l1":
        pred = torch.rand(B, C, H, W, generator=g) * 10
        label = torch.rand(B, C, H, W, generator=g) * 10
        label[torch.rand(B, C, H, W, generator=g) < ignore_frac] = IGNORE
    elif kind == "normals":
        pred = torch.randn(B, C, H, W, generator=g)
        label = torch.randn(B, C, H, W, generator=g)
        label = label / label.norm(dim=1, keepdim=True).clamp_min(1e-3)
        label[torch.rand(B, C, H, W, generator=g) < ignore_frac] = IGNORE
    elif kind == "bce":
        pred = torch.randn(B, C, H, W, generator=g) * 2
        label = (torch.rand(B, C, H, W, generator=g) < 0.3).float()
    else:
        raise ValueError(kind)
    return pred, label


def as_layout(t, layout):
    """t [B,C,H,W] in NCHW-contiguous or channels-last STORAGE (for C = 1 or H = W = 1 the two coincide)"""
    return t.contiguous() if layout == "nchw" else t.contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------------------ the restatement
def class_of(label, C):
    """[B,H,W] int64 class, validity mask and bad-label mask of a CE label ([B,1,H,W] or [B,H,W]; float labels truncate as
    `.long()`).  A label that is neither 255 nor in [0, C) is bad: ignored, and counted."""
    lab = label.reshape(label.shape[0], *label.shape[-2:])
    lab = lab.long() if not lab.dtype.is_floating_point else lab.double().nan_to_num(-1.0, -1.0, -1.0).clamp(-2, 1e6).long()
    valid = (lab >= 0) & (lab < C)
    bad = ~valid & (lab != IGNORE)
    return lab, valid, bad


def ce_ref(pred, label):
    B, C, H, W = pred.shape
    lab, valid, bad = class_of(label.to(pred.device), C)
    idx = lab.clamp(0, C - 1).unsqueeze(1)
    lse = torch.logsumexp(pred, 1)
    xl = pred.gather(1, idx).squeeze(1)
    terms = (lse - xl) * valid
    n = valid.sum()
    loss = terms.sum() / n                                       # 0 / 0 = NaN, as the reference
    coef = torch.where(n > 0, 1.0 / n.clamp_min(1).to(pred.dtype), torch.zeros((), dtype=pred.dtype, device=pred.device))
    p = torch.exp(pred - lse.unsqueeze(1))
    onehot = torch.zeros_like(pred).scatter_(1, idx, 1.0)
    grad = (p - onehot) * valid.unsqueeze(1) * coef
    return dict(loss=loss, grad=grad, n_valid=int(n), n_bad=int(bad.sum()), lse=lse, xl=xl, p=p, onehot=onehot,
                valid=valid, coef=coef, terms=terms)


def l1_ref(pred, label):
    label = label.to(pred.device, pred.dtype)
    valid = label != IGNORE
    d = pred - label
    terms = d.abs() * valid
    n = valid.sum()
    loss = terms.sum() / n
    coef = torch.where(n > 0, 1.0 / n.clamp_min(1).to(pred.dtype), torch.zeros((), dtype=pred.dtype, device=pred.device))
    return dict(loss=loss, grad=torch.sign(d) * valid * coef, n_valid=int(n), terms=terms, coef=coef)


def normals_ref(pred, label, norm=1):
    label = label.to(pred.device, pred.dtype)
    valid = label != IGNORE
    n = pred.norm(p=2, dim=1, keepdim=True)
    q = n + 1e-12
    t = pred / q
    d = t - label
    terms = (d.abs() if norm == 1 else d * d) * valid
    nv = valid.sum()
    den = torch.clamp(nv.to(pred.dtype), min=1e-6)
    loss = terms.sum() / den
    g = (torch.sign(d) if norm == 1 else 2 * d) * valid
    gt = (g * t).sum(1, keepdim=True)
    unit = torch.where(n > 0, pred / n.clamp_min(1e-300 if pred.dtype == torch.float64 else 1e-38), torch.zeros_like(pred))
    grad = (g - gt * unit) / q / den
    return dict(loss=loss, grad=grad, n_valid=int(nv), terms=terms, valid=valid, n=n, q=q, t=t, d=d, g=g, gt=gt, unit=unit,
                coef=1.0 / den)


def bce_ref(pred, label, pos_weight=None):
    label = label.to(pred.device, pred.dtype)
    y = label >= 0.5
    yf = y.to(pred.dtype)
    gt0 = (pred >= 0).to(pred.dtype)
    e = torch.exp(-pred.abs())
    terms = pred * (gt0 - yf) + torch.log1p(e)
    numel = pred.numel()
    n_pos = y.sum()
    n_neg = numel - n_pos
    # the reference forms w from `labels.float()` sums: an fp32 quotient, whatever the dtype of the logits (:49-56)
    w = ((n_neg.float() / torch.tensor(float(numel), dtype=torch.float32)).to(pred.dtype) if pos_weight is None
         else torch.tensor(float(pos_weight), dtype=pred.dtype, device=pred.device))
    s_pos, s_neg = (terms * yf).sum(), (terms * (1 - yf)).sum()
    loss = (w * s_pos + (1 - w) * s_neg) / numel
    k = torch.where(y, w, 1 - w) / numel
    sg = torch.sigmoid(pred)
    return dict(loss=loss, grad=(sg - yf) * k, n_pos=int(n_pos), n_neg=int(n_neg), terms=terms, y=y, sg=sg, k=k, w=w, e=e)


def reference(kind, pred, label, extra=None):
    if kind == "ce":
        return ce_ref(pred, label)
    if kind == "l1":
        return l1_ref(pred, label)
    if kind == "normals":
        return normals_ref(pred, label, extra)
    return bce_ref(pred, label, extra)


class _RefLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, label, kind, extra):
        r = reference(kind, pred.detach(), label, extra)
        ctx.save_for_backward(r["grad"])
        return r["loss"]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return g * grad, None, None, None


class RefLoss(torch.nn.Module):
    """a restated loss as a criterion module (any dtype, any device): differentiable through the closed-form gradient"""

    def __init__(self, kind, extra=None):
        super().__init__()
        self.kind, self.extra = kind, extra

    def forward(self, pred, label, void_pixels=None):
        return _RefLossFn.apply(pred, label, self.kind, self.extra)


TASK_KIND = {"semseg": ("ce", None), "human_parts": ("ce", None), "depth": ("l1", None), "normals": ("normals", 1),
             "edge": ("bce", 0.95), "sal": ("bce", None)}
TASK_C = {"semseg": 7, "human_parts": 4, "depth": 1, "normals": 3, "edge": 1, "sal": 1}
TASK_WEIGHT = {"semseg": 1.0, "human_parts": 2.0, "depth": 1.0, "normals": 10.0, "edge": 50.0, "sal": 5.0}
SCHEME_SIZE = (2, 3, 7)
SCHEMES = {          # name -> (tasks, prediction-key prefixes, multi_level, tam, single_task)
    "plain2": (["semseg", "depth"], [""], False, False, None),
    "plain5": (["semseg", "normals", "edge", "sal", "human_parts"], [""], False, False, None),
    "single": (["semseg", "depth"], [""], False, False, "depth"),
    "multilevel": (["semseg", "depth"], [""], True, False, None),
    "tam": (["semseg", "depth"], ["tam_level0_", "tam_level1_", "tam_level2_", ""], False, True, None),
}


def scheme_inputs(name):
    """(pred dict, gt dict) of float32 CPU tensors for one recorded MultiTaskLoss call.  human_parts has every label ignored:
    its NaN loss is what the scheme replaces by 0."""
    tasks, prefixes, _, _, _ = SCHEMES[name]
    pred, gt = {}, {}
    for ti, task in enumerate(tasks):
        kind, _ = TASK_KIND[task]
        for pi, prefix in enumerate(prefixes):
            x, lab = make_inputs(kind, TASK_C[task], SCHEME_SIZE, seed=100 + 10 * ti + pi)
            pred[prefix + task] = x
            gt[task] = lab
        if task == "human_parts":
            gt[task] = torch.full_like(gt[task], float(IGNORE))
    return pred, gt


# --------------------------------------------------------------------------------------------------- error-bound builders
# Common form (kernel_contract): the reference is fp64 on the dtype-ROUNDED inputs, so only the kernel's own arithmetic is
# charged.  r = the float64 reference dict of the rounded inputs.
#
# A loss value is  fl32( S / n )  with S the sum of the per-element terms: every term passes through at most K fp32 additions
# before the partials are added in double - a thread adds at most 8 terms per pass over a grid of up to 1024 blocks x 256
# threads (n_elements / 2^18 passes; twice that where the channels-last scalar path pads a pixel's lanes to a power of two),
# then 6 shuffle levels of the wave and 3 additions over the four waves -
#     K = n_elements / 2^17 + 8 + 9
# so |S - S_ref| <= sum_i e_i + K u32 sum_i |term_i| with e_i the error of term i itself, and the quotient is rounded once.
def _depth(n_elements):
    return n_elements / 2.0 ** 17 + 17


def _loss_bound(term_err, terms, divisor, loss_ref, n_elements):
    s = term_err.sum() + _depth(n_elements) * U32 * terms.abs().sum()
    lr = loss_ref if math.isfinite(float(loss_ref)) else 0.0
    return SAFETY * (s / divisor + U32 * abs(float(lr)))


def _exp_rel(arg):
    """relative error of the kernels' exp of an fp32 argument: the argument's own rounding and the product with log2 e
    (2 u32 |arg|) and the hardware exp2 (1 ulp) - (2 |arg| + 4) u32"""
    return (2 * arg.abs() + 4) * U32


def ce_bounds(r, pred64, out_dtype, upstream=1.0):
    """cross-entropy: per pixel  lse = m + log s,  s = sum_c exp(x_c - m)  (m: the running maximum; the planar kernel rescales s
    once per 8 channels by exp(m_old - m_new), exponents that telescope to at most the spread max - min).
      s:    every exp has |arg| <= spread: relative (2 spread + 4) u32; the rescales 2 spread u32 + 4 u32 each; C additions:
            eps_s = (4 spread + C + 4 ceil(C / 8) + 8) u32
      lse:  log s absolute eps_s + 4 u32 (1 + log s) (hardware log2 and the product with ln 2), the addition u32 |lse|
      term: lse - x[label], one more rounding u32 |term|
    gradient  (exp(x - lse) - [c == label]) * k,  k = fl(coef * upstream):
      p = exp(x - lse): argument off by e_lse + u32 |x - lse| -> relative; the exp itself (2 |arg| + 4) u32
      p - onehot: u32 |p - onehot|;  k: the rounded coefficient and the product, then the product with k: 3 u32 |ref|; the store."""
    C = pred64.shape[1]
    spread = pred64.amax(1) - pred64.amin(1)
    logs = r["lse"] - pred64.amax(1)
    eps_s = (4 * spread + C + 4 * math.ceil(C / 8) + 8) * U32
    e_lse = eps_s + 4 * U32 * (1 + logs) + U32 * r["lse"].abs()
    term_err = (e_lse + U32 * r["terms"].abs()) * r["valid"]
    nv = max(r["n_valid"], 1)
    loss_b = _loss_bound(term_err, r["terms"], nv, r["loss"], pred64.numel())
    arg = pred64 - r["lse"].unsqueeze(1)
    k = abs(float(r["coef"]) * upstream)
    ref = r["grad"] * upstream
    e_p = r["p"] * (e_lse.unsqueeze(1) + U32 * arg.abs() + _exp_rel(arg)) + ETA32
    grad_b = SAFETY * (k * (e_p + U32 * (r["p"] - r["onehot"]).abs()) * r["valid"].unsqueeze(1) + 3 * U32 * ref.abs()
                       + store(out_dtype, ref))
    return loss_b, grad_b


def l1_bounds(r, pred64, out_dtype, upstream=1.0):
    """masked L1: a term is one subtraction (u32 |term|; its sign is the exact sign); the gradient sign * k carries the rounded
    coefficient and the product with the upstream gradient (3 u32 |ref|) and the store"""
    term_err = U32 * r["terms"]
    loss_b = _loss_bound(term_err, r["terms"], max(r["n_valid"], 1), r["loss"], pred64.numel())
    ref = r["grad"] * upstream
    return loss_b, SAFETY * (3 * U32 * ref.abs() + store(out_dtype, ref))


def normals_bounds(r, pred64, out_dtype, norm, upstream=1.0):
    """normals: per pixel  n = sqrt(sum x^2)  (C fused additions and the root: (C / 2 + 1) u32 relative),  q = n + 1e-12
    (one more; the fp32 constant 1e-12f is off by u32 of itself): eps_q = (C + 3) u32;  t = x / q: e_t = (C + 4) u32 |t|;
    d = t - label: e_d = e_t + u32 |d|;  term |d|: e_d, or d^2: 2 |d| e_d + u32 d^2.
    gradient  (g_k - gt u_k) / q * k  with g = sign(d) or 2 d, gt = sum_c g_c t_c, u = x / n:
      e_g: 0 for a sign - but where |d| <= 2 e_d the fp32 sign may differ from the fp64 one: 2 there - or 2 e_d
      e_gt = sum_c (|g_c| e_t + e_g |t_c|) + C u32 sum_c |g_c t_c|;   e_u = (C + 3) u32 |u|
      e_num = e_g + e_gt |u| + |gt| e_u + u32 |gt u| + u32 |num|
      out: (e_num + |num| (eps_q + u32)) / q * k, then the two products with k (3 u32 |ref|) and the store."""
    C = pred64.shape[1]
    valid = r["valid"]
    t, d, g, gt, unit, q = r["t"], r["d"], r["g"], r["gt"], r["unit"], r["q"]
    e_t = (C + 4) * U32 * t.abs()
    e_d = e_t + U32 * d.abs()
    term_err = (e_d if norm == 1 else 2 * d.abs() * e_d + U32 * d * d) * valid
    div = max(r["n_valid"], 1e-6)
    loss_b = _loss_bound(term_err, r["terms"], div, r["loss"], pred64.numel())
    e_g = (torch.where(d.abs() <= 2 * e_d, 2.0, 0.0) if norm == 1 else 2 * e_d) * valid
    e_gt = (g.abs() * e_t + e_g * t.abs()).sum(1, keepdim=True) + C * U32 * (g * t).abs().sum(1, keepdim=True)
    e_u = (C + 3) * U32 * unit.abs()
    num = g - gt * unit
    e_num = e_g + e_gt * unit.abs() + gt.abs() * e_u + U32 * (gt * unit).abs() + U32 * num.abs()
    k = abs(float(r["coef"]) * upstream)
    ref = r["grad"] * upstream
    grad_b = SAFETY * ((e_num + num.abs() * (C + 4) * U32) / q * k + 3 * U32 * ref.abs() + store(out_dtype, ref))
    return loss_b, grad_b


def bce_bounds(r, pred64, out_dtype, upstream=1.0):
    """balanced BCE: term = x ([x >= 0] - y) + log1p(e), e = exp(-|x|): the product is exact, e carries (2 |x| + 4) u32
    relative (+ the flush below 2^-126), log1p a few ulps (4 u32 log1p(e)), the addition u32 |term|.  The loss weighs the two
    sums by w and 1 - w (double, in the finalize launch).
    gradient (sigmoid(x) - y) * k: sigmoid = 1 / (1 + e) or e / (1 + e): sg ((2 |x| + 8) u32) (e's error, the addition, the
    reciprocal, the product), the subtraction u32 |sg - y|, then the rounded coefficient and two products 3 u32 |ref|; the store."""
    x = pred64
    e = r["e"]
    term_err = e * _exp_rel(x) + ETA32 + 4 * U32 * torch.log1p(e) + U32 * r["terms"].abs()
    numel = x.numel()
    w = float(r["w"])
    yf = r["y"].double()
    depth = _depth(numel) * U32
    s = (w * ((term_err + depth * r["terms"].abs()) * yf).sum() + (1 - w) * ((term_err + depth * r["terms"].abs()) * (1 - yf)).sum())
    loss_b = SAFETY * (s / numel + U32 * abs(float(r["loss"])))
    ref = r["grad"] * upstream
    k = r["k"].abs() * abs(upstream)
    sg = r["sg"]
    grad_b = SAFETY * (k * (sg * (2 * x.abs() + 8) * U32 + ETA32 + U32 * (sg - yf).abs()) + 3 * U32 * ref.abs() + store(out_dtype, ref))
    return loss_b, grad_b


UPSTREAMS = (1.0, 65536.0, float(torch.tensor(1.0 / 3.0)))


def upstream_fits(r, out_dtype, upstream):
    """a scaled gradient must fit the dtype it is stored in: 65536 x a gradient of 1 (one valid pixel) is past the fp16 range
    (65504), where a GradScaler would see the overflow and skip the step.  Such a combination has no finite reference to be
    compared with and is left out - the only narrowing of the inputs; no factor changes."""
    return float(r["grad"].abs().max() * abs(upstream)) < 0.5 * torch.finfo(out_dtype).max


def bounds(kind, r, pred64, out_dtype, extra=None, upstream=1.0):
    if kind == "ce":
        return ce_bounds(r, pred64, out_dtype, upstream)
    if kind == "l1":
        return l1_bounds(r, pred64, out_dtype, upstream)
    if kind == "normals":
        return normals_bounds(r, pred64, out_dtype, extra, upstream)
    return bce_bounds(r, pred64, out_dtype, upstream)


# ------------------------------------------------------------------------------------------------------------ edge cases
def edge_cases():
    """(name, kind, pred float32 NCHW, label, extra, pred dtypes, expectation) - expectation: None (plain value check),
    "nan" (loss NaN, gradient exactly zero), "zero" (loss exactly 0, gradient exactly zero), ("bad", n): n bad labels, result
    equal to the same input with those labels set to 255"""
    out = []
    every = DTYPES
    size = (2, 3, 7)
    for kind, C, extra in (("ce", 7, None), ("ce", 40, None), ("l1", 1, None), ("normals", 3, 1), ("normals", 3, 2)):
        pred, label = make_inputs(kind, C, size, seed=3)
        ign = torch.full_like(label, float(IGNORE))
        out.append((f"{kind}{C}-all-ignored-{extra}", kind, pred, ign, extra, every, "zero" if kind == "normals" else "nan"))
        one = ign.clone()
        one.view(-1)[5] = label.view(-1)[5] if label.view(-1)[5] != IGNORE else 1.0
        out.append((f"{kind}{C}-one-valid-{extra}", kind, pred, one, extra, every, None))
    for C in (7, 40):
        pred, label = make_inputs("ce", C, size, seed=4)
        label.view(-1)[[0, 9, 20, 33]] = torch.tensor([300.0, -3.0, float(C), 254.0 if C < 254 else 256.0])
        out.append((f"ce{C}-bad-labels", "ce", pred, label, None, every, ("bad", 4)))
    pred, label = make_inputs("ce", 21, size, seed=5)
    sign = torch.where(torch.rand(pred.shape, generator=_gen(5)) < 0.5, -1.0, 1.0)
    out.append(("ce21-logits-1e4", "ce", sign * 1e4, label, None, [torch.float32], None))
    out.append(("ce21-logits-6e4", "ce", sign * 6e4, label, None, [torch.float16], None))
    pred, label = make_inputs("bce", 1, size, seed=6)
    out.append(("bce-abs-100", "bce", torch.where(pred >= 0, 100.0, -100.0), label, None, every, None))
    out.append(("bce-all-positive", "bce", pred, torch.ones_like(label), None, every, None))
    out.append(("bce-all-negative", "bce", pred, torch.zeros_like(label), None, every, None))
    pred, label = make_inputs("l1", 1, size, seed=7)
    eq = pred.clone()
    eq.view(-1)[::3] = label.view(-1)[::3].half().float()        # exact equality that survives every pred dtype: 255 or a half
    lab = label.clone()
    lab.view(-1)[::3] = eq.view(-1)[::3].bfloat16().float()
    eq.view(-1)[::3] = lab.view(-1)[::3]
    out.append(("l1-equal", "l1", eq, lab, None, every, None))
    for norm in (1, 2):
        pred, label = make_inputs("normals", 3, size, seed=8)
        pred[0, :, 1, 2] = 0.0
        pred[1, :, 0, 0] = 0.0
        out.append((f"normals-zero-vector-{norm}", "normals", pred, label, norm, [torch.float32], None))
    return out
