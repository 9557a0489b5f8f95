"""The pretraining recipe's closed forms, cases and error bounds, imported by test_pretrain_cpu.py / test_pretrain_gpu.py (not a
conftest: nothing here runs by itself).

* closed forms, value AND gradient, of the two cross-entropy forms of csrc/pretrain.hip, the batch mix, the soft target, the
  rank rule of the evaluation update and the EMA, written from the formulas of include/m3vit_hip.h.  Each computes in the
  dtype it is given (float64: the reference; float32: torch's own fp32 evaluation, which test_pretrain_cpu.py holds to the
  bounds the kernels are held to).
* the case tables and the seeded input makers (logits ~ N(0, 3^2)).
* the error-bound builders, each next to its derivation from the kernel's operation count (U32, store(), SAFETY come from
  kernel_contract and are never tuned per test).

No fixture under tests/golden/ was generated from the reference for these: the reference takes Mixup, the two criteria, the
accuracy and the EMA from `timm`, which is not part of the reference's tree and is not available - parity is against the
float64 closed forms below.
"""
import math

import torch

from kernel_contract import SAFETY, U32, store

ETA32 = 2.0 ** -126               # a flushed / subnormal fp32 exp or product

# ------------------------------------------------------------------------------------------------------- the case tables
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
# (B, C): one element; the smallest pair; odd; below / at / above one wave; 16-byte rows; rows that are not 16-byte aligned;
# more than one unit per thread and past 2^14 classes; more rows than the 1024-workgroup grid takes in one pass
LOSS_SHAPES = [(1, 1), (2, 2), (3, 5), (2, 63), (2, 64), (3, 65), (4, 1000), (3, 1003), (2, 21843), (1030, 5)]
SMOOTHINGS = [0.0, 0.1]
MIX_B = [2, 4, 6]
MIX_CHW = [(1, 1, 1), (3, 7, 9), (3, 8, 8), (3, 32, 40)]
MIX_LAMS = [0.0, 0.3, 1.0]
TARGET_C = [2, 10, 1000]
EMA_SIZES = [1, 3, 1023, 1025, 65537]
EMA_DECAYS = [0.0, 0.9, 0.9999, 1.0]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_logits(B, C, seed=0):
    """float32 [B, C] ~ N(0, 3^2), on the CPU"""
    return torch.randn(B, C, generator=_gen(1000 * seed + 31 * B + C)) * 3


def make_labels(B, C, seed=0):
    return torch.randint(0, C, (B,), generator=_gen(2000 * seed + 7 * B + C))


def make_soft_target(B, C, seed=0):
    """a dense target as mixing makes it: two classes per row over a smoothing floor; float32 [B, C]"""
    g = _gen(3000 * seed + 13 * B + C)
    lam = torch.rand(B, generator=g).double()
    ya, yb = torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B,), generator=g)
    return target_ref(ya, yb, lam, C, 0.1, torch.float64).float()


def boxes(H, W):
    """the box cases of the issue as (yl, yh, xl, xh): empty, the full image, an interior one, one touching a corner"""
    return {"empty": (0, 0, 0, 0), "full": (0, H, 0, W), "interior": (H // 4, H - H // 4, W // 4, W - W // 4 - (W > 2)),
            "corner": (H // 2, H, W // 2, W)}


# ------------------------------------------------------------------------------------------------------ the closed forms
def implied_target(label, C, smoothing, dtype):
    """the dense target form (b) implies: s / C everywhere, + (1 - s) at a label in [0, C); a label outside hits nothing"""
    B = label.numel()
    valid = (label >= 0) & (label < C)
    t = torch.full((B, C), smoothing / C, dtype=dtype)
    rows = torch.arange(B)[valid]
    t[rows, label[valid]] += 1.0 - smoothing
    return t, valid


def softce_ref(x, target=None, label=None, smoothing=0.0):
    """value, gradient (upstream 1) and what the bound builders need, in x's dtype.  Dense target (a):
    loss = (1/B) sum_i [S_i lse_i - sum_c t_ic x_ic], S_i = sum_c t_ic; labels (b): loss = (1/B) sum_i [lse_i - (1-s) x_i[y_i]
    - (s/C) sum_c x_ic]; d x = (softmax(x) S - t) / B with (b)'s implied t and S = 1."""
    B, C = x.shape
    lse = torch.logsumexp(x, 1)
    if target is not None:
        t = target.to(x.dtype)
        S = t.sum(1)
        terms = S * lse - (t * x).sum(1)
        n_bad = 0
    else:
        t, valid = implied_target(label, C, smoothing, x.dtype)
        S = torch.ones(B, dtype=x.dtype)
        xy = torch.where(valid, x.gather(1, label.clamp(0, C - 1).unsqueeze(1)).squeeze(1), torch.zeros((), dtype=x.dtype))
        terms = lse - (1.0 - smoothing) * xy - (smoothing / C) * x.sum(1)
        n_bad = int((~valid).sum())
    p = torch.exp(x - lse.unsqueeze(1))
    grad = (p * S.unsqueeze(1) - t) / B
    return dict(loss=terms.sum() / B, grad=grad, lse=lse, S=S, t=t, p=p, terms=terms, n_bad=n_bad, dense=target is not None)


def mix_ref(x, lam, box):
    """x [B, C, H, W], lam [B], box [B, 4] (yl, yh, xl, xh) -> the mixed batch in x's dtype: sample i against B-1-i; an empty
    box blends (lam 1 / 0 are copies), else the partner's pixels inside the box.  Also the mask of the blended elements."""
    B, _, H, W = x.shape
    out = x.clone()
    blended = torch.zeros_like(x, dtype=torch.bool)
    for i in range(B):
        j = B - 1 - i
        yl, yh, xl, xh = (int(v) for v in box[i])
        li = lam[i].to(x.dtype)
        if yl == yh or xl == xh:
            if float(li) == 1.0:
                continue
            if float(li) == 0.0:
                out[i] = x[j]
                continue
            out[i] = li * x[i] + (1 - li) * x[j]
            blended[i] = True
        else:
            out[i, :, yl:yh, xl:xh] = x[j, :, yl:yh, xl:xh]
    return out, blended


def target_ref(y, y_partner, lam, C, smoothing, dtype):
    """t_i = lam_i s(y_i) + (1 - lam_i) s(y_partner_i); s(y) = smoothing / C everywhere, 1 - smoothing + smoothing / C at y"""
    si = implied_target(y, C, smoothing, dtype)[0]
    sj = implied_target(y_partner, C, smoothing, dtype)[0]
    lam = lam.to(dtype).unsqueeze(1)
    return lam * si + (1 - lam) * sj


def label_pair_loss(x, y, y_partner, lam, smoothing):
    """the mixed loss as the label-pair formula: (1/B) sum_i [lam_i ce_s(x_i, y_i) + (1 - lam_i) ce_s(x_i, y_partner_i)]"""
    B, C = x.shape
    lse = torch.logsumexp(x, 1)

    def ce(lab):
        return lse - (1.0 - smoothing) * x.gather(1, lab.unsqueeze(1)).squeeze(1) - (smoothing / C) * x.sum(1)
    lam = lam.to(x.dtype)
    return (lam * ce(y) + (1 - lam) * ce(y_partner)).sum() / B


def rank_ref(x, y):
    """rank of the target logit per row: #{c : x_c > x_y} + #{c < y : x_c == x_y}; a NaN beats every number, an earlier NaN
    beats a later one.  x [B, C] float64 (NaNs allowed), y [B] valid labels.  int64 [B]."""
    B, C = x.shape
    xy = x.gather(1, y.unsqueeze(1))
    c = torch.arange(C).unsqueeze(0)
    before = c < y.unsqueeze(1)
    xnan, ynan = torch.isnan(x), torch.isnan(xy)
    beats = torch.where(xnan, ~ynan | before, ~ynan & ((x > xy) | ((x == xy) & before)))
    return beats.sum(1)


def eval_ref(x, y):
    """[loss_sum, correct1, correct5, count], n_bad and the per-row terms of one evaluation batch; x [B, C], y [B]"""
    B, C = x.shape
    valid = (y >= 0) & (y < C)
    yc = y.clamp(0, C - 1)
    lse = torch.logsumexp(x, 1)
    xy = torch.where(valid, x.gather(1, yc.unsqueeze(1)).squeeze(1), torch.zeros((), dtype=x.dtype))
    terms = lse - xy
    rank = rank_ref(x.double(), yc)
    c1 = int((valid & (rank < 1)).sum())
    c5 = int((valid & (rank < min(5, C))).sum())
    return dict(state=[float(terms.sum()), float(c1), float(c5), float(B)], n_bad=int((~valid).sum()), terms=terms, lse=lse)


def f32(v):
    """a Python number rounded to float32, as a Python float"""
    return float(torch.tensor(v, dtype=torch.float32))


def ema_ref(ema, p, decay):
    """decay * ema + (1 - decay) * p with both factors formed in double and rounded to fp32 (what the host passes)"""
    d, omd = f32(float(decay)), f32(1.0 - float(decay))
    if d == 1.0:
        return ema.clone()
    if d == 0.0:
        return p.to(ema.dtype).clone()
    return d * ema + omd * p.to(ema.dtype)


# --------------------------------------------------------------------------------------------------- error-bound builders
# Common form (kernel_contract): the reference is fp64 on the dtype-ROUNDED inputs, so only the kernel's own arithmetic is
# charged.
#
# A row of C logits is reduced by one workgroup of 256 threads: a thread takes units t, t + 256, ... of V = 1 or 4 elements
# (ceil(C / 256 V) units), adds a unit's V terms in order, then 6 shuffle levels of the wave and 3 additions over the four
# waves: every term passes through at most
#     K = C / 256 + 13            (V = 1: C / 256 + 1 + 9;  V = 4: C / 1024 + 1 + 3 + 9)
# fp32 additions, so a row sum is off by at most K u32 sum|terms| beyond the terms' own errors.
def _depth(C):
    return C / 256.0 + 13


def _exp_rel(arg):
    """relative error of the kernels' exp of an fp32 argument: the argument's rounding and the product with log2 e
    (2 u32 |arg|) and the hardware exp2 - (2 |arg| + 4) u32"""
    return (2 * arg.abs() + 4) * U32


def lse_bound(x64, lse64):
    """lse = M + log s, s = sum_c exp(x_c - M) accumulated against a per-thread running maximum:
      every exp has |arg| <= spread = max - min: (2 spread + 4) u32 relative; a thread rescales s once per unit by
      exp(m_old - m_new), exponents that telescope to at most spread (2 spread u32 in all, 4 u32 per unit, C / 256 + 1 units),
      and once more by exp(m - M) ((2 spread + 4) u32); K additions:
          eps_s = (6 spread + K + 4 (C / 256 + 1) + 8) u32
      log s: eps_s + 4 u32 (1 + log s) (hardware log2, the product with ln 2); the addition: u32 |lse|."""
    C = x64.shape[1]
    spread = x64.amax(1) - x64.amin(1)
    logs = lse64 - x64.amax(1)
    eps_s = (6 * spread + _depth(C) + 4 * (C / 256.0 + 1) + 8) * U32
    return eps_s + 4 * U32 * (1 + logs) + U32 * lse64.abs()


def softce_bounds(r, x64, out_dtype, smoothing=0.0, upstream=1.0):
    """(loss bound, gradient bound) of m3_loss_softce_fwd / _bwd; r = softce_ref of the rounded inputs in float64.
    dense:  term = fma(S, lse, -dot), dot = sum t x by fma (products exact), S = sum t:
              |S| e_lse + K u32 (sum|t| |lse| + sum|t x|) + u32 |term|  -  one more u32 on each sum for an evaluation that
              rounds the products (torch's), so K + 1
    labels: term = fma(-w_off, sum x, fma(-w_on, x_y, lse)) with w_on = fl(1 - s), w_off = fl(s / C):
              e_lse + |w_off| K u32 sum|x| + 2 u32 (|lse| + |w_on x_y| + |w_off| sum|x|)   (the two weights' and the two fmas'
              roundings, each of at most u32 of the magnitudes it combines)
    the loss: rows added in double, the quotient rounded once.
    gradient  fma(p, S, -t) * k,  p = exp(x - lse),  k = fl(coef * upstream):
      p: argument off by e_lse + u32 |x - lse|, the exp itself (2 |arg| + 4) u32, a flush below 2^-126
      S: K u32 sum|t| (dense; exact 1 for labels);  t (labels): w_off + w_on, three roundings: 3 u32 |t|
      the fma u32 |p S - t|;  k: the rounded coefficient and two products 3 u32 |ref|;  the store."""
    B, C = x64.shape
    K = _depth(C)
    e_lse = lse_bound(x64, r["lse"])
    t, S = r["t"], r["S"]
    if r["dense"]:
        term_err = (S.abs() * e_lse + (K + 1) * U32 * (t.abs().sum(1) * r["lse"].abs() + (t * x64).abs().sum(1))
                    + U32 * r["terms"].abs())
        e_S = (K + 1) * U32 * t.abs().sum(1)
        e_t = torch.zeros_like(t)
    else:
        w_off = smoothing / C
        mag = r["lse"].abs() + (t.amax(1) - w_off) * x64.abs().amax(1) + w_off * x64.abs().sum(1)
        term_err = e_lse + w_off * (K + 1) * U32 * x64.abs().sum(1) + 2 * U32 * mag
        e_S = torch.zeros_like(S)
        e_t = 3 * U32 * t.abs()
    lr = float(r["loss"]) if math.isfinite(float(r["loss"])) else 0.0
    loss_b = SAFETY * (term_err.sum() / B + U32 * abs(lr))
    arg = x64 - r["lse"].unsqueeze(1)
    k = abs(upstream) / B
    ref = r["grad"] * upstream
    p = r["p"]
    e_p = p * (e_lse.unsqueeze(1) + U32 * arg.abs() + _exp_rel(arg)) + ETA32
    inner = S.abs().unsqueeze(1) * e_p + p * e_S.unsqueeze(1) + e_t + U32 * (p * S.unsqueeze(1) - t).abs()
    grad_b = SAFETY * (k * inner + 3 * U32 * ref.abs() + store(out_dtype, ref))
    return loss_b, grad_b


def mix_bound(x64, lam64, ref, blended, out_dtype):
    """m3_mix_batch: a blended element is fma(fl(1 - lam), x_j, fl(lam x_i)): the rounded 1 - lam (u32 |(1 - lam) x_j|), the
    product (u32 |lam x_i|) and the fma (u32 |out| <= u32 (|lam x_i| + |(1 - lam) x_j|)), then the store; every other element
    is a copy: the store alone (0 for an fp32 output - checked bit for bit by the tests)."""
    B = x64.shape[0]
    lam = lam64.view(B, 1, 1, 1)
    mag = (lam * x64).abs() + ((1 - lam) * x64.flip(0)).abs()
    return SAFETY * (2 * U32 * mag * blended + store(out_dtype, ref))


def target_bound(y, y_partner, lam64, C, smoothing):
    """m3_mix_target: off and on are rounded to fp32 (u32 each), then fma(fl(1 - lam), s_j, fl(lam s_i)) as in the blend:
    4 u32 (|lam s_i| + |(1 - lam) s_j|) covers the five roundings of at most u32 of one of the two magnitudes each"""
    si = implied_target(y, C, smoothing, torch.float64)[0]
    sj = implied_target(y_partner, C, smoothing, torch.float64)[0]
    lam = lam64.unsqueeze(1)
    return SAFETY * (4 * U32 * (lam * si + (1 - lam) * sj) + ETA32)


def eval_loss_bound(r, x64):
    """m3_cls_eval_update's loss_sum of one batch: per row lse - x_y (e_lse and one rounding), rows added in double"""
    return SAFETY * float((lse_bound(x64, r["lse"]) + U32 * r["terms"].abs()).sum())


def ema_bound(ref, p64, decay):
    """m3_ema_update, one step from exact inputs: fma(d, ema, fl(omd p)): u32 |omd p| + u32 |out| (+ an underflow)"""
    omd = f32(1.0 - float(decay))
    if f32(float(decay)) in (0.0, 1.0):
        return torch.zeros_like(ref)
    return SAFETY * (U32 * ((omd * p64).abs() + ref.abs()) + ETA32)


def ema_bound_compound(bound_prev, ref, p64, decay):
    """after a further step: the error carried in the shadow is multiplied by d, the step adds its own"""
    return f32(float(decay)) * bound_prev + ema_bound(ref, p64, decay)
