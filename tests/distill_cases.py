"""The distillation loss's closed forms, cases and error bounds, imported by test_distill_cpu.py / test_distill_loss_gpu.py (not a
conftest: nothing here runs by itself).

* closed forms, value AND gradient, of the two teacher terms of pretrain/models/losses.py:50-68 as include/m3vit_hip.h states
  them (m3_loss_distill_fwd / _bwd).  Each computes in the dtype it is given (float64: the reference; float32: torch's own fp32
  evaluation, which test_distill_cpu.py holds to the bounds the kernels are held to).
* the case table: the (B, C) shapes of pretrain_cases.LOSS_SHAPES, soft at tau 1 and 3 and hard, and the (student, teacher)
  dtype pairs - the diagonal and an fp32 student under a 16-bit teacher.
* the error-bound builders, each next to its derivation from the kernel's operation count (U32, store(), SAFETY come from
  kernel_contract and are never tuned per test).
"""
import math

import torch

from kernel_contract import SAFETY, U32, store
from pretrain_cases import ETA32, LOSS_SHAPES, _exp_rel, _gen

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
KINDS = [("soft", 1.0), ("soft", 3.0), ("hard", 1.0)]
DTYPE_PAIRS = [(F32, F32), (F16, F16), (BF16, BF16), (F32, F16)]          # (student, teacher)
SHAPES = LOSS_SHAPES


def kind_id(k):
    return k[0] if k[0] == "hard" else f"soft-tau{k[1]:g}"


def pair_id(p):
    return "-".join(str(d).split(".")[-1] for d in p)


def make_teacher(B, C, seed=0):
    """float32 [B, C] ~ N(0, 3^2), on the CPU: another stream than pretrain_cases.make_logits"""
    return torch.randn(B, C, generator=_gen(5000 * seed + 17 * B + C + 3)) * 3


# ------------------------------------------------------------------------------------------------------ the closed forms
def argmax_low(t):
    """the row argmax with ties to the lowest index, without relying on torch.argmax's tie rule"""
    C = t.shape[1]
    idx = torch.arange(C).unsqueeze(0).expand_as(t)
    return torch.where(t == t.amax(1, keepdim=True), idx, torch.full_like(idx, C)).amin(1)


def distill_ref(x, t, kind, tau=1.0):
    """value, gradient (upstream 1) and what the bound builders need, in x's dtype.
    soft: loss = tau^2 / (B C) sum_i [ sum_c q_ic (t_ic - x_ic) / tau - lse(t_i / tau) + lse(x_i / tau) ], q = softmax(t / tau);
          d x = (softmax(x / tau) - q) tau / (B C)
    hard: loss = (1 / B) sum_i [ lse(x_i) - x_i[y_i] ], y_i = argmax_c t_ic (ties to the lowest index);
          d x = (softmax(x_i) - onehot(y_i)) / B"""
    B, C = x.shape
    t = t.to(x.dtype)
    if kind == "soft":
        xs, ts = x / tau, t / tau
        lx, lt = torch.logsumexp(xs, 1), torch.logsumexp(ts, 1)
        p, q = torch.exp(xs - lx.unsqueeze(1)), torch.exp(ts - lt.unsqueeze(1))
        d = ts - xs
        terms = (q * d).sum(1) - lt + lx
        return dict(kind=kind, tau=tau, loss=terms.sum() * (tau * tau) / (B * C), grad=(p - q) * (tau / (B * C)), lse=lx, lse_t=lt,
                    p=p, q=q, d=d, xs=xs, ts=ts, terms=terms, coef=tau / (B * C))
    y = argmax_low(t)
    lx = torch.logsumexp(x, 1)
    p = torch.exp(x - lx.unsqueeze(1))
    oh = torch.zeros_like(x)
    oh[torch.arange(B), y] = 1.0
    terms = lx - x.gather(1, y.unsqueeze(1)).squeeze(1)
    return dict(kind=kind, tau=1.0, loss=terms.sum() / B, grad=(p - oh) / B, lse=lx, y=y, p=p, q=oh, xs=x, terms=terms,
                coef=1.0 / B)


# --------------------------------------------------------------------------------------------------- error-bound builders
# Common form (kernel_contract): the reference is fp64 on the dtype-ROUNDED inputs, so only the kernel's own arithmetic is
# charged.
#
# A row of C values is reduced by one workgroup of 256 threads: a thread takes units t, t + 256, ... of V = 1, 4 or 8 elements
# (8 as soon as the student or the teacher is 16-bit and C % 8 == 0), adds a unit's V terms in order, then 6 shuffle levels of
# the wave and 3 additions over the four waves: every term passes through at most
#     K = C / 256 + 17            (V = 1: C / 256 + 1 + 9;  V = 4: C / 1024 + 1 + 3 + 9;  V = 8: C / 2048 + 1 + 7 + 9)
# fp32 additions.
def _depth(C):
    return C / 256.0 + 17


def scaled_lse_bound(xs64, lse64):
    """lse of v = fl(x fl(1 / tau)) against lse(x / tau): the scaling is off by 2 u32 |x / tau| per element (the rounded
    reciprocal, the product), which moves the lse by at most 2 u32 max|x / tau|; then pretrain_cases.lse_bound's derivation with
    this file's K: every exp has |arg| <= spread, (2 spread + 4) u32 relative; the rescalings of the running maximum telescope
    (2 spread u32, 4 u32 per unit, C / 256 + 1 units) and one more by exp(m - M); K additions:
        eps_s = (6 spread + K + 4 (C / 256 + 1) + 8) u32
    log s: eps_s + 4 u32 (1 + log s); the addition u32 |lse|."""
    C = xs64.shape[1]
    spread = xs64.amax(1) - xs64.amin(1)
    logs = lse64 - xs64.amax(1)
    eps_s = (6 * spread + _depth(C) + 4 * (C / 256.0 + 1) + 8) * U32
    return eps_s + 4 * U32 * (1 + logs) + U32 * lse64.abs() + 2 * U32 * xs64.abs().amax(1)


def _prob_err(prob, vs64, lse64, e_lse):
    """a probability exp(v - lse): the argument is off by the lse's error, the scaling of v (2 u32 |v|) and its own rounding
    (u32 |arg|); the exp itself (2 |arg| + 4) u32; a flush below 2^-126"""
    arg = vs64 - lse64.unsqueeze(1)
    return prob * (e_lse.unsqueeze(1) + 2 * U32 * vs64.abs() + U32 * arg.abs() + _exp_rel(arg)) + ETA32


def distill_bounds(r, out_dtype, upstream=1.0):
    """(loss bound, gradient bound, student-lse bound) of m3_loss_distill_fwd / _bwd; r = distill_ref of the rounded inputs in
    float64.
    soft: term = fl(dot + fl(lse_x - lse_t)), dot = sum_c fma(q_c, d_c, .) with q_c = exp(ts_c - lse_t), d_c = fl(ts_c - xs_c):
            sum_c (e_q |d| + q e_d), e_d = u32 |d| + 2 u32 (|ts| + |xs|) (the subtraction and the two scalings);
            the sum (K + 1) u32 sum|q d| (one more for an evaluation that rounds the products: torch's);
            e_lse_x + e_lse_t + u32 |lse_x - lse_t| + u32 |term|
    hard: term = fl(lse_x - x_y): e_lse_x + u32 |term|
    the loss: rows added in double, the scale applied in double, one rounding.
    gradient  fl(fl(p - q) k), k = fl(coef * upstream): p (and, soft, q) as _prob_err; hard: q is an exact 0 / 1;
      the subtraction u32 |p - q|;  k: the rounded coefficient and two products 3 u32 |ref|;  the store."""
    xs = r["xs"]
    B, C = xs.shape
    K = _depth(C)
    e_lx = scaled_lse_bound(xs, r["lse"])
    p, q = r["p"], r["q"]
    e_p = _prob_err(p, xs, r["lse"], e_lx)
    if r["kind"] == "soft":
        ts, d = r["ts"], r["d"]
        e_lt = scaled_lse_bound(ts, r["lse_t"])
        e_q = _prob_err(q, ts, r["lse_t"], e_lt)
        e_d = U32 * d.abs() + 2 * U32 * (ts.abs() + xs.abs())
        term_err = ((e_q * d.abs() + q * e_d).sum(1) + (K + 1) * U32 * (q * d).abs().sum(1) + e_lx + e_lt
                    + U32 * (r["lse"] - r["lse_t"]).abs() + U32 * r["terms"].abs())
        scale = r["tau"] ** 2 / (B * C)
    else:
        e_q = torch.zeros_like(q)
        term_err = e_lx + U32 * r["terms"].abs()
        scale = 1.0 / B
    lr = float(r["loss"]) if math.isfinite(float(r["loss"])) else 0.0
    loss_b = SAFETY * (scale * term_err.sum() + U32 * abs(lr))
    ref = r["grad"] * upstream
    inner = e_p + e_q + U32 * (p - q).abs()
    grad_b = SAFETY * (r["coef"] * abs(upstream) * inner + 3 * U32 * ref.abs() + store(out_dtype, ref))
    return loss_b, grad_b, SAFETY * e_lx
