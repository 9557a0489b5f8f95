"""Contract checks for the HIP kernels, imported by the test modules (not a conftest: nothing here runs by itself).

* guarded(rows, cols, dtype, ld) - an output view inside one allocation whose guards, row padding and the view itself start
  out as a sentinel bit pattern (a NaN payload torch never produces).  check() then proves, bitwise, that the call wrote
  nothing outside the view; keep_rows= names rows of the view that must ALSO keep the sentinel (the rows a scatter does
  not own, the slack rows of a grouped call).  Both guards hold at least 256 rows x ld elements - the largest row tile -
  so a tile that runs past its rows lands in memory the test owns and is found after a normal completion.
* guarded_ws(n) - a workspace of exactly the n elements the library reports, sentinel-filled, followed by a guard.
* assert_within(out, ref64, bound64) - the elementwise check |out - ref| <= bound, NaN counting as a failure.
* the error-bound builders, one per kernel family (derivations next to each).
* snapshot() / unchanged() - the inputs of a call keep their bits.
"""
import math

import torch

U32 = 2.0 ** -24
_U = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SAFETY = 2.0                     # one fixed factor over every modelled term; never tuned per test

# sentinel payloads: quiet NaNs (fp) / a fixed word (int32) that differ from torch's canonical NaN (0x7FC00000 / 0x7E00 /
# 0x7FC0), so neither a NaN prefill nor a computed NaN passes for "untouched"
_SENT = {torch.float32: (torch.int32, 0x7FA5A5A5), torch.float16: (torch.int16, 0x7E5A),
         torch.bfloat16: (torch.int16, 0x7FA5), torch.int32: (torch.int32, 0x5A5A5A5A)}
GUARD_ROWS = 256
ALIGN = 256                      # bytes: the view starts where a fresh torch allocation would


# half the smallest subnormal step: the absolute rounding error of a store that underflows
_ETA = {torch.float32: 2.0 ** -150, torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134}


def u(dtype):
    """unit roundoff of a storage dtype (round to nearest)"""
    return _U[dtype]


def store(dtype, v):
    """the error of rounding v to dtype: u |v| above the normal range, plus half a subnormal step where it underflows"""
    return u(dtype) * v.abs() + _ETA[dtype]


def _ival(dtype):
    it, v = _SENT[dtype]
    return it, v


class _Guarded:
    def __init__(self, body, guard, dtype, device):
        it, self.pattern = _ival(dtype)
        es = torch.empty(0, dtype=dtype).element_size()
        slack = ALIGN // es
        lead = -(-guard // slack) * slack
        self.buf = torch.empty(lead + body + guard + slack, dtype=dtype, device=device)
        self.ibuf = self.buf.view(it)
        self.ibuf.fill_(self.pattern)
        shift = (-(self.buf.data_ptr() + lead * es) % ALIGN) // es
        self.start = lead + shift
        self.body = body

    def _bad(self, owned):
        """index (into buf) of the first element outside `owned` (bool mask over buf) whose bits changed, or None"""
        bad = (self.ibuf != self.pattern) & ~owned
        if not bool(bad.any()):
            return None, 0
        idx = bad.nonzero()
        return int(idx[0]), int(idx.numel())


def guarded(rows, cols, dtype, ld=None, device="cuda"):
    """(view [rows, cols] with row stride ld, check).  The view itself starts sentinel-filled too."""
    ld = cols if ld is None else ld
    assert ld >= cols
    g = _Guarded(rows * ld, GUARD_ROWS * max(ld, 1), dtype, device)
    view = torch.as_strided(g.buf, (rows, cols), (ld, 1), g.start)

    def check(keep_rows=None, what="output"):
        owned = torch.zeros(g.buf.numel(), dtype=torch.bool, device=g.buf.device)
        torch.as_strided(owned, (rows, cols), (ld, 1), g.start).fill_(True)
        if keep_rows is not None:
            kr = torch.as_tensor(keep_rows, dtype=torch.long, device=g.buf.device)
            if kr.numel():
                torch.as_strided(owned, (rows, cols), (ld, 1), g.start)[kr] = False
        i, n = g._bad(owned)
        if i is not None:
            r, c = divmod(i - g.start, ld)
            where = ("leading guard" if r < 0 else "trailing guard" if r >= rows else
                     "row padding" if c >= cols else "a row the call does not own")
            raise AssertionError(f"{what}: {n} element(s) outside the written region changed; first at (row {r}, col {c}) "
                                 f"relative to the view [{rows}, {cols}] ld {ld}: {where}")
    return view, check


def guarded_ws(n, dtype=torch.float32, device="cuda"):
    """(workspace of exactly n elements, check): sentinel-filled (a read of a slot the kernel did not write first shows as
    NaN), followed by a guard of at least 64 Ki elements (one 256 x 256 fp32 slab tile)."""
    g = _Guarded(n, max(65536, n // 4), dtype, device)
    view = g.buf[g.start:g.start + n]

    def check(what="workspace"):
        owned = torch.zeros(g.buf.numel(), dtype=torch.bool, device=g.buf.device)
        owned[g.start:g.start + n] = True
        i, cnt = g._bad(owned)
        if i is not None:
            raise AssertionError(f"{what}: {cnt} element(s) outside the reported {n} changed; first at offset {i - g.start}")
    return view, check


def sentinel_like(t):
    """a tensor of t's shape and dtype holding the sentinel bits (for comparisons of untouched rows)"""
    it, v = _ival(t.dtype)
    return torch.full(t.shape, v, dtype=it, device=t.device).view(t.dtype)


def same_bits(a, b):
    """bitwise equality (NaNs included)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.is_floating_point:
        it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        return torch.equal(a.contiguous().view(it), b.contiguous().view(it))
    return torch.equal(a, b)


def snapshot(**tensors):
    """bit copies of a call's inputs; unchanged(snap, **same tensors) asserts the call left them alone"""
    return {k: (v, v.clone()) for k, v in tensors.items() if v is not None}


def unchanged(snap):
    for k, (live, copy) in snap.items():
        assert same_bits(live, copy), f"input {k} was modified by the call"


def assert_within(out, ref64, bound64, what="output"):
    """|out - ref| <= bound elementwise (NaN / Inf in out fail).  Returns the worst err / bound ratio."""
    o = out.detach().double().cpu()
    r = ref64.detach().double().cpu().expand_as(o)
    b = torch.as_tensor(bound64).double().cpu().expand_as(o).clamp_min(1e-300)
    err = (o - r).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    ratio = err / b
    bad = ~(err <= b)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if bool(bad.any()):
        j = int(ratio.flatten().argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(j), o.shape)) if o.dim() else ()
        raise AssertionError(f"{what}: {int(bad.sum())} of {o.numel()} elements exceed their bound; worst at {idx}: "
                             f"got {float(o.flatten()[j])!r}, ref {float(r.flatten()[j])!r}, bound {float(b.flatten()[j]):.3e}, "
                             f"err/bound {worst:.3g}")
    return worst


# --------------------------------------------------------------------------------------------------- error-bound builders
# Common form.  The reference is fp64 on the dtype-ROUNDED inputs, so only the kernel's own arithmetic is charged:
#   * an fp32 sum of K products (any order, products exact or rounded once): |err| <= K * u32 * sum_k |a_k| |b_k|
#     (the classic recursive-summation bound, order independent);
#   * every rounding the documented arithmetic performs on a value v: u_dtype * |v|;
#   * an error e in the argument of a function f carried through: |f'| * e;
# and the sum of the terms is multiplied by SAFETY.

def gemm_bound(A, B, ref, out_dtype, *, K=None, gain=None, extra=None, absacc=None):
    """m3_gemm_nt / m3_wgrad_tn, C = epi(A @ B^T).  A [M, K], B [N, K] (fp64 copies of the rounded operands, gathered /
    scaled as the call reads them); ref = the fp64 result; out_dtype = the stored dtype.
      acc  = K * u32 * |A| @ |B|^T          the fp32 contraction (MFMA products of fp16 / bf16 / fp32 inputs are exact)
      gain = |d out / d acc| of the epilogue (GELU', the row factor, the GELU'(pre) factor), elementwise, default 1
      out  = u_out * |ref| (+ underflow)    the store (kernel_contract.store)
      extra: the epilogue's other roundings, elementwise (e.g. u32 * |acc + bias| for the fp32 bias add, u32 * |residual|
             for the fp32 residual add, u_act * |scaled operand| where an operand is rounded to the activation dtype)
    absacc: |A| @ |B|^T computed by the caller (grouped calls: one product per group; A, B are then not used); K may then be
    a tensor that broadcasts (the contraction length of each group)"""
    if absacc is None:
        absacc = A.abs() @ B.abs().transpose(-2, -1)
    K = A.shape[-1] if K is None else K
    acc = K * U32 * absacc
    if gain is not None:
        acc = acc * gain
    t = acc + store(out_dtype, ref)
    if extra is not None:
        t = t + extra
    return SAFETY * t


def gelu_eval_extra(lin):
    """fp32 GELU = 0.5 x (1 + erf(x / sqrt 2)): a few fp32 ulps of x (the 1 + erf cancellation for x < 0 loses relative
    accuracy, not absolute): 4 u32 |x| + 4 u32"""
    return 4 * U32 * (lin.abs() + 1.0)


def layernorm_bound(x, gamma, beta, ref, out_dtype):
    """m3_layernorm_fwd.  x fp32 [T, D]; the kernel sums a row lane-wise (ceil(D / 64) terms per lane) then over a 64-lane
    wave (6 levels): every element passes through h = ceil(D/64) + 6 fp32 additions, so the mean is off by at most
    h * u32 * mean|x| - the cost of centring in fp32, which a large row offset makes the dominant term:
      centre = h * u32 * mean_row|x| * rstd * |gamma|
    the two-pass variance sums non-negative centred squares: relative error h * u32, half of it in rstd, and the
    centred value (x - mu) is rounded once: (h + 2) * u32 * |xhat| * |gamma|; the affine map in fp32: 2 u32 (|y| + |beta|);
    the store: u_out |ref|.  (A one-pass E[x^2] - mu^2 variance loses ~ u32 * mean(x^2) / var of its relative accuracy and
    fails this bound at offsets of 10^2 and more.)"""
    D = x.shape[-1]
    h = -(-D // 64) + 6
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    rstd = 1.0 / (x.var(-1, unbiased=False, keepdim=True) + 1e-6).sqrt()
    g = gamma.double().abs()
    xhat = (x - mu) * rstd
    t = (h * U32 * x.abs().mean(-1, keepdim=True) * rstd * g + (h + 2) * U32 * xhat.abs() * g
         + 2 * U32 * (ref.abs() + beta.double().abs()) + store(out_dtype, ref))
    return SAFETY * t


def attention_fwd_bounds(q, k, v, o_ref, lse_ref, dtype):
    """m3_attention_fwd, one (image, head) batch as [.., N, dh] fp64 tensors of the rounded q / k / v.
      logits s = scale * q k^T in fp32: ds = dh * u32 * scale * |q| |k|^T + 2 u32 |s| (the folded scale * log2 e, the
      exponent argument s - m);  an error ds_j in the logits moves p_j = softmax by p_j * (ds_j - sum p ds) so
      |d o| <= 2 max_j ds_j * (P @ |v|);
      P is rounded to the MFMA input type for the P V product (u_in * P @ |v|), summed over N keys in fp32
      (N * u32 * P @ |v|), exp itself a few ulps (4 u32);  o is stored: u_out |o|.
      lse = m + log(l): max_j ds_j + (N + 4) u32 + u32 |lse|.
    Returns (o_bound, lse_bound)."""
    dh, N = q.shape[-1], k.shape[-2]
    scale = dh ** -0.5
    s = (q @ k.transpose(-2, -1)) * scale
    ds = dh * U32 * scale * (q.abs() @ k.abs().transpose(-2, -1)) + 2 * U32 * s.abs()
    dmax = ds.amax(-1, keepdim=True)
    P = torch.softmax(s, -1)
    pv = P @ v.abs()
    u_in = u(dtype)
    o_b = SAFETY * ((2 * dmax + u_in + (N + 4) * U32) * pv + store(dtype, o_ref))
    lse_b = SAFETY * (dmax.squeeze(-1) + (N + 4) * U32 + U32 * lse_ref.abs())
    return o_b, lse_b


def attention_bwd_bounds(q, k, v, o, d_o, dq_ref, dk_ref, dv_ref, dtype):
    """m3_attention_bwd, [.., N, dh] fp64 tensors (o: the STORED forward output, as the kernel reads it).
    dS = P o (dP - Dl), dP = dO V^T, Dl = rowsum(dO o o).  Every 16-bit / fp32 operand of the four MFMA products (P, dS,
    and the recomputed logits) is off by at most eps_rel of its own magnitude, with
      eps = 4 u_in (P and dS rounded to the MFMA input type, dP and Dl from rounded operands)
            + (N + dh) u32 (fp32 sums over keys and over head dims) + 2 max ds (the recomputed logits, as in the forward)
    so, with |dS| <= Mag = P o (|dO| |V|^T + rowsum(|dO| o |o|)):
      dV = P^T dO           : eps * P^T |dO|
      dQ = scale * dS K     : eps * scale * Mag |K|
      dK = scale * dS^T Q   : eps * scale * Mag^T |Q|
    plus the store u_out |ref|.  Returns (dq_bound, dk_bound, dv_bound)."""
    dh, N = q.shape[-1], k.shape[-2]
    scale = dh ** -0.5
    s = (q @ k.transpose(-2, -1)) * scale
    ds = dh * U32 * scale * (q.abs() @ k.abs().transpose(-2, -1)) + 2 * U32 * s.abs()
    dmax = ds.amax(-1, keepdim=True).amax(-2, keepdim=True)
    P = torch.softmax(s, -1)
    eps = 4 * u(dtype) + (N + dh) * U32 + 2 * dmax
    mag = P * (d_o.abs() @ v.abs().transpose(-2, -1) + (d_o.abs() * o.abs()).sum(-1, keepdim=True))
    dv_b = SAFETY * (eps * (P.transpose(-2, -1) @ d_o.abs()) + store(dtype, dv_ref))
    dq_b = SAFETY * (eps * scale * (mag @ k.abs()) + store(dtype, dq_ref))
    dk_b = SAFETY * (eps * scale * (mag.transpose(-2, -1) @ q.abs()) + store(dtype, dk_ref))
    return dq_b, dk_b, dv_b


def sum_bound(terms_abs_sum, n, ref, out_dtype):
    """an fp32 sum of n terms (column sums, slab reductions, gather-sums, combine): n * u32 * sum|terms| + the store"""
    return SAFETY * (n * U32 * terms_abs_sum + store(out_dtype, ref))
