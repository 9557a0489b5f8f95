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
* far_rows(rows, cols, ld_bytes, dtype) / reach_stride(rows) - an operand whose rows lie megabytes apart inside one unfilled
  allocation, so that its last rows start past 2 or 4 GiB from its base (tests/test_far_operands_gpu.py); check_outside()
  proves that a far output wrote nothing between its rows.
* topk_agrees() -a kernel's top-k selection against an fp64 top-k, order free only inside the error bound.
* nonfinite_agrees() / independent_same_bits() - Inf and NaN go through a kernel as through torch: nothing is swallowed (the
  output is NaN / +-Inf exactly where torch's float64 result on the same poisoned inputs is), nothing leaks (an output that
  does not depend on the poisoned input keeps the bits of the clean run).
"""
import math

import torch

U32 = 2.0 ** -24
_U = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SAFETY = 2.0                     # one fixed factor over every modelled term; never tuned per test

# sentinel payloads: quiet NaNs (fp) / a fixed word (int32, int64) that differ from torch's canonical NaN (0x7FC00000 / 0x7E00 /
# 0x7FC0), so neither a NaN prefill nor a computed NaN passes for "untouched"
_SENT = {torch.float32: (torch.int32, 0x7FA5A5A5), torch.float16: (torch.int16, 0x7E5A),
         torch.bfloat16: (torch.int16, 0x7FA5), torch.int32: (torch.int32, 0x5A5A5A5A),
         torch.int64: (torch.int64, 0x5A5A5A5A5A5A5A5A)}      # int64: no index or count (idx, load, counts64, splits) is that large
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


REACH = 1 << 32                  # bytes: what a 32-bit lane offset added to an operand base can address


def reach_stride(rows, reach=REACH):
    """the row stride (bytes) of the "just under the reach" cases: the largest multiple of 16 with (rows + 1) * ld < reach -
    the rule of m3_gemm_nt's A panel and of the weight gradient's LDS-DMA forms.  For rows = 300: 14 268 992, so the rows
    151 .. 299 start above 2^31"""
    return (reach - 1) // (rows + 1) // 16 * 16


class _Far:
    """one byte allocation that operands with a huge row stride are windows of; nothing is filled (fill() does)"""

    def __init__(self, rows, ld_bytes, row_bytes, device="cuda"):
        assert ld_bytes % 16 == 0 and 0 < row_bytes <= ld_bytes
        self.rows, self.ld_bytes = rows, ld_bytes
        self.nbytes = -(-((rows - 1) * ld_bytes + row_bytes) // 16) * 16
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 16 == 0

    def view(self, cols, dtype, col_byte=0):
        """the [rows, cols] window whose row r starts col_byte bytes into row r of the allocation"""
        es = torch.empty(0, dtype=dtype).element_size()
        assert col_byte % 16 == 0 and self.ld_bytes % es == 0
        assert (self.rows - 1) * self.ld_bytes + col_byte + cols * es <= self.nbytes, "the window runs past the allocation"
        flat = self.buf[: self.nbytes // es * es].view(dtype)
        return torch.as_strided(flat, (self.rows, cols), (self.ld_bytes // es, 1), col_byte // es)

    def fill(self, dtype):
        """the sentinel of `dtype` over the whole allocation, in one fill_"""
        it, v = _ival(dtype)
        self.buf.view(it).fill_(v)

    def check_outside(self, windows, dtype, what="far output", chunk_bytes=1 << 28):
        """everything outside the windows [(col_byte, row bytes), ..] of every row still holds fill(dtype)'s sentinel.  Row
        chunks of at most chunk_bytes, so that no temporary comes near 2 GiB"""
        it, v = _ival(dtype)
        ies = torch.empty(0, dtype=it).element_size()
        ld = self.ld_bytes // ies
        words = self.buf.view(it)
        step = max(1, chunk_bytes // self.ld_bytes)
        for r0 in range(0, self.rows, step):
            r1 = min(r0 + step, self.rows)
            part = words[r0 * ld: min(r1 * ld, words.numel())]
            bad = part != v
            for cb, nb in windows:
                torch.as_strided(bad, (r1 - r0, nb // ies), (ld, 1), cb // ies).fill_(False)
            if bool(bad.any()):
                i = int(bad.nonzero()[0])
                r, c = divmod(i, ld)
                raise AssertionError(f"{what}: {int(bad.sum())} word(s) outside the written windows changed; first in row {r0 + r} "
                                     f"at byte {c * ies} of the row (row stride {self.ld_bytes} bytes)")


def far_rows(rows, cols, ld_bytes, dtype, col_byte=0, device="cuda"):
    """(view [rows, cols] of `dtype` whose rows are ld_bytes apart, its allocation): one torch.empty of exactly
    (rows - 1) * ld_bytes + col_byte + cols * es bytes rounded up to 16, of which view.copy_() touches the rows' own bytes
    only - so an operand can reach past 2 and 4 GiB while a few hundred KB of it are ever written.  view.data_ptr() and
    view.stride(0) are what the argument structs take; further operands of the same rows are allocation.view(cols, dtype,
    col_byte) (make the first window the one that ends last)"""
    es = torch.empty(0, dtype=dtype).element_size()
    far = _Far(rows, ld_bytes, col_byte + cols * es, device)
    return far.view(cols, dtype, col_byte), far


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


# ------------------------------------------------------------------------------------- the router (gate.hip, route.hip)
# Every builder takes fp64 tensors of the values the kernel READ (the rounded x, w_gate, and - where a kernel consumes an
# earlier kernel's output - that output as stored), so only the kernel's own arithmetic is charged.
ETA_P = 2.0 ** -126              # absolute error of a probability near the fp32 underflow (a flushed or subnormal exp / quotient)


def gate_logit_bound(x, w, bias=None):
    """m3_gate_fwd's clean logits: acc = bias; acc = fma(x_d, w_de, acc) for d = 0 .. D-1 in order.  D fused roundings, each
    of at most u32 times a partial sum bounded by |b| + sum_d |x_d w_de|, and the stored bias itself (one more term):
      |logit - ref| <= (D + 1) u32 (|b| + |x| @ |w|)
    x [T, D], w [D, E], bias [E] or None (fp64)."""
    D = x.shape[-1]
    a = x.abs() @ w.abs()
    if bias is not None:
        a = a + bias.abs()
    return SAFETY * (D + 1) * U32 * a


def noisy_logit_bound(clean_bound, noise=None, std=0.0, noisy=None):
    """noisy = fl(clean + fl(noise * std)) (one mul, one add): the clean error plus u32 |noise std| + u32 |noisy| (the
    SAFETY factor of clean_bound stays on it)"""
    if noise is None or std == 0.0:
        return clean_bound
    return clean_bound + SAFETY * U32 * ((noise * std).abs() + noisy.abs())


def softmax_bound(nz, delta):
    """p_e = q_e / s, q_e = expf(nz_e - m), m = max nz, s = q_0 + ... + q_{E-1} in order, in fp32; nz [T, E] the fp64
    logits the reference uses, delta [T, E] the bound on the kernel's logit error (0 where the kernel reads stored logits).
      logit error: p_e = softmax(nz + d)_e = p_e (1 + d_e - sum_j p_j d_j + O(d^2)), so at most p_e 2 max_j delta_j;
      nz_e - m rounded: u32 |nz_e - m| relative on q_e, and through s at most u32 max_j p_j |nz_j - m|;
      expf a few ulps (4 u32), the sum of E positive terms E u32, the quotient (or reciprocal and product) 2 u32;
      plus ETA_P where q or p underflow.
      |p_e - ref_e| <= p_e (2 max delta + u32 (|nz_e - m| + max_j p_j |nz_j - m|) + (E + 6) u32) + ETA_P"""
    E = nz.shape[-1]
    m = nz.amax(-1, keepdim=True)
    p = torch.softmax(nz, -1)
    dm = delta.amax(-1, keepdim=True) if torch.is_tensor(delta) else delta
    spread = (p * (nz - m).abs()).amax(-1, keepdim=True)
    rel = 2 * dm + U32 * ((nz - m).abs() + spread) + (E + 6) * U32
    return SAFETY * (p * rel + ETA_P)


def load_prob_terms(clean, noisy, thr_in, thr_out, std):
    """the Normal-CDF load term of one token and expert, evaluated in fp64 on the KERNEL's own clean / noisy logits and its
    probability thresholds (thr_in = top_logits[:, k], thr_out = top_logits[:, k-1], [T, 1]):
      is_in = noisy > thr_in ;  z = (clean - (thr_in if is_in else thr_out)) / std ;  term = Phi(z)
    Returns (is_in, z, Phi(z), its error bound).  The kernel's z = fl(fl(clean - thr) * fl(1 / std)): three roundings,
    |dz| <= 3 u32 |z|, carried by phi(z) |dz|; 0.5 erfc(-z / sqrt 2) adds a few ulps of the result (the scaling
    product and erfcf itself: 6 u32 Phi):
      |term - ref| <= phi(z) 3 u32 |z| + 6 u32 Phi(z) + ETA_P"""
    is_in = noisy > thr_in
    z = (clean - torch.where(is_in, thr_in, thr_out)) / std
    Phi = 0.5 * torch.erfc(-z / math.sqrt(2.0))
    phi = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    return is_in, z, Phi, phi * 3 * U32 * z.abs() + 6 * U32 * Phi + ETA_P


def cv2_reference(v):
    """cv^2(v) = var(v, unbiased) / (mean(v)^2 + 1e-10) and its gradient, fp64 autograd; 0 and zeros for one expert"""
    v = v.detach().double().clone().requires_grad_(True)
    if v.numel() < 2:
        return torch.zeros((), dtype=torch.float64), torch.zeros_like(v.detach())
    cv = v.var(unbiased=True) / (v.mean() ** 2 + 1e-10)
    (g,) = torch.autograd.grad(cv, v)
    return cv.detach(), g


def cv2_bound(v):
    """the balance kernel's cv^2 of v [E] (fp64 copy of the kernel's OWN reduced importance / load, so only the loss
    arithmetic is charged), evaluated in fp32 as written in gate.hip:
      mean = (v_0 + ... + v_{E-1}) / E          dm <= (E + 1) u32 mean|v|
      var  = sum_e (v_e - mean)^2 / (E - 1)     each (v_e - mean) is off by dm + u32 |v_e - mean|; the terms linear in dm
                                                cancel (sum_e (v_e - mean) = 0), so
                                                dvar <= ((E + 4) u32 S + E dm^2) / (E - 1),  S = sum_e (v_e - mean)^2
      den  = mean^2 + 1e-10                     dden <= 2 |mean| dm + 3 u32 den
      cv   = var / den                          dcv <= dvar / den + cv dden / den + u32 cv
    As the variance goes to 0 the relative bound grows without limit: cv -> 0 while the E dm^2 / den floor
    (about E^3 u32^2) stays - the absolute bound is what is checked.
      grad_e = 2 (v_e - mean) / ((E - 1) den) - var 2 mean / (E den^2):
        first term  : 2 (dm + 4 u32 |v_e - mean|) / ((E - 1) den) + |first| dden / den
        second term : 2 |mean| dvar / (E den^2) + |second| (dm / |mean| + 2 dden / den + 5 u32)
    Returns (cv bound (0-dim), grad bound [E]); zeros for one expert (the kernel writes exact zeros)."""
    v = v.double()
    E = v.numel()
    if E < 2:
        return torch.zeros((), dtype=torch.float64), torch.zeros_like(v)
    mean = v.mean()
    dm = (E + 1) * U32 * v.abs().mean()
    c = v - mean
    S = (c * c).sum()
    var = S / (E - 1)
    dvar = ((E + 4) * U32 * S + E * dm * dm) / (E - 1)
    den = mean * mean + 1e-10
    dden = 2 * mean.abs() * dm + 3 * U32 * den
    cv = var / den
    b_cv = dvar / den + cv * dden / den + U32 * cv
    first = 2 * c / ((E - 1) * den)
    second = var * 2 * mean / (E * den * den)
    b1 = 2 * (dm + 4 * U32 * c.abs()) / ((E - 1) * den) + first.abs() * dden / den
    b2 = 2 * mean.abs() * dvar / (E * den * den) + second.abs() * (dm / mean.abs().clamp_min(1e-300) + 2 * dden / den + 5 * U32)
    return SAFETY * b_cv, SAFETY * (b1 + b2 + U32 * (first - second).abs())


def gate_bwd_logits_bound(nz, dp_abs, dp_err, g_err, ref):
    """m3_gate_bwd_logits: d_logits_e = p_e (dp_e - dot) + g_e, dot = sum_j p_j dp_j, all in fp32, from the STORED noisy
    logits nz [T, E] (fp64 copies: no logit error is charged, the softmax is the kernel's own arithmetic of softmax_bound:
    eps_p = (E + 6) u32 + u32 (|nz_e - m| + max_j p_j |nz_j - m|) relative, ETA_P absolute).  [T, E] fp64:
      dp_abs  sum of |contributions| to dp_e: d_score, d_top, balance_scale d_importance, and a threshold term d_thr routed
              to that expert (so A_e = dp_abs_e + sum_j p_j dp_abs_j bounds |dp_e - dot|)
      dp_err  the kernel's error on dp_e: 5 u32 dp_abs_e (the adds and the balance-scale products) plus, at the expert a
              threshold term lands on, that term's error (its fp32 sum over E experts: E u32 sum|g| + sum g_err)
      g_err   the error of the CDF term g_e = d_load_prob_e bscale pdf(z) / std: pdf(z) moves by |z| pdf |dz|,
              |dz| <= 3 u32 |z| (load_prob_terms), plus 8 u32 |g_e| for expf and the four products
      |d - ref| <= p_e A_e (eps_p + (E + 3) u32) + p_e (dp_err_e + sum_j p_j dp_err_j) + g_err_e + u32 |ref| + ETA_P A_e
    ((E + 3) u32: the dot product of E terms, the subtraction, the product and the add of g)."""
    E = nz.shape[-1]
    m = nz.amax(-1, keepdim=True)
    p = torch.softmax(nz, -1)
    spread = (p * (nz - m).abs()).amax(-1, keepdim=True)
    eps_p = (E + 6) * U32 + U32 * ((nz - m).abs() + spread)
    A = dp_abs + (p * dp_abs).sum(-1, keepdim=True)
    t = (p * A * (eps_p + (E + 3) * U32) + p * (dp_err + (p * dp_err).sum(-1, keepdim=True)) + g_err + U32 * ref.abs()
         + ETA_P * A)
    return SAFETY * t


def topk_agrees(idx, logits, bound):
    """idx [T, k] (a kernel's selection, in selection order) against the fp64 logits [T, E] whose kernel-side error is
    at most bound [T, E].  At every step j the chosen expert must not be beaten, beyond both bounds, by any expert not
    chosen before it: logits[c] + bound[c] >= logits[e] - bound[e].  Indices must be distinct and in range.  Returns the
    number of steps at which some other remaining expert lies within the bounds of the chosen one (a near-tie: either
    order is accepted there), so that the caller can assert these are rare."""
    idx = idx.long().cpu()
    L = logits.double().cpu()
    B = torch.as_tensor(bound).double().cpu().expand_as(L)
    T, E = L.shape
    k = idx.shape[1]
    assert bool(((idx >= 0) & (idx < E)).all()), "expert index out of range"
    taken = torch.zeros(T, E, dtype=torch.bool)
    rows = torch.arange(T)
    near = 0
    for j in range(k):
        c = idx[:, j]
        assert not bool(taken[rows, c].any()), f"an expert is selected twice (step {j})"
        lo = L[rows, c] - B[rows, c]
        hi = L[rows, c] + B[rows, c]
        others = ~taken
        others[rows, c] = False
        beat = others & (L - B > hi.unsqueeze(1))
        if bool(beat.any()):
            t = int(beat.any(1).nonzero()[0])
            raise AssertionError(f"top-k step {j}, token {t}: expert {int(c[t])} chosen over "
                                 f"{int(beat[t].nonzero()[0])} whose logit is larger beyond the bound")
        near += int((others & (L + B >= lo.unsqueeze(1))).any(1).sum())
        taken[rows, c] = True
    return near


def _blocks(v, nblk, rows=64):
    """[T, E] -> per-64-row block sums [nblk, E] (fp64 / int64)"""
    T, E = v.shape
    pad = torch.zeros(nblk * rows - T, E, dtype=v.dtype, device=v.device)
    return torch.cat((v, pad)).view(nblk, rows, E).sum(1)


def check_gate_fwd(o, x, w, k, bias=None, noise=None, std=0.0):
    """the value checks of one m3_gate_fwd call (the guards are the caller's).  o: dict of the kernel's outputs as torch
    tensors (idx [T, k] int64, score [T, k], top_logits [T, min(k+1, E)], idx_next [T] or None, idx32 or None, clean /
    noisy / gates [T, E] or None, part_importance / part_load / part_count / part_load_prob [nblk, E] or None);
    x [T, D], w [D, E], bias [E], noise [T, E]: the rounded inputs the kernel read (any dtype; compared in fp64).
    Returns (worst err / bound, near-ties of the top-k)."""
    f64 = torch.float64
    dev = o["idx"].device
    x64, w64 = x.to(dev, f64), w.to(dev, f64)
    b64 = None if bias is None else bias.to(dev, f64)
    T, E = x64.shape[0], w64.shape[1]
    kp = min(k + 1, E)
    noisy_on = noise is not None and std != 0.0
    clean64 = x64 @ w64 + (b64 if b64 is not None else 0.0)
    cb = gate_logit_bound(x64, w64, b64)
    nz64, nb = clean64, cb
    if noisy_on:
        nz64 = clean64 + noise.to(dev, f64) * float(torch.tensor(std, dtype=torch.float32))
        nb = noisy_logit_bound(cb, noise.to(dev, f64), float(torch.tensor(std, dtype=torch.float32)), nz64)
    worst = 0.0
    idx = o["idx"]
    near = topk_agrees(idx, nz64, nb) if T else 0
    if o.get("idx32") is not None:
        assert torch.equal(o["idx32"].long(), idx), "idx32 and idx disagree"
    if o.get("clean") is not None:
        worst = max(worst, assert_within(o["clean"], clean64, cb, "clean logits"))
    if o.get("noisy") is not None:
        want = o["clean"] + (noise * torch.tensor(std, dtype=torch.float32)) if noisy_on else o["clean"]
        assert same_bits(o["noisy"], want), "noisy != fl32(clean + fl32(noise * std))"
    pb = softmax_bound(nz64, nb)
    p64 = torch.softmax(nz64, -1)
    worst = max(worst, assert_within(o["score"], p64.gather(1, idx), pb.gather(1, idx), "score"))
    sel = idx
    if kp > k and o.get("idx_next") is None:
        o = dict(o, top_logits=o["top_logits"][:, :k])       # (without idx_next only the first k columns are pinned)
    elif kp > k:
        nxt = o["idx_next"].long().unsqueeze(1)
        assert not bool((nxt == idx).any(1).any()), "idx_next repeats a selected expert"
        topk_agrees(torch.cat((idx, nxt), 1), nz64, nb)
        sel = torch.cat((idx, nxt), 1)
    worst = max(worst, assert_within(o["top_logits"], p64.gather(1, sel), pb.gather(1, sel), "top_logits"))
    assert same_bits(o["top_logits"][:, :k].contiguous(), o["score"]), "top_logits[:, :k] != score"
    dense_g = torch.zeros(T, E, dtype=torch.float32, device=dev).scatter(1, idx, o["score"])
    if o.get("gates") is not None:
        assert same_bits(o["gates"], dense_g), "gates != score scattered at idx (zeros elsewhere)"
        worst = max(worst, assert_within(o["gates"], p64 * (dense_g != 0), pb, "gates"))
    nblk = o["part_importance"].shape[0]
    g64 = dense_g.double()
    worst = max(worst, assert_within(o["part_importance"], _blocks(g64, nblk),
                                     sum_bound(_blocks(g64.abs(), nblk), 64, _blocks(g64, nblk), torch.float32),
                                     "part_importance"))
    assert torch.equal(o["part_load"].long(), _blocks((dense_g > 0).long(), nblk)), "part_load != block count of gates > 0"
    if o.get("part_count") is not None:
        selm = torch.zeros(T, E, dtype=torch.long, device=dev).scatter(1, idx, 1)
        assert torch.equal(o["part_count"].long(), _blocks(selm, nblk)), "part_count != block count of selected entries"
    if o.get("part_load_prob") is not None:
        top64 = o["top_logits"].double()
        _, _, Phi, perr = load_prob_terms(o["clean"].double(), o["noisy"].double(), top64[:, k:k + 1], top64[:, k - 1:k],
                                          float(torch.tensor(std, dtype=torch.float32)))
        ref = _blocks(Phi, nblk)
        worst = max(worst, assert_within(o["part_load_prob"], ref,
                                         SAFETY * _blocks(perr, nblk) + sum_bound(ref, 64, ref, torch.float32),
                                         "part_load_prob"))
    return worst, near


def gate_bwd_reference(noisy, idx, k, *, clean=None, top_logits=None, idx_next=None, d_score=None, d_top=None,
                       d_importance=None, d_load_prob=None, balance_scale=1.0, noise_std=0.0):
    """(d_logits fp64, its bound) of m3_gate_bwd_logits: fp64 autograd through the softmax of the kernel's STORED noisy
    logits with the kernel's own idx / idx_next and its Normal-CDF decisions and thresholds.  The loss differentiated:
      sum d_score p[idx] + sum d_top p[idx, idx_next] + bs sum_e d_imp_e sum_t gates_te
      + bs sum_e d_lp_e sum_t Phi((clean_te - thr_t) / std),  thr = p[idx_next] (is_in) or p[idx[:, k-1]]
    with clean the leaf and noisy = clean + (stored noisy - stored clean) (the gate's gradient reaches x through both).
    balance_scale: the fp32 value the kernel multiplies by (bscale)."""
    f64 = torch.float64
    nzs = noisy.double()
    T, E = nzs.shape
    lp = d_load_prob is not None
    base = clean.double() if lp else nzs
    leaf = base.clone().requires_grad_(True)
    nz = leaf + (nzs - base)
    p = torch.softmax(nz, -1)
    ix = idx.long()
    loss = torch.zeros((), dtype=f64, device=nzs.device)
    dp_abs = torch.zeros(T, E, dtype=f64, device=nzs.device)
    dp_err = torch.zeros_like(dp_abs)
    nxt = idx_next.long().unsqueeze(1) if (idx_next is not None and k < E) else None
    bs = float(balance_scale)
    if d_score is not None:
        loss = loss + (d_score.double() * p.gather(1, ix)).sum()
        dp_abs.scatter_add_(1, ix, d_score.double().abs())
    if d_top is not None:
        sel = torch.cat((ix, nxt), 1) if nxt is not None else ix
        loss = loss + (d_top.double() * p.gather(1, sel)).sum()
        dp_abs.scatter_add_(1, sel, d_top.double().abs())
    if d_importance is not None:
        di = d_importance.double() * bs
        loss = loss + (di.unsqueeze(0).expand(T, E).gather(1, ix) * p.gather(1, ix)).sum()
        dp_abs.scatter_add_(1, ix, di.abs().unsqueeze(0).expand(T, E).gather(1, ix))
    g_err = torch.zeros_like(dp_abs)
    if lp:
        top = top_logits.double()
        is_in = nzs > top[:, k:k + 1]
        # the thresholds take the kernel's stored values, their gradient flows through the softmax
        pin, pout = p.gather(1, nxt), p.gather(1, ix[:, k - 1:k])
        thr = torch.where(is_in, top[:, k:k + 1] + (pin - pin.detach()), top[:, k - 1:k] + (pout - pout.detach()))
        std = float(noise_std)
        z = (leaf - thr) / std
        Phi = 0.5 * torch.erfc(-z / math.sqrt(2.0))
        dl = d_load_prob.double() * bs
        loss = loss + (dl.unsqueeze(0) * Phi).sum()
        zk = (clean.double() - torch.where(is_in, top[:, k:k + 1], top[:, k - 1:k])) / std
        pdf = torch.exp(-0.5 * zk * zk) / math.sqrt(2 * math.pi)
        g = (dl.unsqueeze(0) * pdf / std).abs()
        g_err = g * (8 * U32 + zk.abs() * 3 * U32 * zk.abs())
        for mask, tgt in ((is_in, nxt), (~is_in, ix[:, k - 1:k])):
            gs = (g * mask).sum(1, keepdim=True)
            dp_abs.scatter_add_(1, tgt, gs)
            dp_err.scatter_add_(1, tgt, E * U32 * gs + (g_err * mask).sum(1, keepdim=True))
    dp_err = dp_err + 5 * U32 * dp_abs
    if loss.requires_grad:
        (ref,) = torch.autograd.grad(loss, leaf)
    else:
        ref = torch.zeros_like(nzs)
    return ref, gate_bwd_logits_bound(nzs, dp_abs, dp_err, g_err, ref)


# ------------------------------------------------------------------------------------------ Inf and NaN (non-finite inputs)
FMAX = {torch.float32: float(torch.finfo(torch.float32).max), torch.float16: 65504.0,
        torch.bfloat16: float(torch.finfo(torch.bfloat16).max)}


def _at(j, shape):
    return tuple(int(v) for v in torch.unravel_index(torch.tensor(j), shape)) if len(shape) else ()


def _first(mask):
    """(flat index of the first True, number of True)"""
    f = mask.flatten()
    return int(f.nonzero()[0]), int(f.sum())


def nonfinite_agrees(out, ref64, dtype, bound64=None, what="output"):
    """out (stored as `dtype`) against ref64: torch's own float64 result on the dtype-rounded, poisoned inputs.  Per element
      ref NaN                                 => out NaN
      ref +-Inf or |ref| >= 2 max(dtype)      => out is the Inf of that sign (a store that saturates to max(dtype) fails)
      ref finite, |ref| <= max(dtype) / 2     => out finite, and within bound64 where one is given
    A finite ref in (1/2, 2) x max(dtype) is a fault of the CASE (fp32 arithmetic may or may not overflow there) and is
    asserted as such, on the reference.  Returns {"nonfinite": n, "finite": n}: the elements compared in either class."""
    o = out.detach().double().cpu()
    r = ref64.detach().double().cpu().expand_as(o)
    big = FMAX[dtype]
    grey = torch.isfinite(r) & (r.abs() > big / 2) & (r.abs() < 2 * big)
    if bool(grey.any()):
        j, n = _first(grey)
        raise AssertionError(f"{what}: the case is ill-posed: {n} finite reference value(s) in (1/2, 2) x {big:g}; first at "
                             f"{_at(j, o.shape)}: ref {float(r.flatten()[j])!r}")
    want_nan = torch.isnan(r)
    want_inf = ~want_nan & (r.abs() >= 2 * big)
    want_fin = ~want_nan & ~want_inf
    inf_of = torch.where(r > 0, math.inf, -math.inf)
    bad = (want_nan & ~torch.isnan(o)) | (want_inf & ~(o == inf_of)) | (want_fin & ~torch.isfinite(o))
    if bool(bad.any()):
        j, n = _first(bad)
        rj, oj = float(r.flatten()[j]), float(o.flatten()[j])
        must = "NaN" if math.isnan(rj) else (f"{float(inf_of.flatten()[j])!r}" if abs(rj) >= 2 * big else "finite")
        raise AssertionError(f"{what}: {n} of {o.numel()} elements differ from torch on a non-finite input; first at "
                             f"{_at(j, o.shape)}: got {oj!r}, ref {rj!r}: must be {must}")
    if bound64 is not None and bool(want_fin.any()):
        b = torch.as_tensor(bound64).double().cpu().expand_as(o)
        err = (o - r).abs()
        over = want_fin & ~(err <= b)
        if bool(over.any()):
            j, n = _first(over)
            raise AssertionError(f"{what}: {n} finite element(s) exceed their bound; first at {_at(j, o.shape)}: got "
                                 f"{float(o.flatten()[j])!r}, ref {float(r.flatten()[j])!r}, bound {float(b.flatten()[j]):.3e}")
    return {"nonfinite": int((want_nan | want_inf).sum()), "finite": int(want_fin.sum())}


def _bits(t):
    t = t.detach().contiguous()
    if t.dtype.is_floating_point:
        t = t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t.cpu()


def independent_same_bits(out_clean, out_poisoned, depends_mask, what="output"):
    """every element outside depends_mask (bool, broadcastable to the outputs; derived from the OPERATION: "row r of C",
    "column c of dW of group g", "every token of image b") has the same bits in the clean and in the poisoned run of the
    same shapes and launch plan.  Returns the number of elements held to it."""
    assert out_clean.shape == out_poisoned.shape and out_clean.dtype == out_poisoned.dtype, f"{what}: the two runs differ in shape or dtype"
    a, b = _bits(out_clean), _bits(out_poisoned)
    dep = torch.as_tensor(depends_mask).cpu().expand_as(a)
    bad = (a != b) & ~dep
    if bool(bad.any()):
        j, n = _first(bad)
        oc, op = out_clean.detach().contiguous().flatten()[j], out_poisoned.detach().contiguous().flatten()[j]
        raise AssertionError(f"{what}: {n} element(s) that do not depend on the poisoned input changed; first at "
                             f"{_at(j, a.shape)}: clean run {float(oc)!r}, poisoned run {float(op)!r}")
    return int((~dep).sum())
