"""Cases, float64 restatement, input builder and error bounds of the token blocks' FFN sublayer (m3vit_amd.sharing.TokenFFNStage,
csrc/token_ffn.hip).  A helper: imported by test_token_ffn_cpu.py, test_token_ffn_gpu.py, gen_golden_token_ffn.py and
tools/token_ffn_bench.py; nothing here is collected.

The restatement is step 5 of the reference's TokenBlock.forward for the blocks without a router - dense_mlp_stage(outs,
shared_bits), shared_dense_forward(shared_x), apply_shared_broadcast, or the shared_ffn branch of an MoE block - in DENSE form
(no nonzero, no early return, every row computed and the ones that count selected), written from the formulas:

    private(t, p) = bit t of bits[p] clear;   F(v) = fc2(gelu(fc1(LayerNorm(v))))
    shared_out[p] = sx[p] + shared_path_scale[p] F(sx[p])                   where bits[p] != 0
    y_t[p] = x_t[p] + path_scale[p // N] F(x_t[p])   (mode "all")           where private(t, p)
    y_t[p] = x_t[p]                                  (mode "shared")        where private(t, p)
    y_t[p] = shared_out[p]                                                  where bit t of bits[p] is set

tests/golden/g15_token_ffn.npz holds what the reference's own code gives; test_token_ffn_cpu.py holds the restatement to it.

shared_bits is an INPUT here (any int64 word, single-bit words included), so no comparison is a coin toss and no row is left
out of any comparison.

Bounds, in the manner of kernel_contract: the reference is float64 on the values the kernel read, only the kernel's own
arithmetic is charged, every term is multiplied by SAFETY, nothing is tuned per test.  The LayerNorm-gather reuses
layernorm_bound; the GEMMs between the row passes are m3_gemm_nt / m3_wgrad_tn, whose bounds are kernel_contract.gemm_bound and
are checked by their own tests - the per-kernel tests here feed the row passes given compact buffers instead.
"""
import itertools
import math

import torch

from kernel_contract import SAFETY, U32, layernorm_bound, store

F64 = torch.float64
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
MODES = ("all", "shared")
LN_EPS = 1e-6                                        # the reference's norm_layer = partial(nn.LayerNorm, eps=1e-6)
# the project's stated parity bounds, relative L2 per tensor; bf16 = 8 x the fp16 bound (three mantissa
# bits fewer), as test_bf16_kernels.py takes it
REL_BOUND = {"f32": 2e-5, "f16": 1e-3, "bf16": 8e-3}


# ----------------------------------------------------------------------------------------------------- the restatement
def layernorm(v, gamma, beta, eps=LN_EPS):
    mu = v.mean(-1, keepdim=True)
    var = ((v - mu) ** 2).mean(-1, keepdim=True)
    return (v - mu) / (var + eps).sqrt() * gamma + beta


def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def ffn(v, p):
    """F(v) of rows v [.., C]; p: dict(gamma, beta [C], w1 [H, C], b1 [H], w2 [C, H], b2 [C])"""
    h = layernorm(v, p["gamma"], p["beta"], p.get("eps", LN_EPS))
    return gelu(h @ p["w1"].transpose(-1, -2) + p["b1"]) @ p["w2"].transpose(-1, -2) + p["b2"]


def bit_masks(bits, T):
    """bool [T, P]: bit t of bits[p]"""
    return torch.stack([((bits >> t) & 1).bool() for t in range(T)])


def stage(xs, bits, sx, p, mode, N, path_scale=None, shared_path_scale=None):
    """xs [T, P, C], bits int64 [P] or None (= all zero), sx [P, C], path_scale [P // N] or None, shared_path_scale [P] or
    None -> y [T, P, C].  Everything in the dtype of xs (float64 in the tests)."""
    T, P, _ = xs.shape
    if bits is None:
        bits = torch.zeros(P, dtype=torch.int64)
    M = bit_masks(bits, T)
    a_p = xs.new_ones(P) if path_scale is None else path_scale.to(xs.dtype).repeat_interleave(N)
    a_s = xs.new_ones(P) if shared_path_scale is None else shared_path_scale.to(xs.dtype)
    shared_out = sx + a_s.unsqueeze(-1) * ffn(sx, p)
    priv = xs + a_p.view(1, P, 1) * ffn(xs, p) if mode == "all" else xs
    return torch.where(M.unsqueeze(-1), shared_out.unsqueeze(0), priv)


def worklist(bits, T, mode):
    """the work list by enumeration: rows int64 [R] = seg * P + p (segment-major, ascending p), slot_of int64 [T + 1, P]
    (-1: not listed), R, offsets, tile_starts as m3_route_build writes them for one group"""
    P = bits.numel()
    b = bits & ((1 << T) - 1)
    listed = torch.zeros(T + 1, P, dtype=torch.bool)
    if mode == "all":
        listed[:T] = ~bit_masks(b, T)
    listed[T] = b != 0
    rows = listed.reshape(-1).nonzero().squeeze(1)
    R = rows.numel()
    slot_of = torch.full(((T + 1) * P,), -1, dtype=torch.int64)
    slot_of[rows] = torch.arange(R)
    return dict(rows=rows, slot_of=slot_of.view(T + 1, P), R=R, offsets=[0, R], tile_starts=[0, -(-R // 128)])


def rows_ub(P, T, mode):
    """the derived bound: a position whose word has at most one bit set contributes T rows, any other T - popcount + 1 <=
    T - 1; mode "shared" lists at most one row per position"""
    return T * P if mode == "all" else P


def source_rows(xs, sx, rows, P):
    """the rows the work list names, gathered: xs [T, P, C], sx [P, C], rows int64 [R] -> [R, C]"""
    T = xs.shape[0]
    return torch.cat((xs, sx.unsqueeze(0)))[rows // P, rows % P] if rows.numel() else xs.new_zeros((0, xs.shape[-1]))


# ----------------------------------------------------------------------------------------------------------- bounds
def _hh(D):
    return -(-D // 64) + 6                           # additions an element passes through in a lane-then-wave row sum


def ln_gather_bounds(x_rows, gamma, beta, h_ref, dtype):
    """m3_token_ffn_ln_fwd: (h bound = kernel_contract.layernorm_bound on the gathered rows - a 16-bit row is exact in fp32 -,
    mean bound, rstd bound).  mean: hh u32 mean|x| for the sum plus the division's rounding.  rstd = 1 / sqrt(var + eps):
    the two-pass variance sums non-negative squares of values centred on the kernel's own mean, off by delta <= the mean bound,
    which adds delta^2 to the variance; relative error of the sum (hh + 2) u32; half of both in rstd; the division by D, the
    eps add, sqrtf and the reciprocal 4 u32."""
    x = x_rows.double()
    D = x.shape[-1]
    hh = _hh(D)
    mu = x.mean(-1)
    var = x.var(-1, unbiased=False)
    rstd = 1.0 / (var + LN_EPS).sqrt()
    delta = hh * U32 * x.abs().mean(-1) + U32 * mu.abs()
    mean_b = SAFETY * (delta + 2.0 ** -150)
    rstd_b = SAFETY * rstd * ((hh + 2) / 2 * U32 + 4 * U32 + 0.5 * delta * delta / (var + LN_EPS))
    return layernorm_bound(x_rows.float(), gamma, beta, h_ref, dtype), mean_b, rstd_b


def scatter_fwd_bound(y_ref, dtype):
    """m3_token_ffn_scatter_fwd: a listed row is ONE fma(factor, f, x) in fp32 and the store; a pass-through row is exact"""
    return SAFETY * (U32 * y_ref.abs() + store(dtype, y_ref))


def gather_bwd_bound(df_ref, abs_terms, n_terms, dtype):
    """m3_token_ffn_gather_bwd: a private row is one product; a shared row adds n_terms <= T values in fp32 (n u32 sum |d y_t|)
    and multiplies once; then the store.  abs_terms [R, C] = factor * sum |d y_t|, n_terms [R]."""
    return SAFETY * ((n_terms.unsqueeze(-1) + 1) * U32 * abs_terms + store(dtype, df_ref))


def ln_bwd_terms(x, dh, gamma, mean, rstd):
    """LayerNorm backward of rows x [R, C] given d h, with the mean / rstd THE KERNEL READ (fp32 values as float64):
    (d x [R, C], its error before the store, d gamma contributions d h xhat [R, C], their error).
      xhat = (x - mean) rstd                       2 u32 |xhat|
      g = d h gamma                                u32 |g|
      c1 = sum(g) / D, c2 = sum(g xhat) / D        fp32 sums of D terms (any order): u32 sum |terms| (= D u32 mean |terms|), plus
                                                   the terms' own errors, plus the division
      d x = rstd ((g - c1) - xhat c2)              the errors above carried through, three roundings inside, one outside"""
    xh = (x - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    g = dh * gamma
    c1 = g.mean(-1, keepdim=True)
    c2 = (g * xh).mean(-1, keepdim=True)
    dx = rstd.unsqueeze(-1) * ((g - c1) - xh * c2)
    exh = 2 * U32 * xh.abs()
    eg = U32 * g.abs()
    ec1 = U32 * g.abs().sum(-1, keepdim=True) + eg.mean(-1, keepdim=True) + U32 * c1.abs()
    gx = (g * xh).abs()
    ec2 = U32 * gx.sum(-1, keepdim=True) + (g.abs() * exh + eg * xh.abs() + U32 * gx).mean(-1, keepdim=True) + U32 * c2.abs()
    inner = eg + ec1 + xh.abs() * ec2 + c2.abs() * exh + 3 * U32 * (g.abs() + c1.abs() + (xh * c2).abs())
    edx = rstd.unsqueeze(-1) * inner + 2 * U32 * dx.abs()
    return dx, edx, dh * xh, dh.abs() * exh + U32 * (dh * xh).abs()


def column_sum_bound(terms, terms_err, ref):
    """d gamma / d beta: an fp32 sum over R rows in a fixed order (lane accumulators over the positions of a wave, four waves,
    the workgroups' partial rows): (R + 2) u32 sum |terms| + the terms' own errors + the final rounding"""
    R = terms.shape[0]
    return SAFETY * ((R + 2) * U32 * terms.abs().sum(0) + terms_err.sum(0) + U32 * ref.abs() + 2.0 ** -150)


# ------------------------------------------------------------------------------------------------------------ cases
def case(T, BN, CH, dtype, mode, pattern="mixed"):
    return dict(T=T, B=BN[0], N=BN[1], C=CH[0], H=CH[1], dtype=dtype, mode=mode, pattern=pattern)


def case_id(c):
    return f"T{c['T']}-B{c['B']}N{c['N']}-C{c['C']}H{c['H']}-{c['dtype']}-{c['mode']}-{c['pattern']}"


_TS, _BNS, _CHS, _DTS = (2, 3, 8), ((1, 1), (1, 65), (2, 197)), ((192, 384), (384, 1536)), ("f32", "f16", "bf16")


def stage_cases():
    """Every value of every factor of the issue's grid (T, (B, N), (C, H), dtype, mode) and every PAIR of (T, (B, N)) and of
    ((C, H), dtype), in 9 cases instead of the 108 of the full product - each in BOTH modes: the kernels' instances are
    chosen by T, the dtype, C <= 512 / C > 512 being one chunk per lane here, and the mode, the work list's by (T + 1) B N."""
    out = []
    for i, (T, BN) in enumerate(itertools.product(_TS, _BNS)):
        for mode in MODES:
            out.append(case(T, BN, _CHS[i % 2], _DTS[(i // 2) % 3], mode))
    return out


def degenerate_cases():
    """patterns whose row count R the tests assert (test_token_ffn_gpu.py::test_degenerate_row_counts): the bound itself, an
    empty group, one tile short of / exactly / one row over 128 rows, one shared position, single-bit words"""
    big, small = (2, 197), (1, 65)
    out = []
    for mode in MODES:
        out += [case(3, big, _CHS[0], "f16", mode, "none"), case(3, big, _CHS[0], "bf16", mode, "all"),
                case(3, small, _CHS[1], "f32", mode, "one"), case(3, big, _CHS[0], "f16", mode, "single")]
    out += [case(2, small, _CHS[0], "f16", "all", f"r{r}") for r in (127, 128, 129)]
    out += [case(2, big, _CHS[0], "f32", "shared", f"r{r}") for r in (127, 128, 129)]
    return out


def golden_cases():
    """small enough for the committed file: the reference's own values and gradients"""
    out = []
    for i, (T, BN, CH) in enumerate(((2, (2, 9), (16, 32)), (3, (1, 12), (24, 48)), (5, (2, 9), (16, 32)))):
        out.append(case(T, BN, CH, "f32", "all", "mixed"))
    out += [case(3, (2, 9), (16, 32), "f32", "all", "none"), case(3, (1, 12), (24, 48), "f32", "all", "all"),
            case(3, (2, 9), (16, 32), "f32", "shared", "mixed")]
    return out


def golden_train_case():
    """the one golden case run in training mode with the reference's recorded drop-path draws (key suffix "/train")"""
    return case(3, (2, 9), (16, 32), "f32", "all", "mixed")


def expected_rows(c):
    """R of a degenerate pattern, from the pattern's definition (None for the random ones)"""
    T, P, mode, pat = c["T"], c["B"] * c["N"], c["mode"], c["pattern"]
    if pat == "none":
        return T * P if mode == "all" else 0
    if pat == "all":
        return P
    if pat == "one":
        return (T * P - (T - 1)) if mode == "all" else 1
    if pat == "single":
        return T * P if mode == "all" else P
    if pat.startswith("r"):
        return int(pat[1:])
    return None


# ---------------------------------------------------------------------------------------------------------- builder
def make_bits(c, gen):
    T, P, mode, pat = c["T"], c["B"] * c["N"], c["mode"], c["pattern"]
    full = (1 << T) - 1
    bits = torch.zeros(P, dtype=torch.int64)
    if pat == "all":
        bits[:] = full
    elif pat == "one":
        bits[int(torch.randint(0, P, (1,), generator=gen))] = full
    elif pat == "single":
        bits = torch.ones(P, dtype=torch.int64) << torch.randint(0, T, (P,), generator=gen)
    elif pat.startswith("r"):
        R = int(pat[1:])
        # mode "all", T = 2: an unshared position lists 2 rows, one shared by both lists 1: R = 2 P - k;  mode "shared": R = k
        k = 2 * P - R if mode == "all" else R
        assert T == 2 or mode == "shared"
        assert 0 <= k <= P
        bits[torch.randperm(P, generator=gen)[:k]] = full
    elif pat == "mixed":
        # 40 % of the positions shared by a random set of >= 2 tasks, 10 % carry a word with a single bit, the rest none
        r = torch.rand(P, generator=gen)
        words = torch.randint(0, full + 1, (P,), generator=gen)
        pc = sum(((words >> t) & 1) for t in range(T))
        words = torch.where(pc >= 2, words, torch.full_like(words, full))
        single = torch.ones(P, dtype=torch.int64) << torch.randint(0, T, (P,), generator=gen)
        bits = torch.where(r < 0.4, words, torch.where(r < 0.5, single, bits))
    else:
        assert pat == "none"
    return bits


def make_params(C, H, gen):
    """fp32 parameters of an nn.LayerNorm and the reference's Mlp, of trained-looking sizes"""
    return dict(gamma=1.0 + 0.1 * torch.randn(C, generator=gen), beta=0.1 * torch.randn(C, generator=gen),
                w1=torch.randn(H, C, generator=gen) / math.sqrt(C), b1=0.02 * torch.randn(H, generator=gen),
                w2=torch.randn(C, H, generator=gen) / math.sqrt(H), b2=0.02 * torch.randn(C, generator=gen), eps=LN_EPS)


def make_inputs(c, seed=0):
    """dict(xs [T, P, C] in the case's dtype, bits int64 [P], sx [P, C] (the mean of the participating rows, zero rows where
    bits == 0 - what SharedTokens.x looks like), params fp32, x64 / sx64 / p64: float64 copies of exactly these values, wl: the
    enumerated work list).  CPU tensors."""
    T, P, C, H = c["T"], c["B"] * c["N"], c["C"], c["H"]
    dt = DTYPES[c["dtype"]]
    gen = torch.Generator().manual_seed(1_000_003 * seed + 17)
    bits = make_bits(c, gen)
    xs = (0.3 + torch.randn(T, P, C, generator=gen)).to(dt)
    M = bit_masks(bits, T).float()
    sx = ((M.unsqueeze(-1) * xs.float()).sum(0) / M.sum(0).clamp_min(1.0).unsqueeze(-1)).to(dt)
    params = make_params(C, H, gen)
    p64 = {k: (v.double() if torch.is_tensor(v) else v) for k, v in params.items()}
    return dict(xs=xs, bits=bits, sx=sx, params=params, x64=xs.double(), sx64=sx.double(), p64=p64,
                wl=worklist(bits, T, c["mode"]))


def functional(c, seed=1):
    """the fixed random linear functional of the outputs whose gradient the backward tests compare: coefficients for y
    [T, P, C], float64"""
    gen = torch.Generator().manual_seed(7919 * seed + 13)
    return torch.randn(c["T"], c["B"] * c["N"], c["C"], generator=gen).double()


def reference(c, I, path_scale=None, shared_path_scale=None, cy=None):
    """float64 stage() on the case's values and the gradients of sum(cy * y): dict(y, d_xs, d_sx, and d_<param> for gamma, beta,
    w1, b1, w2, b2)"""
    cy = functional(c) if cy is None else cy
    xs = I["x64"].clone().requires_grad_(True)
    sx = I["sx64"].clone().requires_grad_(True)
    p = {k: (v.clone().requires_grad_(True) if torch.is_tensor(v) else v) for k, v in I["p64"].items()}
    y = stage(xs, I["bits"], sx, p, c["mode"], c["N"], path_scale, shared_path_scale)
    (cy * y).sum().backward()
    out = dict(y=y.detach(), d_xs=xs.grad, d_sx=sx.grad if sx.grad is not None else torch.zeros_like(sx))
    for k in ("gamma", "beta", "w1", "b1", "w2", "b2"):
        out["d_" + k] = p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])
    return out
