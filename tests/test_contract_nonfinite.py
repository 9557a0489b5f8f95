"""GPU contract tests: Inf and NaN go through every hot-path kernel as through torch.

Two properties, per kernel family (kernel_contract.nonfinite_agrees / independent_same_bits):
  1. nothing is swallowed - with +Inf, -Inf, NaN (and, for 16-bit stores, one finite value that overflows the store) planted in
     an input, the output is NaN / the Inf of the right sign exactly where torch's own float64 result on the same dtype-rounded,
     poisoned inputs is, and finite everywhere else;
  2. nothing leaks - every output element that does not depend on the planted value (the mask comes from the operation: "row r
     of C", "column c of dW of group g", "every token of the other image") has the bits of a clean run of the same shapes and
     the same launch plan.  A mask done by multiplying with 0 or a tail tile that reads its neighbour's rows is invisible with
     finite data (0 * x = 0) and fails here (0 * NaN).
The planted positions are where clamping and masking live: the first row, the last row of a partial tile, the rows on both sides
of a tile boundary, the last K column, a row no index refers to, the first row of the group behind a ragged group, the weights
of an empty group.  Outputs sit in guarded() views; where a family has several kernels the case states its kernel and asserts
it through launch_signature / m3_*_plan on the very launch.

Where Inf - Inf decides between Inf and NaN and the kernel's (documented) arithmetic orders the terms differently from torch's
closed form, only NaN is planted; each such place says so next to the case.

The module prints, per family, how many elements were compared as "must be non-finite", "must keep their bits" and "finite
within bound"; every case asserts that its first two classes are not empty."""
import math

import pytest
import torch
import torch.nn.functional as F

import kernel_contract as kc
import launch_signature as ls

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F16, BF16, F32]
NAN, INF = float("nan"), float("inf")
OVER = {F16: 6.0e4, BF16: 3.0e38}          # finite in the dtype; times the factor 8 the cases keep next to it: past 2 x the maximum
TALLY = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    yield _ops
    if TALLY:
        print("\nnon-finite contract, elements compared per family (must be non-finite / must keep their bits / finite within bound):")
        for fam, (a, b, c) in sorted(TALLY.items()):
            print(f"  {fam:<14} {a:>9} {b:>10} {c:>9}")


class Case:
    """one case's comparisons: agree() holds an output to torch's non-finite pattern, same() holds the independent part to the
    clean run's bits; leaving the block asserts that both classes were exercised and adds the counts to the family's"""

    def __init__(self, family):
        self.family, self.nf, self.kept, self.fin = family, 0, 0, 0

    def __enter__(self):
        return self

    def agree(self, out, ref64, dtype, bound64=None, what="output"):
        n = kc.nonfinite_agrees(out, ref64, dtype, bound64, what=what)
        self.nf += n["nonfinite"]
        if bound64 is not None:
            self.fin += n["finite"]

    def same(self, clean, poisoned, depends, what="output"):
        self.kept += kc.independent_same_bits(clean, poisoned, depends, what=what)

    def __exit__(self, et, ev, tb):
        if et is None:
            assert self.nf > 0, f"{self.family}: the case compared no element as 'must be non-finite'"
            assert self.kept > 0, f"{self.family}: the case compared no element as 'must keep its bits'"
            t = TALLY.setdefault(self.family, [0, 0, 0])
            t[0] += self.nf; t[1] += self.kept; t[2] += self.fin
        return False


def rnd(*shape, dtype=F32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def plant(t, *spots):
    """a copy of t with values planted: spots = (index tuple, value), ..."""
    t = t.clone()
    for idx, v in spots:
        t[idx] = v
    return t


def mask(shape, *regions):
    """bool CPU mask, True on every region (an index tuple each)"""
    m = torch.zeros(shape, dtype=torch.bool)
    for r in regions:
        m[r] = True
    return m


def d64(t):
    return None if t is None else t.detach().double().cpu()


def sync():
    torch.cuda.synchronize()


# ============================================================================================ ReLU + bilinear x2 (resize.hip)
def up2x_expected(x64, relu, dy64=None):
    """(y, dx) float64: F.interpolate(F.relu(x), scale_factor=2, mode="bilinear") and its autograd, x64 [N, C, H, W].
    The documented exception: torch gives output row / column 0 the taps (x[0], x[1]) with weights (1, 0), and 0 * NaN = NaN, so a
    non-finite x[1] reaches output 0 (and a non-finite dy[0] reaches dx[1]) through a tap of weight zero; the kernel's clamped
    form (0.25 x[0] + 0.75 x[0], resize.hip) has no such tap.  Expected there is the same torch op on the replicate-padded image,
    cropped - identical everywhere else, which is asserted: the two differ only where the plain form is NaN in row / column 0
    (forward) or 1 (backward)."""
    def run(pad):
        xr = x64.clone().requires_grad_()
        z = F.relu(xr) if relu else xr
        if pad:
            y = F.interpolate(F.pad(z, (1, 1, 1, 1), mode="replicate"), scale_factor=2, mode="bilinear", align_corners=False)[:, :, 2:-2, 2:-2]
        else:
            y = F.interpolate(z, scale_factor=2, mode="bilinear", align_corners=False)
        dx = None
        if dy64 is not None:
            (dx,) = torch.autograd.grad(y, xr, dy64)
        return y.detach(), dx
    (y0, dx0), (y1, dx1) = run(False), run(True)
    for a, b, edge, name in ((y0, y1, 0, "y"), (dx0, dx1, 1, "dx")):
        if a is None:
            continue
        diff = ~((a == b) | (a.isnan() & b.isnan()) | ((a - b).abs() <= 1e-12 * b.abs()))
        inner = diff.clone()
        inner[:, :, edge, :] = False
        inner[:, :, :, edge] = False
        assert not bool(inner.any()) and bool(a[diff].isnan().all()), f"{name}: the two torch forms differ outside the zero-weight tap"
    return y1, dx1


UP2X = [(F16, 16), (BF16, 16), (F32, 8)]
UP2X_SHAPE = (2, 3, 5)


@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "norelu"])
@pytest.mark.parametrize("dtype,C", UP2X)
def test_relu_up2x_forward(ops, dtype, C, relu):
    """m3_relu_up2x_fwd and _fwd_bordered (one kernel; the instance is (dtype, relu, bordered)).  x [N, H, W, C] = (2, 3, 5, C):
    NaN at the corner pixel (0, 0) of image 0, +Inf at its last pixel (2, 4), -Inf at (0, 4) of image 1, NaN at the interior
    pixel (1, 2) of image 1.  An input pixel (y, x) feeds output rows 2y-1 .. 2y+2 and columns 2x-1 .. 2x+2 of its own channel.
    A finite value cannot overflow the store here: every output is a convex combination of inputs.  The border of the bordered
    form stays zero and its interior is the dense result bit for bit."""
    Nb, H, W = UP2X_SHAPE
    x = rnd(Nb, H, W, C, dtype=dtype, seed=85)
    spots = [((0, 0, 0, 0), NAN), ((0, 2, 4, 3), INF), ((1, 0, 4, 5), -INF), ((1, 1, 2, 1), NAN)]
    xp = plant(x, *spots)

    def fwd(xin):
        y, check = kc.guarded(Nb * 2 * H * 2 * W, C, dtype)
        snap = kc.snapshot(x=xin)
        ops.check(ops.lib().m3_relu_up2x_fwd(ops._p(xin), ops.dt_code(dtype), Nb, H, W, C, relu, ops._p(y), ops.dt_code(dtype),
                                             ops._stream()), "m3_relu_up2x_fwd")
        sync(); kc.unchanged(snap); check()
        return y.view(Nb, 2 * H, 2 * W, C).permute(0, 3, 1, 2)

    with Case("relu_up2x") as c:
        y0, y1 = fwd(x), fwd(xp)
        x64 = d64(xp).permute(0, 3, 1, 2)
        ref, _ = up2x_expected(x64, relu)
        ain = torch.nan_to_num(F.relu(x64) if relu else x64, 0, 0, 0).abs()          # (a finite output has no planted tap)
        aref = F.interpolate(ain, scale_factor=2, mode="bilinear", align_corners=False)
        c.agree(y1, ref, dtype, kc.sum_bound(aref, 4, torch.nan_to_num(ref, 0, 0, 0), dtype), what="y")
        dep = mask((Nb, C, 2 * H, 2 * W), *[(n, ch, slice(max(2 * py - 1, 0), 2 * py + 3), slice(max(2 * px - 1, 0), 2 * px + 3))
                                            for (n, py, px, ch), _ in spots])
        c.same(y0, y1, dep, what="y")
        if dtype != F32:
            # the bordered form (16-bit only): the interior is the dense result bit for bit, the border stays zero
            yb, bcheck = kc.guarded(Nb * (2 * H + 2) * (2 * W + 2), C, dtype)
            yb.zero_()
            xcl = xp.permute(0, 3, 1, 2)
            out = ops.relu_up2x_fwd_bordered(xcl, relu=bool(relu), out=yb).view(Nb, 2 * H + 2, 2 * W + 2, C)
            sync(); bcheck(what="bordered ReLU + x2")
            assert kc.same_bits(out[:, 1:-1, 1:-1, :].contiguous(), y1.permute(0, 2, 3, 1).contiguous()), "bordered interior != dense result"
            border = torch.ones(2 * H + 2, 2 * W + 2, dtype=torch.bool, device="cuda")
            border[1:-1, 1:-1] = False
            assert not bool(out[:, border].view(torch.int16).any()), "the border is no longer all zero"



@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "norelu"])
@pytest.mark.parametrize("dtype,C", UP2X)
def test_relu_up2x_backward(ops, dtype, C, relu):
    """m3_relu_up2x_bwd (instance: (dtype, relu)).  NaN and -Inf planted in dy, and NaN, +Inf, -Inf in x at pixels whose gradient
    is finite: with the ReLU on, dx must be the gradient itself where x is NaN or +Inf (torch's threshold_backward passes it),
    0 where x is -Inf - held to the sum bound of tests/test_contract_rowops.py, so a mask that returns 0 for a NaN x fails."""
    Nb, H, W = UP2X_SHAPE
    x = rnd(Nb, H, W, C, dtype=dtype, seed=85)
    with Case("relu_up2x") as c:
        # x: NaN (0,1,1), +Inf (0,1,3), -Inf (1,2,0): pixels whose 4 x 4 windows of dy hold no planted value;
        # dy [N, 2H, 2W, C]: NaN at (0, 5, 9) (the last output pixel: dx (2, 4)), -Inf at (1, 1, 5) (dx rows 0..1, columns 2..3)
        xs = [((0, 1, 1, 2), NAN), ((0, 1, 3, 4), INF), ((1, 2, 0, 6), -INF)]
        ds = [((0, 5, 9, 2), NAN), ((1, 1, 5, 3), -INF)]
        dy = rnd(Nb, 2 * H, 2 * W, C, dtype=dtype, seed=86)
        xq, dyq = plant(x, *xs), plant(dy, *ds)

        def bwd(xin, dyin):
            dx, check = kc.guarded(Nb * H * W, C, dtype)
            snap = kc.snapshot(x=xin, dy=dyin)
            ops.check(ops.lib().m3_relu_up2x_bwd(ops._p(dyin), ops.dt_code(dtype), ops._p(xin), ops.dt_code(dtype), Nb, H, W, C, relu,
                                                 ops._p(dx), ops._stream()), "m3_relu_up2x_bwd")
            sync(); kc.unchanged(snap); check()
            return dx.view(Nb, H, W, C).permute(0, 3, 1, 2)
        g0, g1 = bwd(x, dy), bwd(xq, dyq)
        x64, dy64 = d64(xq).permute(0, 3, 1, 2), d64(dyq).permute(0, 3, 1, 2)
        _, rdx = up2x_expected(x64, relu, dy64)
        _, adx = up2x_expected(torch.ones_like(x64), 0, torch.nan_to_num(dy64, 0, 0, 0).abs())
        if relu:                                                             # torch's own ReLU mask: 1 where x is NaN or > 0
            xm = x64.clone().requires_grad_()
            adx = adx * torch.autograd.grad(F.relu(xm).sum(), xm)[0]
        c.agree(g1, rdx, dtype, kc.sum_bound(adx, 16, torch.nan_to_num(rdx, 0, 0, 0), dtype), what="dx")
        dep = mask((Nb, C, H, W), *[(n, ch, py, px) for (n, py, px, ch), _ in xs],
                   *[(n, ch, slice(max(-(-(oy - 2) // 2), 0), (oy + 1) // 2 + 1), slice(max(-(-(ox - 2) // 2), 0), (ox + 1) // 2 + 1))
                     for (n, oy, ox, ch), _ in ds])
        c.same(g0, g1, dep, what="dx")
        if relu:
            got = g1.double().cpu()
            for (n, py, px, ch), v in xs:
                want = 0.0 if v == -INF else float(rdx[n, ch, py, px])
                assert math.isfinite(want) and (v == -INF or abs(want) > 1e-3), "the case needs a finite, non-zero gradient at the planted x"
                assert float(got[n, ch, py, px]) == pytest.approx(want, rel=4 * kc.u(dtype), abs=1e-6), \
                    f"dx at x = {v}: got {float(got[n, ch, py, px])}, torch passes the gradient {want}"


# ================================================================================= row kernels (combine.hip, cast.hip)
ROW_T, ROW_K, ROW_D = 130, 2, 64
ROWS = (0, 63, 64, 129)            # the first row, both sides of a 64-row boundary, the last row of the partial block


@pytest.mark.parametrize("dtype", DTYPES)
def test_combine_forward_and_backward(ops, dtype):
    """m3_combine_fwd: out[t] = sum_j score[t, j] y[t k + j] + res[t] (fp32 out).  y element (t k + j, c) and res (t, c) reach
    out (t, c) only, score (t, j) reaches row t.  m3_combine_bwd: dy[t k + j] = score[t, j] dout[t], dscore[t, j] =
    <dout[t], y[t k + j]>: dout (t, c) reaches column c of token t's k rows of dy and dscore[t, :].  An fp32 dout of 1e6 times a
    score in [0.5, 1.5) overflows an fp16 dy (bf16 has fp32's range: no fp32 value overflows its store)."""
    T, k, D = ROW_T, ROW_K, ROW_D
    y = rnd(T * k, D, dtype=dtype, seed=71)
    score = (torch.rand(T, k, generator=torch.Generator().manual_seed(72)) + 0.5).cuda()
    res = rnd(T, D, seed=73)

    def fwd(y_, s_, r_):
        out, check = kc.guarded(T, D, F32)
        snap = kc.snapshot(y=y_, score=s_, res=r_)
        ops.combine_fwd(y_, s_, r_, out)
        sync(); kc.unchanged(snap); check()
        return out.clone()

    def ref_fwd(y_, s_, r_):
        return (d64(s_).unsqueeze(2) * d64(y_).view(T, k, D)).sum(1) + d64(r_)
    with Case("rowops") as c:
        yp = plant(y, ((0, 3), NAN), ((63 * k + 1, 5), INF), ((129 * k, 63), -INF))
        sp = plant(score, ((64, 1), NAN))
        rp = plant(res, ((129, 0), INF))
        o0, o1 = fwd(y, score, res), fwd(yp, sp, rp)
        c.agree(o1, ref_fwd(yp, sp, rp), F32, what="combine_fwd out")
        c.same(o0, o1, mask((T, D), (0, 3), (63, 5), (129, 63), (64, slice(None)), (129, 0)), what="combine_fwd out")

    dout = rnd(T, D, seed=74)

    def bwd(d_, y_, s_):
        dy, c1 = kc.guarded(T * k, D, dtype)
        ds, c2 = kc.guarded(T, k, F32)
        snap = kc.snapshot(dout=d_, y=y_, score=s_)
        ops.combine_bwd(d_, y_, s_, dy, ds)
        sync(); kc.unchanged(snap); c1(); c2()
        return dy.clone(), ds.clone()
    with Case("rowops") as c:
        spots = [((0, 2), NAN), ((63, 7), INF), ((64, 0), -INF), ((129, 63), NAN)]
        if dtype == F16:
            spots.append(((65, 9), 1.0e6))
        dp = plant(dout, *spots)
        (dy0, ds0), (dy1, ds1) = bwd(dout, y, score), bwd(dp, y, score)
        rdy = (d64(score).unsqueeze(2) * d64(dp).unsqueeze(1)).reshape(T * k, D)
        rds = (d64(y).view(T, k, D) * d64(dp).unsqueeze(1)).sum(-1)
        c.agree(dy1, rdy, dtype, kc.SAFETY * (kc.U32 * torch.nan_to_num(rdy, 0, 0, 0).abs() + kc.store(dtype, torch.nan_to_num(rdy, 0, 0, 0))), what="combine_bwd dy")
        c.agree(ds1, rds, F32, what="combine_bwd dscore")
        c.same(dy0, dy1, mask((T * k, D), *[(slice(t * k, t * k + k), col) for (t, col), _ in spots]), what="combine_bwd dy")
        c.same(ds0, ds1, mask((T, k), *[(t, slice(None)) for (t, _), _ in spots]), what="combine_bwd dscore")


@pytest.mark.parametrize("dtype", DTYPES)
def test_combine_gate_bwd_and_gather_rows(ops, dtype):
    """m3_combine_gate_bwd: dh[t] = sum_j dxe[t k + j] + d_logits[t] @ w_gate^T: dxe (t k + j, c) reaches dh (t, c), d_logits
    (t, e) reaches row t (w_gate has no zero entry).  m3_gather_rows: dst[i] = sum_j src[idx[i k + j] // div]: a planted src row
    reaches the dst rows whose indices name it, a src row no index names reaches nothing."""
    T, k, D, E = ROW_T, ROW_K, ROW_D, 8
    dxe = rnd(T * k, D, dtype=dtype, seed=90)
    dl, wg = rnd(T, E, seed=91), rnd(D, E, seed=92)

    def run(dxe_, dl_):
        dh, check = kc.guarded(T, D, dtype)
        snap = kc.snapshot(dxe=dxe_, dl=dl_, wg=wg)
        ops.combine_gate_bwd(dxe_, k, dl_, wg, dh)
        sync(); kc.unchanged(snap); check()
        return dh.clone()
    with Case("rowops") as c:
        xp = plant(dxe, ((1, 3), NAN), ((63 * k, 5), INF), ((129 * k + 1, 63), -INF))
        lp = plant(dl, ((64, 7), NAN))
        h0, h1 = run(dxe, dl), run(xp, lp)
        ref = d64(xp).view(T, k, D).sum(1) + d64(lp) @ d64(wg).t()
        c.agree(h1, ref, dtype, what="combine_gate_bwd dh")
        c.same(h0, h1, mask((T, D), (0, 3), (63, 5), (129, 63), (64, slice(None))), what="combine_gate_bwd dh")

    rows = T * k
    src = rnd(rows + 6, D, dtype=dtype, seed=93)
    g = torch.Generator().manual_seed(94)
    idx = (torch.randperm(rows, generator=g) * 2 + torch.randint(0, 2, (rows,), generator=g)).to(torch.int32).cuda()   # rows 0 .. rows-1 once each; rows .. rows+5: unnamed

    def gather(src_):
        dst, check = kc.guarded(T, D, dtype)
        snap = kc.snapshot(src=src_, idx=idx)
        ops.gather_rows(src_, idx, dst, div=2, k=k)
        sync(); kc.unchanged(snap); check()
        return dst.clone()
    with Case("rowops") as c:
        named = (idx.long() // 2).cpu()
        planted = [(int(named[0]), 1, NAN), (int(named[63 * k + 1]), 9, INF), (int(named[129 * k]), 63, -INF)]
        sp = plant(src, *[((r, col), v) for r, col, v in planted], ((rows + 2, 4), NAN), ((rows + 5, 0), INF))
        d0, d1 = gather(src), gather(sp)
        c.agree(d1, d64(sp)[named].view(T, k, D).sum(1), dtype, what="gather_rows")
        c.same(d0, d1, mask((T, D), (0, 1), (63, 9), (129, 63)), what="gather_rows")


@pytest.mark.parametrize("dtype", DTYPES)
def test_casts_and_add(ops, dtype):
    """m3_cast_f32, m3_scale_rows_cast, m3_cast_matrix (plain and transposed), m3_add_f32: element-local.  A cast keeps NaN as NaN
    and +-Inf as +-Inf; an fp32 2e5 (past 2 x 65504) and the fp32 1e5 (past fp16's rounding boundary 65520: torch's own cast
    gives Inf) become fp16 Inf, not 65504."""
    rows, cols = ROW_T, ROW_D + 4
    src = rnd(rows, cols, seed=50)
    spots = [((0, 0), NAN), ((63, 5), INF), ((64, cols - 1), -INF), ((129, cols - 1), NAN)]
    if dtype == F16:
        spots += [((1, 1), 2.0e5), ((128, 3), -2.0e5)]
    sp = plant(src, *spots)
    dep = mask((rows, cols), *[i for i, _ in spots])
    with Case("rowops") as c:
        def cast(s):
            dst, check = kc.guarded(rows, cols, dtype)
            ops.cast_f32(s, dst)
            sync(); check()
            return dst.clone()
        a0, a1 = cast(src), cast(sp)
        c.agree(a1, d64(sp), dtype, kc.store(dtype, torch.nan_to_num(d64(sp), 0, 0, 0)), what="cast_f32")
        c.same(a0, a1, dep, what="cast_f32")
        assert kc.same_bits(a1, sp.to(dtype)), "cast_f32 differs from torch's cast"
        if dtype == F16:
            one = plant(src, ((2, 2), 1.0e5))
            got = cast(one)
            assert float(got[2, 2]) == INF and kc.same_bits(got, one.to(F16)), "fp32 1e5 must become fp16 Inf"

        rs = (torch.rand(rows, generator=torch.Generator().manual_seed(51)) + 0.5).cuda()
        rsp = plant(rs, ((65,), NAN))

        def scale(s, r):
            dst, check = kc.guarded(rows, cols, dtype)
            ops.scale_rows_cast(s, r, 1, dst)
            sync(); check()
            return dst.clone()
        b0, b1 = scale(src, rs), scale(sp, rsp)
        c.agree(b1, d64(rsp).unsqueeze(1) * d64(sp), dtype, what="scale_rows_cast")
        c.same(b0, b1, dep | mask((rows, cols), (65, slice(None))), what="scale_rows_cast")

        m3 = rnd(2, 37, 44, seed=70)
        mspots = [((0, 0, 0), NAN), ((0, 36, 43), INF), ((1, 5, 43), -INF)] + ([((1, 36, 0), 2.0e5)] if dtype == F16 else [])
        mp = plant(m3, *mspots)
        for tr in (False, True):
            shape = (2, 44, 37) if tr else (2, 37, 44)

            def castm(s):
                dst, check = kc.guarded(shape[0] * shape[1], shape[2], dtype)
                ops.cast_matrix(s, dst.view(*shape), transpose=tr)
                sync(); check()
                return dst.view(*shape).clone()
            m0, m1 = castm(m3), castm(mp)
            want = mp.transpose(1, 2) if tr else mp
            c.agree(m1, d64(want), dtype, what="cast_matrix")
            c.same(m0, m1, mask(shape, *[((g, cc, r) if tr else (g, r, cc)) for (g, r, cc), _ in mspots]), what="cast_matrix")
            assert kc.same_bits(m1, want.contiguous().to(dtype))
    if dtype == F32:
        n = 4 * 130 + 3                                    # whole 16-byte vectors and the single-thread tail
        dst0, add = rnd(1, n, seed=60), rnd(1, n, seed=61)
        ap = plant(add, ((0, 0), NAN), ((0, 255), INF), ((0, n - 1), -INF))
        dq = plant(dst0, ((0, 256), INF), ((0, n - 2), NAN))
        with Case("rowops") as c:
            def addf(d, s):
                dst, check = kc.guarded(1, n, F32)
                dst.copy_(d)
                ops.add_f32(dst.view(n), s.view(n))
                sync(); check()
                return dst.clone()
            s0, s1 = addf(dst0, add), addf(dq, ap)
            c.agree(s1, d64(dq) + d64(ap), F32, kc.U32 * torch.nan_to_num(d64(dq) + d64(ap), 0, 0, 0).abs(), what="add_f32")
            c.same(s0, s1, mask((1, n), (0, 0), (0, 255), (0, n - 1), (0, 256), (0, n - 2)), what="add_f32")


# ======================================================================================================== layernorm.hip
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [132, 384])
def test_layernorm_forward_and_backward(ops, dtype, D):
    """m3_layernorm_fwd (one kernel, NCH = ceil(D / 256) = 1 and 2): a NaN, +Inf or -Inf anywhere in a row makes the whole row of
    y NaN (F.layer_norm: the mean is +-Inf or NaN, x - mean is NaN), mean / rstd of that row non-finite as x.mean() / the
    variance give them; every other row keeps its bits.  m3_layernorm_bwd: a NaN in dy (r, c) reaches dx row r, dgamma[c] and
    dbeta[c]; a NaN in x row r (through the kernel's own mean / rstd of it) reaches dx row r and every dgamma (xhat of the row is
    NaN in every column) and no dbeta.  Only NaN is planted in the backward: with an Inf, torch's closed form a dy g + b x + c
    and the kernel's two-mean form (layernorm.hip) meet Inf - Inf at different elements of the row."""
    T = ROW_T
    x = rnd(T, D, seed=20) * 2 + 0.5
    gamma, beta = 1 + rnd(D, seed=11, scale=0.1), rnd(D, seed=12, scale=0.1)

    def fwd(x_):
        y, c1 = kc.guarded(T, D, dtype)
        mean, c2 = kc.guarded(1, T, F32)
        rstd, c3 = kc.guarded(1, T, F32)
        snap = kc.snapshot(x=x_, gamma=gamma, beta=beta)
        ops.layernorm_fwd(x_, gamma, beta, y, mean.view(T), rstd.view(T))
        sync(); kc.unchanged(snap); c1(); c2(); c3()
        return y.clone(), mean.view(T).clone(), rstd.view(T).clone()
    spots = [((0, 0), NAN), ((63, D - 1), INF), ((64, 5), -INF), ((129, D - 1), NAN)]
    xp = plant(x, *spots)
    rows = [r for (r, _), _ in spots]
    with Case("layernorm") as c:
        (y0, m0, r0), (y1, m1, r1) = fwd(x), fwd(xp)
        x64 = d64(xp)
        ref = F.layer_norm(x64, (D,), d64(gamma), d64(beta), 1e-6)
        assert bool(ref[rows].isnan().all())
        c.agree(y1, ref, dtype, what="y")
        c.agree(m1, x64.mean(-1), F32, what="mean")
        c.agree(r1, (x64.var(-1, unbiased=False) + 1e-6).rsqrt(), F32, what="rstd")
        c.same(y0, y1, mask((T, D), *[(r, slice(None)) for r in rows]), what="y")
        c.same(m0, m1, mask((T,), *[(r,) for r in rows]), what="mean")
        c.same(r0, r1, mask((T,), *[(r,) for r in rows]), what="rstd")

    dy = rnd(T, D, dtype=dtype, seed=30)
    dres = rnd(T, D, seed=40)

    def bwd(x_, dy_):
        mean, rstd = torch.empty(T, device="cuda"), torch.empty(T, device="cuda")
        ops.layernorm_fwd(x_, gamma, torch.zeros(D, device="cuda"), torch.empty(T, D, device="cuda"), mean, rstd)
        dx, c1 = kc.guarded(T, D, F32)
        dg, c2 = kc.guarded(1, D, F32)
        db, c3 = kc.guarded(1, D, F32)
        snap = kc.snapshot(dy=dy_, x=x_, mean=mean, rstd=rstd, gamma=gamma, dres=dres)
        ops.layernorm_bwd(dy_, x_, mean, rstd, gamma, dres, dx, dg.view(D), db.view(D))
        sync(); kc.unchanged(snap); c1(); c2(); c3()
        return dx.clone(), dg.view(D).clone(), db.view(D).clone()

    def ref_bwd(x_, dy_):
        xr, gr = d64(x_).requires_grad_(), d64(gamma).requires_grad_()
        br = torch.zeros(D, dtype=torch.float64, requires_grad=True)
        F.layer_norm(xr, (D,), gr, br, 1e-6).backward(d64(dy_))
        return xr.grad + d64(dres), gr.grad, br.grad
    base = bwd(x, dy)
    with Case("layernorm") as c:
        dspots = [((0, 3), NAN), ((63, 0), NAN), ((64, D - 1), NAN), ((129, 7), NAN)]
        dyp = plant(dy, *dspots)
        got, ref = bwd(x, dyp), ref_bwd(x, dyp)
        cols = [cc for (_, cc), _ in dspots]
        for j, (name, dep) in enumerate((("dx", mask((T, D), *[(r, slice(None)) for r in rows])),
                                         ("dgamma", mask((D,), *[(cc,) for cc in cols])), ("dbeta", mask((D,), *[(cc,) for cc in cols])))):
            c.agree(got[j], ref[j], F32, what=name)
            c.same(base[j], got[j], dep, what=name)
    with Case("layernorm") as c:
        xq = plant(x, ((64, 9), NAN))
        got, ref = bwd(xq, dy), ref_bwd(xq, dy)
        assert bool(ref[1].isnan().all()) and bool(ref[2].isfinite().all())
        for j, (name, dep) in enumerate((("dx", mask((T, D), (64, slice(None)))), ("dgamma", mask((D,), (slice(None),))),
                                         ("dbeta", mask((D,))))):
            c.agree(got[j], ref[j], F32, what=name)
            c.same(base[j], got[j], dep, what=name)


# =========================================================================================================== tokens.hip
@pytest.mark.parametrize("dtype", DTYPES)
def test_patchify_and_token_assembly(ops, dtype):
    """m3_im2row (B 2, 2 x 3 patches of 4 x 4 pixels): one pixel reaches one element of one patch row.  m3_assemble_tokens(2):
    patch (i, c) reaches token (b, prefix + p, c); pos (j, c) reaches token j of every image; cls (c) token 0 of every image.
    m3_tokens_bwd(2): dtok (b, j, c) reaches its dpatch element, dpos (j, c) - a sum over the images - and dcls / ddist (c) for
    the prefix tokens: non-finite exactly where the float64 sums are."""
    B, P, H, W, D = 2, 4, 8, 12, 64
    np_ = (H // P) * (W // P)
    img = rnd(B, 3, H, W, seed=80)
    # pixel (b, ch, y, x) -> patch row b np + (y // P) (W // P) + x // P, column ch P P + (y % P) P + x % P
    pix = [((0, 0, 0, 0), NAN), ((0, 2, 7, 11), INF), ((1, 1, 4, 3), -INF)] + ([((1, 0, 3, 8), 2.0e5)] if dtype == F16 else [])
    ip = plant(img, *pix)
    unfold = lambda t: t.unfold(2, P, P).unfold(3, P, P).permute(0, 2, 3, 1, 4, 5).reshape(B * np_, 3 * P * P)     # noqa: E731
    with Case("tokens") as c:
        def im2row(i_):
            rows, check = kc.guarded(B * np_, 3 * P * P, dtype)
            snap = kc.snapshot(img=i_)
            ops.im2row(i_, P, rows)
            sync(); kc.unchanged(snap); check()
            return rows.clone()
        r0, r1 = im2row(img), im2row(ip)
        c.agree(r1, d64(unfold(ip)), dtype, what="im2row")
        c.same(r0, r1, mask((B * np_, 3 * P * P), *[(b * np_ + (y // P) * (W // P) + xx // P, ch * P * P + (y % P) * P + xx % P)
                                                   for (b, ch, y, xx), _ in pix]), what="im2row")
        assert kc.same_bits(r1, unfold(ip).to(dtype))
    if dtype != F32:
        return                                              # the token kernels are fp32 in, fp32 out but for dpatch
    patch, cls, dist = rnd(B * np_, D, seed=81), rnd(D, seed=82), rnd(D, seed=85)
    for pre in (1, 2):
        pos = rnd(np_ + pre, D, seed=83)
        L = np_ + pre

        def assemble(p_, c_, d_, s_):
            tok, check = kc.guarded(B * L, D, F32)
            if pre == 1:
                ops.assemble_tokens(p_, c_, s_, B, np_, D, tok)
            else:
                ops.assemble_tokens2(p_, c_, d_, s_, B, np_, D, tok)
            sync(); check()
            return tok.view(B, L, D).clone()
        with Case("tokens") as c:
            pp = plant(patch, ((0, 0), NAN), ((np_ - 1, D - 1), INF), ((np_, 5), -INF))
            cp = plant(cls, ((7,), NAN))
            sp = plant(pos, ((L - 1, 9), INF))
            t0, t1 = assemble(patch, cls, dist, pos), assemble(pp, cp, dist, sp)
            prefix = [cp.view(1, 1, D).expand(B, 1, D)] + ([dist.view(1, 1, D).expand(B, 1, D)] if pre == 2 else [])
            ref = torch.cat(prefix + [pp.view(B, np_, D)], 1) + sp
            c.agree(t1, d64(ref), F32, what="tokens")
            c.same(t0, t1, mask((B, L, D), (0, pre, 0), (0, L - 1, D - 1), (1, pre, 5), (slice(None), 0, 7), (slice(None), L - 1, 9)), what="tokens")

        dtok = rnd(B * L, D, seed=84)

        def tbwd(d_):
            dpatch, c1 = kc.guarded(B * np_, D, F16)
            dpos, c2 = kc.guarded(L, D, F32)
            dcls, c3 = kc.guarded(1, D, F32)
            dd, c4 = kc.guarded(1, D, F32)
            if pre == 1:
                ops.tokens_bwd(d_, B, np_, D, dpatch, dpos, dcls.view(D), beta=0)
            else:
                ops.tokens_bwd2(d_, B, np_, D, dpatch, dpos, dcls.view(D), dd.view(D), beta=0)
            sync(); c1(); c2(); c3()
            if pre == 2:
                c4()
            return dpatch.view(B, np_, D).clone(), dpos.clone(), dcls.view(D).clone(), dd.view(D).clone()
        with Case("tokens") as c:
            # image 0 token 0 (cls), image 1 token pre - 1 (the last prefix token), image 0's last patch, image 1's first patch
            dsp = [((0, 3), NAN), ((L + pre - 1, 11), INF), ((L - 1, D - 1), -INF), ((L + pre, 0), NAN), ((L + L - 1, 2), 2.0e5)]
            dq = plant(dtok, *dsp)
            a0, a1 = tbwd(dtok), tbwd(dq)
            d3 = d64(dq).view(B, L, D)
            c.agree(a1[0], d3[:, pre:], F16, kc.store(F16, torch.nan_to_num(d3[:, pre:], 0, 0, 0)), what="dpatch")
            c.agree(a1[1], d3.sum(0), F32, what="dpos")
            c.agree(a1[2], d3[:, 0].sum(0), F32, what="dcls")
            c.same(a0[0], a1[0], mask((B, np_, D), (0, np_ - 1, D - 1), (1, 0, 0), (1, np_ - 1, 2)), what="dpatch")
            c.same(a0[1], a1[1], mask((L, D), (0, 3), (pre - 1, 11), (L - 1, D - 1), (pre, 0), (L - 1, 2)), what="dpos")
            c.same(a0[2], a1[2], mask((D,), (3,), *([(11,)] if pre == 1 else [])), what="dcls")
            if pre == 2:
                c.agree(a1[3], d3[:, 1].sum(0), F32, what="ddist")
                c.same(a0[3], a1[3], mask((D,), (11,)), what="ddist")


# ================================================================================================== m3_gemm_nt (gemm*.hip)
import test_contract_gemm as tg                      # noqa: E402  (gemm_args / _slots / Addr: the struct the other module launches)


def gelu_grad64(pre64):
    p = pre64.clone().requires_grad_()
    (g,) = torch.autograd.grad(F.gelu(p).sum(), p)
    return g


def gemm_once(ops, cfg, A, B, bias, res, gpre, kernel):
    """one m3_gemm_nt launch of cfg with guarded C (and pre_out); returns (C, pre_out, signature).  The stated kernel is asserted
    on the launched struct"""
    dtype, M, N, K, epi = cfg["dtype"], cfg["M"], cfg["N"], cfg["K"], cfg["epi"]
    c_dtype = F32 if (dtype == F32 or epi == "res") else dtype
    rows_c = cfg.get("rows_c", M)
    C, c_check = kc.guarded(rows_c, N, c_dtype, ld=N + 8)
    pre, pre_check = kc.guarded(rows_c, N, dtype, ld=N + 8) if epi == "gelu" else (None, None)
    a = tg.gemm_args(ops, A=A, B=B, C=C, c_dtype=c_dtype, M=M, N=N, K=K, G=B.shape[0], dtype=dtype, a_row_idx=cfg.get("a_idx"),
                     a_row_div=cfg.get("a_div", 1), c_row_idx=cfg.get("c_idx"), bias=None if bias is None else bias.view(-1),
                     pre=pre, gpre=gpre, res=res, act=ops.M3_ACT_GELU if epi == "gelu" else 0, offsets=cfg.get("off"),
                     tile_starts=cfg.get("ts"))
    sig = ls.gemm_signature(ops, a)
    assert sig.get("kernel") == kernel, f"the case states the {kernel} kernel and runs\n  {sig}"
    snap = kc.snapshot(A=A, B=B, bias=bias, res=res, gpre=gpre)
    from ctypes import byref
    ops.check(ops.lib().m3_gemm_nt(byref(a), ops._stream()), "m3_gemm_nt")
    sync(); kc.unchanged(snap)
    keep = cfg.get("keep")
    c_check(keep_rows=keep, what="C")
    if pre is not None:
        pre_check(keep_rows=keep, what="pre_out")
    return C.clone(), None if pre is None else pre.clone(), sig


def gemm_ref(cfg, A, B, bias, res, gpre):
    """(C, pre_out) float64 [Mv, N] by slot, torch ops on the CPU: A[arow] @ B[g]^T + bias[g], F.gelu, GELU'(pre) by autograd"""
    arow, crow, grp = cfg["arow"], cfg["crow"], cfg["grp"]
    A64, B64 = d64(A)[arow], d64(B)
    lin = torch.empty(len(arow), cfg["N"], dtype=torch.float64)
    for g in range(B64.shape[0]):
        sel = (grp == g).nonzero().flatten()
        if sel.numel():
            lin[sel] = A64[sel] @ B64[g].t() + (d64(bias)[g] if bias is not None else 0.0)
    v = lin
    if cfg["epi"] == "gelu":
        v = F.gelu(lin)
    if gpre is not None:
        v = v * gelu_grad64(d64(gpre)[crow])
    if res is not None:
        v = v + d64(res)[crow]
    return v, lin


def gemm_contract(ops, c, cfg, kernel, ops_in, poisons):
    """clean run, then one run per poison = (name, {operand: planted copy}, depends mask over slots x N): every run takes the
    same kernel and signature; C (and pre_out) of the poisoned run are torch's non-finite pattern and keep the clean bits
    outside the mask"""
    dtype, epi = cfg["dtype"], cfg["epi"]
    c_dtype = F32 if (dtype == F32 or epi == "res") else dtype
    crow = cfg["crow"]
    C0, P0, sig0 = gemm_once(ops, cfg, kernel=kernel, **ops_in)
    for name, repl, dep in poisons:
        opsp = dict(ops_in, **repl)
        C1, P1, sig1 = gemm_once(ops, cfg, kernel=kernel, **opsp)
        assert sig1 == sig0, "the poisoned run took another launch plan"
        v, lin = gemm_ref(cfg, **opsp)
        full = torch.zeros(C0.shape, dtype=torch.bool)
        full[crow] = dep
        c.agree(C1[crow], v, c_dtype, what=f"{name}: C")
        c.same(C0, C1, full, what=f"{name}: C")
        if P1 is not None:
            c.agree(P1[crow], lin, dtype, what=f"{name}: pre_out")
            c.same(P0, P1, full, what=f"{name}: pre_out")


# dense id: dtype, M, N, K, gemm_set_big mode, the kernel the case states.  M 130 = one whole 128-row tile and two rows; N 136 =
# one column tile and 8 columns; K 64 and 192: one and three 128-byte slices of a 16-bit row.  The last two: one shape of the
# register-staged and one of the 256 x 256 kernel from tests/test_contract_gemm.py's table
GEMM_DENSE = {
    "f16_k64": (F16, 130, 136, 64, None, "dma"), "f16_k192": (F16, 130, 136, 192, None, "dma"),
    "bf16_k64": (BF16, 130, 136, 64, None, "dma"), "bf16_k192": (BF16, 130, 136, 192, None, "dma"),
    "f32_k64": (F32, 130, 136, 64, None, "staged"), "f32_k192": (F32, 130, 136, 192, None, "staged"),
    "f16_staged_n132": (F16, 333, 132, 192, None, "staged"), "f16_big_k512": (F16, 300, 384, 512, 1, "big"),
}
GEMM_EPIS = ["bias", "gelu", "gpre", "res"]


def gemm_dense_cfg(name, epi):
    dtype, M, N, K, big, kernel = GEMM_DENSE[name]
    return dict(dtype=dtype, M=M, N=N, K=K, epi=epi, arow=torch.arange(M), crow=torch.arange(M), grp=torch.zeros(M, dtype=torch.long)), big, kernel


@pytest.mark.parametrize("epi", GEMM_EPIS)
@pytest.mark.parametrize("name", list(GEMM_DENSE))
def test_gemm_dense(ops, name, epi):
    """A (r, c) reaches row r of C (and of pre_out); B (n, c) and bias (n) reach column n.  Planted in A: NaN in the first row,
    +Inf in the last K column of the last row of the first tile, -Inf in the first row of the next tile, NaN in the last row,
    and (16-bit) the overflow value next to a B entry of 8: that one C element is Inf, not the dtype's maximum.  GELU of the
    planted rows is torch's: F.gelu([nan, inf, -inf]) = [nan, inf, nan]."""
    cfg, big, kernel = gemm_dense_cfg(name, epi)
    dtype, M, N, K = cfg["dtype"], cfg["M"], cfg["N"], cfg["K"]
    last_tile = (M - 1) // 128 * 128
    A = rnd(M, K + 8, dtype=dtype, seed=1)[:, :K]
    B = rnd(1, N, K, dtype=dtype, scale=0.06, seed=2)
    B[0, 9, 3] = 8.0
    ins = dict(A=A, B=B, bias=rnd(1, N, scale=0.1, seed=5) if epi in ("bias", "gelu", "res") else None,
               res=rnd(M, N + 8, seed=7)[:, :N] if epi == "res" else None,
               gpre=rnd(M, N + 8, dtype=dtype, seed=6)[:, :N] if epi == "gpre" else None)
    if ins["gpre"] is not None:
        ins["gpre"][64, 9] = 3.0                      # GELU'(3) = 1.01: the overflowing element stays past 2 x the maximum
    a_spots = [((0, 0), NAN), ((last_tile - 1, K - 1), INF), ((last_tile, 5), -INF), ((M - 1, 7), NAN)]
    if dtype != F32:
        a_spots.append(((64, 3), OVER[dtype]))
    b_spots = [((0, 0, 1), NAN), ((0, N - 1, K - 1), INF), ((0, 128, 0), -INF)]
    poisons = [("A rows", dict(A=plant(A, *a_spots)), mask((M, N), *[(r, slice(None)) for (r, _), _ in a_spots])),
               ("B rows", dict(B=plant(B, *b_spots)), mask((M, N), *[(slice(None), n) for (_, n, _), _ in b_spots]))]
    if ins["bias"] is not None:
        poisons.append(("bias", dict(bias=plant(ins["bias"], ((0, 5), NAN), ((0, N - 1), -INF))), mask((M, N), (slice(None), 5), (slice(None), N - 1))))
    if big is not None:
        ops.gemm_set_big(big)
    try:
        with Case("gemm_nt") as c:
            gemm_contract(ops, c, cfg, kernel, ins, poisons)
            if dtype != F32 and epi != "res":
                # the overflowing store, stated on its own: row 64, column 9 is Inf in the poisoned run
                C1, _, _ = gemm_once(ops, cfg, kernel=kernel, **dict(ins, A=poisons[0][1]["A"]))
                assert float(C1[64, 9]) == INF, f"C[64, 9] = {float(C1[64, 9])}: an overflowing store must give Inf"
    finally:
        if big is not None:
            ops.gemm_set_big(-1)


GEMM_GROUPED = {"f16": (F16, "dma"), "bf16": (BF16, "dma"), "f32": (F32, "staged")}
COUNTS = (130, 0, 5)


@pytest.mark.parametrize("epi", ["bias", "gelu"])
@pytest.mark.parametrize("name", list(GEMM_GROUPED))
def test_gemm_grouped_gather_scatter(ops, name, epi):
    """groups of (130, 0, 5) rows, N 136, K 64, A gathered through a_row_idx / 4 (every A row named at most once, five named by
    nothing), C scattered through c_row_idx, 9 slack slots behind the last group.  A row named by slot s reaches C row
    c_row_idx[s] only - the last slot of the ragged group 0 and the first slot of group 2 (the tile behind it) are the ones
    that matter; B (g, n, :) and bias (g, n) reach column n of group g's rows only; an A row no slot names (one named by nothing,
    one named by a slack slot), the empty group's B and bias reach nothing: bitwise."""
    dtype, kernel = GEMM_GROUPED[name]
    G, N, K, div = len(COUNTS), 136, 64, 4
    Mv = sum(COUNTS)
    M = Mv + 9
    off, ts, grp, _ = tg._slots(M, G, list(COUNTS))
    g = torch.Generator().manual_seed(3)
    a_rows = M + 5
    perm = torch.randperm(a_rows, generator=g)
    a_idx = (perm[:M] * div + torch.randint(0, div, (M,), generator=g)).to(torch.int32).cuda()
    rows_c = M + 10
    c_idx = torch.randperm(rows_c, generator=g)[:M].to(torch.int32).cuda()
    arow, crow = perm[:Mv], c_idx.long().cpu()[:Mv]
    owned = torch.zeros(rows_c, dtype=torch.bool)
    owned[crow] = True
    cfg = dict(dtype=dtype, M=M, N=N, K=K, epi=epi, a_idx=a_idx, a_div=div, c_idx=c_idx, off=off, ts=ts, rows_c=rows_c,
               keep=(~owned).nonzero().flatten(), arow=arow, crow=crow, grp=grp.cpu()[:Mv])
    A = rnd(a_rows, K + 8, dtype=dtype, seed=1)[:, :K]
    B = rnd(G, N, K, dtype=dtype, scale=0.06, seed=2)
    B[0, 9, 3] = 8.0
    bias = rnd(G, N, scale=0.1, seed=5)
    ins = dict(A=A, B=B, bias=bias, res=None, gpre=None)
    slots = [0, 127, 128, 129, 130, 134]              # group 0: first, both sides of the tile boundary, last; group 2: first, last
    vals = [NAN, INF, -INF, NAN, INF, NAN]
    a_spots = [((int(arow[s]), (K - 1) if v == INF else s % 7), v) for s, v in zip(slots, vals)]
    if dtype != F32:
        slots.append(64)
        a_spots.append(((int(arow[64]), 3), OVER[dtype]))
    nobody = [((int(perm[M + 1]), 0), NAN), ((int(perm[M + 4]), K - 1), INF), ((int(perm[Mv + 2]), 1), NAN)]
    g2 = mask((Mv, N))
    g2[130:135, 7] = True
    g2[130:135, N - 1] = True
    g0 = mask((Mv, N))
    g0[0:130, 128] = True
    poisons = [("A rows", dict(A=plant(A, *a_spots)), mask((Mv, N), *[(s, slice(None)) for s in slots])),
               ("B and bias of group 2", dict(B=plant(B, ((2, 7, 0), NAN)), bias=plant(bias, ((2, N - 1), INF))), g2),
               ("B of group 0", dict(B=plant(B, ((0, 128, K - 1), -INF))), g0),
               ("unnamed A rows, the empty group's B and bias",
                dict(A=plant(A, *nobody), B=plant(B, ((1, 0, 0), NAN), ((1, N - 1, K - 1), INF)), bias=plant(bias, ((1, 3), NAN))), mask((Mv, N)))]
    with Case("gemm_nt") as c:
        gemm_contract(ops, c, cfg, kernel, ins, poisons)


# ============================================================================== weight gradients (wgrad*.hip, reduce.hip)
import test_contract_wgrad as tw                     # noqa: E402  (routing / knobs)

# id: dtype, N, K, wgrad_set_dma, wgrad_set_big, grouped (130, 0, 5) or plain rows, row splits (1: direct mode where the kernel has
# it, else slabs), the kernel the case states (after the library's step-downs)
WGRAD = {
    "staged_f16_direct": (F16, 136, 64, 0, 0, True, 1, "staged"), "staged_f16_slabs": (F16, 136, 64, 0, 0, True, 4, "staged"),
    "dma_f16_direct": (F16, 136, 64, 2, 0, True, 1, "dma"), "dma_f16_slabs": (F16, 136, 64, 2, 0, True, 4, "dma"),
    "dma_bf16_slabs": (BF16, 136, 64, 2, 0, True, 4, "dma"), "staged_bf16_direct": (BF16, 136, 64, 0, 0, True, 1, "staged"),
    "dma_f32_direct": (F32, 136, 64, 2, 0, True, 1, "dma"), "dma_f32_slabs": (F32, 136, 64, 2, 0, True, 4, "dma"),
    "big_f16_slabs": (F16, 256, 512, None, 1, True, 4, "big"), "big_bf16_direct": (BF16, 512, 256, None, 1, True, 1, "big"),
    "skinny16_f16_slabs": (F16, 384, 16, None, None, False, 2, "skinny"), "skinny32_f32_slabs": (F32, 384, 32, None, None, False, 2, "skinny"),
}


def wgrad_once(ops, dtype, M, N, K, G, off, splits, dC, A, kernel, mode):
    grouped = off is not None
    want_db = kernel != "skinny"                       # (the streaming kernel takes calls without the bias column sums)
    p = ops.wgrad_launch_plan(M, N, K, G, dtype, grouped=grouped, bias=want_db, splits=splits)
    ws, wcheck = kc.guarded_ws(p.ws_elems)
    dW, c1 = kc.guarded(G * N, K, F32)
    db, c2 = kc.guarded(G, N, F32)
    snap = kc.snapshot(dC=dC, A=A)
    with ls.Recorder(ops) as rec:
        ops.wgrad_tn(dC, A, dW.view(G, N, K) if G > 1 else dW, M=M, splits=p.splits, ws=ws, group_offsets=off,
                     db=None if not want_db else (db if G > 1 else db.view(N)))
    ((_, launched, _),) = rec.calls
    sig = ls.wgrad_signature(ops, launched)
    assert sig.get("kernel") == kernel and sig.get("mode") == mode, f"the case states {kernel} / {mode} and runs\n  {sig}"
    sync(); kc.unchanged(snap); wcheck(); c1(); c2(keep_rows=None if want_db else range(G))
    return dW.view(G, N, K).clone(), db.clone() if want_db else None, sig


@pytest.mark.parametrize("name", list(WGRAD))
def test_wgrad_tn(ops, name):
    """dW[g][n, k] = sum over group g's rows of dC[r, n] A[r, k], db[g][n] the column sums of dC.  A (r, c) of group g reaches
    dW[g][:, c] only; dC (r, n) reaches dW[g][n, :] and db[g][n] only; rows behind the last group reach nothing.  Groups (130, 0,
    5): the last row of group 0 and the first row of group 2 - which a tile that runs past a ragged group's end would read - are
    the cases that matter; the empty group's dW and db are zero in both runs."""
    dtype, N, K, dma, big, grouped, splits, kernel = WGRAD[name]
    if grouped:
        G, Mv = 3, sum(COUNTS)
        M = Mv + 9
        off, grp, _ = tw.routing(G, list(COUNTS))
        grp = grp.cpu()
        first2 = COUNTS[0]
    else:
        G, Mv, M, off, first2 = 1, 135, 135, None, 130
        grp = torch.zeros(M, dtype=torch.long)
    dC, A = rnd(M, N, dtype=dtype, seed=1), rnd(M, K, dtype=dtype, seed=2)
    g_of = lambda r: int(grp[r])                                                         # noqa: E731

    def ref(dC_, A_):
        L, R = d64(dC_)[:Mv], d64(A_)[:Mv]
        W = torch.zeros(G, N, K, dtype=torch.float64)
        b = torch.zeros(G, N, dtype=torch.float64)
        for g in range(G):
            sel = (grp[:Mv] == g).nonzero().flatten()
            if sel.numel():
                W[g], b[g] = L[sel].t() @ R[sel], L[sel].sum(0)
        return W, b
    a_spots = [((0, K - 1), -INF), ((first2 - 1, 1), NAN), ((first2, 5), INF), ((Mv - 1, 0), NAN)]
    c_spots = [((127, 3), NAN), ((128, N - 1), INF), ((first2, 9), -INF), ((Mv - 1, 128), NAN)]
    slack = [((r, c), v) for r, c, v in ((Mv, 0, NAN), (M - 1, 7, INF))] if M > Mv else []
    with tw.knobs(ops, dma, big), Case("wgrad") as c:
        mode = "direct" if splits == 1 else ("balanced" if grouped else "slabs")
        W0, b0, sig0 = wgrad_once(ops, dtype, M, N, K, G, off, splits, dC, A, kernel, mode)
        for what, dCp, Ap, depW, depb in (
                ("A", dC, plant(A, *a_spots), mask((G, N, K), *[(g_of(r), slice(None), col) for (r, col), _ in a_spots]), mask((G, N))),
                ("dC", plant(dC, *c_spots), A, mask((G, N, K), *[(g_of(r), n, slice(None)) for (r, n), _ in c_spots]),
                 mask((G, N), *[(g_of(r), n) for (r, n), _ in c_spots])),
                ("rows behind the last group", plant(dC, *slack), plant(A, *slack), mask((G, N, K)), mask((G, N)))):
            if what.startswith("rows") and not slack:
                continue
            W1, b1, sig1 = wgrad_once(ops, dtype, M, N, K, G, off, splits, dCp, Ap, kernel, mode)
            assert sig1 == sig0, "the poisoned run took another launch plan"
            rW, rb = ref(dCp, Ap)
            c.agree(W1, rW, F32, what=f"{what}: dW")
            c.same(W0, W1, depW, what=f"{what}: dW")
            if b1 is not None:
                c.agree(b1, rb, F32, what=f"{what}: db")
                c.same(b0, b1, depb, what=f"{what}: db")


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_wgrad_multi_and_colsum(ops, dtype):
    """m3_wgrad_multi (one kernel per dtype, plain rows 0 .. M-1 of two problems in one launch, M 130): A_j (r, c) reaches column
    c of dW_j only, dC_j (r, n) row n of dW_j and db_j[n]; the other problem and the operand rows behind M reach nothing.
    m3_colsum, grouped (130, 0, 5) through c_row_idx: dC (r, n) reaches db[g][n]; a row no index names reaches nothing."""
    M, shapes = 130, [(136, 72), (128, 264)]
    cs = [(rnd(M + 4, N, dtype=dtype, seed=10 + j), rnd(M + 4, K, dtype=dtype, seed=20 + j)) for j, (N, K) in enumerate(shapes)]
    plan = ops.wgrad_multi_plan([(N, K, True) for N, K in shapes], M, dtype, 0)
    assert plan.allowed

    def multi(ops_in):
        outs, checks = [], []
        for N, K in shapes:
            dW, c1 = kc.guarded(N, K, F32)
            db, c2 = kc.guarded(1, N, F32)
            outs.append((dW, db)); checks += [c1, c2]
        ws, wcheck = kc.guarded_ws(plan.ws_elems)
        with ls.Recorder(ops) as rec:
            ops.wgrad_multi([(cc[0], cc[1], o[0], o[1].view(-1), 0) for cc, o in zip(ops_in, outs)], M, ws=ws)
        ((_, launched, _),) = rec.calls
        sync(); wcheck()
        for chk in checks:
            chk()
        return [(o[0].clone(), o[1].view(-1).clone()) for o in outs], ls.wgrad_multi_signature(ops, launched)
    with Case("wgrad") as c:
        base, sig0 = multi(cs)
        N0, K0 = shapes[0]
        p0 = (plant(cs[0][0], ((0, 3), NAN), ((129, N0 - 1), INF), ((M, 5), NAN), ((M + 3, 0), INF)),
              plant(cs[0][1], ((127, K0 - 1), -INF), ((128, 0), NAN), ((M + 1, 1), NAN)))
        got, sig1 = multi([p0, cs[1]])
        assert sig1 == sig0
        L, R = d64(p0[0])[:M], d64(p0[1])[:M]
        c.agree(got[0][0], L.t() @ R, F32, what="dW_0")
        c.agree(got[0][1], L.sum(0), F32, what="db_0")
        c.same(base[0][0], got[0][0], mask((N0, K0), (3, slice(None)), (N0 - 1, slice(None)), (slice(None), K0 - 1), (slice(None), 0)), what="dW_0")
        c.same(base[0][1], got[0][1], mask((N0,), (3,), (N0 - 1,)), what="db_0")
        c.same(base[1][0], got[1][0], mask(base[1][0].shape), what="dW_1")
        c.same(base[1][1], got[1][1], mask(base[1][1].shape), what="db_1")

    G, N, Mv = 3, 136, sum(COUNTS)
    Mc = Mv + 9
    off, grp, _ = tw.routing(G, list(COUNTS))
    grp = grp.cpu()
    c_idx = torch.randperm(Mc + 6, generator=torch.Generator().manual_seed(6))
    unnamed = c_idx[Mc:]
    c_idx = c_idx[:Mc].to(torch.int32).cuda()
    dC = rnd(Mc + 6, N, dtype=dtype, seed=40)

    def colsum(dC_):
        ws, wcheck = kc.guarded_ws(int(ops.lib().m3_colsum_ws_elems(Mc, N, G)))
        db, check = kc.guarded(G, N, F32)
        snap = kc.snapshot(dC=dC_, c_idx=c_idx)
        ops.colsum(dC_, db, M=Mc, c_row_idx=c_idx, group_offsets=off, ws=ws)
        sync(); kc.unchanged(snap); wcheck(); check()
        return db.clone()
    with Case("wgrad") as c:
        rows = c_idx.long().cpu()
        spots = [((int(rows[0]), 0), NAN), ((int(rows[129]), N - 1), INF), ((int(rows[130]), 7), -INF), ((int(rows[134]), 128), NAN)]
        dCp = plant(dC, *spots, ((int(unnamed[0]), 3), NAN), ((int(unnamed[5]), N - 1), INF), ((int(rows[Mv + 1]), 2), NAN))
        d0, d1 = colsum(dC), colsum(dCp)
        L = d64(dCp)[rows[:Mv]]
        c.agree(d1, torch.stack([L[grp[:Mv] == g].sum(0) for g in range(G)]), F32, what="colsum db")
        c.same(d0, d1, mask((G, N), (0, 0), (0, N - 1), (2, 7), (2, 128)), what="colsum db")


# ======================================================================================================= attention*.hip
import test_contract_attention as ta                 # noqa: E402  (heads / planned)

# (B, N, heads, dh) -> the 16-bit instance the shape states (forward key tiles, backward tiles per wave; None: the streamed
# kernels); fp32 takes attention_f32.hip at every N.  B = 2 on purpose: the other image must not notice
ATTN = {(2, 17, 1, 32): (4, 1), (2, 197, 1, 32): (16, 4), (2, 16, 2, 64): (4, 1), (2, 257, 1, 32): None}


def attn_stated(dtype, shape):
    if dtype == F32:
        return ("f32", 0, "f32", 0)
    inst = ATTN[shape]
    return ("streamed", 0, "streamed", 0) if inst is None else ("resident", inst[0], "resident", inst[1])


def attn_ref(qkv, d_o, B, N, h, dh):
    """torch's float64 attention on the CPU: softmax(q k^T / sqrt dh) v and its autograd.  lse is the kernels' own by-product
    (no tensor of the reference model): logsumexp of the logits, NaN where the softmax row is NaN"""
    qr = d64(qkv).requires_grad_()
    q, k, v = ta.heads(qr, B, N, h, dh, 3)
    s = (q @ k.transpose(-2, -1)) * dh ** -0.5
    p = torch.softmax(s, -1)
    o = p @ v
    lse = torch.where(p.detach().isnan().any(-1), torch.full((), NAN, dtype=torch.float64), torch.logsumexp(s.detach(), -1))
    (do_h,) = ta.heads(d64(d_o), B, N, h, dh, 1)
    (g,) = torch.autograd.grad(o, qr, do_h)
    return o.detach(), lse, g, p.detach()


@pytest.mark.parametrize("shape", list(ATTN), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_forward_and_backward(ops, dtype, shape):
    """m3_attention_fwd / _bwd.  One run per planted tensor (q, k, v, d_o), each with a value in the LAST token of image 0 (head
    0) and one in the FIRST token of image 1 (the last head): every element of o, lse and dqkv that belongs to another (image,
    head) than the planted ones keeps its bits; inside, the pattern is the reference's.  q: NaN / +Inf (the query row, and
    through dK and dV of the backward the whole (image, head)); k: NaN / -Inf (a -Inf logit is probability 0 for the queries
    whose q component is positive: those rows of o stay finite); v: NaN / +Inf with the flat logits this test uses (the
    smallest probability is far above 2^-100, so no fp32 probability underflows to 0 in front of an Inf); d_o: NaN only - with
    an Inf in d_o the kernel's D = rowsum(dO o O) (finite o: +-Inf) and torch's sum_j P_j dP_j (Inf - Inf: NaN) differ by
    algebra, not by a defect."""
    B, N, h, dh = shape
    C = h * dh
    assert ta.planned(ops, dtype, shape) == attn_stated(dtype, shape)
    qkv = ta.make_qkv(B, N, h, dh, "flat", dtype, seed=N + dh)
    d_o = torch.randn(B * N, C, generator=torch.Generator().manual_seed(7)).to(dtype).cuda()
    need = int(ops.lib().m3_attention_bwd_ws_elems(B, N, h, dh))

    def run(qkv_, d_o_):
        o, c1 = kc.guarded(B * N, C, dtype)
        lse, c2 = kc.guarded(B * h, N, F32)
        snap = kc.snapshot(qkv=qkv_)
        ops.attention_fwd(qkv_, B, N, h, dh, o, lse.view(B, h, N))
        sync(); kc.unchanged(snap); c1(); c2()
        ws, wcheck = kc.guarded_ws(need) if need else (None, None)
        dqkv, c3 = kc.guarded(B * N, 3 * C, dtype)
        o_in = o.clone()
        snap = kc.snapshot(qkv=qkv_, o=o_in, d_o=d_o_, lse=lse)
        ops.attention_bwd(qkv_, o_in, d_o_, lse.view(B, h, N), B, N, h, dh, dqkv, dq_ws=ws)
        sync(); kc.unchanged(snap); c3()
        if wcheck:
            wcheck()
        return o_in, lse.view(B, h, N).clone(), dqkv.clone()
    o0, l0, g0 = run(qkv, d_o)
    _, _, _, p0 = attn_ref(qkv, d_o, B, N, h, dh)
    assert float(p0.min()) > 2.0 ** -100, "the logits are not flat enough for an Inf in V"
    # column of component (part, head, d) in a qkv row; the planted (image, head) pairs
    col = lambda part, hh, d: (part * h + hh) * dh + d                                   # noqa: E731
    t0, t1, hl = N - 1, N, h - 1
    for part, name, v0, v1 in ((0, "q", NAN, INF), (1, "k", NAN, -INF), (2, "v", INF, NAN), (3, "d_o", NAN, NAN)):
        for tok, hh, d, val, b in ((t0, 0, 3, v0, 0), (t1, hl, dh - 1, v1, 1)):             # separately: one image per run
            dep_bh = mask((B, h, N, 1), (b, hh))
            with Case("attention") as c:
                if part < 3:
                    qp, dp = plant(qkv, ((tok, col(part, hh, d)), val)), d_o
                else:
                    qp, dp = qkv, plant(d_o, ((tok, hh * dh + d), val))
                o1, l1, g1 = run(qp, dp)
                ro, rl, rg, _ = attn_ref(qp, dp, B, N, h, dh)
                what = f"{name} of image {b}"
                (o_k,), (o_c,) = ta.heads(o1, B, N, h, dh, 1), ta.heads(o0, B, N, h, dh, 1)
                c.agree(o_k, ro, dtype, what=f"{what}: o")
                c.agree(l1, rl, F32, what=f"{what}: lse")
                c.same(o_c.contiguous(), o_k.contiguous(), dep_bh, what=f"{what}: o")
                c.same(l0, l1, dep_bh.squeeze(-1), what=f"{what}: lse")
                for got, clean, ref, nm in zip(ta.heads(g1, B, N, h, dh, 3), ta.heads(g0, B, N, h, dh, 3), ta.heads(rg, B, N, h, dh, 3), "qkv"):
                    c.agree(got, ref, dtype, what=f"{what}: d{nm}")
                    c.same(clean.contiguous(), got.contiguous(), dep_bh, what=f"{what}: d{nm}")


# ================================================================================================ the router (gate.hip)
import test_contract_gate as tgate                   # noqa: E402  (gate_call: m3_gate_fwd through the C ABI, every output guarded)


@pytest.mark.parametrize("E,k", [(8, 2), (5, 4)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gate_forward(ops, dtype, E, k):
    """m3_gate_fwd (instance: dtype, EPAD 8, exact E = 8 / padded E = 5), T 130 = two whole 64-token blocks and two tokens, D 64.
    One token's x holds NaN, +Inf or -Inf (token 64, the first of block 1; token 129, the last of the partial block; token 0).
    That token's clean / noisy logits are torch's x @ w_gate; its score, top_logits and the gates at its selected experts are
    NaN (softmax of a row with NaN or +-Inf), and idx, idx32, idx_next stay distinct and in [0, E): the kernel's `>` scan takes
    the lowest remaining index when every comparison is false, where torch.topk ranks NaN highest - a deliberate difference
    (any valid expert id keeps the routing in range; m3_route_build reports no out-of-range id).  Every other token's outputs
    and the part_* rows of the other 64-token blocks keep their bits."""
    T, D = ROW_T, ROW_D
    x = rnd(T, D, dtype=dtype, seed=E)
    w = rnd(D, E, scale=0.3, seed=E + 1)
    w = torch.where(w == 0, torch.full_like(w, 0.1), w)
    base = tgate.gate_call(ops, x, w, k)
    nblk = ops.lib().m3_gate_num_blocks(T)
    for t, d, val in ((64, 5, NAN), (129, D - 1, INF), (0, 0, -INF)):
        with Case("gate") as c:
            xp = plant(x, ((t, d), val))
            o = tgate.gate_call(ops, xp, w, k)
            sel = torch.cat((o["idx"][t].cpu(), o["idx_next"][t:t + 1].long().cpu()))
            assert sel.unique().numel() == k + 1 and int(sel.min()) >= 0 and int(sel.max()) < E, f"token {t}: experts {sel.tolist()}"
            assert torch.equal(o["idx32"].long(), o["idx"])
            ops.route_build(o["idx32"].contiguous(), E).check()                       # raises on an id outside [0, E)
            logits = d64(xp) @ d64(w)
            p = torch.softmax(logits, -1)
            assert bool(p[t].isnan().all())
            c.agree(o["clean"], logits, F32, what="clean")
            c.agree(o["noisy"], logits, F32, what="noisy")
            c.agree(o["score"], p.gather(1, o["idx"].cpu()), F32, what="score")
            c.agree(o["top_logits"], p.gather(1, torch.cat((o["idx"].cpu(), o["idx_next"].long().cpu().unsqueeze(1)), 1)), F32, what="top_logits")
            c.agree(o["gates"], torch.zeros(T, E, dtype=torch.float64).scatter(1, o["idx"].cpu(), p.gather(1, o["idx"].cpu())), F32, what="gates")
            row = mask((T, 1), (t,))
            for n in ("idx", "idx32", "score", "top_logits", "clean", "noisy", "gates"):
                c.same(base[n], o[n], row, what=n)
            c.same(base["idx_next"], o["idx_next"], row.squeeze(1), what="idx_next")
            blk = mask((nblk, 1), (t // 64,))
            for n in ("part_importance", "part_load", "part_count"):
                c.same(base[n], o[n], blk, what=n)
            assert bool(o["part_importance"][t // 64].isnan().any()), "the block's importance partial must carry the NaN"


@pytest.mark.parametrize("dtype", DTYPES)
def test_gate_backward(ops, dtype):
    """m3_gate_bwd_logits: d_logits[t] = p (dp - <p, dp>) from token t's stored logits and upstream gradients: a NaN or Inf in
    d_score[t] reaches row t only (the reference: float64 autograd through torch.softmax, kernel_contract.gate_bwd_reference).
    m3_gate_bwd_params: d_w_gate = x^T d_logits (a sum over the tokens), dx = d_logits w_gate^T: d_logits (t, e) reaches column e
    of d_w_gate and row t of dx."""
    T, D, E, k = ROW_T, ROW_D, 8, 2
    x = rnd(T, D, dtype=dtype, seed=3)
    w = rnd(D, E, scale=0.3, seed=4)
    f = ops.gate_fwd(x, w, k)
    d_score, d_imp = rnd(T, k, seed=5), rnd(E, seed=6)

    def logits_bwd(ds_):
        out, check = kc.guarded(T, E, F32)
        ops.gate_bwd_logits(f["noisy"], f["idx"], ds_, d_imp, k, out=out)
        sync(); check()
        return out.clone()
    with Case("gate") as c:
        dsp = plant(d_score, ((64, 0), NAN), ((129, 1), INF), ((0, 0), -INF))
        l0, l1 = logits_bwd(d_score), logits_bwd(dsp)
        ref, _ = kc.gate_bwd_reference(f["noisy"].cpu(), f["idx"].cpu(), k, d_score=dsp.cpu(), d_importance=d_imp.cpu())
        c.agree(l1, ref, F32, what="d_logits")
        c.same(l0, l1, mask((T, E), (64, slice(None)), (129, slice(None)), (0, slice(None))), what="d_logits")

    dl = rnd(T, E, scale=0.01, seed=7)

    def params(dl_):
        dW, c1 = kc.guarded(D, E, F32)
        dx, c2 = kc.guarded(T, D, F32)
        snap = kc.snapshot(x=x, w=w, dl=dl_)
        ops.gate_bwd_params(x, w, dl_, d_w_gate=dW, dx=dx)
        sync(); kc.unchanged(snap); c1(); c2()
        return dW.clone(), dx.clone()
    with Case("gate") as c:
        dlp = plant(dl, ((63, 0), NAN), ((64, E - 1), INF), ((129, 3), -INF))
        (W0, X0), (W1, X1) = params(dl), params(dlp)
        c.agree(W1, d64(x).t() @ d64(dlp), F32, what="d_w_gate")
        c.agree(X1, d64(dlp) @ d64(w).t(), F32, what="dx")
        c.same(W0, W1, mask((D, E), (slice(None), 0), (slice(None), E - 1), (slice(None), 3)), what="d_w_gate")
        c.same(X0, X1, mask((T, D), (63, slice(None)), (64, slice(None)), (129, slice(None))), what="dx")


# ============================================================================================== 3 x 3 convolutions (conv.hip)
import conv_common as CC                             # noqa: E402


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def test_conv3x3_forward_and_gradients(ops):
    """m3_pad_border_nhwc, m3_conv3x3_fwd, m3_conv3x3_wgrad on (N, H, W) = (2, 3, 5), 384 -> 40 channels, fp16 - the smallest case of
    tests/test_conv_gpu.py's FWD_CASES that has an interior pixel; m3_conv3x3_dgrad on its smallest DGRAD case with one,
    (2, 3, 5) 256 <- 256 bf16.  One planted pixel (one channel) reaches the outputs of its 3 x 3 footprint - clipped at the
    image's edge for the corner pixel - in every output channel, and nothing in the other image; in the weight gradient it
    reaches its own input channel (every output channel, the taps that see the pixel) and no bias gradient.  Reference:
    F.conv2d in float64 and its autograd."""
    from m3vit_amd import conv as MC
    (N, H, W), Cc, Cout, dtype = (2, 3, 5), 384, 40, F16
    M = N * H * W
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, Cc, H, W, generator=g).to(dtype)
    w = (torch.randn(Cout, Cc, 3, 3, generator=g) * 0.05).to(dtype)
    b = torch.randn(Cout, generator=g)
    dy = torch.randn(N, Cout, H, W, generator=g).to(dtype)
    p = ops.conv3x3_plan(dtype, N, H, W, Cc, Cout)
    assert p.ok
    w_fwd = MC.weight_operands(w.cuda(), dtype)[0]
    spots = [((0, 7, 0, 0), NAN), ((1, 200, 1, 2), INF)]                        # image 0's corner, image 1's interior pixel
    xp = plant(x, *spots)
    foot = mask((N, 1, H, W), (0, 0, slice(0, 2), slice(0, 2)), (1, 0, slice(0, 3), slice(1, 4)))

    def fwd(x_):
        pb, c0 = kc.guarded(N * (H + 2) * (W + 2), Cc, dtype)
        xb = ops.pad_border(_cl(x_), out=pb).view(N, H + 2, W + 2, Cc)
        sync(); c0(what="pad_border")
        assert kc.same_bits(xb, CC.bordered(x_).cuda()), "pad_border is not a bit copy inside a zero border"
        out, c1 = kc.guarded(M, Cout, dtype)
        ops.conv3x3_fwd(xb, w_fwd, b.cuda(), out=out)
        dw3, c2 = kc.guarded(3 * Cout, 3 * Cc, F32)
        db, c3 = kc.guarded(1, Cout, F32)
        ws, c4 = kc.guarded_ws(p.wgrad_ws_elems)
        ops.conv3x3_wgrad(xb, CC.rows(dy).cuda().contiguous(), dw3=dw3.view(3, Cout, 3 * Cc), db=db.view(Cout), ws=ws)
        sync(); c1(what="conv3x3_fwd"); c2(what="dw3"); c3(what="db"); c4(what="wgrad workspace")
        dw = MC.assemble_weight_grad(dw3.view(3, Cout, 3 * Cc), Cout, Cc)                 # [Cout, C, 3, 3]: moves values only
        return out.view(N, H, W, Cout).permute(0, 3, 1, 2).clone(), dw.clone(), db.view(Cout).clone()
    with Case("conv3x3") as c:
        (y0, w0, b0), (y1, w1, b1) = fwd(x), fwd(xp)
        y_ref, _, dw_ref, db_ref = CC.conv_reference(xp, w, b, dy)
        c.agree(y1, y_ref, dtype, what="conv3x3_fwd")
        c.same(y0, y1, foot, what="conv3x3_fwd")
        c.agree(w1, dw_ref, F32, what="conv3x3_wgrad")
        c.agree(b1, db_ref, F32, what="conv3x3_wgrad db")
        c.same(w0, w1, mask((Cout, Cc, 3, 3), (slice(None), 7), (slice(None), 200)), what="conv3x3_wgrad")
        c.same(b0, b1, mask((Cout,)), what="conv3x3_wgrad db")
        assert bool(dw_ref[:, 200].isinf().all()) and bool(dw_ref[:, 7, 2, 2].isfinite().all()), "the case's own footprint"

    (N, H, W), Cc, Cout, dtype = (2, 3, 5), 256, 256, BF16
    M = N * H * W
    g = torch.Generator().manual_seed(23)
    w = (torch.randn(Cout, Cc, 3, 3, generator=g) * 0.05).to(dtype)
    dy = torch.randn(N, Cout, H, W, generator=g).to(dtype)
    w_flip = MC.weight_operands(w.cuda(), dtype)[1]
    dyp = plant(dy, ((0, 9, 2, 4), NAN), ((1, 255, 1, 1), -INF))                # image 0's last (corner) pixel, image 1's interior

    def dgrad(dy_):
        out, check = kc.guarded(M, Cc, dtype)
        ops.conv3x3_dgrad(ops.pad_border(_cl(dy_)), w_flip, out=out)
        sync(); check(what="conv3x3_dgrad")
        return out.view(N, H, W, Cc).permute(0, 3, 1, 2).clone()
    with Case("conv3x3") as c:
        d0, d1 = dgrad(dy), dgrad(dyp)
        _, dx_ref, _, _ = CC.conv_reference(torch.zeros(N, Cc, H, W), w, None, dyp)
        c.agree(d1, dx_ref, dtype, what="conv3x3_dgrad")
        c.same(d0, d1, mask((N, 1, H, W), (0, 0, slice(1, 3), slice(3, 5)), (1, 0, slice(0, 3), slice(0, 3))), what="conv3x3_dgrad")


# ======================================================================================================== composed paths
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_backbone_forward_keeps_a_nan_pixel_in_its_image(ops, dtype):
    """BackboneEngine.forward on the configuration of tests/test_engine.py::test_backbone_fwd_bwd_matches_oracle at B = 3: one
    NaN pixel in image 1.  Every token of image 1 is NaN and the balance loss is NaN - as the oracle's are - while the tokens
    of images 0 and 2 have the bits of the clean run, although the NaN tokens move the expert groups (a row's result does not
    depend on its slot: tests/test_full_size.py::test_full_size_fp16_rows_do_not_depend_on_batch_position).  A clean step
    behind the poisoned one gives the first clean run's bits again: nothing non-finite stays in the engine's buffers."""
    from m3vit_amd.engine import BackboneEngine
    from oracle import ref_torch as R
    cfg = R.BackboneCfg(img_size=(32, 48), embed_dim=64, depth=4, num_heads=2, mlp_ratio=4.0, moe_mlp_ratio=1.0,
                        moe_experts=4, moe_top_k=2, gate_dim=66, multi_gate=True)
    B = 3
    P = R.init_backbone_params(cfg, seed=5)
    torch.manual_seed(0)
    img = torch.randn(B, 3, *cfg.img_size)
    imgp = plant(img, ((1, 2, 17, 30), NAN))
    eng = BackboneEngine(cfg, P, batch=B, dtype=dtype)

    def fwd(i_):
        tok, cv = eng.forward(i_.cuda(), 0)
        sync()
        return tok.detach().clone(), cv.detach().clone()
    (t0, cv0), (t1, cv1), (t2, cv2) = fwd(img), fwd(imgp), fwd(img)
    with torch.no_grad():
        tr, cvr, _ = R.backbone_forward({k: v.double() for k, v in P.items()}, cfg, imgp.double(), 0)
    assert bool(tr[1].isnan().all()) and bool(cvr.isnan()) and bool(tr[[0, 2]].isfinite().all())
    with Case("backbone") as c:
        c.agree(t1, tr, F32, what="tokens")
        c.same(t0, t1, mask((B, 1, 1), (1,)), what="tokens")
        assert math.isfinite(float(cv0)) and math.isnan(float(cv1)), f"balance loss: clean {float(cv0)}, poisoned {float(cv1)}"
    assert kc.same_bits(t2, t0) and kc.same_bits(cv2.view(1), cv0.view(1)), "a clean step behind the poisoned one differs from the first"


def test_head_fused_path_keeps_a_nan_token(ops):
    """VisionTransformerUpHead in eval mode on the fused ReLU + x2 path (the construction of tests/test_modules_gpu.py::
    test_head_fused_resize_matches_torch_stages), one input token of image 1 NaN: image 0's and image 2's logits have the clean
    run's bits, and image 1's non-finite mask is the one of the same head on torch's relu + interpolate stages.  The token is
    patch (1, 1): its footprint behind the first 3 x 3 convolution holds row 0 and column 0, so torch's zero-weight tap at
    output 0 (up2x_expected) sees nothing the fused kernel does not.  A ReLU that turns NaN into 0 ends the NaN at the first
    stage: the fused head would then return finite logits where the reference has NaN."""
    from m3vit_amd.heads import ReluUp2xFn, VisionTransformerUpHead
    torch.manual_seed(4)
    a = VisionTransformerUpHead(img_size=(64, 96), embed_dim=64, num_classes=40, amp=True, fused_resize=True).cuda().eval()
    b = VisionTransformerUpHead(img_size=(64, 96), embed_dim=64, num_classes=40, amp=True, fused_resize=False).cuda().eval()
    b.load_state_dict(a.state_dict())
    tok = torch.randn(3, 4 * 6 + 1, 64, device="cuda")
    tokp = plant(tok, ((1, 1 + 1 * 6 + 1, 5), NAN))
    calls = []
    orig = ReluUp2xFn.forward
    ReluUp2xFn.forward = staticmethod(lambda ctx, x, relu, out_fp32: (calls.append((relu, out_fp32)), orig(ctx, x, relu, out_fp32))[1])
    # MIOpen's default solvers for the head's 256-channel convolutions are not repeatable from one run to the next (measured: two
    # clean runs of this head differ in the last bits); its deterministic ones are, and only then can bits be compared
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.no_grad():
            y0, y0b, y1 = a(tok), a(tok), a(tokp)
            yb = b(tokp)
        sync()
    finally:
        ReluUp2xFn.forward = orig
        torch.backends.cudnn.deterministic = det
    assert calls == ([(True, False)] * 3 + [(False, True)]) * 3, f"not the fused path: {calls}"
    assert kc.same_bits(y0, y0b), "two clean runs of the head differ: the comparison with the poisoned run would say nothing"
    assert y1.shape == yb.shape == (3, 40, 64, 96)
    ref_mask = ~torch.isfinite(yb)
    assert bool(ref_mask[1].any()) and not bool(ref_mask[[0, 2]].any()), "the torch-stage head: NaN in image 1 and only there"
    with Case("head") as c:
        c.same(y0, y1, mask((3, 1, 1, 1), (1,)), what="logits")
        got_mask = ~torch.isfinite(y1)
        c.nf += int(ref_mask.sum())
        if not torch.equal(got_mask, ref_mask):
            j = int((got_mask != ref_mask).flatten().nonzero()[0])
            at = tuple(int(v) for v in torch.unravel_index(torch.tensor(j), y1.shape))
            raise AssertionError(f"logits: {int((got_mask != ref_mask).sum())} element(s) are non-finite in one head only; first at {at}: "
                                 f"fused {float(y1.flatten()[j])!r}, torch stages {float(yb.flatten()[j])!r}")
