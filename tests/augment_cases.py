"""Cases, float64 restatement and error bounds of m3_augment_batch / m3vit_amd.augment.BatchAugment, shared by
test_augment_cpu.py and test_augment_gpu.py (imported, not collected).

cv2 is not installed where this project is built, so nothing here is a cv2 output: the transform is restated from its published
formulas in float64 - the matrices of m3vit_amd.augment.affine_params, the tap rules and post-operations of
include/m3vit_hip.h - and test_augment_cpu.py checks that restatement against torch's own grid_sample.

Coordinates.  u = (a00 x + a01 y) + a02 as four separately rounded float64 operations, in torch on the CPU exactly as in the
kernel: the same bits.  Nearest taps, the t == 0 rule and the uint8 truncation are therefore decided on identical numbers, and
maps sampled `nearest` are compared EXACTLY.  t = float32(u - floor(u)) is the kernel's fraction; the restatement evaluates the
weights in float64 from that same t, in the textbook Keys form (the kernel uses a factored one).

Bound on a resampled value (before the post-operation), from the kernel's operation counts, u32 = 2^-24:
  * weights.  linear: 1 - t is one rounding, e1 = u32.  cubic, a = -0.75, t in (0, 1), s = 1 - t (one rounding, u32):
      w0 = a t s^2, w3 = a s t^2         three products of magnitudes <= 0.75 * 4/27:          <= 1 u32
      w1 = 1 - t^2 (2.25 - 1.25 t)       2.25 - 1.25 t: u32 * 2.25;  t^2: u32;  their product (<= 2.25): u32 * 2.25;
                                         the final difference: u32;  in all <= 5.5 u32
      w2 the same in s, plus s's own rounding through |dW/ds| = |(3.75 s - 4.5) s| <= 1.35:    <= 6.85 u32
    so every 1-D weight is within e1 = 7 u32 (cubic).  An axis with t == 0 has exact weights: e1 = 0 there.
  * the 2-D weight w = wx wy: |dw| <= e1x |wy| + e1y |wx| + e1x e1y + u32 |w|.
  * the sum acc = fma(w, tap, acc) over K taps of non-zero weight: (K + 1) u32 sum |w| |tap| including the product above.
  |val - ref| <= e1x sum |wy| |tap| + e1y sum |wx| |tap| + e1x e1y sum |tap| + (K + 1) u32 sum |w| |tap|
  and 0 where both axes have t == 0 or the mode is nearest (one tap of weight 1: a copy).
Post-operations add their own roundings (postop()).  Everything is multiplied by kernel_contract.SAFETY once.

The one exclusion (image, quantize): an element whose float64 value before the truncation lies within delta of an integer
1 .. 255 may truncate either way and is compared with the extra tolerance 1 / (255 std_c); delta is the element's own bound
above.  Elements with exact weights have delta = 0 and are never excluded.  At most EXCLUDE_CAP of a case's image elements may
be excluded - asserted for the restatement alone (CPU) and again where the kernel is checked (GPU).
"""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_contract import SAFETY, U32, assert_within, store   # noqa: E402

F64 = torch.float64
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
EPS32 = 2.0 ** -23
EXCLUDE_CAP = 0.02
E1 = {"nearest": 0.0, "linear": U32, "cubic": 7.0 * U32}
NTAPS = {"nearest": 1, "linear": 2, "cubic": 4}
SIZE = (24, 40)

FIVE = {"image": ("image", "cubic"), "semseg": ("label", "nearest"), "depth": ("depth", "nearest"),
        "normals": ("normals", "cubic"), "edge": ("label", "nearest")}
PASCAL = {"image": ("image", "cubic"), "semseg": ("label", "nearest"), "human_parts": ("label", "nearest"),
          "sal": ("label", "nearest"), "normals": ("normals", "cubic"), "edge": ("label", "nearest"),
          "depth": ("depth", "nearest")}
TESTFORM = {"image": ("image", "cubic"), "semseg": ("label", "nearest"), "edge": ("label", "linear"),
            "depth": ("depth", "linear"), "normals": ("normals", "linear")}
EIGHT = dict(PASCAL, sal2=("label", "linear"))


class Case:
    def __init__(self, name, maps, rot, sc, flip, size=SIZE, out=None, border="zero", image_dtype=torch.float32,
                 image_src=torch.uint8, quantize=True, seed=0):
        self.name, self.maps, self.rot, self.sc, self.flip = name, maps, list(rot), list(sc), list(flip)
        self.size, self.out, self.border = size, out or size, border
        self.image_dtype, self.image_src, self.quantize, self.seed = image_dtype, image_src, quantize, seed
        self.B = len(self.rot)

    def __repr__(self):
        return self.name


_NYUD = ([0, 0, 0], [1.0, 1.2, 1.5], [True, False, True])
_PASCAL = ([13.0, -20.0, 7.5], [0.9, 1.25, 0.75], [True, False, False])
_ID = ([0, 0], [1.0, 1.0], [False, False])
CASES = {c.name: c for c in [
    Case("identity_flip", FIVE, [0, 0], [1.0, 1.0], [False, True], seed=1),
    # 25 x 41: with an even size the scales 1.2 and 1.5 put every 6th / 3rd output column within 1e-15 of a source column
    # WITHOUT hitting it (5/6 and 2/3 are no doubles), and each such pixel of an integer image lies that close to an integer:
    # 4.5 % of the elements would be excluded.  Half-integer centres have no such columns; "dyadic" below has exact ones.
    Case("nyud", FIVE, *_NYUD, size=(25, 41), seed=2),
    Case("dyadic", FIVE, [0, 0], [2.0, 0.5], [False, True], seed=18),
    Case("pascal", PASCAL, *_PASCAL, seed=3),
    Case("train_down", FIVE, [13.0, 0], [0.9, 1.2], [True, False], out=(16, 24), seed=4),
    Case("train_up", FIVE, [13.0, 0], [0.9, 1.2], [True, False], out=(48, 80), seed=5),
    Case("test_down", TESTFORM, *_ID, out=(16, 24), border="replicate", seed=6),
    Case("test_up", TESTFORM, *_ID, out=(48, 80), border="replicate", seed=7),
    Case("src_1x1", FIVE, [13.0, 0], [0.9, 1.0], [True, False], size=(1, 1), out=(5, 7), seed=8),
    Case("src_1x40", FIVE, [13.0, 0], [0.9, 1.0], [True, False], size=(1, 40), out=(2, 40), seed=9),
    Case("src_1x40_replicate", TESTFORM, *_ID, size=(1, 40), out=(2, 20), border="replicate", seed=10),
    Case("wo_37", FIVE, [7.5, 0], [0.75, 1.0], [False, True], out=(24, 37), seed=11),
    Case("wo_37_f16", FIVE, [7.5, 0], [0.75, 1.0], [False, True], out=(24, 37), image_dtype=torch.float16, seed=11),
    Case("b_1", FIVE, [-20.0], [1.25], [True], seed=12),
    Case("one_map", {"depth": ("depth", "nearest")}, [13.0, 0], [0.9, 1.5], [False, True], seed=13),
    Case("eight_maps", EIGHT, *_PASCAL, seed=14),
    Case("two_blocks", FIVE, [13.0], [0.9], [True], size=(24, 40), out=(40, 150), seed=15),
    Case("image_f32_in", FIVE, [13.0, 0], [0.9, 1.2], [True, False], image_src=torch.float32, seed=16),
    Case("image_raw", FIVE, [13.0, 0], [0.9, 1.2], [True, False], image_src=torch.float32, quantize=False, seed=16),
    Case("image_f16", FIVE, [13.0, 0], [0.9, 1.2], [True, False], image_dtype=torch.float16, seed=17),
    Case("image_bf16", FIVE, [13.0, 0], [0.9, 1.2], [True, False], image_dtype=torch.bfloat16, seed=17),
]}


def channels(kind):
    return 3 if kind in ("image", "normals") else 1


@functools.lru_cache(maxsize=None)
def make_batch(name):
    """the raw batch of a case as CPU tensors [B, H, W, C] / [B, H, W]: random uint8 image (fp32 copies of the same integers
    plus a fraction where image_src is float32), fp32 labels with zeros and 255s planted.  Callers must not modify it."""
    c = CASES[name]
    g = torch.Generator().manual_seed(1000 + c.seed)
    B, (H, W) = c.B, c.size
    out = {}
    for m, (kind, _) in c.maps.items():
        plant = torch.rand(B, H, W, generator=g)
        if kind == "image":
            t = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
            if c.image_src == torch.float32:
                t = t.float() + (0.0 if c.quantize else 1.0) * torch.rand(B, H, W, 3, generator=g)
        elif kind == "normals":
            t = torch.randn(B, H, W, 3, generator=g)
            t = t / t.norm(dim=-1, keepdim=True)
            t[plant < 0.08] = 0.0                                  # no annotation: norm 0
        elif kind == "depth":
            t = torch.rand(B, H, W, generator=g) * 9.0 + 0.5
            t[plant < 0.08] = 0.0                                  # invalid depth
            t[plant > 0.95] = 255.0
        else:
            t = torch.randint(0, 40, (B, H, W), generator=g).float()     # classes, 0 among them
            t[plant > 0.92] = 255.0
        out[m] = t.contiguous()
    return out


def params(c):
    """(A float64 [B, 6], aux float32 [B, 4]) of a case, as numpy arrays"""
    from m3vit_amd.augment import affine_params
    return affine_params(c.rot, c.sc, c.flip, c.size, c.out)


# ------------------------------------------------------------------------------------------------------- restatement
def coords(A_row, Ho, Wo):
    """u, v float64 [Ho, Wo]: two rounded products, their rounded sum, the rounded sum with the offset"""
    a = [float(v) for v in A_row]
    x = torch.arange(Wo, dtype=F64).view(1, Wo).expand(Ho, Wo).contiguous()
    y = torch.arange(Ho, dtype=F64).view(Ho, 1).expand(Ho, Wo).contiguous()
    u = torch.add(torch.add(torch.mul(x, a[0]), torch.mul(y, a[1])), a[2])
    v = torch.add(torch.add(torch.mul(x, a[3]), torch.mul(y, a[4])), a[5])
    return u, v


def keys(x, a=-0.75):
    """the Keys cubic convolution kernel (float64)"""
    x = x.abs()
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    far = ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a
    return torch.where(x <= 1.0, near, torch.where(x < 2.0, far, torch.zeros_like(x)))


def axis(u, mode, t32=True):
    """(first tap index int64 [..], weights float64 [n, ..], t float64 [..]) of one axis; t32=False keeps the fraction in
    float64 (the closed form itself, for the comparison with a float64 grid_sample)"""
    if mode == "nearest":
        return torch.floor(u + 0.5).long(), torch.ones((1,) + u.shape, dtype=F64), torch.zeros_like(u)
    f = torch.floor(u)
    t = (u - f).float().double() if t32 else u - f                # the kernel's fp32 fraction
    if mode == "linear":
        return f.long(), torch.stack([1.0 - t, t]), t
    return f.long() - 1, torch.stack([keys(t + 1.0), keys(t), keys(1.0 - t), keys(2.0 - t)]), t


def sample(src, u, v, mode, border, t32=True):
    """src float64 [H, W, C] at (u, v) [Ho, Wo] -> (val [Ho, Wo, C], bound [Ho, Wo, C] without SAFETY)"""
    H, W, C = src.shape
    ix, wx, tx = axis(u, mode, t32)
    iy, wy, ty = axis(v, mode, t32)
    n = NTAPS[mode]
    val = torch.zeros(u.shape + (C,), dtype=F64)
    s_w, s_x, s_y, s_1 = (torch.zeros_like(val) for _ in range(4))
    for j in range(n):
        for i in range(n):
            xx, yy = ix + i, iy + j
            if border == "zero":
                inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            else:
                inside = torch.ones_like(xx, dtype=torch.bool)
            tap = src[yy.clamp(0, H - 1), xx.clamp(0, W - 1)] * inside.unsqueeze(-1)
            w = (wx[i] * wy[j]).unsqueeze(-1)
            val = val + torch.where(w != 0, w * tap, torch.zeros_like(tap))      # a zero weight contributes nothing
            a = tap.abs()
            s_w, s_1 = s_w + w.abs() * a, s_1 + a
            s_x, s_y = s_x + wy[j].abs().unsqueeze(-1) * a, s_y + wx[i].abs().unsqueeze(-1) * a
    e1x = torch.where(tx == 0, 0.0, E1[mode]).unsqueeze(-1)
    e1y = torch.where(ty == 0, 0.0, E1[mode]).unsqueeze(-1)
    K = ((wx != 0).sum(0) * (wy != 0).sum(0)).unsqueeze(-1).double()
    bound = e1x * s_x + e1y * s_y + e1x * e1y * s_1 + (K + 1.0) * U32 * s_w
    exact = ((tx == 0) & (ty == 0)).unsqueeze(-1)
    return val, torch.where(exact, torch.zeros_like(bound), bound)


def postop(kind, val, b, aux_row, mode, out_dtype, quantize=True):
    """the post-operation of a map kind on val [Ho, Wo, C] with bound b (no SAFETY yet) ->
    (ref [C, Ho, Wo] float64, bound [C, Ho, Wo] with SAFETY and the store, excluded bool [C, Ho, Wo] or None)"""
    sc, cs, sn, flip = (float(x) for x in aux_row)
    excluded = None
    if kind == "image":
        mean = torch.tensor([float(np.float32(m)) for m in MEAN], dtype=F64)
        std = torch.tensor([float(np.float32(s)) for s in STD], dtype=F64)
        q = val
        if quantize:
            q = torch.trunc(val.clamp(0.0, 255.0))
            k = torch.round(val)
            excluded = ((val - k).abs() <= SAFETY * b) & (k >= 1) & (k <= 255) & (b > 0)
            b = torch.zeros_like(b)                               # a truncated value carries no error, or it is excluded
        z = q / 255.0
        ref = (z - mean) / std
        bound = (b / 255.0 + U32 * z.abs() + U32 * (z - mean).abs()) / std + U32 * ref.abs()
        if excluded is not None:
            bound = bound + excluded * (1.0 / (255.0 * std)) / SAFETY
    elif kind == "label":
        ref, bound = val, b
    elif kind == "depth":
        if mode == "nearest":                                     # one correctly rounded fp32 division of a copied value
            ref = (val.float() / torch.tensor(sc, dtype=torch.float32)).double()
            bound = torch.zeros_like(b)
        else:
            ref = val / sc
            bound = b / sc + U32 * ref.abs()
        ref = torch.where(ref == 0, torch.full_like(ref, 255.0), ref)
    else:
        n0 = -val[..., 0] if flip else val[..., 0]
        n1, n2 = val[..., 1], val[..., 2]
        r0, r1 = n0 * cs + n1 * sn, n1 * cs - n0 * sn
        e0 = b[..., 0] * abs(cs) + b[..., 1] * abs(sn) + 2 * U32 * ((n0 * cs).abs() + (n1 * sn).abs())
        e1 = b[..., 1] * abs(cs) + b[..., 0] * abs(sn) + 2 * U32 * ((n1 * cs).abs() + (n0 * sn).abs())
        e2 = b[..., 2]
        nn = torch.sqrt(r0 * r0 + r1 * r1 + n2 * n2)
        safe = nn.clamp_min(1e-300)
        e_nn = (r0.abs() * e0 + r1.abs() * e1 + n2.abs() * e2) / safe + 3 * U32 * nn      # two squares' sums and the root
        den = nn + EPS32
        e_den = e_nn + U32 * den
        r = torch.stack([r0, r1, n2], -1)
        e = torch.stack([e0, e1, e2], -1)
        ref = r / den.unsqueeze(-1)
        bound = e / den.unsqueeze(-1) + r.abs() * (e_den / (den * den)).unsqueeze(-1) + U32 * ref.abs()
        dead = (nn == 0).unsqueeze(-1)
        ref = torch.where(dead, torch.full_like(ref, 255.0), ref)
        bound = torch.where(dead, torch.zeros_like(bound), bound)
    ref, bound = ref.permute(2, 0, 1).contiguous(), bound.permute(2, 0, 1).contiguous()
    bound = SAFETY * bound
    bound = torch.where(bound > 0, bound + SAFETY * store(out_dtype, ref), bound)     # an exact value is stored exactly
    return ref, bound, None if excluded is None else excluded.permute(2, 0, 1).contiguous()


@functools.lru_cache(maxsize=None)
def reference(name):
    """{map: (ref [B, C, Ho, Wo] float64, bound, excluded or None)} of a case: computed once, shared, never modified"""
    c = CASES[name]
    batch = make_batch(name)
    A, aux = params(c)
    Ho, Wo = c.out
    out = {}
    for m, (kind, mode) in c.maps.items():
        refs, bounds, excl = [], [], []
        for b in range(c.B):
            u, v = coords(A[b], Ho, Wo)
            src = batch[m][b].double()
            src = src if src.dim() == 3 else src.unsqueeze(-1)
            val, bv = sample(src, u, v, mode, c.border)
            r, bd, ex = postop(kind, val, bv, aux[b], mode, c.image_dtype if kind == "image" else torch.float32,
                               c.quantize)
            refs.append(r), bounds.append(bd), excl.append(ex)
        out[m] = (torch.stack(refs), torch.stack(bounds), None if excl[0] is None else torch.stack(excl))
    return out


def excluded_share(name):
    """the share of a case's image elements that the quantisation rule excludes (0.0 without a quantised image)"""
    shares = [float(ex.double().mean()) for _, _, ex in reference(name).values() if ex is not None]
    return max(shares) if shares else 0.0


def check(name, outs, what=""):
    """outs {map: tensor [B, C, Ho, Wo]} against the case's reference: a map whose bound is zero everywhere (nearest
    sampling) bit for bit up to the sign of zero, the others within their bounds; the exclusion cap.  Returns the worst
    err / bound ratio."""
    c = CASES[name]
    worst = 0.0
    assert excluded_share(name) <= EXCLUDE_CAP, f"{name}: {excluded_share(name):.4f} of the image elements are excluded"
    for m, (ref, bound, _) in reference(name).items():
        o = outs[m]
        want = c.image_dtype if c.maps[m][0] == "image" else torch.float32
        assert o.dtype == want and tuple(o.shape) == tuple(ref.shape), (name, m, o.dtype, tuple(o.shape))
        if not bool((bound > 0).any()):
            assert torch.equal(o.detach().cpu().double(), ref), f"{what}{name}/{m}: not equal to the restatement"
        else:
            worst = max(worst, assert_within(o, ref, bound, f"{what}{name}/{m}"))
    return worst
