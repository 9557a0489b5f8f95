"""CPU: the float64 restatement of the device augmentation (tests/augment_cases.py) against independent evaluations - torch's
grid_sample in float64 and in float32, explicit indexing - and the host half of m3vit_amd.augment (matrices, draws,
configurations).  No GPU is needed; the kernel itself is checked in test_augment_gpu.py against the same restatement."""
import math
import os
import random
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_cases as AC                                        # noqa: E402
from kernel_contract import assert_within                         # noqa: E402

F64 = torch.float64


def _grid(u, v, H, W, dtype):
    """grid_sample's normalised coordinates (align_corners=True) of source coordinates (u, v)"""
    return torch.stack([2.0 * u / (W - 1) - 1.0, 2.0 * v / (H - 1) - 1.0], -1).unsqueeze(0).to(dtype)


@pytest.mark.parametrize("mode, torch_mode", [("linear", "bilinear"), ("cubic", "bicubic")])
def test_restatement_equals_grid_sample_float64(mode, torch_mode):
    """linear and cubic sampling with a zero border on the coordinates of the PASCAL draws, against torch's CPU grid_sample
    in float64 (the same Keys kernel, a = -0.75; zeros padding).  Held to 1e-9 absolute on values up to 255: the round trip
    u -> 2 u / (W - 1) - 1 -> u moves a coordinate by at most 4 * 2^-53 * (|u| + W) < 5e-14, the interpolant's slope is at
    most 3 * 255 per axis, so the values differ by less than 1e-10; float64 summation adds 1e-12."""
    c = AC.CASES["pascal"]
    A, _ = AC.params(c)
    img = AC.make_batch("pascal")["image"].double()
    H, W = c.size
    for b in range(c.B):
        u, v = AC.coords(A[b], *c.out)
        val, _ = AC.sample(img[b], u, v, mode, "zero", t32=False)  # the fraction as float64, as torch keeps it
        got = F.grid_sample(img[b].permute(2, 0, 1).unsqueeze(0), _grid(u, v, H, W, F64), mode=torch_mode,
                            padding_mode="zeros", align_corners=True)[0].permute(1, 2, 0)
        assert float((val - got).abs().max()) <= 1e-9, (mode, b)
        assert float(val.abs().max()) > 100.0                     # the check saw the image, not a border


def test_nearest_equals_explicit_indexing():
    c = AC.CASES["pascal"]
    A, _ = AC.params(c)
    lab = AC.make_batch("pascal")["semseg"]
    H, W = c.size
    Ho, Wo = c.out
    for b in range(c.B):
        u, v = AC.coords(A[b], Ho, Wo)
        val, bound = AC.sample(lab[b].double().unsqueeze(-1), u, v, "nearest", "zero")
        assert float(bound.max()) == 0.0
        a = [float(x) for x in A[b]]
        for y in range(Ho):
            for x in range(Wo):
                xs = math.floor((a[0] * x + a[1] * y) + a[2] + 0.5)
                ys = math.floor((a[3] * x + a[4] * y) + a[5] + 0.5)
                want = float(lab[b, ys, xs]) if 0 <= xs < W and 0 <= ys < H else 0.0
                assert float(val[y, x, 0]) == want, (b, y, x)


def _post32(kind, val, aux_row, quantize=True):
    """the post-operations in float32 torch arithmetic, written from include/m3vit_hip.h: val [Ho, Wo, C] -> [C, Ho, Wo]"""
    sc, cs, sn, flip = (torch.tensor(float(x), dtype=torch.float32) for x in aux_row)
    if kind == "image":
        q = torch.trunc(val.clamp(0.0, 255.0)) if quantize else val
        out = (q / 255.0 - torch.tensor(AC.MEAN, dtype=torch.float32)) / torch.tensor(AC.STD, dtype=torch.float32)
    elif kind == "label":
        out = val
    elif kind == "depth":
        out = val / sc
        out = torch.where(out == 0, torch.full_like(out, 255.0), out)
    else:
        n0 = -val[..., 0] if bool(flip) else val[..., 0]
        r0, r1 = n0 * cs + val[..., 1] * sn, val[..., 1] * cs - n0 * sn
        nn = torch.sqrt(r0 * r0 + r1 * r1 + val[..., 2] * val[..., 2])
        out = torch.stack([r0, r1, val[..., 2]], -1) / (nn + torch.tensor(AC.EPS32, dtype=torch.float32)).unsqueeze(-1)
        out = torch.where((nn == 0).unsqueeze(-1), torch.full_like(out, 255.0), out)
    return out.permute(2, 0, 1)


@pytest.mark.parametrize("mode, torch_mode", [("linear", "bilinear"), ("cubic", "bicubic")])
def test_bounds_hold_torch_float32_grid_sample(mode, torch_mode):
    """The bounds of augment_cases are derived from the kernel's operation counts; here ANOTHER float32 implementation -
    torch's CPU grid_sample plus the post-operations in float32 torch arithmetic - is held to them, so they are not fitted to
    the kernel.  grid_sample in float32 also forms its coordinates in float32, which the kernel does not (its coordinates are
    doubles); that is kept out by a source of 17 x 33 (W - 1 and H - 1 powers of two) and quarter-pixel dyadic matrices, for
    which the normalised and the recovered coordinates are exact in float32 (so are the weights: what is checked is the
    weighted fp32 sum and the post-operation).  Zero border, a flip, taps outside the source.  The exclusion cap is not
    asserted here: dyadic weights on an integer image give multiples of 1/16 and 1/4096, so integers are hit by construction."""
    H, W, Ho, Wo = 17, 33, 20, 40
    g = torch.Generator().manual_seed(5)
    mats = [[0.5, 0.0, 0.25, 0.0, 0.5, -1.25], [-0.5, 0.0, 20.25, 0.0, 1.0, 0.75], [1.0, 0.0, -1.5, 0.0, 0.25, 0.5]]
    aux = [[1.25, math.cos(0.3), math.sin(0.3), 0.0], [0.75, 1.0, 0.0, 1.0], [1.0, math.cos(-0.2), math.sin(-0.2), 0.0]]
    srcs = {"image": torch.randint(0, 256, (H, W, 3), generator=g).double(),
            "label": torch.randint(0, 40, (H, W, 1), generator=g).double(),
            "depth": (torch.rand(H, W, 1, generator=g) * 9 + 0.5).float().double(),
            "normals": torch.randn(H, W, 3, generator=g).float().double()}
    srcs["depth"][2:5, 3:9] = 0.0
    srcs["normals"][6:9, 10:20] = 0.0
    for A_row, aux_row in zip(mats, aux):
        aux_row = np.asarray(aux_row, dtype=np.float32)
        u, v = AC.coords(A_row, Ho, Wo)
        grid = _grid(u, v, H, W, torch.float32)
        assert torch.equal(grid.double(), _grid(u, v, H, W, F64))            # exact in float32
        for kind, src in srcs.items():
            val, bv = AC.sample(src, u, v, mode, "zero")
            ref, bound, ex = AC.postop(kind, val, bv, aux_row, mode, torch.float32)
            got = F.grid_sample(src.float().permute(2, 0, 1).unsqueeze(0), grid, mode=torch_mode, padding_mode="zeros",
                                align_corners=True)[0].permute(1, 2, 0)
            assert_within(_post32(kind, got, aux_row), ref, bound, f"{mode} {kind}")


@pytest.mark.parametrize("name", list(AC.CASES))
def test_exclusion_cap_holds_for_the_restatement_alone(name):
    """every case of the GPU file: at most 2 % of the image elements lie within their own bound of an integer"""
    share = AC.excluded_share(name)
    print(f"{name}: excluded share {share:.4f}")
    assert share <= AC.EXCLUDE_CAP
    for m, (ref, bound, _) in AC.reference(name).items():
        assert bool(torch.isfinite(ref).all()) and bool((bound >= 0).all()), (name, m)
        if AC.CASES[name].maps[m][1] == "nearest":
            assert float(bound.max()) == 0.0, (name, m)          # compared exactly, no exclusions


def test_params_identity_flip_and_inverse():
    from m3vit_amd.augment import affine_params, rotation_matrix, rotation_matrix_inv
    H, W = 24, 40
    A, aux = affine_params([0, 0], [1.0, 1.0], [False, True], (H, W), (H, W))
    assert A[0].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]                    # exactly the identity
    assert A[1].tolist() == [-1.0, 0.0, W - 1.0, 0.0, 1.0, 0.0]               # exactly the mirror
    assert aux.dtype == np.float32 and aux.tolist() == [[1.0, 1.0, 0.0, 0.0], [1.0, 1.0, 0.0, 1.0]]
    assert A.dtype == np.float64
    rng = np.random.RandomState(3)
    for _ in range(200):
        rot, sc = rng.uniform(-20, 20), rng.uniform(0.75, 1.25)
        P = rotation_matrix((H, W), rot, sc) @ rotation_matrix_inv((H, W), rot, sc)
        assert np.abs(P - np.eye(3)).max() <= 1e-12, (rot, sc)
    # the resize alone: half-pixel centres, and an upscale by two reads between the source pixels
    A, _ = affine_params([0], [1.0], [False], (H, W), (2 * H, 2 * W))
    assert A[0].tolist() == [0.5, 0.0, -0.25, 0.0, 0.5, -0.25]
    # a quarter turn about the centre maps the centre to itself
    A, aux = affine_params([90.0], [1.0], [False], (H, W), (H, W))
    assert abs(A[0, 0] * 20 + A[0, 1] * 12 + A[0, 2] - 20) < 1e-12 and abs(A[0, 3] * 20 + A[0, 4] * 12 + A[0, 5] - 12) < 1e-12
    assert abs(aux[0, 1]) < 1e-7 and aux[0, 2] == 1.0


def test_draws_land_in_the_configured_sets_and_ranges():
    from m3vit_amd.augment import BatchAugment
    random.seed(11)
    np.random.seed(11)
    nyud = BatchAugment.from_config("NYUD", ["semseg", "depth"])
    rot, sc, flip = nyud.draw_values(4096)
    assert set(rot.tolist()) == {0.0} and set(sc.tolist()) == {1.0, 1.2, 1.5}
    counts = [int((sc == s).sum()) for s in (1.0, 1.2, 1.5)]
    sigma = math.sqrt(4096 * (1 / 3) * (2 / 3))
    assert all(abs(k - 4096 / 3) <= 5 * sigma for k in counts), counts     # a uniform choice, the last entry included
    assert abs(int(flip.sum()) - 2048) <= 5 * math.sqrt(4096 * 0.25)       # binomial, 5 sigma
    pas = BatchAugment.from_config("PASCALContext", ["semseg", "human_parts", "sal", "normals", "edge"])
    rot, sc, flip = pas.draw_values(4096)
    assert -20 <= rot.min() < -19 and 19 < rot.max() <= 20 and 0.75 <= sc.min() < 0.76 and 1.24 < sc.max() <= 1.25
    assert abs(int(flip.sum()) - 2048) <= 5 * math.sqrt(4096 * 0.25)
    p = 0.2
    some = BatchAugment({"image": ("image", "cubic")}, out_size=(8, 8), flip_prob=p)
    flip = some.draw_values(4096)[2]
    assert abs(int(flip.sum()) - 4096 * p) <= 5 * math.sqrt(4096 * p * (1 - p))
    random.seed(11)
    np.random.seed(11)
    again = nyud.draw_values(4096)
    random.seed(11)
    np.random.seed(11)
    once_more = nyud.draw_values(4096)
    assert all(np.array_equal(a, b) for a, b in zip(again, once_more))     # seeded: repeatable


def test_from_config_reproduces_get_transformations():
    from m3vit_amd.augment import BatchAugment
    a = BatchAugment.from_config("NYUD", ["semseg", "depth", "normals", "edge"])
    assert a.maps == {"image": ("image", "cubic"), "semseg": ("label", "nearest"), "depth": ("depth", "nearest"),
                      "normals": ("normals", "cubic"), "edge": ("label", "nearest")}
    assert (a.out_size, a.rots, a.scales, a.flip_prob, a.border) == ((480, 640), [0], [1.0, 1.2, 1.5], 0.5, "zero")
    assert a.mean == (0.485, 0.456, 0.406) and a.std == (0.229, 0.224, 0.225) and a.quantize
    c = BatchAugment.from_config("CityScapes", ["semseg", "depth"])
    assert (c.out_size, c.rots, c.scales) == ((128, 256), [0], [1.0, 1.2, 1.5])
    p = BatchAugment.from_config("PASCALContext", ["semseg", "human_parts", "sal", "normals", "edge"])
    assert (p.out_size, p.rots, p.scales) == ((512, 512), (-20, 20), (.75, 1.25))
    assert p.maps["human_parts"] == ("label", "nearest") and p.maps["sal"] == ("label", "nearest")
    t = BatchAugment.from_config("NYUD", ["semseg", "depth"], train=False, out_size=(16, 24))
    assert (t.out_size, t.flip_prob, t.border) == ((16, 24), 0.0, "replicate")
    assert t.draw_values(5)[0].tolist() == [0.0] * 5 and t.draw_values(5)[1].tolist() == [1.0] * 5
    assert not t.draw_values(64)[2].any()
    with pytest.raises(ValueError):
        BatchAugment.from_config("ImageNet", [])
    with pytest.raises(ValueError):
        BatchAugment({"image": ("image", "cubic")}, rots=(0, 1), scales=[1.0])


def test_cpu_tensors_are_refused():
    from m3vit_amd import _lib
    from m3vit_amd.augment import BatchAugment
    aug = BatchAugment({"semseg": ("label", "nearest")}, out_size=(4, 4), rots=[0], scales=[1.0])
    with pytest.raises(_lib.M3Error):
        aug({"semseg": torch.zeros(1, 4, 4)})
    with pytest.raises(_lib.M3Error):
        aug({"image": torch.zeros(1, 4, 4, 3)})
