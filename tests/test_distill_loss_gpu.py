"""GPU: the distillation loss kernels (csrc/pretrain.hip: m3_loss_distill_fwd / _bwd) and pretrain.DistillationLoss against the
float64 closed forms and the derived bounds of tests/distill_cases.py.  Outputs, workspaces and records are guarded allocations;
inputs keep their bits; a second run gives the same bits."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distill_cases as DC                                         # noqa: E402
import pretrain_cases as PC                                        # noqa: E402
from kernel_contract import assert_within, guarded, guarded_ws, same_bits, snapshot, unchanged   # noqa: E402
from test_pretrain_gpu import no_host_sync                         # noqa: E402

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


def run_distill(x, t, kind, tau, upstream=1.0):
    """one forward + backward through ops with every output guarded.  Returns dict(loss, grad, lse, aux, record)."""
    from m3vit_amd import ops
    B, C = x.shape
    d2, d_check = guarded(B, C, x.dtype)
    l2, l_check = guarded(1, B, F32)
    a2, a_check = guarded(1, B, torch.int32)
    r2, r_check = guarded(1, ops.LOSS_REC_WORDS, torch.int32)
    need = ops.distill_ws_elems(B)
    assert need == B
    ws, ws_check = guarded_ws(need)
    gout = torch.tensor([upstream], dtype=F32, device="cuda")
    snap = snapshot(logits=x, teacher=t, grad_out=gout)
    record, lse, aux = ops.loss_distill_fwd(x, t, kind, tau, lse=l2.view(-1), aux=a2.view(-1), ws=ws, record=r2.view(-1))
    ops.loss_distill_bwd(x, t if kind == "soft" else None, kind, lse, aux, record, gout, tau, dlogits=d2)
    torch.cuda.synchronize()
    for chk, what in ((d_check, "dlogits"), (l_check, "lse"), (a_check, "aux"), (r_check, "record"), (ws_check, "ws")):
        chk(what=what)
    unchanged(snap)
    return dict(loss=record[:1].view(F32).clone(), grad=d2.clone(), lse=lse.clone(), aux=aux.clone(), record=record.clone())


def _on_gpu(v32, dtype, offset):
    """CPU float32 values as a [B, C] GPU tensor of dtype whose storage starts `offset` elements past an aligned address"""
    B, C = v32.shape
    store_ = torch.empty(B * C + offset, dtype=dtype, device="cuda")
    out = store_[offset:].view(B, C)
    out.copy_(v32)
    return out


def check_distill(x32, t32, kind, tau, pair, upstream=1.0, offset=0, t_offset=None):
    """x32 / t32: float32 CPU logits of the student / the teacher; pair: their dtypes on the device.  Checks value, gradient,
    both per-row states, the record, guards, input bits and run-to-run bits."""
    B, C = x32.shape
    x, t = _on_gpu(x32, pair[0], offset), _on_gpu(t32, pair[1], offset if t_offset is None else t_offset)
    r = DC.distill_ref(x.double().cpu(), t.double().cpu(), kind, tau)
    loss_b, grad_b, lse_b = DC.distill_bounds(r, pair[0], upstream=upstream)
    out = run_distill(x, t, kind, tau, upstream)
    print(f"{kind} tau {tau} {DC.pair_id(pair)} {(B, C)}: loss {float(out['loss']):.9g} ref {float(r['loss']):.9g} "
          f"bound {float(loss_b):.3e}")
    assert_within(out["loss"], r["loss"].reshape(1), loss_b, "loss")
    assert_within(out["lse"], r["lse"], lse_b, "student lse")
    if kind == "soft":
        assert_within(out["aux"].view(F32), r["lse_t"], DC.SAFETY * DC.scaled_lse_bound(r["ts"], r["lse_t"]), "teacher lse")
    else:
        assert torch.equal(out["aux"].cpu().long(), r["y"]), "the teacher's argmax"
    assert_within(out["grad"], r["grad"] * upstream, grad_b, "gradient")
    rec = out["record"].cpu()
    coef = float(rec[1:2].view(F32))
    assert abs(coef - r["coef"]) <= 2.0 ** -23 * r["coef"] and rec[3:].tolist() == [B, 0, 0, 0, 0]
    again = run_distill(x, t, kind, tau, upstream)
    for k in ("loss", "grad", "lse", "aux", "record"):
        assert same_bits(out[k], again[k]), f"{k}: a second run gave other bits"
    return out, r


@pytest.mark.parametrize("pair", DC.DTYPE_PAIRS, ids=DC.pair_id)
@pytest.mark.parametrize("kind", DC.KINDS, ids=DC.kind_id)
@pytest.mark.parametrize("B,C", DC.SHAPES, ids=lambda v: str(v))
def test_distill_values_guards_and_same_bits(B, C, kind, pair):
    check_distill(PC.make_logits(B, C), DC.make_teacher(B, C), kind[0], kind[1], pair)


@pytest.mark.parametrize("kind", DC.KINDS, ids=DC.kind_id)
def test_distill_rows_off_a_16_byte_boundary(kind):
    """C % 8 == 0 but a storage starts one element past an aligned address - both, or the teacher's alone: the scalar path"""
    x, t = PC.make_logits(4, 1000), DC.make_teacher(4, 1000)
    check_distill(x, t, kind[0], kind[1], (F32, F32), offset=1)
    check_distill(x, t, kind[0], kind[1], (F16, F16), offset=1)
    check_distill(x, t, kind[0], kind[1], (F32, F16), offset=0, t_offset=1)


@pytest.mark.parametrize("pair", DC.DTYPE_PAIRS, ids=DC.pair_id)
@pytest.mark.parametrize("B,C", [(3, 5), (4, 1000)])
def test_distill_upstream_65536_through_the_device_pointer(B, C, pair):
    """a GradScaler's scale arrives as a device scalar"""
    for kind in DC.KINDS:
        check_distill(PC.make_logits(B, C, seed=1), DC.make_teacher(B, C, seed=1), kind[0], kind[1], pair, upstream=65536.0)


@pytest.mark.parametrize("pair", DC.DTYPE_PAIRS, ids=DC.pair_id)
def test_distill_hard_ties_go_to_the_lower_index(pair):
    B, C = 4, 1000
    t = DC.make_teacher(B, C, seed=2).clamp(-8.0, 8.0)
    t[0, 700] = t[0, 13] = 9.0                                     # two maxima in one row: 13 wins
    t[1, 999] = t[1, 0] = 9.0                                      # first against last element: 0 wins
    t[2, 257] = t[2, 256] = t[2, 513] = 9.0                        # neighbours owned by different threads / units: 256 wins
    t[3] = 1.0                                                     # a constant row: 0 wins
    out, r = check_distill(PC.make_logits(B, C, seed=2), t, "hard", 1.0, pair)
    assert out["aux"].tolist() == [13, 0, 256, 0]


def test_distill_logits_of_6e4_in_fp16():
    B, C = 3, 65
    g = PC._gen(5)
    sx = torch.where(torch.rand(B, C, generator=g) < 0.5, -1.0, 1.0)
    st = torch.where(torch.rand(B, C, generator=g) < 0.5, -1.0, 1.0)
    for kind in ("soft", "hard"):
        out, _ = check_distill(sx * 6e4, st * 6e4, kind, 1.0, (F16, F16))
        assert math.isfinite(float(out["loss"])) and bool(torch.isfinite(out["lse"]).all())
        assert bool(torch.isfinite(out["grad"].float()).all())


def test_distill_wrappers_refuse_bad_arguments():
    from m3vit_amd import _lib, ops
    x, t = torch.zeros(2, 8, device="cuda"), torch.zeros(2, 8, device="cuda", dtype=F16)
    rec, lse, aux = ops.loss_distill_fwd(x, t, "hard")
    g = torch.ones(1, device="cuda")
    for bad in (lambda: ops.loss_distill_fwd(x.cpu(), t, "soft"),
                lambda: ops.loss_distill_fwd(x, t.cpu(), "soft"),
                lambda: ops.loss_distill_fwd(x, t[:, :4].contiguous(), "soft"),
                lambda: ops.loss_distill_fwd(x, t.t(), "soft"),
                lambda: ops.loss_distill_fwd(x.t(), t.t().contiguous(), "soft"),
                lambda: ops.loss_distill_fwd(x, t.long(), "hard"),
                lambda: ops.loss_distill_fwd(x.double(), t, "hard"),
                lambda: ops.loss_distill_fwd(x, None, "hard"),
                lambda: ops.loss_distill_fwd(x, t, "medium"),
                lambda: ops.loss_distill_fwd(x, t, "soft", tau=0.0),
                lambda: ops.loss_distill_fwd(x, t, "soft", tau=float("inf")),
                lambda: ops.loss_distill_fwd(x, t, "soft", ws=torch.zeros(1, device="cuda")),
                lambda: ops.loss_distill_fwd(x, t, "soft", aux=torch.zeros(2, device="cuda")),
                lambda: ops.loss_distill_fwd(x.view(16), t.view(16), "soft"),
                lambda: ops.loss_distill_bwd(x, None, "soft", lse, aux, rec, g),
                lambda: ops.loss_distill_bwd(x, t, "hard", lse[:1], aux, rec, g),
                lambda: ops.loss_distill_bwd(x, t, "hard", lse, aux, rec, g.cpu()),
                lambda: ops.loss_distill_bwd(x, t, "hard", lse, aux, rec, g, dlogits=torch.zeros(2, 8, device="cuda", dtype=F16))):
        with pytest.raises(_lib.M3Error):
            bad()


# -------------------------------------------------------------------------------------------------------- the criterion
class _Teacher(torch.nn.Module):
    """a small teacher: mean-pooled pixels -> Linear; returns its logits in out_dtype (a teacher under autocast: 16 bits)"""

    def __init__(self, classes, out_dtype):
        super().__init__()
        self.fc = torch.nn.Linear(3, classes)
        self.out_dtype = out_dtype

    def forward(self, x):
        return (self.fc(x.mean((2, 3))) * 4).to(self.out_dtype)


@pytest.mark.parametrize("kind,tau", [("soft", 3.0), ("hard", 1.0)])
@pytest.mark.parametrize("t_dtype", [F32, F16], ids=["teacher-fp32", "teacher-fp16"])
def test_distillation_loss_end_to_end(kind, tau, t_dtype):
    from m3vit_amd.pretrain import DistillationLoss, SoftTargetCrossEntropy
    B, C, alpha = 6, 10, 0.3
    g = PC._gen(11)
    torch.manual_seed(5)
    teacher = _Teacher(C, t_dtype).cuda()
    crit = DistillationLoss(SoftTargetCrossEntropy(), teacher, kind, alpha, tau)
    images = torch.randn(B, 3, 8, 8, generator=g).cuda()
    o_cls = (torch.randn(B, C, generator=g) * 3).cuda().requires_grad_()
    o_dist = (torch.randn(B, C, generator=g) * 3).cuda().requires_grad_()
    target = PC.make_soft_target(B, C).cuda()
    with torch.no_grad():
        t_out = teacher(images)                                    # (also warms the teacher's kernels up before the sync check)
    crit(images, (o_cls.detach(), o_dist.detach()), target)
    with no_host_sync():
        total = crit(images, (o_cls, o_dist), target)
        (total * 2.0).backward()
    assert total.dim() == 0 and total.is_cuda
    base_r = PC.softce_ref(o_cls.detach().double().cpu(), target=target.cpu())
    dist_r = DC.distill_ref(o_dist.detach().double().cpu(), t_out.double().cpu(), kind, tau)
    base_lb, base_gb = PC.softce_bounds(base_r, o_cls.detach().double().cpu(), F32, upstream=2.0 * (1 - alpha))
    dist_lb, dist_gb, _ = DC.distill_bounds(dist_r, F32, upstream=2.0 * alpha)
    ref_total = (1 - alpha) * base_r["loss"] + alpha * dist_r["loss"]
    # the two products and the sum in fp32: 3 u32 of the magnitudes, over the two kernels' own bounds
    comb = (1 - alpha) * base_lb + alpha * dist_lb + DC.SAFETY * 3 * DC.U32 * ((1 - alpha) * base_r["loss"].abs() + alpha * dist_r["loss"].abs())
    assert_within(total.detach().reshape(1), ref_total.reshape(1), comb, "total")
    # upstream of each kernel: fl(2 (1 - alpha)) / fl(2 alpha), one more rounding each: u32 |ref|
    assert_within(o_cls.grad, base_r["grad"] * 2.0 * (1 - alpha), base_gb + DC.SAFETY * DC.U32 * (base_r["grad"] * 2.0).abs(), "d logits_cls")
    assert_within(o_dist.grad, dist_r["grad"] * 2.0 * alpha, dist_gb + DC.SAFETY * DC.U32 * (dist_r["grad"] * 2.0).abs(), "d logits_dist")
    assert all(p.grad is None for p in teacher.parameters()), "the teacher got a gradient"
    st = crit.last_stats
    assert set(st) == {"loss_base", "loss_distill", "loss_no_cv"} and all(v.is_cuda and v.dim() == 0 for v in st.values())
    assert_within(st["loss_base"].reshape(1), base_r["loss"].reshape(1), base_lb, "loss_base")
    assert_within(st["loss_distill"].reshape(1), dist_r["loss"].reshape(1), dist_lb, "loss_distill")
    assert float(st["loss_no_cv"]) == float(total.detach())
    for outputs in (o_cls, (o_cls, None)):
        with pytest.raises(ValueError):
            crit(images, outputs, target)
