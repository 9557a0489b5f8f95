"""CPU: the host half of the fused optimizer (m3vit_amd.optim, ops.OptimPlan) and the yardstick of its GPU tests.

* torch's own fp32 optimizers stay inside every bound tests/test_optim_gpu.py uses, on that test's own inputs: the bound is
  one the reference arithmetic keeps, so a kernel that breaks it is wrong and not unlucky;
* the descriptor table: chunk_start prefix, vec_ok rule, the struct's layout; the hyper-parameter row's hi / lo betas;
* unsupported options are refused with a clear message; state_dict() carries torch's key names."""
import ctypes

import pytest
import torch

import optim_cases as oc


@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_torch_fp32_keeps_the_bounds_of_the_gpu_test(name):
    cls, group_kw, group_of, clip, lr_change, lrs = oc.case(name)
    params, grads = oc.inputs_of(name)
    got, _ = oc.run_torch(cls, group_kw, params, grads, torch.float32, group_of, clip, lr_change)
    worst = oc.check_run(got, oc.reference(name), grads, group_kw, group_of, cls, f"torch fp32 {name}", lrs=lrs)
    print(f"torch fp32 against fp64, {name}: worst err / bound {worst:.3f}")
    assert worst <= 1.0


def test_inputs_cover_what_they_claim():
    params, grads = oc.inputs()
    assert sum(p.numel() for p in params) * 4 < 1_000_000                  # p, g, m, v together under 1 M elements
    offs, o = [], 0
    for n in oc.SIZES:
        offs.append(o % 4)
        o += n
    assert {1, 2, 3} <= set(offs) and offs.count(0) >= 3                    # packed gradients: every misalignment, and aligned ones
    assert not bool(params[oc.ZERO_PARAM].any())
    g = torch.cat([x.abs() for x in grads[0]])
    assert float(g.max()) > 10 and float(g[g > 0].min()) < 1e-6
    for name in ("clip",):                                                  # the clip case clips: the norm is above max_norm
        assert all(float(r["norm"]) > 5 * oc.CASES[name]["clip"] for r in oc.reference(name))


def test_descriptor_table_layout_prefix_and_alignment_rule():
    from m3vit_amd import _lib, ops
    assert ctypes.sizeof(_lib.OptimDesc) == 56 and _lib.OptimDesc.n.offset == 32 and _lib.OptimDesc.vec_ok.offset == 48
    base = 1 << 20
    rows = [(base, base + 4096, base, base, 1, 0),                          # all aligned
            (base + 16, base + 4, base, base, 4096, 1),                     # g at element offset 1
            (base, base + 32, base + 8, base, 4097, 0),                     # m at element offset 2
            (base, base, base, base + 12, 3 * 4096, 1),                     # v at element offset 3
            (base + 48, base + 64, base + 80, 0, 4095, 0)]                  # SGD: no v, all aligned
    arr, total = ops.optim_table(rows)
    assert [d.chunk_start for d in arr] == [0, 1, 2, 4, 7] and total == 8
    assert [d.vec_ok for d in arr] == [1, 0, 0, 0, 1]
    assert [d.group for d in arr] == [0, 1, 0, 1, 0] and [d.n for d in arr] == [1, 4096, 4097, 3 * 4096, 4095]
    assert arr[4].v is None and arr[0].g == base + 4096
    with pytest.raises(_lib.M3Error):
        ops.optim_table([(base, base, base, base, 0, 0)])


def test_hyper_row_carries_the_betas_as_hi_plus_lo():
    from m3vit_amd import _lib, ops
    row = ops.optim_hyper_row(1e-3, 0.9, 0.999, 1e-8, 0.05, decoupled=True)
    assert len(row) == _lib.M3_OPTIM_HYPER and row[5] == _lib.M3_OPTIM_DECOUPLED
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float64).to(torch.float32))          # noqa: E731
    for hi, lo, b in ((row[1], row[6], 0.9), (row[2], row[7], 0.999)):
        assert hi == f32(b) and abs(lo) <= 2.0 ** -24 * b                   # the fp32 value and what its rounding lost
        assert abs((hi + f32(lo)) - b) <= 2.0 ** -47 * b                    # as two fp32 numbers they are the double
    # what the device then forms in double is the bias correction torch forms on the host
    assert abs((1.0 - (row[2] + row[7])) - (1.0 - 0.999)) <= 1e-12 * (1.0 - 0.999)
    assert ops.optim_hyper_row(0.1, 0.9, weight_decay=1e-4, nesterov=True)[5] == _lib.M3_OPTIM_NESTEROV


def test_unsupported_options_are_refused():
    from m3vit_amd.optim import FusedAdam, FusedAdamW, FusedSGD
    p = [torch.nn.Parameter(torch.zeros(4))]
    for make in (lambda: FusedAdamW(p, amsgrad=True), lambda: FusedAdam(p, amsgrad=True),
                 lambda: FusedAdamW(p, maximize=True), lambda: FusedSGD(p, maximize=True),
                 lambda: FusedSGD(p, momentum=0.9, dampening=0.1)):
        with pytest.raises(NotImplementedError, match="not supported"):
            make()
    with pytest.raises(ValueError):
        FusedAdamW(p, max_grad_norm=0.0)
    with pytest.raises(ValueError):
        FusedSGD(p, nesterov=True)
    opt = FusedAdamW(p)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))], "amsgrad": True})
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        opt.last_grad_norm


def test_cpu_tensors_are_refused_like_every_other_op():
    from m3vit_amd import _lib
    from m3vit_amd.optim import FusedAdamW
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(_lib.M3Error, match="GPU"):
        FusedAdamW([p]).step()


def test_param_groups_and_state_dict_use_torchs_names():
    from m3vit_amd.optim import FusedAdam, FusedAdamW, FusedSGD
    for ours, theirs, kw in ((FusedAdamW, torch.optim.AdamW, {}), (FusedAdam, torch.optim.Adam, {}),
                             (FusedSGD, torch.optim.SGD, dict(momentum=0.9))):
        a = ours([torch.nn.Parameter(torch.zeros(4))], **kw)
        b = theirs([torch.nn.Parameter(torch.zeros(4))], **kw)
        assert set(a.param_groups[0]) == set(b.param_groups[0])
        assert {k: v for k, v in a.defaults.items()} == {k: v for k, v in b.defaults.items()}
        assert a._step_supports_amp_scaling
    # a torch checkpoint loads (state under torch's keys; the flat buffers are filled on the first GPU step) and differing
    # step counts are refused
    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(3))]
    t = torch.optim.AdamW(ps, foreach=False)
    for p in ps:
        p.grad = torch.randn_like(p)
    t.step()
    f = FusedAdamW(ps)
    f.load_state_dict(t.state_dict())
    sd = f.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][1]["step"]) == 1.0
    assert torch.equal(sd["state"][0]["exp_avg"], t.state[ps[0]]["exp_avg"])
    t2 = torch.optim.AdamW(ps, foreach=False)
    t2.load_state_dict(sd)                                                  # and back into torch
    assert float(t2.state[ps[1]]["step"]) == 1.0
    bad = t.state_dict()
    bad["state"][1]["step"] = torch.tensor(7.0)
    with pytest.raises(ValueError, match="one step counter"):
        FusedAdamW(ps).load_state_dict(bad)
