"""Generate tests/golden/g12_losses.npz from the reference's OWN criterion classes.  Run where a reference checkout is
available; not collected by pytest:

    python tests/gen_golden_losses.py /path/to/reference        (or M3VIT_REFERENCE=/path/to/reference)

The reference modules used (never copied; only their INPUTS and OUTPUTS are stored):
  losses/loss_functions.py   SoftMaxwithLoss, BalancedCrossEntropyLoss, DepthLoss, NormalsLoss
  losses/loss_schemes.py     MultiTaskLoss
Both import with torch and numpy alone, and every class runs in float64 on the CPU.

Written, for every case of loss_cases.fixture_cases() under the key k = loss_cases.case_id(case):
  {k}/pred   float32 [B,C,H,W]   the inputs (loss_cases.make_inputs, seed 0), evaluated by the reference in float64
  {k}/label  float32
  {k}/loss   float64             the reference's loss (NaN where it gives NaN)
  {k}/grad   float64 [B,C,H,W]   d loss / d pred from the reference's autograd
and for every scheme of loss_cases.SCHEMES (one MultiTaskLoss call each: plain two-task, five-task with an all-ignored
human_parts, single_task, multi_level, TAM level keys) under mt/{scheme}/:
  pred/{key}, gt/{task}   the inputs;  out/{key}  every entry of the returned dictionary, `total` included;
  grad/{key}              d total / d pred[key]
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("M3VIT_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "losses")):
    raise SystemExit("usage: python tests/gen_golden_losses.py /path/to/reference (a checkout with losses/loss_functions.py)")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from losses import loss_functions as LF            # noqa: E402
from losses import loss_schemes as LS              # noqa: E402
import loss_cases as LC                            # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_losses.npz")


def reference_module(kind, extra):
    with contextlib.redirect_stdout(io.StringIO()):              # the reference's constructors print
        if kind == "ce":
            return LF.SoftMaxwithLoss()
        if kind == "l1":
            return LF.DepthLoss("l1")
        if kind == "normals":
            return LF.NormalsLoss(normalize=True, size_average=True, norm=extra)
        return LF.BalancedCrossEntropyLoss(size_average=True, pos_weight=extra)


def main():
    data = {}
    for case in LC.fixture_cases():
        kind, C, size, extra = case
        k = LC.case_id(case)
        pred, label = LC.make_inputs(kind, C, size)
        x = pred.double().requires_grad_(True)
        loss = reference_module(kind, extra)(x, label.double())
        loss.backward()
        data[f"{k}/pred"] = pred.numpy()
        data[f"{k}/label"] = label.numpy()
        data[f"{k}/loss"] = np.float64(loss.item())
        data[f"{k}/grad"] = x.grad.numpy()
    for name, (tasks, prefixes, multi_level, tam, single) in LC.SCHEMES.items():
        pred, gt = LC.scheme_inputs(name)
        loss_ft = torch.nn.ModuleDict({t: reference_module(*LC.TASK_KIND[t]) for t in tasks})
        with contextlib.redirect_stdout(io.StringIO()):
            crit = LS.MultiTaskLoss(list(tasks), loss_ft, {t: LC.TASK_WEIGHT[t] for t in tasks}, multi_level,
                                    {"model_kwargs": {"tam": tam}})
        xs = {key: v.double().requires_grad_(True) for key, v in pred.items()}
        gts = {t: v.double() for t, v in gt.items()}
        out = crit(xs, gts) if single is None else crit(xs, gts, single_task=single)
        out["total"].backward()
        for key, v in pred.items():
            data[f"mt/{name}/pred/{key}"] = v.numpy()
            g = xs[key].grad
            data[f"mt/{name}/grad/{key}"] = (torch.zeros_like(xs[key]) if g is None else g).numpy()
        for t, v in gt.items():
            data[f"mt/{name}/gt/{t}"] = v.numpy()
        for key, v in out.items():
            data[f"mt/{name}/out/{key}"] = np.float64(float(v.detach()))
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {len(data)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
