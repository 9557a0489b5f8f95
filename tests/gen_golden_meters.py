"""Generate tests/golden/g13_meters.npz from the reference's OWN meter classes.  Run where a reference checkout is
available; not collected by pytest:

    python tests/gen_golden_meters.py /path/to/reference        (or M3VIT_REFERENCE=/path/to/reference)

The reference code used (never copied; only its INPUTS and OUTPUTS are stored):
  utils/utils.py                    get_output
  evaluation/eval_semseg.py         SemsegMeter          evaluation/eval_human_parts.py   HumanPartsMeter
  evaluation/eval_depth.py          DepthMeter           evaluation/eval_normals.py       NormalsMeter
  evaluation/eval_sal.py            SaliencyMeter        evaluation/eval_edge.py          EdgeMeter
  evaluation/evaluate_utils.py      calculate_multi_task_performance
They import with torch, numpy, scipy and PIL once cv2 and imageio are IMPORT-LINE-ONLY placeholder modules whose every
attribute raises when used (tests/gen_golden.py's device); the generator asserts that none was read.  Everything runs on the
CPU, in float64 where the class allows it (the saliency and edge meters convert to float32 themselves).

Written, for every case of meter_cases.FIXTURES under its key k, for the updates u = 0, 1 of one meter object:
  {k}/pred{u}, {k}/label{u}   float32: the inputs (meter_cases.fixture_inputs)
  {k}/acc{u}/...              the meter's accumulators after update u (tp / fp / fn; n_valid, total_rmses, total_log_rmses; the
                              eval_dict entries; the per-image jaccards / prec / rec of the update; loss, n)
  {k}/score{u}/...            get_score(verbose=False) after update u, every key
and mtl/eval, mtl/single (JSON) and mtl/value: one calculate_multi_task_performance call.
The conditions on the inputs under which the integer counts are the same in any precision (meter_cases.conditions_hold: no
two equal logits in a pixel outside the tie case, no probability within 1e-5 of a threshold, no angle within 0.05 degrees of a
cut, positive valid depth labels) are asserted here.
"""
import contextlib
import io
import json
import os
import sys
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("M3VIT_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "evaluation")):
    raise SystemExit("usage: python tests/gen_golden_meters.py /path/to/reference (a checkout with evaluation/eval_semseg.py)")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meter_cases as MC                           # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_meters.npz")


class _Placeholder(types.ModuleType):
    """stands for a module this machine lacks: importing it works, reading any attribute of it is recorded and raises"""
    reads = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        _Placeholder.reads.append(f"{self.__name__}.{name}")
        raise RuntimeError(f"placeholder attribute {self.__name__}.{name} was used: the fixture would not be the reference's output")


for _n in ("cv2", "imageio"):
    if _n not in sys.modules:
        sys.modules[_n] = _Placeholder(_n)

from utils.utils import get_output                                   # noqa: E402
from evaluation.eval_semseg import SemsegMeter                       # noqa: E402
from evaluation.eval_human_parts import HumanPartsMeter              # noqa: E402
from evaluation.eval_depth import DepthMeter                         # noqa: E402
from evaluation.eval_normals import NormalsMeter                     # noqa: E402
from evaluation.eval_sal import SaliencyMeter                        # noqa: E402
from evaluation.eval_edge import EdgeMeter                           # noqa: E402
from evaluation.evaluate_utils import calculate_multi_task_performance   # noqa: E402


def reference_meter(task, db):
    with contextlib.redirect_stdout(io.StringIO()):
        if task == "semseg":
            return SemsegMeter(db)
        if task == "human_parts":
            return HumanPartsMeter(db)
        return {"depth": DepthMeter, "normals": NormalsMeter, "sal": SaliencyMeter}[task]() if task != "edge" else EdgeMeter(MC.EDGE_W)


def accumulators(task, m):
    if task in ("semseg", "human_parts"):
        return dict(tp=np.array(m.tp, dtype=np.int64), fp=np.array(m.fp, dtype=np.int64), fn=np.array(m.fn, dtype=np.int64))
    if task == "depth":
        return dict(n_valid=np.float64(m.n_valid), total_rmses=np.float64(m.total_rmses), total_log_rmses=np.float64(m.total_log_rmses))
    if task == "normals":
        return {k: np.float64(v) for k, v in m.eval_dict.items()}
    if task == "sal":
        return dict(jaccards=np.asarray(m.all_jacards[-1], dtype=np.float64), prec=np.asarray(m.prec[-1], dtype=np.float64),
                    rec=np.asarray(m.rec[-1], dtype=np.float64))
    return dict(loss=np.float64(m.loss), n=np.float64(m.n))


def main():
    data = {}
    for key, task, db, C, size in MC.FIXTURES:
        kind = MC.TASK_KIND[task]
        m = reference_meter(task, db)
        for u in (0, 1):
            pred, label = MC.fixture_inputs(key, u)
            assert MC.conditions_hold(kind, pred, label), key
            if kind == "iou" and not key.endswith("-ties"):
                s = pred.sort(dim=1).values
                assert bool((s[:, 1:] != s[:, :-1]).all()), f"{key}: two equal logits in a pixel"
            wide = task not in ("sal", "edge")
            x = pred.double() if wide else pred
            gt = label.double() if wide else label
            m.update(get_output(x, task), gt.clone())                # (the normals meter overwrites its label in place)
            data[f"{key}/pred{u}"] = pred.numpy()
            data[f"{key}/label{u}"] = label.numpy()
            for k, v in accumulators(task, m).items():
                data[f"{key}/acc{u}/{k}"] = v
            with contextlib.redirect_stdout(io.StringIO()):
                sc = m.get_score(verbose=False)
            for k, v in sc.items():
                if k not in ("all_jaccards", "prec", "rec"):
                    data[f"{key}/score{u}/{k}"] = np.asarray(v, dtype=np.float64)
    ev = {"semseg": {"mIoU": 0.41}, "depth": {"rmse": 0.62}, "normals": {"mean": 21.5}, "sal": {"mIoU": 0.66},
          "human_parts": {"mIoU": 0.58}, "edge": {"odsF": 0.7}}
    st = {"semseg": {"mIoU": 0.40}, "depth": {"rmse": 0.60}, "normals": {"mean": 20.0}, "sal": {"mIoU": 0.67},
          "human_parts": {"mIoU": 0.60}, "edge": {"odsF": 0.68}}
    data["mtl/eval"], data["mtl/single"] = np.array(json.dumps(ev)), np.array(json.dumps(st))
    data["mtl/value"] = np.float64(calculate_multi_task_performance(ev, st))
    assert not _Placeholder.reads, f"a placeholder module was read while reference code ran: {_Placeholder.reads}"
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {len(data)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
