"""CPU: the token sharing stage without a GPU - the float64 restatement of sharing_cases.py against what the reference's own
code gave (tests/golden/g14_sharing.npz), the input builder's separation and draw cap, the module surface of
m3vit_amd.sharing, and the C ABI's refusals (which return before anything is launched)."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sharing_cases as SC                                       # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_sharing.npz")
F64 = torch.float64


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _t(g, key):
    return torch.from_numpy(g[key])


def _close(a, b, what):
    a, b = a.double(), b.double()
    scale = max(float(b.abs().max()) if b.numel() else 0.0, 1e-300)
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert a.shape == b.shape and err <= 1e-12 * scale, f"{what}: max |diff| {err:.3e} against a scale of {scale:.3e}"


@pytest.mark.parametrize("c", SC.golden_cases(), ids=SC.case_id)
def test_restatement_equals_the_reference(golden, c):
    """values and gradients to 1e-12 relative, integers exact"""
    k = SC.case_id(c)
    T, P, D, Dg = c["T"], c["B"] * c["N"], c["D"], c["Dg"]
    xs = _t(golden, f"{k}/xs").double().requires_grad_(True)
    w = _t(golden, f"{k}/w_gate").double().requires_grad_(True)
    emb = _t(golden, f"{k}/task_emb").double().requires_grad_(True) if Dg else None
    prev = _t(golden, f"{k}/prev") if c["prev"] else None
    r = SC.stage(xs, w, emb, _t(golden, f"{k}/noise"), c["tau"], c["hard"], c["gamma"], c["eps"], prev)
    _close(r["G"].detach(), _t(golden, f"{k}/G"), "G")
    assert torch.equal(r["bits"], _t(golden, f"{k}/bits"))
    assert torch.equal(r["flat_idx"], _t(golden, f"{k}/flat_idx"))
    _close(r["shared_x"].detach()[r["flat_idx"]], _t(golden, f"{k}/shared_x"), "shared_x")
    assert float(r["shared_x"].detach()[r["bits"] == 0].abs().sum()) == 0.0
    _close(r["y"].detach(), _t(golden, f"{k}/y"), "y")
    s = r["stats"]
    assert [s["shared_positions"], s["shared_tasktoken_count"], s["partial_split_count"], s["partial_split_total"],
            s["shared_bits_flip_count"], s["shared_bits_flip_total"]] == golden[f"{k}/stats"].tolist()
    assert s["S"] == s["shared_positions"] and sum(s["S_t"]) == s["shared_tasktoken_count"]
    assert float(SC.share_loss(r["bits"], T)) == float(golden[f"{k}/loss"])
    cy, cs, cg = SC.functional(c)
    ((cy * r["y"]).sum() + (cs * r["shared_x"]).sum() + (cg * r["G"]).sum()).backward()
    _close(xs.grad, _t(golden, f"{k}/d_xs"), "d xs")
    _close(w.grad, _t(golden, f"{k}/d_w_gate"), "d w_gate")
    if Dg:
        _close(emb.grad, _t(golden, f"{k}/d_task_emb"), "d task_emb")
    # Aggregation / AggregationStage
    xa = _t(golden, f"{k}/xs").double().requires_grad_(True)
    need = _t(golden, f"{k}/agg_need")
    y, agg = SC.aggregate(xa, _t(golden, f"{k}/agg_masks"), need)
    _close(agg.detach(), _t(golden, f"{k}/agg"), "agg")
    _close(y.detach(), _t(golden, f"{k}/agg_y"), "agg y")
    ((cy * y).sum() + (cs * agg).sum()).backward()
    _close(xa.grad, _t(golden, f"{k}/agg_d_xs"), "agg d xs")


def test_golden_has_shared_and_unshared_cases(golden):
    ks = [SC.case_id(c) for c in SC.golden_cases()]
    assert any(golden[f"{k}/flat_idx"].size == 0 for k in ks) and any(golden[f"{k}/flat_idx"].size > 0 for k in ks)
    assert any(float(golden[f"{k}/loss"]) > 0 for k in ks) and os.path.getsize(GOLDEN) < 512 * 1024


@pytest.mark.parametrize("c", SC.all_cases(), ids=SC.case_id)
def test_builder_separates_every_score_inside_the_draw_cap(c):
    I = SC.make_inputs(c)
    assert 1 <= I["draws"] <= SC.MAX_DRAWS
    delta = 4 * I["gb"]
    assert float(I["gb"].min()) > 0.0
    assert bool(((I["ref"]["soft"] - 0.5).abs() >= delta).all()) and bool(((I["ref"]["G"] - c["gamma"]).abs() >= delta).all())
    again = SC.make_inputs(c)                                   # the same seed and counter give the same bits
    assert torch.equal(again["xs"], I["xs"]) and torch.equal(again["noise"], I["noise"])


def test_degenerate_routings_are_what_they_claim():
    none, every, one, two = (SC.make_inputs(c)["ref"] for c in SC.degenerate_cases())
    assert none["stats"]["shared_positions"] == 0 and not bool(none["bits"].any())
    T, P = every["G"].shape
    assert bool((every["bits"] == (1 << T) - 1).all()) and every["stats"]["partial_split_count"] == 0
    assert bool(((one["G"] >= 0.5).sum(0) == 1).all()) and not bool(one["bits"].any())
    assert two["stats"]["partial_split_count"] == two["G"].shape[1] == two["stats"]["shared_positions"]


def test_case_grid_covers_the_issue():
    cs = SC.stage_cases()
    assert {c["T"] for c in cs} == {2, 3, 5, 8} and {(c["B"], c["N"]) for c in cs} == {(1, 1), (1, 65), (2, 197), (6, 197)}
    assert {c["D"] for c in cs} >= {192, 384, 768} and {c["Dg"] for c in cs} == {0, 64}
    assert {(c["D"], c["dtype"]) for c in cs} >= {(D, d) for D in (192, 384, 768) for d in ("f32", "f16", "bf16")}
    assert {(c["dtype"], c["hard"]) for c in cs} == {(d, h) for d in ("f32", "f16", "bf16") for h in (False, True)}
    assert {c["prev"] for c in cs} == {False, True} and 6 * 197 > SC.SCAN_WIDTH > 2 * 197


# ------------------------------------------------------------------------------------------------------ module surface
def _params(f):
    return list(inspect.signature(f).parameters)


def test_names_and_signatures():
    from m3vit_amd import sharing as S
    assert _params(S.ShareabilityPredictor.__init__) == ["self", "d_model", "d_task_emb", "temperature", "hard"]
    assert _params(S.ShareabilityPredictor.forward)[:3] == ["self", "inp", "task_emb"] and "noise" in _params(S.ShareabilityPredictor.forward)
    assert _params(S.Aggregation.__init__) == ["self", "eps"]
    assert _params(S.Aggregation.forward) == ["self", "task_outputs", "curr_shared_masks", "aggregation_mask"]
    assert _params(S.AggregationStage.__init__) == ["self", "aggregation_module", "num_tasks"]
    assert _params(S.AggregationStage.forward) == ["self", "outs", "shared_masks", "agg_needed_mask"]
    assert _params(S.SharingRegularizationLoss.__init__) == ["self", "lambda_share"]
    assert _params(S.SharingRegularizationLoss.forward) == ["self", "shared_bits", "num_tasks"]
    assert _params(S.transition_stage) == ["outs", "prev_shared_bits", "g_shared", "gamma", "eps", "num_tasks"]
    assert _params(S.apply_shared_broadcast)[:4] == ["outs", "shared_bits", "shared_x", "shared_flat_idx"]
    assert _params(S.SharingStage.forward) == ["self", "outs", "prev_shared_bits", "task_emb_T_E", "gamma", "noise"]
    d = inspect.signature(S.ShareabilityPredictor.__init__).parameters
    assert (d["d_task_emb"].default, d["temperature"].default, d["hard"].default) == (0, 1.0, False)
    assert inspect.signature(S.Aggregation.__init__).parameters["eps"].default == 1e-6
    assert inspect.signature(S.SharingRegularizationLoss.__init__).parameters["lambda_share"].default == 0.01
    import m3vit_amd
    assert m3vit_amd.SharingStage is S.SharingStage and m3vit_amd.ShareabilityPredictor is S.ShareabilityPredictor


def test_state_dict_keys_and_init():
    from m3vit_amd.sharing import AggregationStage, Aggregation, ShareabilityPredictor, SharingStage
    torch.manual_seed(0)
    p = ShareabilityPredictor(384, 64)
    assert list(p.state_dict()) == ["w_gate"] and p.w_gate.shape == (448, 2) and p.w_gate.requires_grad
    assert list(ShareabilityPredictor(192).state_dict()) == ["w_gate"] and ShareabilityPredictor(192).w_gate.shape == (192, 2)
    # kaiming_uniform_(a = sqrt 5) of a [d_input, 2] tensor: fan_in 2, bound sqrt(6 / (6 * 2))
    assert 0.69 < float(p.w_gate.detach().abs().max()) <= 2 ** -0.5
    assert list(SharingStage(p, 3).state_dict()) == ["share_pred.w_gate"]
    assert list(AggregationStage(Aggregation(), 3).state_dict()) == []


def test_cpu_tensors_raise():
    from m3vit_amd import sharing as S
    from m3vit_amd._lib import M3Error
    x = {t: torch.randn(2, 5, 16) for t in range(3)}
    pred = S.ShareabilityPredictor(16, 8)
    with pytest.raises(M3Error, match="GPU"):
        pred(x[0], torch.randn(8))
    with pytest.raises(M3Error, match="GPU"):
        S.SharingStage(pred, 3)(x, None, torch.randn(3, 8))
    masks = [torch.ones(2, 5, dtype=torch.bool)] * 3
    with pytest.raises(M3Error, match="GPU"):
        S.Aggregation()(x, masks, masks[0])
    with pytest.raises(M3Error, match="GPU"):
        S.AggregationStage(S.Aggregation(), 3)(dict(x), masks, masks[0])
    with pytest.raises(M3Error, match="GPU"):
        S.SharingRegularizationLoss()(torch.zeros(2, 5, dtype=torch.int64), 3)
    with pytest.raises(M3Error, match="GPU"):
        S.transition_stage(x, None, {t: torch.rand(2, 5) for t in range(3)})
    with pytest.raises(M3Error, match="GPU"):
        S.apply_shared_broadcast(dict(x), torch.zeros(2, 5, dtype=torch.int64), torch.zeros(1, 16), torch.zeros(1, dtype=torch.int64))


@pytest.mark.parametrize("T", [1, 9])
def test_task_counts_outside_2_to_8_are_refused_with_a_message(T):
    from m3vit_amd import _lib
    from m3vit_amd import sharing as S
    pred = S.ShareabilityPredictor(16)
    with pytest.raises(_lib.M3Error, match=f"num_tasks={T}.*2 to 8"):
        S.SharingStage(pred, T)
    x = {t: torch.randn(2, 5, 16) for t in range(T)}
    with pytest.raises(_lib.M3Error, match="2 to 8"):
        S.transition_stage(x, None, {t: torch.rand(2, 5) for t in range(T)})
    # the C entry points themselves refuse before anything is launched (no GPU needed)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.lib()
    rows = _lib.ShareRows()
    z = ctypes.c_void_p(None)
    rc = L.m3_share_stage_fwd(ctypes.byref(rows), _lib.M3_F16, T, 8, 16, z, z, 0, z, 1.0, 0, 0.5, 1e-6, ctypes.byref(rows), z,
                              z, z, z, z)
    assert rc == _lib.M3_ERR_UNSUPPORTED and f"T={T}" in L.m3_last_error().decode()
    rc = L.m3_share_aggregate_fwd(ctypes.byref(rows), _lib.M3_F16, T, 8, 16, z, z, 1e-6, ctypes.byref(rows), z, z)
    assert rc == _lib.M3_ERR_UNSUPPORTED and f"T={T}" in L.m3_last_error().decode()


def test_row_lengths_outside_the_stated_limit_are_refused():
    from m3vit_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.lib()
    rows = _lib.ShareRows()
    z = ctypes.c_void_p(None)
    assert _lib.M3_SHARE_MAX_D == 1024 and _lib.M3_SHARE_MAX_T == 8
    for D, rc_want in ((1032, _lib.M3_ERR_UNSUPPORTED), (100, _lib.M3_ERR_UNSUPPORTED), (0, _lib.M3_ERR_UNSUPPORTED)):
        rc = L.m3_share_predict_fwd(z, _lib.M3_F32, 8, D, z, z, 0, z, 1.0, 0, z, z, z)
        assert rc == rc_want and f"D={D}" in L.m3_last_error().decode()
    assert L.m3_share_predict_fwd(z, _lib.M3_F32, 8, 16, z, z, -1, z, 1.0, 0, z, z, z) == _lib.M3_ERR_ARG    # Dg < 0
    for D in (192, 384, 768, 1024):                     # the widths the backbone configurations use pass the shape check
        assert L.m3_share_predict_fwd(z, _lib.M3_F32, 8, D, z, z, 0, z, 1.0, 0, z, z, z) == _lib.M3_ERR_ARG  # (null operand)
        assert "null operand" in L.m3_last_error().decode()


def test_header_entries_are_bound():
    from m3vit_amd import _lib, ops
    names = ["m3_share_num_blocks", "m3_share_bwd_ws_elems", "m3_share_stage_fwd", "m3_share_stage_bwd", "m3_share_predict_fwd",
             "m3_share_predict_bwd", "m3_share_aggregate_fwd", "m3_share_aggregate_bwd", "m3_share_compact"]
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("m3_share_")) == sorted(names)
    assert _lib.SIGNATURES["m3_share_stage_fwd"][1][0] is ctypes.POINTER(_lib.ShareRows)          # the table of task tensors
    p = dict(_lib.ShareRows._fields_)["p"]
    assert issubclass(p, ctypes.Array) and p._type_ is ctypes.c_void_p and p._length_ == _lib.M3_SHARE_MAX_T
    assert _lib.SIGNATURES["m3_share_bwd_ws_elems"][0] is ctypes.c_int64
    for f in ("share_stage_fwd", "share_stage_bwd", "share_predict_fwd", "share_predict_bwd", "share_aggregate_fwd",
              "share_aggregate_bwd", "share_compact", "share_bwd_ws_elems"):
        assert callable(getattr(ops, f))
    from m3vit_amd import functional as Fn
    assert all(hasattr(Fn, n) for n in ("ShareStageFn", "SharePredictFn", "ShareAggregateFn"))
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        assert L.m3_share_num_blocks(25216) == _lib.M3_SHARE_MAX_BLOCKS and L.m3_share_num_blocks(5) == 2
        assert L.m3_share_bwd_ws_elems(25216, 2, 384, 64) == 1024 * (384 + 64 + 128) == ops.share_bwd_ws_elems(25216, 2, 384, 64)
