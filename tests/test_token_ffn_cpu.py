"""CPU: the token blocks' FFN sublayer (m3vit_amd.sharing.TokenFFNStage) without a GPU - the float64 restatement of
token_ffn_cases.py against the reference's own results (tests/golden/g15_token_ffn.npz: values and every gradient, the recorded
drop-path draws of its training case included), the derived row bounds over random words, the work list's enumeration, the
module's refusals and its state-dict keys, and the C ABI's host-side entries."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import token_ffn_cases as TC                       # noqa: E402

F64 = torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_token_ffn.npz")


def _golden_keys():
    return [TC.case_id(c) for c in TC.golden_cases()] + [TC.case_id(TC.golden_train_case()) + "/train"]


def _case_of(key):
    if key.endswith("/train"):
        return TC.golden_train_case()
    return next(c for c in TC.golden_cases() if TC.case_id(c) == key)


def golden_inputs(z, key):
    """the stored inputs of a golden case as float64 CPU tensors: (case, xs, bits, sx, params, path_scale, shared_path_scale)"""
    c = _case_of(key)
    g = lambda n: torch.from_numpy(z[f"{key}/{n}"])                                   # noqa: E731
    p = {n: g(n).double() for n in ("gamma", "beta", "w1", "b1", "w2", "b2")}
    p["eps"] = TC.LN_EPS
    ps = g("path_scale").double() if f"{key}/path_scale" in z.files else None
    sps = g("shared_path_scale").double() if f"{key}/shared_path_scale" in z.files else None
    return c, g("xs").double(), g("bits"), g("sx").double(), p, ps, sps


@pytest.mark.parametrize("key", _golden_keys())
def test_restatement_equals_the_reference(key):
    """values and all gradients at float64 round-off: the two differ in summation order only"""
    z = np.load(GOLDEN)
    c, xs, bits, sx, p, ps, sps = golden_inputs(z, key)
    assert xs.shape == (c["T"], c["B"] * c["N"], c["C"]) and p["w1"].shape == (c["H"], c["C"]) and c["H"] == 2 * c["C"]
    xs.requires_grad_(True); sx.requires_grad_(True)
    for n in ("gamma", "beta", "w1", "b1", "w2", "b2"):
        p[n].requires_grad_(True)
    y = TC.stage(xs, bits, sx, p, c["mode"], c["N"], ps, sps)
    (TC.functional(c) * y).sum().backward()

    def close(a, name):
        b = torch.from_numpy(z[f"{key}/{name}"])
        a = torch.zeros_like(b) if a is None else a.detach()
        assert torch.allclose(a, b, rtol=1e-10, atol=1e-12 * max(1.0, float(b.abs().max()))), (name, float((a - b).abs().max()))
    close(y, "y")
    close(xs.grad, "d_xs"); close(sx.grad, "d_sx")
    for n in ("gamma", "beta", "w1", "b1", "w2", "b2"):
        close(p[n].grad, "d_" + n)
    # what the formulas promise, on the reference's own numbers: an overwritten row passes nothing back, an unshared position
    # has no representative
    M = TC.bit_masks(bits, c["T"])
    assert not bool(torch.from_numpy(z[f"{key}/d_xs"])[M].count_nonzero())
    assert not bool(torch.from_numpy(z[f"{key}/d_sx"])[bits == 0].count_nonzero())
    if key.endswith("/train"):
        assert set(np.unique(z[f"{key}/path_scale"])) == {0.0, 1 / 0.75} and 0.0 in z[f"{key}/shared_path_scale"]


def test_golden_file_covers_the_issue_shapes():
    z = np.load(GOLDEN)
    cs = TC.golden_cases()
    assert {c["T"] for c in cs} == {2, 3, 5} and {(c["B"], c["N"]) for c in cs} == {(2, 9), (1, 12)}
    assert {c["C"] for c in cs} == {16, 24} and {c["pattern"] for c in cs} == {"mixed", "none", "all"}
    assert {c["mode"] for c in cs} == set(TC.MODES)
    for k in _golden_keys():
        assert f"{k}/y" in z.files and f"{k}/d_w1" in z.files
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_row_bounds_over_random_words():
    """R <= T P (mode "all") and R <= P (mode "shared") for any words - popcount 0, 1 (the case that reaches T rows with a
    shared row among them) and more - and the count per position is the derived one"""
    gen = torch.Generator().manual_seed(5)
    for T in (2, 3, 5, 8):
        for P in (1, 7, 65, 394):
            for kind in ("any", "single", "zero_or_single", "full"):
                words = torch.randint(0, 1 << T, (P,), generator=gen)
                if kind == "single":
                    words = torch.ones(P, dtype=torch.int64) << torch.randint(0, T, (P,), generator=gen)
                elif kind == "zero_or_single":
                    words = torch.where(torch.rand(P, generator=gen) < 0.5, torch.zeros_like(words),
                                        torch.ones(P, dtype=torch.int64) << torch.randint(0, T, (P,), generator=gen))
                elif kind == "full":
                    words[:] = (1 << T) - 1
                words = words | (torch.randint(0, 4, (P,), generator=gen) << T)        # bits at and above T are ignored
                pc = sum(((words >> t) & 1) for t in range(T))
                for mode in TC.MODES:
                    w = TC.worklist(words, T, mode)
                    per = torch.where(pc <= 1, torch.full_like(pc, T), T - pc + 1) if mode == "all" else (pc > 0).long()
                    assert w["R"] == int(per.sum()) <= TC.rows_ub(P, T, mode)
                    if kind == "single":
                        assert w["R"] == TC.rows_ub(P, T, mode)
                    assert bool((per[pc >= 2] <= T - 1).all())


def test_worklist_enumeration():
    bits = torch.tensor([0b000, 0b011, 0b100, 0b111, 0b000], dtype=torch.int64)
    w = TC.worklist(bits, 3, "all")
    # segment 0: positions 0, 2, 4; segment 1: 0, 2, 4; segment 2: 0, 1, 4; segment 3 (shared): 1, 2, 3
    assert w["rows"].tolist() == [0, 2, 4, 5, 7, 9, 10, 11, 14, 16, 17, 18] and w["R"] == 12
    assert w["slot_of"].tolist() == [[0, -1, 1, -1, 2], [3, -1, 4, -1, 5], [6, 7, -1, -1, 8], [-1, 9, 10, 11, -1]]
    assert w["offsets"] == [0, 12] and w["tile_starts"] == [0, 1]
    s = TC.worklist(bits, 3, "shared")
    assert s["rows"].tolist() == [16, 17, 18] and s["slot_of"][:3].eq(-1).all() and s["slot_of"][3].tolist() == [-1, 0, 1, 2, -1]
    assert TC.worklist(torch.zeros(4, dtype=torch.int64), 2, "shared")["tile_starts"] == [0, 0]
    assert TC.worklist(torch.zeros(129, dtype=torch.int64), 2, "all")["tile_starts"] == [0, 3]


def test_degenerate_patterns_have_their_row_counts():
    for c in TC.degenerate_cases():
        I = TC.make_inputs(c)
        assert I["wl"]["R"] == TC.expected_rows(c), TC.case_id(c)
        assert not bool(I["sx"][I["bits"] == 0].count_nonzero())


def test_case_grid_covers_every_pair():
    cs = TC.stage_cases()
    assert {(c["T"], c["B"], c["N"]) for c in cs} == {(T, B, N) for T in (2, 3, 8) for B, N in ((1, 1), (1, 65), (2, 197))}
    assert {(c["C"], c["H"], c["dtype"]) for c in cs} == {(C, H, d) for C, H in ((192, 384), (384, 1536)) for d in ("f32", "f16", "bf16")}
    assert all(sum(TC.case_id(c) == TC.case_id(o) for o in cs) == 1 for c in cs)
    for c in cs:
        assert any(o["mode"] != c["mode"] and {**o, "mode": c["mode"]} == c for o in cs)


def _mlp(C=16, H=32, **kw):
    from m3vit_amd.vit import Mlp
    return Mlp(C, H, **kw)


def test_state_dict_keys_and_exports():
    import m3vit_amd
    from m3vit_amd.sharing import TokenFFNStage
    assert m3vit_amd.TokenFFNStage is TokenFFNStage
    norm2, mlp = torch.nn.LayerNorm(16, eps=1e-6), _mlp()
    st = TokenFFNStage(norm2, mlp, 3)
    assert list(st.state_dict()) == ["norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"]
    assert st.norm2 is norm2 and st.mlp is mlp and st.ffn is mlp and (st.mode, st.drop_path, st.num_tasks) == ("all", 0.0, 3)
    sh = TokenFFNStage(norm2, mlp, 3, mode="shared", drop_path=0.1)
    assert list(sh.state_dict()) == ["norm2.weight", "norm2.bias", "shared_ffn.fc1.weight", "shared_ffn.fc1.bias",
                                     "shared_ffn.fc2.weight", "shared_ffn.fc2.bias"]
    # a TokenBlock's keys load unchanged
    block = {"norm2.weight": torch.full((16,), 2.0), "norm2.bias": torch.zeros(16), "mlp.fc1.weight": torch.ones(32, 16),
             "mlp.fc1.bias": torch.zeros(32), "mlp.fc2.weight": torch.ones(16, 32), "mlp.fc2.bias": torch.zeros(16)}
    st.load_state_dict(block, strict=True)
    assert float(norm2.weight.detach()[0]) == 2.0


def test_refusals():
    from m3vit_amd import _lib
    from m3vit_amd.sharing import SharedTokens, TokenFFNStage
    E = _lib.M3Error
    ln = torch.nn.LayerNorm(16, eps=1e-6)
    for T in (1, 9):
        with pytest.raises(E, match="num_tasks"):
            TokenFFNStage(ln, _mlp(), T)
    with pytest.raises(E, match="mode"):
        TokenFFNStage(ln, _mlp(), 2, mode="private")
    with pytest.raises(E, match="GELU"):
        TokenFFNStage(ln, _mlp(act_layer=torch.nn.ReLU), 2)
    with pytest.raises(E, match="GELU"):
        TokenFFNStage(ln, _mlp(act_layer=lambda: torch.nn.GELU(approximate="tanh")), 2)
    with pytest.raises(E, match="multiples of 8"):
        TokenFFNStage(torch.nn.LayerNorm(12), _mlp(12, 24), 2)
    with pytest.raises(E, match="multiples of 8"):
        TokenFFNStage(ln, _mlp(16, 36), 2)
    with pytest.raises(E, match="at most 1024"):
        TokenFFNStage(torch.nn.LayerNorm(1032), _mlp(1032, 64), 2)
    with pytest.raises(E, match="residual FFN"):
        TokenFFNStage(torch.nn.LayerNorm(24), _mlp(), 2)
    with pytest.raises(E, match="drop_path"):
        TokenFFNStage(ln, _mlp(), 2, drop_path=1.0)
    outs = {t: torch.zeros(1, 4, 16) for t in range(2)}
    st = TokenFFNStage(ln, _mlp(drop=0.1), 2)
    with pytest.raises(E, match="drop.p=0.1"):
        st(outs)                                                        # training: element-wise dropout is not built here
    st.eval()
    with pytest.raises(E, match="GPU tensor"):
        st(outs)                                                        # eval: the dropout is off; CPU tensors have no path
    st2 = TokenFFNStage(ln, _mlp(), 2)
    with pytest.raises(E, match="GPU tensor"):
        st2(outs)
    with pytest.raises(E, match="num_tasks|GPU tensor"):
        st2({0: outs[0]})
    with pytest.raises((E, KeyError)):
        TokenFFNStage(ln, _mlp(), 3)(outs)                              # a task tensor is missing
    assert SharedTokens is not None


def test_c_abi_host_entries():
    from m3vit_amd import _lib, ops
    S = _lib.SIGNATURES
    names = ["m3_token_ffn_bwd_ws_elems", "m3_token_ffn_gather_bwd", "m3_token_ffn_list_ws_elems", "m3_token_ffn_ln_fwd",
             "m3_token_ffn_rows_ub", "m3_token_ffn_scatter_bwd", "m3_token_ffn_scatter_fwd", "m3_token_ffn_worklist"]
    assert sorted(n for n in S if n.startswith("m3_token_ffn_")) == names
    assert S["m3_token_ffn_ln_fwd"][1][0] is ctypes.POINTER(_lib.ShareRows) and S["m3_token_ffn_rows_ub"][0] is ctypes.c_int64
    assert (_lib.M3_TOKEN_FFN_ALL, _lib.M3_TOKEN_FFN_SHARED) == (0, 1) and ops.TOKEN_FFN_MODES == {"all": 0, "shared": 1}
    for P, T in ((394, 3), (25216, 2), (1, 8)):
        assert ops.token_ffn_rows_ub(P, T, "all") == TC.rows_ub(P, T, "all") == T * P
        assert ops.token_ffn_rows_ub(P, T, "shared") == TC.rows_ub(P, T, "shared") == P
        n = (T + 1) * P
        assert int(_lib.lib().m3_token_ffn_list_ws_elems(P, T)) == 3 * n + 4 + int(_lib.lib().m3_route_ws_elems(n, 1))
        assert ops.token_ffn_bwd_ws_elems(P, 384) == 2 * _lib.lib().m3_share_num_blocks(P) * 384
    with pytest.raises(_lib.M3Error, match="neither"):
        ops.token_ffn_rows_ub(4, 2, "private")
    # (T + 1) * B*N >= 2^31 is refused by the host code before any launch (no pointer is looked at)
    one = ctypes.c_void_p(16)
    L = _lib.lib()
    for P, T in (((1 << 31) // 3 + 1, 2), ((1 << 31) // 9 + 1, 8), (1 << 31, 2)):
        assert L.m3_token_ffn_worklist(one, P, T, 0, one, one, one, one, one, one, None) == _lib.M3_ERR_ARG
        assert b"2^31" in L.m3_last_error()
