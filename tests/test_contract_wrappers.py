"""GPU: every m3vit_amd.ops wrapper that hands tensors to the C ABI checks device, dtype, contiguity and size against its
partner tensors, and raises M3Error before anything is launched.  For each wrapper one valid call runs, then one tensor
at a time is replaced by a wrong-dtype, a non-contiguous and an undersized copy."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from m3vit_amd import ops as _ops
    return _ops


def _t(*shape, dtype=torch.float32):
    if dtype == torch.int32:
        return torch.zeros(*shape, dtype=dtype, device="cuda")
    return torch.randn(*shape, device="cuda").to(dtype)


F16 = torch.float16
T_, D_, K_ = 70, 64, 2
B_, N_, H_, DH_ = 2, 33, 2, 32
C_ = H_ * DH_


def _calls(ops):
    """name -> (factory of the keyword tensors, call, the tensors to corrupt)"""
    return {
        "layernorm_fwd": (lambda: dict(x=_t(T_, D_), gamma=_t(D_), beta=_t(D_), y=_t(T_, D_, dtype=F16), mean=_t(T_), rstd=_t(T_)),
                          lambda a: ops.layernorm_fwd(**a), ("x", "gamma", "y", "mean", "rstd")),
        "layernorm_bwd": (lambda: dict(dy=_t(T_, D_, dtype=F16), x=_t(T_, D_), mean=_t(T_), rstd=_t(T_).abs(), gamma=_t(D_),
                                       dx_res=_t(T_, D_), dx=_t(T_, D_), dgamma=_t(D_), dbeta=_t(D_)),
                          lambda a: ops.layernorm_bwd(**a), ("dy", "x", "mean", "rstd", "gamma", "dx_res", "dx", "dgamma")),
        "attention_fwd": (lambda: dict(qkv=_t(B_ * N_, 3 * C_, dtype=F16), o=_t(B_ * N_, C_, dtype=F16), lse=_t(B_, H_, N_)),
                          lambda a: ops.attention_fwd(a["qkv"], B_, N_, H_, DH_, a["o"], a["lse"]), ("qkv", "o", "lse")),
        "attention_bwd": (lambda: dict(qkv=_t(B_ * N_, 3 * C_, dtype=F16) * 0.1, o=_t(B_ * N_, C_, dtype=F16),
                                       d_o=_t(B_ * N_, C_, dtype=F16), lse=_t(B_, H_, N_).abs() + 4,
                                       dqkv=_t(B_ * N_, 3 * C_, dtype=F16)),
                          lambda a: ops.attention_bwd(a["qkv"], a["o"], a["d_o"], a["lse"], B_, N_, H_, DH_, a["dqkv"]),
                          ("qkv", "o", "d_o", "lse", "dqkv")),
        "combine_fwd": (lambda: dict(y=_t(T_ * K_, D_, dtype=F16), score=_t(T_, K_), residual=_t(T_, D_), out=_t(T_, D_)),
                        lambda a: ops.combine_fwd(**a), ("y", "score", "residual", "out")),
        "combine_bwd": (lambda: dict(dout=_t(T_, D_), y=_t(T_ * K_, D_, dtype=F16), score=_t(T_, K_), dy=_t(T_ * K_, D_, dtype=F16),
                                     dscore=_t(T_, K_)),
                        lambda a: ops.combine_bwd(**a), ("dout", "y", "score", "dy", "dscore")),
        "combine_gate_bwd": (lambda: dict(dxe=_t(T_ * K_, D_, dtype=F16), d_logits=_t(T_, 8), w_gate=_t(D_, 8), dh=_t(T_, D_)),
                             lambda a: ops.combine_gate_bwd(a["dxe"], K_, a["d_logits"], a["w_gate"], a["dh"]),
                             ("dxe", "d_logits", "w_gate", "dh")),
        "gather_rows": (lambda: dict(src=_t(T_, D_, dtype=F16), idx=_t(T_ * K_, dtype=torch.int32), dst=_t(T_, D_, dtype=F16)),
                        lambda a: ops.gather_rows(a["src"], a["idx"], a["dst"], div=1, k=K_), ("src", "idx", "dst")),
        "cast_matrix": (lambda: dict(src=_t(3, 40, 24), dst=_t(3, 24, 40, dtype=F16)),
                        lambda a: ops.cast_matrix(a["src"], a["dst"], transpose=True), ("src", "dst")),
        "cast_f32": (lambda: dict(src=_t(T_, D_), dst=_t(T_, D_, dtype=F16)), lambda a: ops.cast_f32(**a), ("src", "dst")),
        "scale_rows_cast": (lambda: dict(src=_t(T_, D_), row_scale=_t(T_), dst=_t(T_, D_, dtype=F16)),
                            lambda a: ops.scale_rows_cast(a["src"], a["row_scale"], 1, a["dst"]), ("src", "row_scale", "dst")),
        "im2row": (lambda: dict(img=_t(2, 3, 32, 32), rows=_t(2 * 4, 3 * 16 * 16, dtype=F16)),
                   lambda a: ops.im2row(a["img"], 16, a["rows"]), ("img", "rows")),
        "assemble_tokens": (lambda: dict(patch=_t(2 * 4, D_), cls=_t(D_), pos=_t(5, D_), tokens=_t(2, 5, D_)),
                            lambda a: ops.assemble_tokens(a["patch"], a["cls"], a["pos"], 2, 4, D_, a["tokens"]),
                            ("patch", "cls", "pos", "tokens")),
        "tokens_bwd": (lambda: dict(dtok=_t(2, 5, D_), dpatch=_t(2 * 4, D_, dtype=F16), dpos=_t(5, D_), dcls=_t(D_)),
                       lambda a: ops.tokens_bwd(a["dtok"], 2, 4, D_, a["dpatch"], a["dpos"], a["dcls"]),
                       ("dtok", "dpatch", "dpos", "dcls")),
        "colsum": (lambda: dict(dC=_t(T_, D_, dtype=F16), db=_t(D_)), lambda a: ops.colsum(a["dC"], a["db"]), ("dC", "db")),
        "add_f32": (lambda: dict(dst=_t(T_ * D_), src=_t(T_ * D_)), lambda a: ops.add_f32(**a), ("dst", "src")),
        "gate_bwd_params": (lambda: dict(x=_t(T_, D_, dtype=F16), w_gate=_t(D_, 8), d_logits=_t(T_, 8), d_w_gate=_t(D_, 8),
                                         dx=_t(T_, D_)),
                            lambda a: ops.gate_bwd_params(a["x"], a["w_gate"], a["d_logits"], d_w_gate=a["d_w_gate"], dx=a["dx"]),
                            ("x", "w_gate", "d_logits", "d_w_gate", "dx")),
        "gate_fwd": (lambda: dict(x=_t(T_, D_, dtype=F16), w_gate=_t(D_, 8), logit_bias=_t(8), noise=_t(T_, 8),
                                  loss_acc=_t(1)),
                     lambda a: ops.gate_fwd(a["x"], a["w_gate"], K_, logit_bias=a["logit_bias"], noise=a["noise"],
                                            noise_std=0.1, loss_acc=a["loss_acc"]),
                     ("x", "w_gate", "logit_bias", "noise")),
        "gate_bwd_logits": (lambda: dict(noisy=_t(T_, 8), clean=_t(T_, 8), top_logits=_t(T_, K_ + 1).abs(),
                                         idx=torch.arange(K_, device="cuda").repeat(T_, 1),
                                         idx_next=torch.full((T_,), K_, dtype=torch.int32, device="cuda"),
                                         d_score=_t(T_, K_), d_top=_t(T_, K_ + 1), d_importance=_t(8), d_load_prob=_t(8),
                                         out=_t(T_, 8), out_act=_t(T_, 8, dtype=F16), balance_scale_dev=_t(1)),
                            lambda a: ops.gate_bwd_logits(a["noisy"], a["idx"], a["d_score"], a["d_importance"], K_,
                                                          d_top=a["d_top"], idx_next=a["idx_next"],
                                                          d_load_prob=a["d_load_prob"], clean=a["clean"],
                                                          top_logits=a["top_logits"], noise_std=0.5, out=a["out"],
                                                          balance_scale_dev=a["balance_scale_dev"], out_act=a["out_act"]),
                            ("noisy", "clean", "top_logits", "idx", "idx_next", "d_score", "d_top", "d_importance",
                             "d_load_prob", "out", "out_act")),
        "ep_plan": (lambda: dict(send=torch.full((3 * 4,), 5, dtype=torch.int64, device="cuda"),
                                 recv=torch.full((3 * 4,), 7, dtype=torch.int64, device="cuda"),
                                 buf=torch.zeros(3 * 4 * 7, dtype=torch.int32, device="cuda")),
                    lambda a: ops.ep_plan(a["send"], a["recv"], 3, 4, a["buf"]), ("send", "recv", "buf")),
        "layernorm_bwd_reduce": (lambda: dict(ws=_t(3, 2, ops.lib().m3_ln_bwd_blocks(T_, D_), D_)),
                                 lambda a: ops.layernorm_bwd_reduce(a["ws"], ops.lib().m3_ln_bwd_blocks(T_, D_), D_,
                                                                    ops.LnGradTable([(_t(D_), _t(D_)) for _ in range(3)], "cuda"),
                                                                    0, 3, beta=0), ("ws",)),
        "relu_up2x_fwd": (lambda: dict(x=_t(2, 5, 7, 16, dtype=F16).permute(0, 3, 1, 2)),
                          lambda a: ops.relu_up2x_fwd(a["x"]), ("x",)),
        "relu_up2x_bwd": (lambda: dict(dy=_t(2, 10, 14, 16, dtype=F16).permute(0, 3, 1, 2),
                                       x=_t(2, 5, 7, 16, dtype=F16).permute(0, 3, 1, 2)),
                          lambda a: ops.relu_up2x_bwd(a["dy"], a["x"]), ("dy", "x")),
    }


def _wrong_dtype(t):
    return t.to(torch.int64 if t.dtype == torch.int32 else torch.float64)      # no entry point takes either


def _non_contiguous(t):
    wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)[..., ::2]
    wide.copy_(t)
    assert not wide.is_contiguous()
    return wide


def _undersized(t):
    return t[:-1].clone() if t.shape[0] > 1 else t.flatten()[:-1]          # (clone keeps a channels-last layout)


# tensors whose row count the call takes from the tensor itself (or reads through device-resident indices): any size is valid
UNSIZED = {("gather_rows", "src"), ("gather_rows", "dst"), ("colsum", "dC"), ("relu_up2x_fwd", "x")}
NAMES = list(_calls(None).keys())


@pytest.mark.parametrize("name", NAMES)
def test_wrappers_reject_bad_tensors_before_launch(ops, name):
    make, call, targets = _calls(ops)[name]
    call(make())                                   # the valid call is accepted
    torch.cuda.synchronize()
    for tgt in targets:
        for bad in (_wrong_dtype, _non_contiguous, _undersized):
            args = make()
            if bad is _undersized and (name, tgt) in UNSIZED:
                continue
            args[tgt] = bad(args[tgt])
            with pytest.raises(ops._lib.M3Error):
                call(args)
            torch.cuda.synchronize()
    args = make()
    args[targets[0]] = args[targets[0]].cpu()
    with pytest.raises(ops._lib.M3Error):
        call(args)


def test_one_element_operands_are_sized(ops):
    """loss_acc and balance_scale_dev must hold exactly one f32 (the column trick of _non_contiguous does not apply)"""
    x, w = _t(T_, D_, dtype=F16), _t(D_, 8)
    with pytest.raises(ops._lib.M3Error):
        ops.gate_fwd(x, w, K_, loss_acc=_t(2))
    with pytest.raises(ops._lib.M3Error):
        ops.gate_fwd(x, w, K_, loss_acc=_t(1, dtype=torch.float16))
    idx = torch.arange(K_, device="cuda").repeat(T_, 1)
    with pytest.raises(ops._lib.M3Error):
        ops.gate_bwd_logits(_t(T_, 8), idx, _t(T_, K_), _t(8), K_, balance_scale_dev=_t(2))
    with pytest.raises(ops._lib.M3Error):
        ops.gate_bwd_logits(_t(T_, 8), idx.int(), _t(T_, K_), _t(8), K_)          # int32 idx is not reinterpreted
