"""Generate tests/golden/g15_token_ffn.npz from the reference's OWN code for step 5 of TokenBlock.forward.  Run where a
reference checkout is available; not collected by pytest:

    python tests/gen_golden_token_ffn.py /path/to/reference        (or M3VIT_REFERENCE=/path/to/reference)

The reference code that runs (never copied; only its INPUTS and OUTPUTS are stored), all in float64 on the CPU:
  models/moe/token/vision_transformer_moe.py  TokenBlock.dense_mlp_stage, TokenBlock.shared_dense_forward,
      TokenBlock.apply_shared_broadcast and TokenBlock._shared_drop_path, called unbound on a types.SimpleNamespace carrying
      num_tasks, training, norm2 (an nn.LayerNorm(C, eps=1e-6)), mlp, drop_path and _shared_drop_path - all they use of self;
      the module imports with the placeholders of gen_golden_sharing.py (its reference_modules() is what imports it)
  models/moe/token/layers.py                  Mlp (the namespace's mlp), DropPath (the training case's drop_path)
Mode "shared" (the shared branch of an MoE block, vision_transformer_moe.py:1002-1014) is an expression inside
TokenBlock.forward, not a method: shared_x + self.drop_path(self.shared_ffn(self.norm2(shared_x))).  shared_dense_forward is
the same expression over self.mlp, so those cases call it with the namespace's mlp standing for shared_ffn, skip
dense_mlp_stage (the private rows are the router's) and broadcast.

Drop path.  The reference's draws CAN be recorded by wrapping its two sources: _shared_drop_path returns its per-sample mask
(the wrapper keeps mask / keep_prob: path_scale [B]), and DropPath.forward draws keep_prob + rand(K, 1) for the compact [K, C]
tensor (the wrapper saves torch's generator state, lets the reference draw, then replays the same draw from the saved state
and restores the state after the call: shared_path_scale, scattered to [P], 1 where nothing is shared).  One training case
carries them, key suffix "/train".

Written, for every case c of token_ffn_cases.golden_cases() under the key k = token_ffn_cases.case_id(c) (+ "/train"):
  {k}/xs f32 [T,P,C], {k}/bits i64 [P], {k}/sx f32 [P,C] (dense, zero rows where bits == 0), {k}/gamma, beta, w1, b1, w2, b2 f32,
  {k}/y f64 [T,P,C], and the gradients of sum(cy * y), cy = token_ffn_cases.functional(c): {k}/d_xs f64 [T,P,C], {k}/d_sx f64
  [P,C], {k}/d_gamma .. {k}/d_b2 f64;  the training case also {k}/path_scale f64 [B], {k}/shared_path_scale f64 [P].
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_sharing as GS                    # noqa: E402  (checks the reference path, holds the placeholders)
import token_ffn_cases as TC                       # noqa: E402

OUT = os.path.join(HERE, "golden", "g15_token_ffn.npz")
F64 = torch.float64
DROP = 0.25


class _RecordedDropPath:
    """the reference's DropPath module, its factor recorded at every call"""

    def __init__(self, module):
        self.module, self.drop_prob, self.factors = module, module.drop_prob, []

    def __call__(self, x):
        state = torch.get_rng_state()
        out = self.module(x)
        after = torch.get_rng_state()
        torch.set_rng_state(state)                                      # the same draw, from the same generator state
        keep = 1 - self.drop_prob
        draw = torch.rand((x.shape[0],) + (1,) * (x.ndim - 1), dtype=x.dtype)
        torch.set_rng_state(after)
        factor = torch.floor(keep + draw) / keep
        assert torch.equal(out, x.div(keep) * torch.floor(keep + draw)), "the replayed draw is not the reference's"
        self.factors.append(factor.reshape(-1))
        return out


def one_case(c, RM, RLY, data, train=False, seed=97):
    k = TC.case_id(c) + ("/train" if train else "")
    T, B, N, C, H = c["T"], c["B"], c["N"], c["C"], c["H"]
    P = B * N
    I = TC.make_inputs(c, seed=200 + (7 if train else 0))
    xs = I["x64"].clone().requires_grad_(True)
    sx = I["sx64"].clone().requires_grad_(True)
    norm2 = torch.nn.LayerNorm(C, eps=TC.LN_EPS).double()
    mlp = RLY.Mlp(in_features=C, hidden_features=H).double()
    with torch.no_grad():
        for dst, name in ((norm2.weight, "gamma"), (norm2.bias, "beta"), (mlp.fc1.weight, "w1"), (mlp.fc1.bias, "b1"),
                          (mlp.fc2.weight, "w2"), (mlp.fc2.bias, "b2")):
            dst.copy_(I["p64"][name])
    ns = types.SimpleNamespace(num_tasks=T, training=train, norm2=norm2, mlp=mlp)
    masks = []
    if train:
        mlp.train()
        dp = RLY.DropPath(DROP)
        dp.train()
        ns.drop_path = _RecordedDropPath(dp)

        def shared_drop_path(x):
            out, mask = RM.TokenBlock._shared_drop_path(ns, x)
            masks.append(mask)
            return out, mask
        ns._shared_drop_path = shared_drop_path
        torch.manual_seed(seed)
    else:
        mlp.eval()
        ns.drop_path = torch.nn.Identity()
        ns._shared_drop_path = lambda x: RM.TokenBlock._shared_drop_path(ns, x)
    bits = I["bits"]
    flat_idx = (bits != 0).nonzero().squeeze(1)
    outs = {t: xs[t].view(B, N, C) for t in range(T)}
    if c["mode"] == "all":
        outs = RM.TokenBlock.dense_mlp_stage(ns, outs, shared_bits=bits.view(B, N))
    if flat_idx.numel():                                                # (TokenBlock.forward: `if shared_x is not None`)
        shared_out = RM.TokenBlock.shared_dense_forward(ns, sx[flat_idx])
        outs = RM.TokenBlock.apply_shared_broadcast(ns, outs=outs, shared_bits=bits.view(B, N), shared_x=shared_out,
                                                    shared_flat_idx=flat_idx)
    y = torch.stack([outs[t].reshape(P, C) for t in range(T)])
    (TC.functional(c) * y).sum().backward()
    data[f"{k}/xs"] = I["xs"].float().numpy()
    data[f"{k}/bits"] = bits.numpy()
    data[f"{k}/sx"] = I["sx"].float().numpy()
    for name in ("gamma", "beta", "w1", "b1", "w2", "b2"):
        data[f"{k}/{name}"] = I["params"][name].numpy()
    data[f"{k}/y"] = y.detach().numpy()
    data[f"{k}/d_xs"] = (torch.zeros_like(xs) if xs.grad is None else xs.grad).numpy()
    data[f"{k}/d_sx"] = (torch.zeros_like(sx) if sx.grad is None else sx.grad).numpy()
    for name, prm in (("gamma", norm2.weight), ("beta", norm2.bias), ("w1", mlp.fc1.weight), ("b1", mlp.fc1.bias),
                      ("w2", mlp.fc2.weight), ("b2", mlp.fc2.bias)):
        data[f"{k}/d_{name}"] = (torch.zeros_like(prm) if prm.grad is None else prm.grad).numpy()
    if train:
        assert len(masks) == 1 and len(ns.drop_path.factors) == (1 if flat_idx.numel() else 0)
        data[f"{k}/path_scale"] = (masks[0].reshape(-1) / (1.0 - DROP)).numpy()
        sps = torch.ones(P, dtype=F64)
        if flat_idx.numel():
            sps[flat_idx] = ns.drop_path.factors[0]
        data[f"{k}/shared_path_scale"] = sps.numpy()
        return bool((data[f"{k}/path_scale"] == 0).any()) and bool((data[f"{k}/shared_path_scale"] == 0).any())
    return True


def main():
    _, _, _, RM = GS.reference_modules()
    import models.moe.token.layers as RLY
    data = {}
    for c in TC.golden_cases():
        one_case(c, RM, RLY, data)
    for seed in range(97, 97 + 64):                                     # the first seed whose draws drop a sample AND a shared row
        tmp = {}
        if one_case(TC.golden_train_case(), RM, RLY, tmp, train=True, seed=seed):
            data.update(tmp)
            break
    else:
        raise AssertionError("no seed whose recorded draws contain a factor of 0 on both paths")
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {len(data)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
