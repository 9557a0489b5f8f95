"""Generate tests/golden/g14_sharing.npz from the reference's OWN sharing code.  Run where a reference checkout is available;
not collected by pytest:

    python tests/gen_golden_sharing.py /path/to/reference        (or M3VIT_REFERENCE=/path/to/reference)

The reference code that runs (never copied; only its INPUTS and OUTPUTS are stored), all in float64 on the CPU:
  models/moe/token/shareability.py          ShareabilityPredictor, Aggregation
  models/moe/aggregation_stages.py          AggregationStage
  models/moe/token/sharing_loss.py          SharingRegularizationLoss
  models/moe/token/vision_transformer_moe.py  TokenBlock.transition_stage, TokenBlock.apply_shared_broadcast, called unbound
      on a types.SimpleNamespace(num_tasks=T) (both use nothing else of self); the module imports with cv2, timm,
      timm.layers and tree as tripwire placeholders and fmoe = this repository's shim, as tests/gen_golden.py does.

The Gumbel draws: torch is seeded before the reference's predictor calls, the same draws are regenerated with the same seed
and call sequence, the closed form with those draws is asserted equal to the reference's output, and the draws are stored.

Written, for every case c of sharing_cases.golden_cases() under the key k = sharing_cases.case_id(c):
  {k}/xs f32 [T,P,D], {k}/w_gate f32, {k}/task_emb f32 [T,Dg] (absent when Dg = 0), {k}/noise f64 [T,P,2], {k}/prev i64 [P]
  {k}/G f64 [T,P] (the predictor's outputs), {k}/bits i64 [P], {k}/flat_idx i64 [K], {k}/shared_x f64 [K,D] (K may be 0:
  the reference returned None), {k}/y f64 [T,P,D] (after apply_shared_broadcast), {k}/stats i64 [6] (shared_positions,
  shared_tasktoken_count, partial_split_count, partial_split_total, shared_bits_flip_count, shared_bits_flip_total),
  {k}/loss f32 (SharingRegularizationLoss(0.01) of bits), and the gradients of the functional sharing_cases.functional(c)
  - sum(cy * y) + sum(cs[flat_idx] * shared_x) + sum(cg * G) - as {k}/d_xs, {k}/d_w_gate, {k}/d_task_emb;
  {k}/agg_masks bool [T,P], {k}/agg_need bool [P], {k}/agg f64 [P,D] (Aggregation; zeros where it returned None),
  {k}/agg_y f64 [T,P,D] (AggregationStage), {k}/agg_d_xs: the gradient of sum(cy * agg_y) + sum(cs * agg).
"""
import os
import sys
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("M3VIT_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "models", "moe", "token")):
    raise SystemExit("usage: python tests/gen_golden_sharing.py /path/to/reference (a checkout with models/moe/token/)")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, HERE)
import sharing_cases as SC                         # noqa: E402

OUT = os.path.join(HERE, "golden", "g14_sharing.npz")
F64 = torch.float64


class _Tripwire:
    def __init__(self, name):
        object.__setattr__(self, "_name", name)

    def _boom(self, *a, **k):
        raise RuntimeError(f"placeholder attribute {self._name} was used: the fixture would not be the reference's output")
    __call__ = __getattr__ = __getitem__ = __iter__ = __mul__ = __add__ = __bool__ = _boom


class _Placeholder(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return _Tripwire(self.__name__ + "." + k)


def reference_modules():
    import importlib.machinery
    for n in ("cv2", "timm", "timm.layers", "tree"):
        if n not in sys.modules:
            m = _Placeholder(n)
            m.__path__ = []
            m.__spec__ = importlib.machinery.ModuleSpec(n, None)
            sys.modules[n] = m
    sys.path.insert(0, os.path.dirname(HERE))
    import m3vit_amd
    m3vit_amd.install_fmoe_shim()
    import models.moe.token.shareability as RS
    import models.moe.token.sharing_loss as RL
    import models.moe.aggregation_stages as RA
    import models.moe.token.vision_transformer_moe as RM
    return RS, RL, RA, RM


def one_case(c, RS, RL, RA, RM, data):
    k = SC.case_id(c)
    T, B, N, D, Dg = c["T"], c["B"], c["N"], c["D"], c["Dg"]
    P = B * N
    for attempt in range(SC.MAX_DRAWS):
        I = SC.make_inputs(c, seed=100 + attempt)
        xs = I["x64"].clone().requires_grad_(True)
        emb = None if Dg == 0 else I["e64"].clone().requires_grad_(True)
        pred = RS.ShareabilityPredictor(D, Dg, temperature=c["tau"], hard=c["hard"]).double()
        with torch.no_grad():
            pred.w_gate.copy_(I["w64"])
        pred.train()                                                   # training: hard = self.hard
        torch.manual_seed(4242 + attempt)
        outs = {t: xs[t].view(B, N, D) for t in range(T)}
        g_shared = {t: pred(outs[t], task_emb=None if emb is None else emb[t]) for t in range(T)}
        torch.manual_seed(4242 + attempt)                               # the same draws, in the same call sequence
        noise = torch.stack([-torch.empty(P, 2, dtype=F64).exponential_().log() for _ in range(T)])
        G = torch.stack([g_shared[t].reshape(-1) for t in range(T)])
        closed = torch.stack([SC.predictor(I["x64"][t], I["w64"], None if emb is None else I["e64"][t], noise[t], c["tau"],
                                           c["hard"])[0] for t in range(T)])
        assert torch.allclose(closed, G.detach(), rtol=1e-12, atol=1e-14), "the regenerated Gumbel draws are not the reference's"
        ref = SC.stage(I["x64"], I["w64"], I["e64"], noise, c["tau"], c["hard"], c["gamma"], c["eps"], I["prev"])
        gb = SC.g_bound(I["x64"], I["w64"], I["e64"], noise, c["tau"])
        if bool(((ref["soft"] - 0.5).abs() >= torch.clamp(4 * gb, min=1e-4)).all()):
            break
    else:
        raise AssertionError(f"{k}: no separated draw")
    ns = types.SimpleNamespace(num_tasks=T)
    prev = None if I["prev"] is None else I["prev"].view(B, N)
    bits, shared_x, flat_idx, aux = RM.TokenBlock.transition_stage(ns, outs=dict(outs), prev_shared_bits=prev,
                                                                   g_shared=g_shared, gamma=c["gamma"], eps=c["eps"])
    outs2 = dict(outs)
    if shared_x is not None:
        outs2 = RM.TokenBlock.apply_shared_broadcast(ns, outs=outs2, shared_bits=bits, shared_x=shared_x,
                                                     shared_flat_idx=flat_idx)
    y = torch.stack([outs2[t].reshape(P, D) for t in range(T)])
    cy, cs, cg = SC.functional(c)
    f = (cy * y).sum() + (cg * G).sum()
    if shared_x is not None:
        f = f + (cs[flat_idx] * shared_x).sum()
    f.backward()
    loss = RL.SharingRegularizationLoss(0.01)(bits, T)
    data[f"{k}/xs"] = I["xs"].float().numpy()
    data[f"{k}/w_gate"] = I["w_gate"].numpy()
    if Dg:
        data[f"{k}/task_emb"] = I["task_emb"].numpy()
        data[f"{k}/d_task_emb"] = emb.grad.numpy()
    data[f"{k}/noise"] = noise.numpy()
    if I["prev"] is not None:
        data[f"{k}/prev"] = I["prev"].numpy()
    data[f"{k}/G"] = G.detach().numpy()
    data[f"{k}/bits"] = bits.reshape(-1).numpy()
    data[f"{k}/flat_idx"] = (torch.zeros(0, dtype=torch.int64) if flat_idx is None else flat_idx).numpy()
    data[f"{k}/shared_x"] = (torch.zeros(0, D, dtype=F64) if shared_x is None else shared_x.detach()).numpy()
    data[f"{k}/y"] = y.detach().numpy()
    st, an = aux["stats"], aux["analysis"]
    data[f"{k}/stats"] = np.array([st["shared_positions"], st["shared_tasktoken_count"], an["partial_split_count"],
                                   an["partial_split_total"], an["shared_bits_flip_count"], an["shared_bits_flip_total"]],
                                  dtype=np.int64)
    data[f"{k}/loss"] = np.float32(float(loss))
    data[f"{k}/d_xs"] = (torch.zeros_like(xs) if xs.grad is None else xs.grad).numpy()
    data[f"{k}/d_w_gate"] = pred.w_gate.grad.numpy()

    # Aggregation / AggregationStage on the same rows, masks of their own
    gen = torch.Generator().manual_seed(99)
    masks = torch.rand(T, P, generator=gen) < 0.6
    need = (masks.sum(0) >= 2) & (torch.rand(P, generator=gen) < 0.8)
    if c["pattern"] == "none":
        need = torch.zeros(P, dtype=torch.bool)
    xa = I["x64"].clone().requires_grad_(True)
    outs_a = {t: xa[t].view(B, N, D) for t in range(T)}
    mlist = [masks[t].view(B, N) for t in range(T)]
    agg_mod = RS.Aggregation()
    agg = agg_mod(outs_a, mlist, need.view(B, N))
    outs_b = RA.AggregationStage(agg_mod, T)(dict(outs_a), mlist, need.view(B, N))
    agg_y = torch.stack([outs_b[t].reshape(P, D) for t in range(T)])
    fa = (cy * agg_y).sum()
    if agg is not None:
        fa = fa + (cs * agg.reshape(P, D) * need.unsqueeze(-1)).sum()       # valid only where aggregation is needed
    fa.backward()
    data[f"{k}/agg_masks"] = masks.numpy()
    data[f"{k}/agg_need"] = need.numpy()
    data[f"{k}/agg"] = (torch.zeros(P, D, dtype=F64) if agg is None else (agg.reshape(P, D) * need.unsqueeze(-1)).detach()).numpy()
    data[f"{k}/agg_y"] = agg_y.detach().numpy()
    data[f"{k}/agg_d_xs"] = xa.grad.numpy()


def main():
    mods = reference_modules()
    data = {}
    for c in SC.golden_cases():
        one_case(c, *mods, data)
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {len(data)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
