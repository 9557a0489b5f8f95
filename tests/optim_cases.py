"""Inputs, float64 references and error bounds shared by tests/test_optim_cpu.py and tests/test_optim_gpu.py (imported by
them; nothing here runs by itself).

Yardstick: torch.optim.{AdamW, Adam, SGD}(foreach=False) in float64 on the CPU, from the same fp32 inputs.
Bound per element after s steps: 4 s 2^-24 (|p_ref| + lr_group) for a parameter, and the same form with the tensor's largest
|g| in place of lr for exp_avg, exp_avg_sq and momentum_buffer.  The CPU test asserts that torch's own fp32 optimizers stay
inside these bounds on exactly these inputs, so a bound the reference arithmetic breaks is found without a GPU."""
import functools

import torch

U32 = 2.0 ** -24
# 1, 3, 4, 5: below / at / above one float4; 384, 1000: one partial chunk; 4095 .. 4097: around one 4096-element chunk;
# 3 x 4096 + 2: several chunks and a 2-element tail; 197 x 384: a pos_embed, 19 chunks.  In this order and packed without
# padding the gradient views start at element offsets 0 1 2 1 1 1 0 0 1 1 3 mod 4: 384 and 4097 (a whole chunk, then a chunk
# that holds one element only) take the 16-byte path, the others the scalar one.
SIZES = (1, 5, 3, 4, 1000, 4095, 384, 4097, 4096, 3 * 4096 + 2, 197 * 384)
STEPS = 3
ZERO_PARAM = 6                      # the 384-element tensor starts at exactly 0 (a bias): there the bound is 4 s u lr alone

KINDS = {
    "adamw": (torch.optim.AdamW, dict(lr=1e-3, weight_decay=0.05)),
    "adamw_nodecay": (torch.optim.AdamW, dict(lr=1e-3, weight_decay=0.0)),
    "adam": (torch.optim.Adam, dict(lr=1e-3, weight_decay=0.05)),
    "sgd": (torch.optim.SGD, dict(lr=1e-3, momentum=0.9, weight_decay=1e-4, nesterov=False)),
    "sgd_nesterov": (torch.optim.SGD, dict(lr=1e-3, momentum=0.9, weight_decay=1e-4, nesterov=True)),
}
STATE_KEYS = {torch.optim.AdamW: ("exp_avg", "exp_avg_sq"), torch.optim.Adam: ("exp_avg", "exp_avg_sq"),
              torch.optim.SGD: ("momentum_buffer",)}


@functools.lru_cache(maxsize=None)
def inputs(seed=0, sizes=SIZES, steps=STEPS, lo=-6.0, hi=1.0):
    """(params, grads[step]) as CPU fp32 tensors: parameters ~ 0.5 N(0, 1), gradient magnitudes spread over 10^lo .. 10^hi"""
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=g) * 0.5 for n in sizes]
    if len(params) > ZERO_PARAM:
        params[ZERO_PARAM].zero_()
    grads = [[torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * (hi - lo) + lo) for n in sizes]
             for _ in range(steps)]
    return params, grads


def two_groups(n):
    """tensor i belongs to group i % 2: the groups interleave in descriptor order"""
    return [i % 2 for i in range(n)]


def run_torch(cls, group_kw, params, grads, dtype, group_of=None, clip=None, lr_change=None):
    """`len(grads)` steps of a torch optimizer (foreach=False) in `dtype` on the CPU.
    group_kw: one dict of hyper-parameters per group; group_of[i]: the group of tensor i (default all 0);
    clip: torch.nn.utils.clip_grad_norm_(.., clip) before every step; lr_change: (step index, group, new lr) applied
    before that step.  Returns a list over steps of {"p": [...], state key: [...], "norm": clip_grad_norm_'s result}."""
    group_of = group_of or [0] * len(params)
    ps = [torch.nn.Parameter(p.detach().to(dtype).clone()) for p in params]
    groups = [dict(params=[p for p, g in zip(ps, group_of) if g == gi], **kw) for gi, kw in enumerate(group_kw)]
    opt = cls(groups, foreach=False)
    out = []
    for s, gs in enumerate(grads):
        if lr_change is not None and lr_change[0] == s:
            opt.param_groups[lr_change[1]]["lr"] = lr_change[2]
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.detach().to(dtype).clone()        # None: the parameter sits the step out
        norm = torch.nn.utils.clip_grad_norm_(ps, clip, foreach=False) if clip is not None else None
        opt.step()
        rec = {"p": [p.detach().clone() for p in ps], "norm": norm}
        for key in STATE_KEYS[cls]:
            rec[key] = [opt.state[p][key].detach().clone() if key in opt.state[p] else None for p in ps]
        out.append(rec)
    return out, opt


def param_bound(p_ref, lr, s):
    return 4 * s * U32 * (p_ref.double().abs() + lr)


def state_bound(ref, gmax, s):
    return 4 * s * U32 * (ref.double().abs() + gmax)


def gmax_of(grads, i, s, factor=1.0):
    """largest |g| tensor i has seen in steps 0 .. s"""
    return factor * max(float(grads[t][i].abs().max()) for t in range(s + 1))


def check_run(got, ref, grads, group_kw, group_of, cls, what, lrs=None, worst=None):
    """got, ref: lists over steps as run_torch returns them (got in any dtype / on any device).  Asserts every parameter
    and state tensor inside its bound; returns the worst err / bound ratio."""
    import kernel_contract as kc
    w = 0.0
    for s, (a, r) in enumerate(zip(got, ref)):
        for i, (pa, pr) in enumerate(zip(a["p"], r["p"])):
            lr = (lrs[s] if lrs is not None else [kw["lr"] for kw in group_kw])[group_of[i]]
            w = max(w, kc.assert_within(pa, pr, param_bound(pr, lr, s + 1), f"{what}: p[{i}] after step {s + 1}"))
            for key in STATE_KEYS[cls]:
                w = max(w, kc.assert_within(a[key][i], r[key][i], state_bound(r[key][i], gmax_of(grads, i, s), s + 1),
                                            f"{what}: {key}[{i}] after step {s + 1}"))
    if worst is not None:
        worst[what] = w
    return w


# ---------------------------------------------------------------------------------------------- the cases both tests run
CASES = {
    "adamw": dict(kind="adamw"),
    "adam": dict(kind="adam"),
    # SGD: gradients up to 0.1.  The bound's absolute term is lr: it covers an update of the order of lr, which Adam's
    # normalised update always is.  SGD's update is lr |buf|; where it cancels most of |p| the result's error, a few
    # u lr |buf|, is set against 4 s u (|p_ref| + lr) with |p_ref| small, so the bound holds for |buf| up to about 1
    # (three steps of |g| <= 0.45) and not for |buf| of 30 (measured: torch fp32 at 1.3 x the bound with gradients up to 10)
    "sgd": dict(kind="sgd", inputs=dict(seed=2, hi=-1.0)),
    "sgd_nesterov": dict(kind="sgd_nesterov", inputs=dict(seed=2, hi=-1.0)),
    # two groups interleaved in descriptor order: no decay against 0.05, lr x 100; group 0's lr halves before step 3
    "groups": dict(kind="adamw", group_kw=[dict(lr=1e-3, weight_decay=0.0), dict(lr=1e-1, weight_decay=0.05)],
                   interleave=True, lr_change=(2, 0, 5e-4)),
    # max_norm below the norm (about 1100 on these inputs) clips every step.  Gradients from 1e-3 up here: where a clipped
    # |g| comes down to eps = 1e-8 the update lr g / (|g| + eps) is proportional to the clip coefficient and inherits the
    # relative error of the norm - a sum of 1e5 fp32 squares, n u and not 4 u, in torch's own fp32 clip_grad_norm_ as in any
    # other (measured: torch fp32 at 1.3 x the bound on the 1e-6 .. 10 inputs clipped to 1); five decades above eps the
    # update is scale-free again and the bound is about the optimizer, which is what this case is for
    "clip": dict(kind="adamw", clip=100.0, inputs=dict(seed=1, lo=-3.0)),
}
# The norm of many chunks: inputs(**MANY_CHUNKS_INPUTS) is 303 chunks, so the one-workgroup finalize launch, whose 256 threads
# add the norm partials t, t + 256, ..., goes round twice, the second time raggedly (47), and the last chunk's tail is no
# multiple of 4; every case above has 33 partials.  It is no entry of CASES, because only its NORM is checked (against float64:
# test_clip_matches_clip_grad_norm_then_step).  The per-element bounds above are not kept at this size by torch's own fp32
# optimizer - measured over four seeds, AdamW with and without decay: worst err / bound 0.95 .. 1.21 after one step, one or
# two elements of 1.2 M past it - and torch's fp32 clip_grad_norm_ is 6e-5 off here, which a clipped update would inherit.
MANY_CHUNKS_INPUTS = dict(seed=3, sizes=(5, 4097, 300 * 4096 - 5), steps=1)


def inputs_of(name):
    return inputs(**CASES[name].get("inputs", {}))


def case(name):
    """(torch class, [hyper-parameters per group], group of each tensor, clip, lr_change, lrs); lrs[s][group] is the lr the
    bound after step s + 1 takes: the largest the group has stepped with so far (each step adds an error of its own lr's size)"""
    c = CASES[name]
    cls, kw = KINDS[c["kind"]]
    group_kw = c.get("group_kw", [kw])
    group_of = two_groups(len(SIZES)) if c.get("interleave") else [0] * len(SIZES)
    lrs = []
    cur = [g["lr"] for g in group_kw]
    for s in range(STEPS):
        if c.get("lr_change") and c["lr_change"][0] == s:
            cur = list(cur)
            cur[c["lr_change"][1]] = c["lr_change"][2]
        lrs.append([max(a, b) for a, b in zip(cur, lrs[-1])] if lrs else list(cur))
    return cls, group_kw, group_of, c.get("clip"), c.get("lr_change"), lrs


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 run of a case: computed once per process, shared by every test that needs it, never modified"""
    cls, group_kw, group_of, clip, lr_change, _ = case(name)
    params, grads = inputs_of(name)
    ref, _ = run_torch(cls, group_kw, params, grads, torch.float64, group_of, clip, lr_change)
    return ref
