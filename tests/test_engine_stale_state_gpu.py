"""GPU: no engine step reads stale scratch as the routing moves (the engine-level analogue of the kernel sentinel tests).

Every buffer a BackboneEngine / MultiTaskStep owns is torch.empty and reused for ever, and which rows, tiles and slab units
of the routed buffers are live is decided on the device by each step's routing.  Here the routing moves hard between steps,
everything a step may not read is poisoned before it (tests/engine_scratch.py: sentinel NaNs, integer metadata 0), and
every step must (1) be finite and meet the float64 oracle - per tensor and per EXPERT SLICE of the experts' gradients, a
dead expert's slice exactly zero -, (2) give the same bits whatever ran before it, (3) leave the poison where it had no
business writing, (4) under every weight-gradient launch plan.

CONFIGURATION (conditions asserted on the engine's own Route.counts every step - _geometry()):
  96 x 96 images, patch 16, batch 28: N = 37, T = 1036 (16 gate blocks of 64 + 12; 8 row tiles of 128 + 12); D = 64, 2 heads,
  depth 4 (MoE blocks 1 and 3 share the backward scratch), two task passes with a gate each (multi_gate), w_gate scaled by
  0.5 so that the steering offsets below leave second-choice scores of 0.05 .. 0.3 (a fp16 gradient row does not underflow).
  "noisy": E = 8, k = 2 (R = 2072, mean load 259), Hm = 128, vmoe_noisy_std = 1: the Normal-CDF load form; steered through
           the caller-supplied noises (engine and oracle scale them by 1 / E): E * N(0, 1) on every expert, + 4 E on the
           hot one, - 30 E on the dead ones.
  "bias":  E = 16, k = 4 (R = 4144, mean load 259), Hm = 64, no noise: the count load form; steered through the logit bias
           (MultiTaskStep.bind(logit_bias=) / tsf_bias; oracle.backbone_forward(logit_bias=)): + 4 hot, - 30 dead.
  steps A (no hot expert), B (hot 2, dead 5 and 6), C (hot 5, dead 0 and 3), A' = A's inputs bit for bit.
  Per-step counts, oracle seconds and worst errors: MEASURED at the end of this docstring.

WHAT THE WALK POISONS AND A STEP LEGITIMATELY REWRITES (every one of them is written before it is read in each step):
  activations act[i][*] (x_in aliases, h1, qkv, o, lse, x1, h2, mean / rstd, pre, u, hid_pre, hid, y, x2), rows, patch, x0, the
  backward scratch s_dxa, s_dxb, s_dx_t, s_dpre, s_dh, s_dh32, s_do, s_dqkv, s_dxe, s_dscore, s_dpatch, s_dl, s_dl_t, the
  workspaces ws_colsum, ws_ln, ws_gate_dw, ws_wgrad / WgradQueue.ws, cv_acc (zeroed by forward_begin), the gate's output
  dict and its Route (per call; fixed graph-pool buffers after capture), the backward cursor _bw.  Exempt, with reasons:
  engine_scratch.EXEMPT.  Check 3 asserts sentinel bits only on the weight-gradient slab workspaces past the largest slab
  need of any call of the step (include/m3vit_hip.h: a call's slabs are units * N * K (+ units * N) floats of ws; direct mode
  writes no slabs); ws_dq is not allocated at N <= 256 and s_dpre has no tail here (it is exactly max(T Hd, R Hm)); the
  slack slab units of a balanced call are not promised unwritten and are left out.

Tolerances are the ones the suite already uses: tokens 2e-4 (fp32) / F16_TOL (fp16) from tests/test_engine.py, 8e-3 (bf16)
from tests/test_fused_module_gpu.py and tests/test_modules_gpu.py; gradients GRAD_FACTOR times that, per tensor AND per
live expert slice; the balance loss 1e-3 max(1, |cv|) (tests/test_engine.py).

MEASURED (one MI355X; the oracle on that machine's host CPU, 16 threads; `pytest -s` prints all of it again):
  Route.counts per (task pass, MoE block), fp32 engine (16-bit runs move a few near-tied tokens, never a dead expert):
    noisy A  251..294 / 224..324 / 224..282 / 228..286 rows per expert (no expert under 224)
    noisy B  expert 2: 1025 / 1027 / 1012 / 1026 rows (8 row tiles + a partial one), experts 5 and 6: 0, the rest 173..255
    noisy C  expert 5: 1020 / 1027 / 1024 / 1021 rows, experts 0 and 3: 0, the rest 159..260
    bias A   198..361 rows per expert;  bias B  expert 2: 1036 (all tokens), 5 and 6: 0, the rest 165..369;
    bias C   expert 5: 1036, 0 and 3: 0, the rest 167..372.   A -> B -> C -> A': two experts die and two come back each time.
  oracle: 0.1 s per step (both task passes, forward + backward) on the GPU machine's host, 0.1 - 0.3 s on the development
    machine; the whole module (39 tests, ~60 oracle steps cached across runner kinds) runs in 11 s.
  worst errors over every runner kind and step, next to the reused bound (tokens | cv | worst tensor | worst expert slice):
    noisy fp32  5.0e-7 (2e-4) | 9.4e-8 (1e-3) | 9.5e-7 w_gate              | 7.7e-7 htoh4.weight[1], 422 rows   (6e-4)
    noisy fp16  2.9e-4 (1e-3) | 4.9e-6 (1e-3) | 7.1e-4 blocks.2.norm2.weight | 6.2e-4 h4toh.weight[1], 372 rows (3e-3)
    bias  fp32  5.1e-7 (2e-4) | 1.7e-7 (1e-3) | 9.5e-7 w_gate              | 9.7e-7 htoh4.bias[12], 479 rows    (6e-4)
    bias  fp16  2.9e-4 (1e-3) | 4.4e-6 (1e-3) | 7.6e-4 w_gate              | 6.2e-4 h4toh.weight[15], 484 rows  (3e-3)
    bias  bf16  2.4e-3 (8e-3) | 4.4e-5 (1e-3) | 5.6e-3 blocks.1.norm1.weight | 5.1e-3 htoh4.bias[14], 588 rows  (2.4e-2)
    module path fp32 5.0e-7 (2e-4) | worst tensor 9.6e-7, slice 1.0e-6 (1.3e-3);  fp16 2.9e-4 (1e-3) | 7.9e-4, 7.0e-4 (3.7e-3)
  No live slice here has fewer than 341 rows over the two passes (fp32 routing) and every one meets the tensor-level bound
  on its own: no floor for small slices is used.  Launch-plan variants against the default plan: fp32 within 1e-5; fp16
  within 4e-3 (largest seen: 3.2e-4 on blocks.3.mlp.experts.h4toh.weight with the LDS-DMA kernel forced and direct mode
  off - the call that scales its d x rows by the score, whose rounding to the operand dtype is the u_act term of
  tests/test_contract_wgrad.py's bound).
  Every bitwise check holds; no stale read was found in the engine.

THE CHECKS BITE (temporary Python-side edits of m3vit_amd/engine.py, each run once on [engine-noisy-fp32], none committed):
  (i)   forward_begin() without cv_acc.zero_(): under poison "step A: Inf / NaN in ['cv0', 'cv1']"; without poison the
        overflow test's check 2: "A after an overflowed step: cv of pass 0 differs (0.2004941999912262 vs 0.06683140248060226)".
  (ii)  backward_begin(): dx.add_(self.s_dxb, alpha=0.0) behind the copy - a stale scratch read masked by a zero factor:
        under poison "step A: Inf / NaN in ['blocks.3.norm1.weight', ... 'cls_token', 'pos_embed']" (every gradient);
        with the poison call switched off the same test PASSES - finite leftovers hide it, which is all the older tests had.
  (iii) block 3's FC2 weight-gradient call handed the PREVIOUS pass's Route.row_of_slot: tokens and every other tensor
        pass, "step A: gradients beyond 6e-04: [('blocks.3.mlp.experts.h4toh.weight', 0.92), ('blocks.3.mlp.experts.h4toh.
        weight[0] (528 rows)', 0.94), ... [6] (496 rows)', 0.86)]" (rel 3.4 when that Route had been poisoned to zeros).
"""
import time

import pytest
import torch

import engine_scratch as es
from test_engine import F16_TOL, GRAD_FACTOR, rel

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
TOL = {F32: 2e-4, F16: F16_TOL, BF16: 8e-3}
CVW = 0.01
B, IMG = 28, (96, 96)
TASKS, MOE = (0, 1), (1, 3)
PLAN = {"A": (None, ()), "B": (2, (5, 6)), "C": (5, (0, 3))}            # step -> (hot expert, dead experts)
HOT, DEAD = 4.0, -30.0                                                   # logit offsets
WORST = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------------------------------------ the cases
class Case:
    """configuration, parameters and the inputs of steps A, B, C (host tensors; A' is A)"""

    def __init__(self, name):
        from oracle import ref_torch as R
        self.name = name
        E, k, ratio, std = (8, 2, 2.0, 1.0) if name == "noisy" else (16, 4, 1.0, 0.0)
        self.cfg = R.BackboneCfg(img_size=IMG, embed_dim=64, depth=4, num_heads=2, mlp_ratio=4.0, moe_mlp_ratio=ratio,
                                 moe_experts=E, moe_top_k=k, gate_dim=66, multi_gate=True, vmoe_noisy_std=std)
        self.E, self.k = E, k
        self.T = B * self.cfg.num_tokens
        assert self.T % 64 and self.T % 128 and self.T * k / E > 128
        self.P = R.init_backbone_params(self.cfg, seed=17)
        for n in self.P:
            if n.endswith("w_gate"):
                self.P[n] = self.P[n] * 0.5
        self.steps = {}
        for j, (s, (hot, dead)) in enumerate(PLAN.items()):
            g = torch.Generator().manual_seed(500 + j)
            d = dict(img=torch.randn(B, 3, *IMG, generator=g), dtok=torch.randn(B, self.cfg.num_tokens, 64, generator=g) * 0.1,
                     noises=None, bias=None)
            off = torch.zeros(E)
            if hot is not None:
                off[hot] = HOT
                off[list(dead)] = DEAD
            if name == "noisy":                      # the gate adds noise * (vmoe_noisy_std / E): offsets are sized by E
                d["noises"] = {t: {i: (torch.randn(self.T, E, generator=g) + off) * E for i in MOE} for t in TASKS}
            else:
                d["bias"] = {i: off.clone() for i in MOE}
            self.steps[s] = d


_CASES, _ORACLE = {}, {}


def case_of(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def oracle_step(case, s, ovr=None):
    """float64 oracle of one step (both task passes, gradients of the summed loss); ovr: {task: {block: idx}} to follow.
    Cached: every runner kind of one dtype meets the same reference."""
    from oracle import ref_torch as R
    key = (case.name, s, None if ovr is None else tuple(hash(ovr[t][i].numpy().tobytes()) for t in TASKS for i in MOE))
    if key in _ORACLE:
        return _ORACLE[key]
    t0 = time.time()
    d = case.steps[s]
    Pr = {n: v.clone().double().requires_grad_() for n, v in case.P.items()}
    tot, toks, cvs, idx = 0.0, [], [], {}
    for t in TASKS:
        nz = None if d["noises"] is None else {i: v.double() for i, v in d["noises"][t].items()}
        lb = None if d["bias"] is None else {i: v.double() for i, v in d["bias"].items()}
        tok, cv, aux = R.backbone_forward(Pr, case.cfg, d["img"].double(), t, noises=nz, logit_bias=lb,
                                          route_override=None if ovr is None else ovr[t])
        tot = tot + (tok * d["dtok"].double()).sum() + CVW * cv
        toks.append(tok.detach()); cvs.append(float(cv.detach()))
        for i in MOE:
            idx[t, i] = aux[i]["idx"]
    tot.backward()
    out = dict(tok=toks, cv=cvs, idx=idx, grads={n: p.grad for n, p in Pr.items()}, seconds=time.time() - t0)
    _ORACLE[key] = out
    return out


# ---------------------------------------------------------------------------------------------------------- the runners
class Driver:
    """one executor of a case: kind "engine" (a BackboneEngine driven directly, the task passes one after the other and
    poisoned before EACH pass), "eager" (MultiTaskStep, one stream per pass) or "graph" (the same after capture()).  The
    inputs live in device tensors that are bound once and rewritten in place."""

    def __init__(self, case, kind, dtype, first="A", **kw):
        from m3vit_amd.engine import BackboneEngine
        from m3vit_amd.step import MultiTaskStep
        self.case, self.kind, self.dtype = case, kind, dtype
        a = case.steps[first]                      # what the bound tensors hold when a graph is captured
        self.img, self.dtok = a["img"].cuda(), a["dtok"].cuda()
        self.noises = None if a["noises"] is None else {t: {i: v.cuda() for i, v in a["noises"][t].items()} for t in TASKS}
        self.bias = None if a["bias"] is None else {i: v.cuda() for i, v in a["bias"].items()}
        if kind == "engine":
            self.obj = self.eng = BackboneEngine(case.cfg, case.P, batch=B, dtype=dtype, **kw)
        else:
            self.obj = self.run = MultiTaskStep(case.cfg, case.P, batch=B, dtype=dtype, cv_weight=CVW, tasks=list(TASKS), **kw)
            assert len(self.run.engs) == 2 and self.run.par
            self.run.bind(self.img, self.dtok, noises=self.noises, logit_bias=self.bias)
            self.eng = self.run.eng
            if kind == "graph":
                assert self.run.capture(), self.run.capture_error
                assert self.run.launch.startswith("hipGraph replay") and self.run.graphs is not None

    def load(self, s):
        d = self.case.steps[s]
        torch.cuda.synchronize()
        self.img.copy_(d["img"]); self.dtok.copy_(d["dtok"])
        if self.noises is not None:
            for t in TASKS:
                for i in MOE:
                    self.noises[t][i].copy_(d["noises"][t][i])
        if self.bias is not None:
            for i in MOE:
                self.bias[i].copy_(d["bias"][i])
        torch.cuda.synchronize()

    def _record(self, e, t, out):
        out["tok"].append(e.act[-1]["x2"].view(B, -1, 64).clone())
        out["cv"].append(e.cv_acc.clone())
        for i in MOE:
            out["idx"][t, i] = e.act[i]["gate"]["idx"].cpu()
            out["counts"][t, i] = e.act[i]["route"].counts.cpu().long()
            out["h2"][t, i] = e.act[i]["h2"].double().cpu()

    def step(self, s, poison=True, scale=None):
        """zero_grad, poison, the step on inputs s (scale: d_tokens multiplied in place first) -> its results, cloned"""
        self.load(s)
        if scale is not None:
            self.dtok.mul_(scale)
        out = dict(tok=[], cv=[], idx={}, counts={}, h2={})
        if self.kind == "engine":
            self.eng.zero_grad()
            for t in TASKS:
                if poison:
                    es.poison(es.scratch_tensors(self.eng))
                self.eng.forward(self.img, t, tsf_bias=self.bias, noises=None if self.noises is None else self.noises[t])
                torch.cuda.synchronize()
                self._record(self.eng, t, out)
                self.eng.backward(self.dtok, cv_weight=CVW)
            torch.cuda.synchronize()
        else:
            for e in self.run.engs:
                e.zero_grad()
            if poison:
                es.poison(es.scratch_tensors(self.run))
            self.run.step()
            torch.cuda.synchronize()
            for t, e in zip(TASKS, self.run.engs):
                self._record(e, t, out)
        out["flat"] = self.eng.flat_grads.clone()
        out["grads"] = {n: g.clone() for n, g in self.eng.grads.items()}
        return out


def same_bits(a, b, what=""):
    for j in range(len(TASKS)):
        assert torch.equal(a["tok"][j], b["tok"][j]), f"{what}: tokens of pass {j} differ"
        assert torch.equal(a["cv"][j], b["cv"][j]), f"{what}: cv of pass {j} differs ({float(a['cv'][j])} vs {float(b['cv'][j])})"
    assert torch.equal(a["flat"], b["flat"]), f"{what}: gradients differ (rel {rel(a['flat'], b['flat']):.2e})"


def _geometry(case, outs):
    """the conditions of the issue, on the engine's own Route.counts, for every task pass and MoE block"""
    seq = list(outs)
    for key in outs[seq[0]]["counts"]:
        c = {s: outs[s]["counts"][key] for s in seq}
        for s in seq:
            assert int(c[s].sum()) == case.T * case.k
            hot, dead = PLAN[s[0]]
            if hot is not None:
                assert int(c[s].argmax()) == hot and int(c[s][hot]) >= 4 * 128, (s, key, c[s].tolist())
                assert all(int(c[s][e]) == 0 for e in dead), (s, key, c[s].tolist())
        for a, b in zip(seq, seq[1:]):
            moved = int((((c[a] > 128) & (c[b] == 0)) | ((c[a] == 0) & (c[b] > 128))).sum())
            assert moved >= 2, (a, b, key, c[a].tolist(), c[b].tolist())
            assert PLAN[a[0]][0] != PLAN[b[0]][0], "the hot expert changes"


def verify(case, s, out, dtype, tag):
    """check 1: finite, and right against the float64 oracle - per tensor and per expert slice"""
    from oracle import ref_torch as R
    tol = TOL[dtype]
    bad = es.nonfinite(dict({f"tok{j}": t for j, t in enumerate(out["tok"])}, **{f"cv{j}": c for j, c in enumerate(out["cv"])},
                            **out["grads"]))
    assert not bad, f"{tag} step {s}: Inf / NaN in {bad}"
    free = oracle_step(case, s[0])
    d = case.steps[s[0]]
    if dtype == F32:
        ref = free
        for key, ix in out["idx"].items():
            assert torch.equal(ix, ref["idx"][key]), f"{tag} step {s}: routing differs in (task, block) {key}"
    else:                                        # 16-bit storage: follow the engine's routing (tests/test_engine.py)
        for (t, i), ix in out["idx"].items():
            w = case.P[f"blocks.{i}.mlp.gate.{t}.w_gate"].double()
            nz = None if d["noises"] is None else d["noises"][t][i].double()
            lb = None if d["bias"] is None else d["bias"][i].double()
            (own, _), *_ = R.gate_vmoe(out["h2"][t, i], w, case.k, nz, case.cfg.vmoe_noisy_std, logit_bias=lb)
            assert torch.equal(ix, own), f"{tag} step {s} {t, i}: indices are not the top-k of the engine's own gate input"
            flipped = float((ix != free["idx"][t, i]).any(1).float().mean())
            assert flipped < 0.2, f"{tag} step {s} {t, i}: {flipped:.2%} of the tokens routed differently"
        ref = oracle_step(case, s[0], {t: {i: out["idx"][t, i] for i in MOE} for t in TASKS})
    w = WORST.setdefault((case.name, str(dtype)), dict(tok=0.0, cv=0.0, grad=("", 0.0), slice=("", 0.0), oracle_s=0.0))
    w["oracle_s"] = max(w["oracle_s"], ref["seconds"])
    for j in range(len(TASKS)):
        e = rel(out["tok"][j], ref["tok"][j])
        w["tok"] = max(w["tok"], e)
        assert e < tol, f"{tag} step {s}: tokens of pass {j} rel {e:.2e} (bound {tol:.0e})"
        ce = abs(float(out["cv"][j]) - ref["cv"][j]) / max(1.0, abs(ref["cv"][j]))
        w["cv"] = max(w["cv"], ce)
        assert ce < 1e-3, f"{tag} step {s}: cv of pass {j} {float(out['cv'][j])} vs {ref['cv'][j]}"
    rows = {i: sum(out["counts"][t, i] for t in TASKS) for i in MOE}          # rows of expert e of block i over both passes
    fails = []
    for n, g in out["grads"].items():
        r = ref["grads"][n]
        if r is None:
            assert float(g.abs().max()) == 0.0, n
            continue
        e = rel(g, r)
        if e > w["grad"][1]:
            w["grad"] = (n, e)
        if e > tol * GRAD_FACTOR:
            fails.append((n, e))
        if ".mlp.experts." in n:
            blk = int(n.split(".")[1])
            for x in range(case.E):
                if int(rows[blk][x]) == 0:
                    if float(g[x].abs().max()) != 0.0:
                        fails.append((f"{n}[{x}] (no rows: must be exactly zero)", float(g[x].abs().max())))
                    continue
                ex = rel(g[x], r[x])
                if ex > w["slice"][1]:
                    w["slice"] = (f"{n}[{x}] ({int(rows[blk][x])} rows)", ex)
                if ex > tol * GRAD_FACTOR:
                    fails.append((f"{n}[{x}] ({int(rows[blk][x])} rows)", ex))
    assert not fails, f"{tag} step {s}: gradients beyond {tol * GRAD_FACTOR:.0e}: {fails[:8]}"


def _report(case, dtype, outs=None):
    w = WORST.get((case.name, str(dtype)))
    if outs is not None:
        for s, o in outs.items():
            print(f"[{case.name}] step {s} counts:", {k: v.tolist() for k, v in o["counts"].items()})
    if w:
        print(f"[{case.name} {dtype}] oracle {w['oracle_s']:.1f} s/step; tokens {w['tok']:.2e} (bound {TOL[dtype]:.0e}); cv {w['cv']:.2e} "
              f"(1e-3); worst gradient {w['grad'][0]} {w['grad'][1]:.2e}, worst expert slice {w['slice'][0]} {w['slice'][1]:.2e} "
              f"(bound {TOL[dtype] * GRAD_FACTOR:.0e})")


def sequence(drv, names=("A", "B", "C", "A'"), check=True, tag=""):
    outs = {}
    for s in names:
        outs[s] = drv.step(s[0])
        if check:
            verify(drv.case, s, outs[s], drv.dtype, tag or drv.kind)
    return outs


# ------------------------------------------------------------------------------------- checks 1 and 2, every runner kind
@pytest.mark.parametrize("name,dtype", [("noisy", F32), ("noisy", F16), ("bias", F32), ("bias", F16), ("bias", BF16)])
@pytest.mark.parametrize("kind", ["engine", "eager", "graph"])
def test_steps_are_right_and_history_independent(kind, name, dtype):
    """A, B, C, A' with zero_grad + poison before every step (kind "engine": before every task pass).  Check 1 on every step;
    check 2: A' == A bit for bit, a FRESH runner that only ever sees A (poisoned first) gives those bits, and so does one that
    runs C, B, A; a replayed step equals the same runner's eager step at 1e-5 (the existing runner test's level: the streams
    may order the final gradient add differently)."""
    _need_gpu()
    case = case_of(name)
    drv = Driver(case, "eager" if kind == "graph" else kind, dtype)
    eager_a = None
    if kind == "graph":                          # the same runner's eager step first, then capture
        eager_a = drv.step("A")
        assert drv.run.capture(), drv.run.capture_error
        assert drv.run.launch.startswith("hipGraph replay") and drv.run.graphs is not None
        drv.kind = "graph"
    outs = sequence(drv, tag=f"{kind} {name} {dtype}")
    _geometry(case, outs)
    same_bits(outs["A'"], outs["A"], "A' after B and C against A")
    if eager_a is not None:
        for j in range(len(TASKS)):
            assert rel(outs["A"]["tok"][j], eager_a["tok"][j]) < 1e-5
        assert rel(outs["A"]["flat"], eager_a["flat"]) < 1e-5
    fresh = Driver(case, kind, dtype)
    same_bits(fresh.step("A"), outs["A"], "a fresh runner that only sees A")
    back = Driver(case, kind, dtype, first="C")
    rev = sequence(back, names=("C", "B", "A"), check=False)
    same_bits(rev["A"], outs["A"], "A after C, B")
    same_bits(rev["C"], outs["C"], "C first against C after A, B")
    _report(case, dtype, outs)


# ------------------------------------------------------------------------------------------ check 4: launch-plan variants
def knobs(ops, monkeypatch, direct=True, dma=1):
    monkeypatch.setattr(ops, "_WGRAD_DIRECT", direct)
    ops.wgrad_set_dma(dma)


VARIANT_TOL = {F32: 1e-5, F16: 4e-3}      # fp32 summation order; fp16: test_shared_stem_step_matches_per_task_stems' figure


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("variant", ["no_direct", "no_direct_dma0", "no_direct_dma2", "dma0", "dma2", "wgrad_streams", "checkpoint",
                                     "share_stem"])
def test_launch_plan_variants(variant, dtype, monkeypatch):
    """the weight-gradient plans (direct mode off: balanced units + m3_wgrad_reduce_grouped riding on the next launch; the
    LDS-DMA kernel forced off / on; a wgrad stream per pass instead of the ride-along queue, eager only), checkpoint=True
    (shared per-kind activation buffers) and share_stem=True: A, B, C, A' poisoned, check 2, and the gradients of every
    step against the DEFAULT plan's at the summation-order level; `no_direct` also meets the oracle (check 1)."""
    _need_gpu()
    from m3vit_amd import ops
    case = case_of("noisy")
    kw, kn = {}, {}
    if variant.startswith("no_direct"):
        kn = dict(direct=False, dma={"no_direct": 1, "no_direct_dma0": 0, "no_direct_dma2": 2}[variant])
    elif variant.startswith("dma"):
        kn = dict(direct=True, dma=int(variant[3:]))
    else:
        kw = {"wgrad_streams": dict(wgrad_streams=True), "checkpoint": dict(checkpoint=True),
              "share_stem": dict(share_stem=True)}[variant]
    base = sequence(Driver(case, "eager", dtype), names=("A", "B", "C"), check=False)
    try:
        knobs(ops, monkeypatch, **kn)
        kinds = ("eager",) if variant == "wgrad_streams" else ("eager", "graph")
        for kind in kinds:
            drv = Driver(case, kind, dtype, **kw)
            if variant == "wgrad_streams":
                assert drv.run.eng.wg_stream is not None and drv.run.eng.wq is None and not drv.run.want_graph
            if variant == "share_stem":
                assert drv.run.share_stem
            outs = sequence(drv, check=variant == "no_direct", tag=f"{variant} {kind} {dtype}")
            _geometry(case, outs)
            same_bits(outs["A'"], outs["A"], f"{variant} {kind}: A' against A")
            for s in ("A", "B", "C"):
                bad = es.nonfinite(dict(outs[s]["grads"], tok0=outs[s]["tok"][0], tok1=outs[s]["tok"][1]))
                assert not bad, (variant, kind, s, bad)
                for j in range(len(TASKS)):
                    assert rel(outs[s]["tok"][j], base[s]["tok"][j]) < 1e-5, (variant, kind, s, j)
                for n, g in outs[s]["grads"].items():
                    e = rel(g, base[s]["grads"][n])
                    assert e < VARIANT_TOL[dtype], (variant, kind, s, n, e)
    finally:
        ops.wgrad_set_dma(-1)


# ------------------------------------------------------------------------------------------ check 3: poison stays put
@pytest.mark.parametrize("direct", [True, False])
def test_poison_stays_where_nothing_should_write(direct, monkeypatch):
    """the slab workspaces of the weight gradients past the largest slab need of any call of the step keep the sentinel
    (include/m3vit_hip.h: slabs are units * N * K (+ units * N) floats from the start of ws; a direct-mode call writes none).
    The need of each call is ops.wgrad_launch_plan's, recorded by a wrapper around ops.wgrad_tn - not taken from the buffers."""
    _need_gpu()
    from m3vit_amd import engine as eng_mod
    from m3vit_amd import ops
    case = case_of("noisy")
    monkeypatch.setattr(ops, "_WGRAD_DIRECT", direct)
    need = [0]
    real = ops.wgrad_tn

    def spy(dC, A, dW, *, M=None, splits=None, group_offsets=None, db=None, c_row_idx=None, **kw):
        G = 1 if dW.dim() == 2 else dW.shape[0]
        N, K = dW.shape[-2], dW.shape[-1]
        m = M if M is not None else (c_row_idx.numel() if c_row_idx is not None else dC.shape[0])
        p = ops.wgrad_launch_plan(m, N, K, G, dC.dtype, grouped=group_offsets is not None, bias=db is not None, splits=splits or 0,
                           direct_ok=ops._WGRAD_DIRECT and dW.data_ptr() % 16 == 0)
        assert p.ws_elems == (0 if p.direct else p.units * N * K + (p.units * N if db is not None else 0))
        need[0] = max(need[0], p.ws_elems)
        return real(dC, A, dW, M=M, splits=splits, group_offsets=group_offsets, db=db, c_row_idx=c_row_idx, **kw)

    monkeypatch.setattr(eng_mod.ops, "wgrad_tn", spy)
    drv = Driver(case, "engine", F16)
    for s in ("A", "B"):
        out = drv.step(s)
        assert not es.nonfinite(out["grads"])
        for j, ws in enumerate(drv.eng.wq.ws):
            assert need[0] <= ws.numel()
            assert es.holds_sentinel(ws[need[0]:]), f"step {s}: slab workspace {j} written past the largest need {need[0]}"
        if not direct:
            assert need[0] > 0 and not es.holds_sentinel(drv.eng.wq.ws[0][:need[0]])


# --------------------------------------------------------------------------------------------------- after an overflow
@pytest.mark.parametrize("kind", ["engine", "eager", "graph"])
def test_step_after_an_fp16_overflow_is_clean(kind):
    """step A, then X = A with d_tokens scaled until the fp16 activation gradients overflow (flat must hold Inf / NaN, or
    the test proves nothing), NO poison call, zero_grad, then A again: bit-identical to the first A.  This is the state an
    AMP trainer is in after its first skipped step."""
    _need_gpu()
    case = case_of("noisy")
    drv = Driver(case, kind, F16)
    a0 = drv.step("A", poison=False)
    assert not es.nonfinite(a0["grads"])
    x = drv.step("A", poison=False, scale=2.0 ** 40)
    assert not bool(torch.isfinite(x["flat"]).all()), "the scaled step must overflow"
    a1 = drv.step("A", poison=False)
    assert not es.nonfinite(dict(a1["grads"], tok0=a1["tok"][0], tok1=a1["tok"][1]))
    same_bits(a1, a0, "A after an overflowed step")


def test_amp_step_after_a_skipped_step_equals_the_step_without_it():
    """cls.amp_train_step on fp16 activations (noisy gate, GradScaler, clipping, AdamW): from one snapshot of parameters and
    optimizer state, a good step - then, from the same snapshot, the 2^40 step (overflow: skipped) followed by the same good
    step with a fresh scaler.  Loss and updated parameters must be the same bits: nothing the skipped step left behind (Inf
    and NaN all over the executor's scratch) may reach the next one.  The compared steps replay the encoder's hipGraphs."""
    _need_gpu()
    import copy
    import torch.nn.functional as F
    from m3vit_amd.cls import MoEViTForImageNet, amp_train_step
    from test_modules_gpu import _cls_cfg
    torch.manual_seed(7)
    m = MoEViTForImageNet(_cls_cfg(vmoe_noisy_std=1.0), act_dtype=F16).cuda().train()
    opt = torch.optim.AdamW(m.parameters(), lr=2e-3, weight_decay=0.05)
    x = torch.randn(16, 3, 32, 32, device="cuda")
    y = torch.randint(0, 16, (16,), device="cuda")
    crit = lambda samples, logits, targets: F.cross_entropy(logits, targets)          # noqa: E731
    warm = torch.amp.GradScaler("cuda", init_scale=1024.0)
    for _ in range(4):                                   # eager, capture, two replays
        amp_train_step(m, crit, opt, warm, x, y, moe_cv_weight=0.01, clip_grad=1.0)
    assert m.encoder.fused_fallback_reason is None
    slot = m.encoder._fused.slots[0]
    assert slot.graphs_f and slot.graphs_b, "the compared steps must be hipGraph replays"
    gf, gb = dict(slot.graphs_f), dict(slot.graphs_b)
    torch.cuda.synchronize()
    params = [p.detach().clone() for p in m.parameters()]
    state = copy.deepcopy(opt.state_dict())

    def restore(p_too=True):
        with torch.no_grad():
            if p_too:
                for p, s in zip(m.parameters(), params):
                    p.copy_(s)
        opt.load_state_dict(copy.deepcopy(state))

    def good():
        torch.manual_seed(123)                           # the gate draws its noise with the default generator
        sc = torch.amp.GradScaler("cuda", init_scale=1024.0)
        loss, cv = amp_train_step(m, crit, opt, sc, x, y, moe_cv_weight=0.01, clip_grad=1.0)
        torch.cuda.synchronize()
        assert sc.get_scale() == 1024.0
        return loss, cv, [p.detach().clone() for p in m.parameters()]

    l0, c0, p0 = good()
    assert any(not torch.equal(a, b) for a, b in zip(p0, params))
    restore()
    big = torch.amp.GradScaler("cuda", init_scale=2.0 ** 40)
    amp_train_step(m, crit, opt, big, x, y)
    assert big.get_scale() == 2.0 ** 39                                               # overflow found, step skipped
    assert all(torch.equal(a, b.detach()) for a, b in zip(params, m.parameters()))
    restore(p_too=False)
    l1, c1, p1 = good()
    assert slot.graphs_f == gf and slot.graphs_b == gb, "a graph was captured again: the compared steps were not replays"
    assert l1 == l0 and c1 == c0, (l0, l1, c0, c1)
    bad = [n for (n, _), a, b in zip(m.named_parameters(), p0, p1) if not torch.equal(a, b)]
    assert not bad, f"parameters differ after a skipped step: {bad[:6]}"


# ------------------------------------------------------------------------------------------------------ the module path
@pytest.mark.parametrize("dtype,tol", [(F32, 2e-4), (F16, 1e-3)])
def test_module_path_steps_are_right_and_history_independent(dtype, tol):
    """VisionTransformerMoE.forward + loss.backward() (fused="auto", views delivery) at the size where the routing geometry
    moves: tests/test_fused_module_gpu.py::test_fused_module_joint_multitask_steps_match_oracle with A, B, C, A', both slots'
    engines poisoned before every step, its bounds (tokens tol, cv 2e-3, gradients 3 tol + 7e-4) per tensor and per expert
    slice, A' == A on tokens and on every p.grad.  The module draws its own gate noise, so the routing is steered through
    parameters the oracle takes too: in both MoE blocks norm2.weight[0] = 0 and norm2.bias[0] = 1 make column 0 of the gate's
    input the constant 1 for every token, and row 0 of each task's w_gate is then a logit bias: set before each step to the
    step's offsets (+ 4 hot, - 30 dead; A: 0), rewritten in place, A' gets A's bits back; no optimizer step in between.
    (A task-conditioned gate steered through w_gate[D:] was tried first: the task embedding's gradient is then
    w_gate[D:] @ colsum(d logits), one cancelling sum over all tokens, and its fp16 error - 5.8e-3 in step C - is not what
    the per-tensor figure of 3.7e-3 was set for; as row 0 of w_gate the same sum is one row of a [D, E] tensor.)
    Two warm steps first, so that A .. A' are all hipGraph replays."""
    _need_gpu()
    from m3vit_amd.vit import VisionTransformerMoE
    from oracle import ref_torch as R
    E, k, D = 8, 2, 64
    kw = dict(img_size=IMG, embed_dim=D, depth=4, num_heads=2, moe_top_k=k, gate_dim=66, multi_gate=True, moe_experts=E)
    cfg = R.BackboneCfg(mlp_ratio=4.0, moe_mlp_ratio=1.0, vmoe_noisy_std=0.0, **kw)
    P = R.init_backbone_params(cfg, seed=23)
    for n in P:
        if n.endswith("w_gate"):
            P[n] = P[n] * 0.5
            P[n][0] = 0.0
    for i in MOE:
        P[f"blocks.{i}.norm2.weight"][0] = 0.0
        P[f"blocks.{i}.norm2.bias"][0] = 1.0
    m = VisionTransformerMoE(mlp_ratio=4.0, moe_mlp_ratio=1, vmoe_noisy_std=0.0, fused="auto", act_dtype=dtype, **kw).cuda()
    m.load_state_dict(P)
    m.train()
    named = dict(m.named_parameters())
    inputs = {}
    for j, (s, (hot, dead)) in enumerate(PLAN.items()):
        g = torch.Generator().manual_seed(700 + j)
        off = torch.zeros(E)
        if hot is not None:
            off[hot] = HOT
            off[list(dead)] = DEAD
        inputs[s] = dict(img=torch.randn(B, 3, *IMG, generator=g), dtok=torch.randn(B, cfg.num_tokens, D, generator=g) * 0.1,
                         rows=off)
    img_dev = torch.empty(B, 3, *IMG, device="cuda")
    worst = dict(tok=0.0, grad=0.0, slice=0.0)

    def step(s, check):
        d = inputs[s[0]]
        torch.cuda.synchronize()
        with torch.no_grad():
            for i in MOE:
                for t in TASKS:
                    named[f"blocks.{i}.mlp.gate.{t}.w_gate"][0].copy_(d["rows"])
        img_dev.copy_(d["img"])
        dtok = d["dtok"].cuda()
        for p in m.parameters():
            p.grad = None
        fb = m._fused
        if fb is not None:
            assert not any(sl.busy for sl in fb.slots)
            for sl in fb.slots:
                es.poison(es.scratch_tensors(sl.eng))
        loss, outs = 0.0, []
        for t in TASKS:
            tok, cv = m(img_dev, task_id=t)
            assert m.fused_fallback_reason is None
            loss = loss + (tok * dtok).sum() + CVW * cv
            outs.append((tok.detach().clone(), cv.detach().clone()))
        fb = m._fused
        torch.cuda.synchronize()
        route = {(t, i): (fb.slots[j].eng.act[i]["gate"]["idx"].cpu(), fb.slots[j].eng.act[i]["route"].counts.cpu().long(),
                          fb.slots[j].eng.act[i]["h2"].double().cpu()) for j, t in enumerate(TASKS) for i in MOE}
        loss.backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
        out = dict(tok=[o[0] for o in outs], cv=[o[1] for o in outs], grads=grads, counts={key: v[1] for key, v in route.items()})
        if not check:
            return out
        bad = es.nonfinite(dict(grads, tok0=out["tok"][0], tok1=out["tok"][1], cv0=out["cv"][0], cv1=out["cv"][1]))
        assert not bad, f"step {s}: Inf / NaN in {bad}"
        Pr = {n: v.detach().clone().double().cpu().requires_grad_() for n, v in m.state_dict().items()}
        ref_loss = 0.0
        for j, t in enumerate(TASKS):
            ovr = None
            with torch.no_grad():
                free = R.backbone_forward(Pr, cfg, d["img"].double(), t)[2]
            if dtype == F32:
                for i in MOE:
                    assert torch.equal(route[t, i][0], free[i]["idx"]), f"step {s}: routing differs in {t, i}"
            else:
                ovr = {i: route[t, i][0] for i in MOE}
                for i in MOE:
                    (own, _), *_ = R.gate_vmoe(route[t, i][2], free[i]["w_gate"], k)
                    assert torch.equal(ovr[i], own), f"step {s} {t, i}: indices are not the top-k of the module's own gate input"
                    assert float((ovr[i] != free[i]["idx"]).any(1).float().mean()) < 0.2
            tr, cr, _ = R.backbone_forward(Pr, cfg, d["img"].double(), t, route_override=ovr)
            e = rel(out["tok"][j], tr)
            worst["tok"] = max(worst["tok"], e)
            assert e < tol, (s, t, e)
            assert abs(float(out["cv"][j]) - float(cr.detach())) < 2e-3 * max(1.0, float(cr.detach())), (s, t)
            ref_loss = ref_loss + (tr * d["dtok"].double()).sum() + CVW * cr
        ref_loss.backward()
        gtol = 3 * tol + 7e-4
        rows_of = {i: sum(route[t, i][1] for t in TASKS) for i in MOE}
        fails = []
        for n, g_ in grads.items():
            r = Pr[n].grad
            if r is None:
                continue
            worst["grad"] = max(worst["grad"], rel(g_, r))
            if rel(g_, r) > gtol:
                fails.append((n, rel(g_, r)))
            if ".mlp.experts." in n:
                blk = int(n.split(".")[1])
                for x in range(E):
                    if int(rows_of[blk][x]) == 0:
                        if float(g_[x].abs().max()) != 0.0:
                            fails.append((f"{n}[{x}] (no rows)", float(g_[x].abs().max())))
                    else:
                        worst["slice"] = max(worst["slice"], rel(g_[x], r[x]))
                        if rel(g_[x], r[x]) > gtol:
                            fails.append((f"{n}[{x}] ({int(rows_of[blk][x])} rows)", rel(g_[x], r[x])))
        assert not fails, (s, fails[:8])
        return out

    step("C", False)
    step("C", False)
    outs = {s: step(s, True) for s in ("A", "B", "C", "A'")}
    fb = m._fused
    assert len(fb.slots) == 2 and all(fb.slots[j].graphs_f and fb.slots[j].graphs_b for j in (0, 1)), "A .. A' must replay graphs"

    class _C:
        T, k = B * cfg.num_tokens, 2
    _geometry(_C, outs)
    a, a2 = outs["A"], outs["A'"]
    for j in range(len(TASKS)):
        assert torch.equal(a["tok"][j], a2["tok"][j]) and torch.equal(a["cv"][j], a2["cv"][j]), f"A' against A: pass {j}"
    bad = [n for n in a["grads"] if not torch.equal(a["grads"][n], a2["grads"][n])]
    assert not bad, f"A' against A: p.grad differs for {bad[:6]}"
    print(f"[module path {dtype}] tokens {worst['tok']:.2e} (bound {tol:.0e}); worst gradient {worst['grad']:.2e}, worst expert "
          f"slice {worst['slice']:.2e} (bound {3 * tol + 7e-4:.1e}); counts of step B:", {k_: v.tolist() for k_, v in outs["B"]["counts"].items()})
