#!/usr/bin/env python3
"""The token blocks' FFN sublayer (m3vit_amd.sharing.TokenFFNStage, mode "all": the dense block's step 5) at T = 2 tasks,
B = 128, N = 197, C = 384, H = 1536, fp16 - the token backbone's ViT-Small shape - with 0, 0.5 and 0.9 of the positions shared
by both tasks, in three forms, alternating rounds, device events around `--iters` iterations after a warm-up, best of
`--rounds`:
  (i)   TokenFFNStage forward, and forward + backward
  (a)   the same arithmetic in stock torch ops in the reference's form: nonzero() per task, indexed gathers, a clone() per
        task, nn.LayerNorm / nn.Linear / GELU on the gathered rows, the indexed broadcast (host reads included: that is the form)
  (b)   T calls of the existing Mlp + HipLayerNorm on the full [B, N, C] tensors - what a caller does today, nothing saved
and the two forward row passes by themselves against m3_add_f32 on the same number of bytes (12 B per element), the
streaming rate this project measures its row kernels against.  Bytes are algorithmic: the LayerNorm-gather reads and writes
R rows of C values plus 12 B of index and statistics per row; the scatter reads the T task rows of every position, the R rows
of f and the shared rows of shared_x, and writes T rows per position.
    python tools/token_ffn_bench.py [--iters 50] [--rounds 3] [--out profiles/token_ffn.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters            # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fractions", default="0,0.5,0.9")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_ffn.txt"))
    args = ap.parse_args()
    import token_ffn_cases as TC
    from m3vit_amd import ops
    from m3vit_amd.sharing import SharedTokens, TokenFFNStage
    from m3vit_amd.vit import HipLayerNorm, Mlp
    T, B, N, C, H, dt = 2, args.batch, 197, 384, 1536, torch.float16
    P = B * N
    gen = torch.Generator().manual_seed(0)
    params = TC.make_params(C, H, gen)
    norm2, mlp = HipLayerNorm(C, eps=TC.LN_EPS), Mlp(C, H)
    norm2.act_dtype = dt
    with torch.no_grad():
        for dst, name in ((norm2.weight, "gamma"), (norm2.bias, "beta"), (mlp.fc1.weight, "w1"), (mlp.fc1.bias, "b1"),
                          (mlp.fc2.weight, "w2"), (mlp.fc2.bias, "b2")):
            dst.copy_(params[name])
    stage = TokenFFNStage(norm2, mlp, T).cuda().train()
    prm = [norm2.weight, norm2.bias, mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias]
    # (a): stock torch modules holding the same values in the activation dtype
    t_ln = torch.nn.LayerNorm(C, eps=TC.LN_EPS).cuda().to(dt)
    t_fc1, t_fc2 = torch.nn.Linear(C, H).cuda().to(dt), torch.nn.Linear(H, C).cuda().to(dt)
    with torch.no_grad():
        for dst, src in ((t_ln.weight, norm2.weight), (t_ln.bias, norm2.bias), (t_fc1.weight, mlp.fc1.weight), (t_fc1.bias, mlp.fc1.bias),
                         (t_fc2.weight, mlp.fc2.weight), (t_fc2.bias, mlp.fc2.bias)):
            dst.copy_(src)
    t_prm = list(t_ln.parameters()) + list(t_fc1.parameters()) + list(t_fc2.parameters())

    def t_ffn(v):
        return t_fc2(torch.nn.functional.gelu(t_fc1(t_ln(v))))

    xs = [(0.3 + torch.randn(B, N, C, generator=gen)).to(dt).cuda().requires_grad_(True) for _ in range(T)]
    dys = [torch.randn(B, N, C, generator=gen).to(dt).cuda() for _ in range(T)]
    lines = [f"token FFN stage (mode all): T = {T}, B = {B}, N = {N}, C = {C}, H = {H}, fp16; {P} positions; best of {args.rounds} "
             f"alternating rounds x {args.iters} iterations, device events", f"device: {torch.cuda.get_device_name(0)}", ""]
    for frac in [float(v) for v in args.fractions.split(",")]:
        bits = torch.where(torch.rand(P, generator=gen) < frac, (1 << T) - 1, 0).to(torch.int64).cuda()
        M = [((bits >> t) & 1).bool() for t in range(T)]
        sx = (sum(x.detach().view(P, C).float() for x in xs) / T * (bits != 0).unsqueeze(-1)).to(dt).requires_grad_(True)
        shared = SharedTokens(bits.view(B, N), sx, None, None, None, None, T)
        K = int((bits != 0).sum())
        R = T * (P - K) + K

        def ours(train):
            out = stage({t: xs[t] for t in range(T)}, shared)
            if train:
                return torch.autograd.grad([out[t] for t in range(T)], xs + [sx] + prm, dys)
            return out

        def ref_form(train):                         # the reference's dense_mlp_stage + shared_dense_forward + apply_shared_broadcast
            outs = []
            flat_idx = (bits != 0).nonzero(as_tuple=False).squeeze(1)
            for t in range(T):
                x_flat = xs[t].reshape(P, C)
                ts_idx = (~M[t]).nonzero(as_tuple=False).squeeze(1)
                out_flat = x_flat.clone()
                if ts_idx.numel():
                    out_flat[ts_idx] = out_flat[ts_idx] + t_ffn(x_flat[ts_idx])
                outs.append(out_flat)
            if flat_idx.numel():
                sc = sx[flat_idx]
                shared_out = sc + t_ffn(sc)
                lookup = flat_idx.new_full((P,), -1)
                lookup[flat_idx] = torch.arange(flat_idx.numel(), device=flat_idx.device)
                for t in range(T):
                    idx_t = (M[t] & (bits != 0)).nonzero(as_tuple=False).squeeze(1)
                    if idx_t.numel():
                        o = outs[t].clone()
                        o[idx_t] = shared_out[lookup[idx_t]]
                        outs[t] = o
            if train:
                return torch.autograd.grad(outs, xs + [sx] + t_prm, [d.view(P, C) for d in dys], allow_unused=True)
            return outs

        def today(train):                            # (b): nothing saved
            outs = [xs[t] + mlp(norm2(xs[t])) for t in range(T)]
            if train:
                return torch.autograd.grad(outs, xs + prm, dys)
            return outs

        # faster and different is not faster: the forms agree before anything is timed
        with torch.no_grad():
            a, b = ours(False), ref_form(False)
            for t in range(T):
                torch.testing.assert_close(a[t].view(P, C).float(), b[t].float(), rtol=2e-2, atol=2e-2)
            if frac == 0.0:
                c = today(False)
                torch.testing.assert_close(a[0].float(), c[0].float(), rtol=2e-2, atol=2e-2)
        xd, sxd = [x.detach().view(P, C) for x in xs], sx.detach()
        wl = ops.token_ffn_worklist(bits, T, "all")
        ga, be = norm2.weight.detach(), norm2.bias.detach()
        h, _, _ = ops.token_ffn_ln_fwd(xd, sxd, wl, ga, be)
        f = torch.randn(wl.M_ub, C, device="cuda", dtype=dt)
        ln_bytes = R * (2 * C * 2 + 12)
        sc_bytes = P * (2 * T * C * 2 + (T + 1) * 4 + 8) + R * C * 2 + K * C * 2
        n_add = (ln_bytes + sc_bytes) // 24
        buf_a, buf_b = torch.zeros(n_add, device="cuda"), torch.ones(n_add, device="cuda")

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    return fn(False)
            return run
        forms = {"(i) TokenFFNStage forward": no_grad(ours), "(i) TokenFFNStage forward + backward": lambda: ours(True),
                 "(a) torch ops, reference form, forward": no_grad(ref_form), "(a) torch ops, reference form, forward + backward": lambda: ref_form(True),
                 "(b) T x (HipLayerNorm + Mlp), forward": no_grad(today), "(b) T x (HipLayerNorm + Mlp), forward + backward": lambda: today(True),
                 "m3_token_ffn_worklist": lambda: ops.token_ffn_worklist(bits, T, "all"),
                 "m3_token_ffn_ln_fwd": lambda: ops.token_ffn_ln_fwd(xd, sxd, wl, ga, be, h=h),
                 "m3_token_ffn_scatter_fwd": lambda: ops.token_ffn_scatter_fwd(xd, sxd, f, wl, bits, N),
                 "m3_add_f32 (yardstick)": lambda: ops.add_f32(buf_a, buf_b)}
        times = {k: [] for k in forms}
        for _ in range(args.rounds):                 # alternating: a drift of the clocks lands on every form alike
            for k, fn in forms.items():
                times[k].append(timed(fn, args.iters))
        best = {k: min(v) for k, v in times.items()}
        lines.append(f"shared fraction {frac:g}: {K} of {P} positions shared, R = {R} work rows of the bound {T * P} (R / (T P) = {R / (T * P):.3f})")
        for k, v in times.items():
            lines.append(f"  {k:52s} best {best[k]:8.4f} ms   rounds " + " ".join(f"{x:.4f}" for x in v))
        add_rate = 12 * n_add / best["m3_add_f32 (yardstick)"] / 1e9
        for k, nbytes in (("m3_token_ffn_ln_fwd", ln_bytes), ("m3_token_ffn_scatter_fwd", sc_bytes)):
            r = nbytes / best[k] / 1e9
            lines.append(f"  {k}: {nbytes / 1e6:.1f} MB -> {r:.3f} TB/s = {r / add_rate:.2f} of m3_add_f32's {add_rate:.3f} TB/s")
        for tag in ("forward", "forward + backward"):
            o = best[f"(i) TokenFFNStage {tag}"]
            lines.append(f"  {tag}: (a) / (i) = {best[f'(a) torch ops, reference form, {tag}'] / o:.2f}x, "
                         f"(b) / (i) = {best[f'(b) T x (HipLayerNorm + Mlp), {tag}'] / o:.2f}x")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
