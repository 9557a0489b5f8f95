#!/usr/bin/env python3
"""Phase timeline of the LDS-DMA GEMM kernel (gemm_dma.hip) from in-kernel s_memtime stamps, at four launches of configs[1]
(batch 128 x 197 tokens, width 384, 16 experts, top-4): proj (RES, 591 workgroups), qkv (PLAIN, 1773), the experts' FC1
forward (grouped, A gathered through the slot map / 4, GELU + pre_out) and the experts' FC2 input gradient (grouped, A gathered,
GELU'(pre), the gate score through row_scale_idx).  Needs a diagnostic build of the library:

    (cd m3vit_amd/csrc && make CXXFLAGS="-O3 -fPIC -std=c++17 --offload-arch=gfx950 -DM3_GEMM_STAMPS" \
         OBJDIR=../../build/gstamps OUT=../libm3vit_hip_gstamps.so)
    M3VIT_LIB=$PWD/m3vit_amd/libm3vit_hip_gstamps.so python tools/gemm_stamps.py [proj|qkv|efc1|efc2 ...]

Operands are streamed (a ring of operand sets larger than the Infinity Cache); the time per launch is by device events over
the ring, the stamps are those of one more launch.  Stamped: lane 0 of wave 0 of every workgroup (the first 4096); all
figures are differences inside one workgroup (the XCDs' counters are not aligned), mean over the live workgroups.  With
the shipped library the tool prints the time per launch only."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from m3vit_amd import _lib, ops  # noqa: E402

shapes = sys.argv[1:] or ["proj", "qkv", "efc1", "efc2"]
T, k, E, D, ring, reps = 128 * 197, 4, 16, 384, 6, 5
R = T * k
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(3)
pick = torch.rand(T, E, generator=g).argsort(dim=1)[:, :k].reshape(-1)          # expert of routed entry t * k + j
row_of_slot = torch.sort(pick, stable=True).indices.to(torch.int32).to(dev)
counts = torch.bincount(pick, minlength=E)
off = torch.zeros(E + 1, dtype=torch.int32)
off[1:] = counts.cumsum(0)
ts = torch.zeros(E + 1, dtype=torch.int32)
ts[1:] = ((counts + 127) // 128).cumsum(0)
off, ts = off.to(dev), ts.to(dev)
score = (torch.rand(R, generator=g) + 0.5).to(dev)
L = _lib.lib()
stamped = hasattr(L, "m3_debug_gemm_stamps")
if stamped:
    L.m3_debug_gemm_stamps.restype = ctypes.c_int
    L.m3_debug_gemm_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
WGS, SN, EP = 4096, 64, 56


def half(*shape, scale=1.0):
    return (torch.randn(*shape, device=dev) * scale).half()


for shape in shapes:
    grouped = shape in ("efc1", "efc2")
    N = {"proj": D, "qkv": 3 * D, "efc1": D, "efc2": D}[shape]
    rows_a, rows_c = (T, R) if grouped else (T, T)
    B = half(E, N, D, scale=0.05) if grouped else half(N, D, scale=0.05)
    bias = torch.zeros(E * N if grouped else N, device=dev)
    sets = []
    for _ in range(ring):
        s = dict(A=half(rows_a, D))
        if shape == "proj":
            s.update(C=torch.empty(T, N, device=dev), res=torch.randn(T, N, device=dev))
        else:
            s.update(C=torch.empty(rows_c, N, dtype=torch.float16, device=dev))
        if shape == "efc1":
            s.update(pre=torch.empty(R, N, dtype=torch.float16, device=dev))
        if shape == "efc2":
            s.update(A=half(T, D), gpre=half(R, N))
        sets.append(s)
    gk = dict(M=R, a_row_idx=row_of_slot, a_row_div=k, group_offsets=off, tile_starts=ts)

    def call(i):
        s = sets[i % ring]
        if shape == "proj":
            ops.gemm_nt(s["A"], B, s["C"], bias=bias, residual=s["res"])
        elif shape == "qkv":
            ops.gemm_nt(s["A"], B, s["C"], bias=bias)
        elif shape == "efc1":
            ops.gemm_nt(s["A"], B, s["C"], bias=bias, act=ops.M3_ACT_GELU, pre_out=s["pre"], **gk)
        else:
            ops.gemm_nt(s["A"], B, s["C"], gelu_grad_pre=s["gpre"], row_scale=score, row_scale_idx=row_of_slot, **gk)
    for i in range(ring):
        call(i)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for i in range(reps * ring):
        call(i)
    ev[1].record()
    torch.cuda.synchronize()
    nk = D * 2 // 128
    print(f"{shape}: N {N} K {D}, {nk} K slices; {ev[0].elapsed_time(ev[1]) * 1000 / (reps * ring):.1f} us per launch by events")
    if not stamped:
        continue
    assert L.m3_debug_gemm_stamps(None, WGS, 1) == 0                 # clear, then one more launch to analyse
    call(0)
    torch.cuda.synchronize()
    buf = np.zeros((WGS, SN), dtype=np.uint64)
    assert L.m3_debug_gemm_stamps(buf.ctypes.data, WGS, 0) == 0
    st = buf.astype(np.int64)
    st = st[st[:, EP + 1] > 0]                                        # workgroups that reached their second epilogue half
    life = st[:, EP + 1] - st[:, 0]
    wait = np.stack([st[:, 2 + 2 * s] - (st[:, 1] if s == 0 else st[:, 1 + 2 * s]) for s in range(nk)], 1)
    comp = np.stack([st[:, 3 + 2 * s] - st[:, 2 + 2 * s] for s in range(nk)], 1)

    def pct(x):
        return f"{x.mean():8.0f} ({100 * x.mean() / life.mean():4.1f} %)"
    print(f"  {st.shape[0]} workgroups stamped; per workgroup (ticks, mean; share of its lifetime {life.mean():.0f}):")
    print(f"  set-up (entry -> the first DMA instruction)   {pct(st[:, 1] - st[:, 0])}")
    print(f"  first slice (DMA issue + wait + barrier)      {pct(wait[:, 0])}")
    print(f"  entry -> first MFMA                           {pct(st[:, 2] - st[:, 0])}")
    print(f"  later slices (DMA issue + wait + barrier)     {pct(wait[:, 1:].sum(1))}   per slice {wait[:, 1:].mean():.0f}")
    print(f"  MFMA phases + barrier                         {pct(comp.sum(1))}   per slice {comp.mean():.0f}")
    print(f"  epilogue half 0 (stage, bias, store)          {pct(st[:, EP] - st[:, 1 + 2 * nk])}")
    print(f"  epilogue half 1                               {pct(st[:, EP + 1] - st[:, EP])}")
    print(f"  (until the stores are acknowledged            {(st[:, EP + 2] - st[:, EP + 1]).mean():8.0f})")
    del sets
