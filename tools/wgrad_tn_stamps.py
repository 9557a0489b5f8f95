#!/usr/bin/env python3
"""The experts' weight-gradient launches of configs[1] by themselves (register-staged kernel, balanced units: 100 864 routed
rows, 16 experts, N = K = 384 -> 3 / 2368 / 58), operands streamed through a ring: time per call, and with a diagnostic build
of the library the in-kernel timeline of the steady-state loop from s_memtime stamps.

    (cd m3vit_amd/csrc && make CXXFLAGS="-O3 -fPIC -std=c++17 --offload-arch=gfx950 -DM3_WGRAD_STAMPS" \
         OBJDIR=../../build/wstamps OUT=../libm3vit_hip_wstamps.so)
    M3VIT_LIB=$PWD/m3vit_amd/libm3vit_hip_wstamps.so python tools/wgrad_tn_stamps.py [fc1|fc2|plain ...]

fc1: A rows gathered through a_row_idx / 4.  fc2: dC rows gathered through c_row_idx / 4 and scaled by c_row_scale, fused bias
gradient.  plain: the same groups and units on plain rows (no index, no factor).  The slot map is the router's: every token
picks 4 of 16 experts, slots sorted by expert, token order inside an expert.  Stamped: lane 0 of wave 0 of the workgroup of
output tile 0 of every unit; per 32-row step, cycles from the previous barrier to "loads issued" (contains the gathered rows'
addresses and every fourth pair of steps a stage of the gather table), "MFMAs issued", "LDS stores issued" (contains the wait for the step's data), "barrier passed"."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from m3vit_amd import _lib, ops  # noqa: E402

forms = sys.argv[1:] or ["fc1", "fc2", "plain"]
T, k, E, N, K, ring, reps = 25216, 4, 16, 384, 384, 6, 5
R = T * k
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(3)
pick = torch.rand(T, E, generator=g).argsort(dim=1)[:, :k].reshape(-1)          # expert of routed entry t * k + j
row_of_slot = torch.sort(pick, stable=True).indices.to(torch.int32).to(dev)
counts = torch.bincount(pick, minlength=E)
off = torch.zeros(E + 1, dtype=torch.int32)
off[1:] = counts.cumsum(0)
off = off.to(dev)
score = (torch.rand(R, generator=g) + 0.5).to(dev)
p = ops.wgrad_launch_plan(R, N, K, E, torch.float16, grouped=True)
print(f"# rows per expert min {int(counts.min())} max {int(counts.max())}; plan {p.splits}/{p.chunk_rows}/{p.units}")
L = _lib.lib()
stamped = hasattr(L, "m3_debug_wtn_stamps")
if stamped:
    L.m3_debug_wtn_stamps.restype = ctypes.c_int
    L.m3_debug_wtn_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
WGS, STEPS = 128, 80
SN = 2 + 4 * STEPS

for form in forms:
    rows_c = T if form == "fc2" else R
    rows_a = T if form == "fc1" else R
    sets = [(torch.randn(rows_c, N, device=dev).half(), torch.randn(rows_a, K, device=dev).half()) for _ in range(ring)]
    dW = torch.zeros(E, N, K, device=dev)
    db = torch.zeros(E, N, device=dev)
    kw = dict(M=R, group_offsets=off)
    if form == "fc1":
        kw.update(a_row_idx=row_of_slot, a_row_div=k)
    elif form == "fc2":
        kw.update(c_row_idx=row_of_slot, c_row_div=k, c_row_scale=score, db=db)
    ws = torch.empty(p.ws_elems, dtype=torch.float32, device=dev)

    def call(i):
        dC, A = sets[i % ring]
        ops.wgrad_tn(dC, A, dW, ws=ws, **kw)
    for i in range(ring):
        call(i)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for i in range(reps * ring):
        call(i)
    ev[1].record()
    torch.cuda.synchronize()
    print(f"{form}: {ev[0].elapsed_time(ev[1]) * 1000 / (reps * ring):.1f} us per call (launch + slab reduction, operands streamed)")
    if not stamped:
        continue
    assert L.m3_debug_wtn_stamps(None, WGS, 1) == 0                  # clear, then one more launch to analyse
    call(0)
    torch.cuda.synchronize()
    buf = np.zeros((WGS, SN), dtype=np.uint64)
    assert L.m3_debug_wtn_stamps(buf.ctypes.data, WGS, 0) == 0
    st = buf.astype(np.int64)
    st = st[st[:, 0] > 0]
    nst = np.array([(row[2:] > 0).sum() // 4 for row in st])          # stamped steady-state steps per workgroup
    full = st[nst >= nst.max() - 2]
    n = int(nst[nst >= nst.max() - 2].min())
    print(f"  {st.shape[0]} workgroups stamped, {full.shape[0]} of them with {n}+ loop steps; prologue (entry -> step 0 in LDS) "
          f"{np.median(full[:, 1] - full[:, 0]):.0f} cycles; entry -> last stamped barrier {np.median(full[:, 1 + 4 * n] - full[:, 0]):.0f}")
    prev = full[:, 1]
    acc = np.zeros((n, 5))
    for t in range(n):
        a, b, c, d = (full[:, 2 + 4 * t + j] for j in range(4))
        acc[t] = [np.median(a - prev), np.median(b - a), np.median(c - b), np.median(d - c), np.median(d - prev)]
        prev = d
    print("  steps      loads   mfma  data+lds  barrier   total   (median over workgroups, mean over the steps)")
    for lo in range(0, n, 16):
        hi = min(n, lo + 16)
        m = acc[lo:hi].mean(0)
        print(f"  {lo:3d}-{hi - 1:3d} {m[0]:8.0f} {m[1]:6.0f} {m[2]:9.0f} {m[3]:8.0f} {m[4]:7.0f}")
    m = acc.mean(0)
    print(f"  all     {m[0]:8.0f} {m[1]:6.0f} {m[2]:9.0f} {m[3]:8.0f} {m[4]:7.0f}")
    del sets
