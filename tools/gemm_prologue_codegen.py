#!/usr/bin/env python3
"""Codegen record of gemm_nt_dma_kernel (no GPU): registers, scratch and occupancy of every instance, and for the four
instances the benchmark stamps (tools/gemm_stamps.py) the waits between kernel entry and the first LDS-DMA instruction.

    cd m3vit_amd/csrc
    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \
        gemm_dma.hip -o gemm_dma.s 2> gemm_dma.res
    python ../../tools/gemm_prologue_codegen.py gemm_dma.s gemm_dma.res

The prologue is read in program order up to the first global_load_lds: every basic block between entry and that instruction
counts, whichever launch form takes it, so the figures are upper bounds for one form (a dense launch skips the blocks of the
grouped lookup and of the index loads)."""
import re
import sys

asm_path, res_path = sys.argv[1], sys.argv[2]
KIND = {0: "ANY", 1: "GPRE", 2: "RES", 3: "PLAIN", 4: "GELU"}


def label(mangled):
    m = re.search(r"gemm_nt_dma_kernelI(DF16_|DF16b)Li(\d)ELb([01])E", mangled)
    if not m:
        return None
    return ("f16" if m.group(1) == "DF16_" else "bf16", KIND[int(m.group(2))], "hint" if m.group(3) == "1" else "")


res = {}
cur = None
for line in open(res_path):
    m = re.search(r"Function Name: (\S+)", line) or re.search(r" Name: (\S+)", line)
    if m:
        cur = label(m.group(1))
        res[cur] = {}
        continue
    for key in ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"):
        m = re.search(re.escape(key) + r": (\d+)", line)
        if m and cur in res and not (key == "VGPRs" and "AGPRs" in line.split("VGPRs")[0][-1:]):
            res[cur].setdefault(key, int(m.group(1)))

print("instance              VGPRs  SGPRs  scratch B/lane  waves/SIMD")
for k in sorted(k for k in res if k):
    r = res[k]
    print(f"  {k[0]:4s} {k[1]:5s} {k[2]:4s}    {r.get('VGPRs', -1):5d}  {r.get('TotalSGPRs', -1):5d}  {r.get('ScratchSize [bytes/lane]', -1):14d}  "
          f"{r.get('Occupancy [waves/SIMD]', -1):10d}")

# the prologue of the stamped instances
body = {}
cur = None
for line in open(asm_path):
    m = re.match(r"^(_ZN2m318gemm_nt_dma_kernel\S+):", line)
    if m:
        cur = label(m.group(1))
        body[cur] = []
        continue
    if cur is not None:
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            cur = None
            continue
        body[cur].append(line.strip())

print("\nentry -> first global_load_lds (program order, all blocks):")
print("instance              s_load batches  lgkmcnt(0) waits  vmcnt waits  v_loads  instructions")
for k in (("f16", "RES", ""), ("f16", "PLAIN", ""), ("f16", "GELU", "hint"), ("f16", "GPRE", "hint")):
    ins = [s for s in body.get(k, []) if s and not s.startswith((".", ";")) and not s.endswith(":")]
    first = next((i for i, s in enumerate(ins) if s.startswith("global_load_lds")), len(ins))
    pro = ins[:first]
    sl = [i for i, s in enumerate(pro) if s.startswith("s_load")]
    batches = sum(1 for j, i in enumerate(sl) if j == 0 or any(p.startswith("s_waitcnt") and "lgkmcnt" in p for p in pro[sl[j - 1]:i]))
    lg = sum(1 for s in pro if s.startswith("s_waitcnt") and "lgkmcnt(0)" in s)
    vm = sum(1 for s in pro if s.startswith("s_waitcnt") and "vmcnt" in s)
    vl = sum(1 for s in pro if s.startswith("global_load_") or s.startswith("flat_load_"))
    print(f"  {k[0]:4s} {k[1]:5s} {k[2]:4s}    {batches:14d}  {lg:16d}  {vm:11d}  {vl:7d}  {len(pro):12d}")
