"""CPU: the C-ABI library loads and exports every symbol include/m3vit_hip.h declares
(no compute calls without a GPU)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "m3vit_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(m3_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_all_bound_and_exported():
    from m3vit_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    names = _declared()
    assert len(names) >= 25
    assert sorted(_lib.SIGNATURES) == names, set(names) ^ set(_lib.SIGNATURES)
    L = _lib.lib()
    for n in names:
        assert hasattr(L, n), n
    assert L.m3_version() >= 100
    assert L.m3_gate_num_blocks(25216) == 394
    assert L.m3_route_ws_elems(100864, 16) > 0


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from m3vit_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.M3Error):
        _lib.lib()


def test_wgrad_plan_covers_every_group_layout():
    """host logic of the balanced grouped weight gradient: for any split of M rows over G groups the slab slots the
    host reserves (M // chunk + G) cover the units the kernel deals out (sum of ceil(rows_g / chunk)), the chunk is a
    multiple of the 32-row step, and groups at the mean size keep `splits` units"""
    import random
    import torch
    from m3vit_amd import ops
    rng = random.Random(7)
    for _ in range(300):
        G = rng.choice([2, 4, 16, 64])
        M = rng.randint(1, 200000)
        N, K = rng.choice([(384, 384), (1536, 384), (768, 3072)])
        p = ops.wgrad_launch_plan(M, N, K, G, torch.float16, grouped=True)
        splits, chunk, units = p.splits, p.chunk_rows, p.units
        assert splits == ops.default_wgrad_splits(M, N, K, G, torch.float16)
        assert chunk % 32 == 0 and chunk >= 32
        cuts = sorted(rng.randint(0, M) for _ in range(G - 1))
        rows = [b - a for a, b in zip([0] + cuts, cuts + [M])]
        if rng.random() < 0.3:                      # everything on one group
            rows = [M] + [0] * (G - 1)
        need = sum(-(-r // chunk) for r in rows)
        assert need <= units, (M, G, splits, chunk, rows)
        assert -(-(M // G) // chunk) <= splits
        assert ops.wgrad_ws_elems(M, N, K, G, grouped=True, dtype=torch.float16) == units * N * (K + 1) == p.ws_elems
        assert ops.wgrad_ws_elems(M, N, K, G, grouped=True, bias=False, dtype=torch.float16) == units * N * K
        assert ops.wgrad_plan(M, G, splits, grouped=True) == (chunk, units)
    assert ops.wgrad_plan(1000, 1, 4, grouped=True) == (0, 4)          # one group: equal parts
    assert ops.wgrad_plan(1000, 128, 2, grouped=True) == (0, 256)      # more groups than lanes: equal parts


def test_wgrad_tile_rule_and_splits_on_the_host():
    """m3_wgrad_tile is host code: the tile rule (256 x 256 for 16-bit weights whose N and K are multiples of 256, else
    128 x 128) and the split heuristic that goes with it (one-per-CU slots for the big tile; grouped calls with more tiles
    than slots take one unit per expert)"""
    import torch
    from m3vit_amd import ops
    h = torch.float16
    for N, K in ((384, 384), (1000, 384), (1536, 384), (384, 1536)):
        assert ops.wgrad_tile(N, K, h) == (128, 128) and ops.wgrad_tile(N, K, torch.float32) == (128, 128), (N, K)
    # the default split rule follows the kernel that takes the launch (m3_wgrad_set_dma's rule): 1024 slots where the LDS-DMA
    # kernel runs (fp32; 16-bit weights of >= 1.5 M elements or launches whose tiles fill the chip), 512 for the register-staged one
    assert ops.default_wgrad_splits(25216, 1536, 384, 1, h) == 14 and ops.default_wgrad_splits(25216, 1536, 384, 1, torch.float32) == 28
    assert ops.wgrad_tile(3072, 768, h) == (256, 256) and ops.default_wgrad_splits(25216, 3072, 768, 1, h) == 7   # ViT-Base fc1: 36 big tiles on 256 slots
    ops.wgrad_set_big(0)
    try:
        assert ops.wgrad_tile(3072, 768, h) == (128, 128)
        assert ops.default_wgrad_splits(25216, 3072, 768, 1, h) == 7                # 144 tiles on 1024 slots
        ops.wgrad_set_dma(0)
        try:
            assert ops.default_wgrad_splits(25216, 3072, 768, 1, h) == 3 and ops.default_wgrad_splits(25216, 1536, 384, 1, torch.float32) == 14
        finally:
            ops.wgrad_set_dma(-1)
        assert ops.default_wgrad_splits(38432, 3072, 768, 16, h) == 1              # the ViT-Base experts: tiles fill the chip -> direct mode
    finally:
        ops.wgrad_set_big(-1)
    assert ops.default_wgrad_splits(38432, 3072, 768, 16, h) == 1                  # (and with the big tile: 576 tiles on 256 slots)
    # dense row parts come in whole multiples of the 8 XCDs where that costs at most an eighth of them: one 128 x 128 tile and
    # 512 n rows would be cut into n parts (fp32: up to 128; 16 bit: up to 32)
    ns = (1, 7, 8, 9, 14, 18, 28, 32, 37)
    assert [ops.default_wgrad_splits(512 * n, 128, 128, 1, torch.float32) for n in ns] == [1, 7, 8, 8, 14, 16, 28, 32, 37]
    assert [ops.default_wgrad_splits(512 * n, 128, 128, 1, h) for n in ns] == [1, 7, 8, 8, 14, 16, 28, 32, 32]
    assert ops.default_wgrad_splits(25216, 1152, 384, 1, h) == 16 and ops.default_wgrad_splits(25216, 2304, 768, 1, h) == 8
    # the eight weight-gradient shapes the engine sizes its workspace for (engine.py: shapes = [...]) in BASELINE's three
    # benchmarked configurations, as splits / chunk_rows / units: fc1, fc2, qkv, proj, expert fc1, expert fc2, patch, gate
    f = torch.float32
    table = {
        (25216, 25088, 384, 1536, 384, 16, 100864, h): "14/0/14 14/0/14 16/0/16 32/0/32 3/2368/58 3/2368/58 28/0/28 256/0/256",
        (25216, 25088, 384, 1536, 384, 16, 100864, f): "28/0/28 28/0/28 37/0/37 48/0/48 7/1024/114 7/1024/114 48/0/48 256/0/256",
        (25216, 25088, 768, 3072, 768, 64, 100864, h): "7/0/7 7/0/7 8/0/8 28/0/28 1/1792/120 1/1792/120 28/0/28 32/0/32",
        (25216, 25088, 768, 3072, 768, 64, 100864, f): "7/0/7 7/0/7 8/0/8 28/0/28 1/1792/120 1/1792/120 28/0/28 48/0/48",
        (9608, 9600, 768, 3072, 3072, 16, 38432, h): "7/0/7 7/0/7 8/0/8 16/0/16 1/2752/29 1/2752/29 16/0/16 150/0/150",
        (9608, 9600, 768, 3072, 3072, 16, 38432, f): "7/0/7 7/0/7 8/0/8 16/0/16 1/2752/29 1/2752/29 16/0/16 150/0/150",
    }
    direct = 0
    for (T, Tp, D, Hd, Hm, E, R, dt), want in table.items():
        shapes = [(T, Hd, D, 1), (T, D, Hd, 1), (T, 3 * D, D, 1), (T, D, D, 1), (R, Hm, D, E), (R, D, Hm, E), (Tp, D, 768, 1), (T, D, E, 1)]
        got = [ops.wgrad_launch_plan(M, N, K, G, dt, grouped=G > 1) for M, N, K, G in shapes]
        assert " ".join(f"{p.splits}/{p.chunk_rows}/{p.units}" for p in got) == want, (T, D, E, dt)
        for (M, N, K, G), p in zip(shapes, got):
            assert not p.direct and p.ws_elems == p.units * N * (K + 1)
            q = ops.wgrad_launch_plan(M, N, K, G, dt, grouped=G > 1, direct_ok=True)
            if p.splits == 1:                    # one part per group: the caller that can take direct mode gets it
                assert (q.splits, q.direct, q.chunk_rows, q.units, q.ws_elems) == (1, 1, 0, G, 0)
                direct += 1
            else:
                assert (q.splits, q.direct, q.chunk_rows, q.units, q.ws_elems) == (p.splits, 0, p.chunk_rows, p.units, p.ws_elems)
    assert direct == 8
