"""CPU: the unit map of the balanced grouped weight gradient through the host query m3_wgrad_unit_of, which walks the groups
with the two functions the kernels and m3_wgrad_reduce_grouped compute the map with (csrc/wgrad_dev.h:
wgrad_units_of_group, wgrad_unit_rows).  Group g gets ceil(rows_g / chunk) units that share its rows equally in whole 64-row
granules; the slab slots m3_wgrad_plan reserves cover them; the benchmarked plan table is unchanged."""
import ctypes
import random

import pytest
import torch

WG_ROWS = 64
CHUNKS = [64, 128, 2368]


def unit_of(offsets, chunk, unit):
    from m3vit_amd import _lib
    off = (ctypes.c_int32 * len(offsets))(*offsets)
    g, b, e = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    rc = _lib.lib().m3_wgrad_unit_of(off, len(offsets) - 1, chunk, unit, ctypes.byref(g), ctypes.byref(b), ctypes.byref(e))
    assert rc == 0, _lib.lib().m3_last_error()
    return g.value, b.value, e.value


def offsets_of(rows):
    off = [0]
    for r in rows:
        off.append(off[-1] + r)
    return off


def edge_rows(chunk):
    """0, 1, around one granule, around one and two chunks, and one group of 5.9 x the mean of all nine"""
    base = [0, 1, 63, 64, 65, chunk, chunk + 1, 2 * chunk - 1]
    hot = round(5.9 * sum(base) / (len(base) + 1 - 5.9))
    rows = base + [hot]
    assert abs(hot / (sum(rows) / len(rows)) - 5.9) < 0.01
    return rows


def check_layout(rows, chunk, slots):
    """every property of the map for one layout; returns the units per group"""
    off = offsets_of(rows)
    G = len(rows)
    per_group = [[] for _ in rows]
    total = sum(-(-r // chunk) for r in rows)
    assert total <= slots, (rows, chunk, slots)
    last_g = -1
    for u in range(total):
        g, b, e = unit_of(off, chunk, u)
        assert 0 <= g < G and g >= last_g, (u, g)                       # dealt to the groups in order
        last_g = g
        per_group[g].append((b, e))
    for u in range(total, slots + 1):                                   # surplus slots: no group, no rows
        assert unit_of(off, chunk, u) == (-1, 0, 0)
    for g, units in enumerate(per_group):
        assert len(units) == -(-rows[g] // chunk), (g, rows[g], units)  # ceil(rows / chunk) - none for an empty group
        pos = off[g]
        for j, (b, e) in enumerate(units):
            assert b == pos and e > b, (g, j, units)                    # once, in order, never empty
            assert e - b <= chunk
            if j + 1 < len(units):
                assert (e - b) % WG_ROWS == 0, (g, j, units)
            pos = e
        assert pos == off[g + 1]
        if units:                                                       # equal shares: ceil(rows / n) rounded up to whole granules,
            n = len(units)                                              # the last unit takes what is left
            each = -(-rows[g] // n)
            share = -(-each // WG_ROWS) * WG_ROWS
            assert [e - b for b, e in units] == [share] * (n - 1) + [rows[g] - (n - 1) * share]
    return per_group


@pytest.mark.parametrize("chunk", CHUNKS)
def test_units_tile_every_group_in_equal_shares(chunk):
    rows = edge_rows(chunk)
    rng = random.Random(chunk)
    for layout in (rows, rows[::-1], rng.sample(rows, len(rows))):
        check_layout(layout, chunk, sum(layout) // chunk + len(layout))   # the slots the header promises suffice


def test_near_mean_expert_of_the_benchmarked_plan():
    """configs[1]'s expert launches: 100 864 routed rows over 16 experts plan as 3 / 2368 / 58; an expert at the mean (6 304
    rows) runs as 2112 + 2112 + 2080, not 2368 + 2368 + 1568, and random layouts stay inside the plan's 58 slots"""
    from m3vit_amd import ops
    p = ops.wgrad_launch_plan(100864, 384, 384, 16, torch.float16, grouped=True)
    assert (p.splits, p.chunk_rows, p.units) == (3, 2368, 58)
    per_group = check_layout([6304] * 16, p.chunk_rows, p.units)
    assert [e - b for b, e in per_group[5]] == [2112, 2112, 2080]
    rng = random.Random(11)
    for _ in range(20):
        cuts = sorted(rng.randint(0, 100864) for _ in range(15))
        rows = [b - a for a, b in zip([0] + cuts, cuts + [100864])]
        check_layout(rows, p.chunk_rows, p.units)
    check_layout([100864] + [0] * 15, p.chunk_rows, p.units)              # everything on one expert


def test_bad_arguments_are_refused():
    from m3vit_amd import _lib
    off = (ctypes.c_int32 * 3)(0, 10, 5)
    g, b, e = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    L = _lib.lib()
    out = (ctypes.byref(g), ctypes.byref(b), ctypes.byref(e))
    assert L.m3_wgrad_unit_of(off, 2, 64, 1, *out) != 0                   # offsets that decrease
    good = (ctypes.c_int32 * 3)(0, 10, 15)
    assert L.m3_wgrad_unit_of(good, 2, 48, 0, *out) != 0                  # chunk_rows no multiple of 64
    assert L.m3_wgrad_unit_of(good, 65, 64, 0, *out) != 0                 # more groups than lanes
    assert L.m3_wgrad_unit_of(good, 2, 64, -1, *out) != 0
    assert L.m3_wgrad_unit_of(good, 2, 64, 1, *out) == 0 and (g.value, b.value, e.value) == (1, 10, 15)


def test_benchmarked_plan_table_is_unchanged():
    """the table tests/test_cabi_symbols.py pins, asserted again (read-only): splits / chunk_rows / units of fc1, fc2, qkv,
    proj, expert fc1, expert fc2, patch, gate in the three benchmarked configurations"""
    from m3vit_amd import ops
    h, f = torch.float16, torch.float32
    table = {
        (25216, 25088, 384, 1536, 384, 16, 100864, h): "14/0/14 14/0/14 16/0/16 32/0/32 3/2368/58 3/2368/58 28/0/28 256/0/256",
        (25216, 25088, 384, 1536, 384, 16, 100864, f): "28/0/28 28/0/28 37/0/37 48/0/48 7/1024/114 7/1024/114 48/0/48 256/0/256",
        (25216, 25088, 768, 3072, 768, 64, 100864, h): "7/0/7 7/0/7 8/0/8 28/0/28 1/1792/120 1/1792/120 28/0/28 32/0/32",
        (25216, 25088, 768, 3072, 768, 64, 100864, f): "7/0/7 7/0/7 8/0/8 28/0/28 1/1792/120 1/1792/120 28/0/28 48/0/48",
        (9608, 9600, 768, 3072, 3072, 16, 38432, h): "7/0/7 7/0/7 8/0/8 16/0/16 1/2752/29 1/2752/29 16/0/16 150/0/150",
        (9608, 9600, 768, 3072, 3072, 16, 38432, f): "7/0/7 7/0/7 8/0/8 16/0/16 1/2752/29 1/2752/29 16/0/16 150/0/150",
    }
    for (T, Tp, D, Hd, Hm, E, R, dt), want in table.items():
        shapes = [(T, Hd, D, 1), (T, D, Hd, 1), (T, 3 * D, D, 1), (T, D, D, 1), (R, Hm, D, E), (R, D, Hm, E), (Tp, D, 768, 1), (T, D, E, 1)]
        got = [ops.wgrad_launch_plan(M, N, K, G, dt, grouped=G > 1) for M, N, K, G in shapes]
        assert " ".join(f"{p.splits}/{p.chunk_rows}/{p.units}" for p in got) == want, (T, D, E, dt)
