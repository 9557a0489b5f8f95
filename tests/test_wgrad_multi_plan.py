"""CPU: m3_wgrad_multi_plan is host code - which batches of dense weight gradients one launch may take, and how it cuts them:
one common number of row parts, the fewest that fill 432 workgroups without exceeding the 512 resident ones, at most 16 and
at least 16 32-row steps each."""
import pytest
import torch

h, bf, f32 = torch.float16, torch.bfloat16, torch.float32
T = 128 * 197                                            # configs[1]: batch 128, 197 tokens
D, Hd = 384, 1536
DENSE = [(D, Hd, True), (Hd, D, True), (D, D, True), (3 * D, D, True)]        # fc2, fc1, proj, qkv
MOE = [(D, D, True), (3 * D, D, True)]


@pytest.fixture(scope="module")
def ops():
    from m3vit_amd import ops as _ops
    return _ops


def test_configs1_batches(ops):
    for dt in (h, bf):
        p = ops.wgrad_multi_plan(DENSE, T, dt)
        assert p.allowed and (p.tiles, p.parts, p.workgroups) == (108, 4, 432)
        assert p.ws_elems == 4 * sum(N * (K + 1) for N, K, _ in DENSE) == ops.wgrad_multi_ws_elems(DENSE, T, dt)
        q = ops.wgrad_multi_plan(MOE, T, dt)
        assert q.allowed and (q.tiles, q.parts, q.workgroups) == (36, 12, 432)
        assert q.ws_elems == 12 * sum(N * (K + 1) for N, K, _ in MOE)
        for pl in (p, q):
            assert 432 <= pl.parts * pl.tiles <= 512
    # slabs: problem after problem, then the bias slabs; no bias, no bias slabs
    p = ops.wgrad_multi_plan([(D, D, False), (3 * D, D, True)], T, h)
    assert list(p.ws_off[:2]) == [0, 12 * D * D] and p.bias_off[1] == 12 * 4 * D * D and p.ws_elems == 12 * (4 * D * D + 3 * D)


def test_parts_rule(ops):
    one = [(128, 128, False)]
    # at least 16 steps of 32 rows (the last may be partial) per part, at most 16 parts
    assert [ops.wgrad_multi_plan(one, M, h).parts for M in (1, 65, 591, 992, 993, 2048, 8192, 1 << 20)] == [1, 1, 1, 1, 2, 4, 16, 16]
    # never a second round of workgroups: 130 tiles x 4 parts = 520 > 512 -> 3 parts; more tiles than slots -> 1
    assert ops.wgrad_multi_plan([(130 * 128, 128, False)], T, h).parts == 3
    assert ops.wgrad_multi_plan([(8 * 128, 128, False)] * 8, T, h).parts == 7          # 64 tiles: 448 workgroups
    assert ops.wgrad_multi_plan([(600 * 128, 128, False)], T, h).parts == 1
    # the caller's parts are taken as they are
    p = ops.wgrad_multi_plan(DENSE, 65, h, 3)
    assert (p.parts, p.workgroups) == (3, 324)


def test_allowed_and_refused_batches(ops):
    ok = lambda shapes, dt=h, M=T: bool(ops.wgrad_multi_plan(shapes, M, dt).allowed)          # noqa: E731
    assert ok(DENSE) and ok(MOE) and ok(DENSE, bf) and ok([(136, 72, True), (8, 8, False), (128, 264, True)], h, 65)
    assert not ok(DENSE, f32) and not ok(MOE, f32)                      # fp32 keeps its launch per weight
    assert not ok(DENSE, h, 0)                                          # nothing to contract over
    for vitb in ([(768, 768, True)], [(2304, 768, True)], [(768, 3072, True)], MOE + [(3072, 768, True)]):
        assert not ok(vitb), vitb                                       # the 256 x 256 kernel's shapes
    assert not ok([(4608, 384, True)])                                  # N K >= 1.5 M: the LDS-DMA kernel's
    assert not ok([(384, 16, False)])                                   # the router's weight: the streaming kernel's
    ops.wgrad_set_big(0); ops.wgrad_set_dma(0)
    try:
        assert ok([(768, 768, True)]) and ok([(4608, 384, True)])       # the rule follows the kernel choice of the single call
    finally:
        ops.wgrad_set_big(-1); ops.wgrad_set_dma(-1)
    with pytest.raises(AssertionError):
        ops.wgrad_multi_plan([], T, h)
    with pytest.raises(AssertionError):
        ops.wgrad_multi_plan([(8, 8, False)] * 9, T, h)
