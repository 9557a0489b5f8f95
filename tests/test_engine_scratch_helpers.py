"""CPU: tests/engine_scratch.py has teeth.  A small fake executor with the attribute shapes of BackboneEngine / MultiTaskStep
(parameters, a flat gradient buffer with views, operand copies, act[i] dicts holding a gate dict and a Route-like record with
__slots__, a WgradQueue, aliases everywhere): the walk finds the nested tensors, names each storage once, honours the
exemptions by name AND by storage, poison() never changes an exempt tensor's bits, integer buffers get 0, a buffer added
later is poisoned without anyone listing it, and a planted stale read - a step that sums a slack row nobody wrote this step,
masked by a zero factor - is reported."""
import pytest
import torch

import engine_scratch as es
import kernel_contract as kc


class Route:
    __slots__ = ("counts", "offsets", "pos", "row_of_slot", "tile_starts", "counts64", "n", "E", "k")


class WgradQueue:
    def __init__(self):
        self.ws = [torch.empty(32), torch.empty(32)]
        self.i, self.pending = 0, None


class FakeEngine:
    def __init__(self, share=None, dtype=torch.float16, stale_read=False):
        T, D, E, k = 12, 8, 4, 2
        self.T, self.D, self.E, self.k, self.dt = T, D, E, k, dtype
        self.stale_read = stale_read
        if share is None:
            g = torch.Generator().manual_seed(0)
            self.params = {"w": torch.randn(D, D, generator=g), "b": torch.randn(D, generator=g)}
            self.wc = {"w": self.params["w"].to(dtype)}
            self.wt = {"w": self.params["w"].t().contiguous().to(dtype)}
        else:
            self.params, self.wc, self.wt = share.params, share.wc, share.wt
        self.flat_grads = torch.zeros(D * D + D)
        self.grads = {"w": self.flat_grads[:D * D].view(D, D), "b": self.flat_grads[D * D:]}
        self.ones_k = torch.ones(T, k)
        self.act = []
        for i in range(2):
            a = {"_moe": i == 1, "x_in": None, "h": torch.empty(T, D, dtype=dtype), "x2": torch.empty(T, D)}
            if i == 1:
                a["y"] = torch.empty(T * k, D, dtype=dtype)          # expert-major: rows past this step's count are slack
            self.act.append(a)
        self.x0 = torch.empty(T, D)
        self.s_dpre = torch.empty(T * D, dtype=dtype)
        self.wq = WgradQueue()
        self.ws_wgrad = None
        self.cv_acc = torch.zeros(1)
        self.stats_rec = torch.zeros(3, dtype=torch.int32)
        self._fwd_ctx = (None, None, None, None)
        self._bw = None

    def step(self, x, rows):
        """rows: how many expert-major rows of act[1]['y'] this step's routing fills"""
        self.cv_acc.zero_()
        self.x0.copy_(x)
        a0, a1 = self.act
        a0["x_in"] = self.x0
        a0["h"].copy_(self.x0 @ self.params["w"])
        a0["x2"].copy_(a0["h"].float() + self.params["b"])
        a1["x_in"] = a0["x2"]                                        # alias of the block below, as in the engine
        meta = torch.empty(3 * self.E + 2, dtype=torch.int32)
        r = Route()
        r.counts, r.offsets, r.tile_starts = meta[:self.E], meta[self.E:2 * self.E + 1], meta[2 * self.E + 1:]
        r.pos, r.row_of_slot, r.counts64 = torch.arange(24, dtype=torch.int32), torch.arange(24, dtype=torch.int32), None
        r.n, r.E, r.k = 24, self.E, self.k
        meta.fill_(1)
        small = torch.empty(4, self.E)
        small.fill_(0.25)
        a1["gate"] = dict(route=r, score=torch.full((self.T, self.k), 0.5), importance=small[0], d_importance=small[2],
                          noise_std=0.0)
        a1["route"] = r
        a1["y"][:rows] = 1.0
        live = a1["y"][:rows].float().sum()
        if self.stale_read:
            live = live + 0.0 * a1["y"][rows:].float().sum()         # the masked read of rows nobody wrote this step
        a1["x2"].copy_(a0["x2"] + live)
        self.cv_acc += 1.0
        self._bw = dict(dx=self.x0, other=a1["x2"], cv_weight=torch.ones(1))
        self.flat_grads += 1.0
        return a1["x2"].clone(), self.cv_acc.clone()


class FakeStep:
    def __init__(self, **kw):
        self.eng = FakeEngine(**kw)
        self.engs = [self.eng, FakeEngine(share=self.eng, **kw)]
        self.flat = self.eng.flat_grads
        self.images = torch.ones(12, 8)
        self.dtok = torch.ones(12, 8)
        self.noises = {0: {1: torch.ones(12, 4)}}
        self.logit_bias = None
        self._linear_keep = (None, [], torch.zeros(1))


def _bits(t):
    return t.clone()


def test_walk_finds_nested_tensors_and_names_each_storage_once():
    e = FakeEngine()
    e.step(torch.ones(12, 8), 10)
    s = es.scratch_tensors(e)
    names = set(s)
    for want in ("act[0]['h']", "act[0]['x2']", "act[1]['y']", "x0", "s_dpre", "wq.ws[0]", "wq.ws[1]", "cv_acc",
                 "act[1]['gate']['score']", "act[1]['gate']['importance']", "act[1]['gate']['route'].counts",
                 "act[1]['gate']['route'].pos", "act[1]['gate']['route'].row_of_slot"):
        assert want in names, (want, sorted(names))
    # aliases: x_in of both blocks, a["route"] (the gate's Route again), _bw's views, offsets / tile_starts (one storage with
    # counts), d_importance (one storage with importance)
    assert not any("x_in" in n or n.startswith("_bw") or n.startswith("act[1]['route']") for n in names), sorted(names)
    assert not any(n.endswith((".offsets", ".tile_starts", "['d_importance']")) for n in names)
    ptrs = [t.untyped_storage().data_ptr() for t in s.values()]
    assert len(ptrs) == len(set(ptrs))
    # each entry covers the WHOLE storage: the gate's [4, E] block through its first row, the Route's meta through counts
    assert s["act[1]['gate']['importance']"].numel() == 16 and s["act[1]['gate']['route'].counts"].numel() == 14


def test_exemptions_by_name_and_by_storage_keep_their_bits():
    run = FakeStep()
    for e in run.engs:
        e.step(torch.ones(12, 8), 10)
    run.engs[1]._fwd_ctx = (0, None, {1: torch.ones(12, 4)}, None)
    detached = run.eng.params["w"].detach()                  # a detached parameter kept under a scratch name
    run.eng.leaf = detached
    s = es.scratch_tensors(run)
    assert any(n.startswith("engs[1].act[1]") for n in s) and "engs[0].x0" in s and "_linear_keep[2]" in s
    for n in s:
        assert not any(f".{x}" in n or n.startswith(x) for x in ("params", "flat", "grads", "wc", "wt", "ones_k", "stats_rec",
                                                                  "images", "dtok", "noises", "_fwd_ctx", "engs[0].leaf")), n
    exempt = [run.images, run.dtok, run.noises[0][1], run.flat, run.engs[1].flat_grads, run.engs[1].ones_k,
              run.engs[1].stats_rec, run.engs[1]._fwd_ctx[2][1], run.eng._bw["cv_weight"]]
    exempt += list(run.eng.params.values()) + list(run.eng.wc.values()) + list(run.eng.wt.values())
    before = [_bits(t) for t in exempt]
    es.poison(s)
    for t, b in zip(exempt, before):
        assert kc.same_bits(t, b)
    # ... and everything else is poisoned: floats hold the sentinel payload (not torch's NaN), integers 0
    assert es.holds_sentinel(run.eng.x0) and es.holds_sentinel(run.engs[1].act[1]["y"]) and es.holds_sentinel(run.eng.cv_acc)
    assert es.holds_sentinel(run.eng.wq.ws[1]) and es.holds_sentinel(run.engs[1].act[1]["gate"]["d_importance"])
    assert not es.holds_sentinel(torch.full((3,), float("nan")))
    r = run.engs[1].act[1]["route"]
    for t in (r.counts, r.offsets, r.tile_starts, r.pos, r.row_of_slot):
        assert int(t.abs().max()) == 0
    assert run.eng.x0.data_ptr() == s["engs[0].x0"].data_ptr()          # in place: same addresses


def test_a_buffer_added_later_is_poisoned_unless_it_is_argued_out():
    e = FakeEngine()
    e.s_new = torch.zeros(5, dtype=torch.bfloat16)
    e.s_new64 = torch.zeros(5, dtype=torch.float64)
    e.table = {"k": [torch.ones(3, dtype=torch.int64)]}
    s = es.scratch_tensors(e)
    assert {"s_new", "s_new64", "table['k'][0]"} <= set(s)
    es.poison(s)
    assert es.holds_sentinel(e.s_new) and es.holds_sentinel(e.s_new64) and int(e.table["k"][0].sum()) == 0
    s2 = es.scratch_tensors(e, exempt=dict(es.EXEMPT, s_new="kept between steps on purpose"))
    assert "s_new" not in s2 and "s_new64" in s2


@pytest.mark.parametrize("stale", [False, True])
def test_a_planted_stale_read_is_reported(stale):
    """steps with 24 (all), then 4 live rows: the second step's slack rows 4..23 hold the first step's values.  With finite
    leftovers the masked read (times zero) changes nothing - the older style of test passes; under poison it is a NaN in
    the step's output, and nonfinite() names it."""
    x = torch.ones(12, 8)
    e = FakeEngine(stale_read=stale)
    e.step(x, 24)
    out_plain, _ = e.step(x, 4)
    assert es.nonfinite({"tokens": out_plain}) == []                    # invisible without poison
    es.poison(es.scratch_tensors(e))
    out, cv = e.step(x, 4)
    bad = es.nonfinite({"tokens": out, "cv": cv, "flat": e.flat_grads})
    assert bad == (["tokens"] if stale else []), bad
    if not stale:
        assert torch.equal(out, out_plain) and float(cv) == 1.0
