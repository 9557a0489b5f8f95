"""m3vit_amd.ops.graph_capture - every hipGraph capture of the package (m3vit_amd/step.py, m3vit_amd/fused.py) - holds
Python's cyclic garbage collector off while the capture is open (a collection inside a capture runs finalizers whose HIP
calls are not allowed on a capturing thread) and gives it back afterwards, also when the captured code raises; decided
without touching the GPU (torch.cuda.graph replaced by a recorder)."""
import contextlib
import gc

import pytest
import torch


def test_graph_capture_holds_the_collector_off_and_restores_it(monkeypatch):
    from m3vit_amd import ops
    seen = []

    @contextlib.contextmanager
    def fake_graph(g, capture_error_mode="global"):
        seen.append(("enter", g, capture_error_mode, gc.isenabled()))
        yield
        seen.append(("exit", gc.isenabled()))
    monkeypatch.setattr(torch.cuda, "graph", fake_graph)
    was = gc.isenabled()
    gc.enable()
    try:
        with ops.graph_capture("g0"):
            seen.append(("body", gc.isenabled()))
        assert seen == [("enter", "g0", "thread_local", False), ("body", False), ("exit", False)]
        assert gc.isenabled()
        with pytest.raises(RuntimeError, match="boom"):
            with ops.graph_capture("g1"):
                raise RuntimeError("boom")
        assert gc.isenabled()
        gc.disable()                                  # a caller that runs with the collector off keeps it off
        with ops.graph_capture("g2"):
            pass
        assert not gc.isenabled()
    finally:
        (gc.enable if was else gc.disable)()
