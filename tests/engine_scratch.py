"""Engine-level analogue of kernel_contract's sentinel guards, imported by the test modules (not a conftest).

A training step may depend on this step's inputs and on the parameters only - never on what an earlier step left in the
executor's buffers.  Everything a BackboneEngine / MultiTaskStep touches is torch.empty and reused for ever, so the tests
poison all of it before every step:

* scratch_tensors(obj) - {name: flat tensor over one whole storage} of every tensor the object owns, found by walking
  vars(engine), the act[i] dicts (the gate's output dicts and the Route objects in them included), WgradQueue.ws and, for a
  step runner, every engine in `engs` and the runner's own attributes.  POISON BY DEFAULT, EXEMPT BY NAME: a buffer added to
  the engine later is poisoned unless someone adds it to EXEMPT with a reason.  Aliases are deduplicated by storage; a
  tensor that shares its storage with an exempt one (a gradient view, a detached parameter) is exempt with it.
* poison(tensors) - floating storages get kernel_contract's sentinel NaN payloads, integer ones 0: pos, row_of_slot, offsets,
  tile_starts, idx32 ... are row indices and tile counts, and a stale read of one must stay inside the engine's buffers
  (0 is in range for all of them; a wrong-but-in-range index shows in the parity and bit checks).  In place, between two
  synchronisations, so that the addresses a captured graph holds stay valid.
* nonfinite(named) / holds_sentinel(t) - what the checks ask afterwards.
"""
import torch

import kernel_contract as kc

# float64 is no kernel dtype (kernel_contract has no payload for it) but torch glue may own such a buffer
_SENT64 = 0x7FF5A5A5A5A5A5A5

# attribute names that are NOT poisoned, each with the reason it is state and not scratch
EXEMPT = {
    # ---- BackboneEngine
    "params": "the fp32 master parameters",
    "flat_grads": "the step's result; zero_grad() clears it, the caller reads it",
    "grads": "per-parameter views of flat_grads",
    "wc": "operand copies of the weights, refreshed by prepare_weights() only",
    "wt": "transposed operand copies, refreshed by prepare_weights() only",
    "wgate_c": "operand copies of w_gate, refreshed by prepare_weights() only",
    "cast_plan": "pointer table of prepare_weights()' batched cast, built once",
    "ones_k": "constant ones, written once at construction",
    "ln_table": "pointer table of the LayerNorm gradient reduction, built once",
    "stats_rec": "the routing-statistics record the caller reads after the step",
    "_fwd_ctx": "this pass's inputs (noises, DropPath factors, logit bias) as the caller handed them over",
    "_tsf": "autograd graph of the task embedding over detached parameters, rebuilt by forward_begin()",
    "ep_regroup": "expert-parallel plan state", "ep_regroup_c": "expert-parallel plan state",
    "ep_splits_host": "expert-parallel plan state (pinned host memory)", "ep_splits_host_c": "expert-parallel plan state",
    "ep_key": "expert-parallel routing keys, built once", "ep_overflow": "expert-parallel overflow flag the step reads",
    "ep_fx": "expert-parallel fixed-capacity buffers (zeroed once by design)",
    "ep_fx_bwd": "expert-parallel fixed-capacity buffers (zeroed once by design)",
    "ep_native": "expert-parallel communicator", "ep": "expert-parallel exchange plan of a block",
    "ps": "a block's DropPath factors: the caller's input",
    "cv_weight": "the upstream gradient of the balance loss: the caller's input",
    # ---- MultiTaskStep
    "images": "bound input", "dtok": "bound input", "noises": "bound input", "logit_bias": "bound input",
    "flat": "alias of the first engine's flat_grads",
}


# names that only ever alias another buffer (a block's input is the output of the block below, the backward's cursor points
# at s_dxa / s_dxb): walked last, so that they name a storage only if nothing else does
ALIASES = ("x_in", "_bw")


def _sid(t):
    return t.untyped_storage().data_ptr()


def _whole(t):
    """flat tensor of t's dtype over t's whole storage (the unit a stale read can hit)"""
    st = t.untyped_storage()
    n = st.nbytes() // t.element_size()
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(st, 0, (n,), (1,))


def _walk(obj, name, out, skip_names):
    """every tensor reachable from obj through dicts, lists, tuples and __slots__ records -> out(name, tensor).  Objects
    with a __dict__ (engines, configs, streams, graphs) are not entered: engines are walked explicitly."""
    if torch.is_tensor(obj):
        out(name, obj)
    elif isinstance(obj, dict):
        for k, v in obj.items():
            if not (isinstance(k, str) and k in skip_names):
                _walk(v, f"{name}[{k!r}]", out, skip_names)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            _walk(v, f"{name}[{i}]", out, skip_names)
    elif hasattr(type(obj), "__slots__") and not hasattr(obj, "__dict__"):
        for k in type(obj).__slots__:
            if k not in skip_names:
                _walk(getattr(obj, k, None), f"{name}.{k}", out, skip_names)
    elif type(obj).__name__ == "WgradQueue":
        _walk(obj.ws, f"{name}.ws", out, skip_names)


def _owners(obj):
    """[(prefix, object whose vars() are walked)]: a step runner and each of its engines, or one engine"""
    if hasattr(obj, "engs"):
        return [("", obj)] + [(f"engs[{j}].", e) for j, e in enumerate(obj.engs)]
    return [("", obj)]


def exempt_storages(obj, exempt=EXEMPT):
    """storage pointers of everything under an exempt name"""
    keep = set()
    for prefix, o in _owners(obj):
        for attr, v in vars(o).items():
            if attr in exempt:
                _walk(v, prefix + attr, lambda n, t: keep.add(_sid(t)) if t.numel() else None, ())
        for i, a in enumerate(getattr(o, "act", None) or []):
            for k, v in a.items():
                if k in exempt:
                    _walk(v, f"{prefix}act[{i}][{k!r}]", lambda n, t: keep.add(_sid(t)) if t.numel() else None, ())
    return keep


def scratch_tensors(obj, exempt=EXEMPT):
    """{name: flat tensor over the whole storage} of every non-exempt tensor obj owns, one entry per storage (named by the
    first path that reaches it)."""
    keep = exempt_storages(obj, exempt)
    found, seen = {}, set()

    def add(name, t):
        if t.numel() == 0:
            return
        s = _sid(t)
        if s in keep or s in seen:
            return
        seen.add(s)
        found[name] = _whole(t)

    # two passes, so that a storage is named by its owner and not by an alias met earlier in the walk
    for skip in (set(exempt) | set(ALIASES), exempt):
        for prefix, o in _owners(obj):
            for attr, v in vars(o).items():
                if attr in skip or attr in ("engs", "eng"):
                    continue
                _walk(v, prefix + attr, add, skip)
    return found


def poison(tensors):
    """sentinel bits into every floating buffer, 0 into every integer / bool buffer, in place"""
    cuda = any(t.is_cuda for t in tensors.values())
    if cuda:
        torch.cuda.synchronize()
    for t in tensors.values():
        if t.dtype in kc._SENT and t.dtype.is_floating_point:
            it, v = kc._SENT[t.dtype]
            t.view(it).fill_(v)
        elif t.dtype == torch.float64:
            t.view(torch.int64).fill_(_SENT64)
        elif t.dtype.is_floating_point or t.dtype.is_complex:
            raise TypeError(f"no sentinel for {t.dtype}")
        else:
            t.zero_()
    if cuda:
        torch.cuda.synchronize()


def holds_sentinel(t):
    """True when every element of the floating tensor t still has the sentinel bits"""
    if t.dtype == torch.float64:
        return bool((t.contiguous().view(torch.int64) == _SENT64).all())
    return kc.same_bits(t.contiguous(), kc.sentinel_like(t.contiguous()))


def nonfinite(named):
    """names of the tensors in {name: tensor} that hold an Inf or NaN"""
    return [n for n, t in named.items() if t.dtype.is_floating_point and not bool(torch.isfinite(t).all())]
