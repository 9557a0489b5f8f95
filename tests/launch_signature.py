"""What a call of m3_gemm_nt / m3_wgrad_tn / m3_wgrad_multi / m3_attention_fwd / m3_attention_bwd IS, for the purpose of
coverage: a signature made only of what the library's own plan reports for the argument struct (m3_gemm_plan,
m3_wgrad_kernel, m3_attention_plan: the kernel, its template instance, the tile) and of the call's option pattern (which
optional operands are there, how rows are gathered, which tiles are partial).  Shapes and pointers do not enter: two calls
with the same signature run the same code on the device.

The contract modules compute the signature of every case from the struct they launch; the engine census
(test_engine_launch_census_gpu.py) computes it from the structs `ops` filled for the engine, recorded at the C-ABI boundary
by Recorder; the CPU test (test_launch_paths_cpu.py) computes it from dummy structs.  Everything here is host code."""
from collections import Counter

import torch

DT_NAME = {0: "f32", 1: "f16", 2: "bf16"}
ROWB = 128                  # bytes of K per row per step of the GEMM kernels: K * elem % ROWB != 0 is a K tail
DUMMY = 0x10000             # an aligned non-null address for a struct that is only planned, never launched


def _es(code):
    return 4 if code == 0 else 2


def _div_kind(ptr, div):
    """how rows are gathered: none, a power-of-two divisor (the kernels shift) or another one (they divide)"""
    if not ptr:
        return "none"
    return "pow2" if div >= 1 and div & (div - 1) == 0 else "other"


class Sig(tuple):
    """a signature: a tuple of (field, value) pairs that prints as one line"""

    def __str__(self):
        return " ".join(f"{k}={v}" for k, v in self)

    def get(self, key):
        return dict(self)[key]


def copy_struct(a, **fields):
    b = type(a).from_buffer_copy(a)
    for k, v in fields.items():
        setattr(b, k, v)
    return b


def gemm_signature(ops, a) -> Sig:
    from m3vit_amd import _lib
    p = ops.gemm_plan(a)
    es = _es(a.dtype)
    grouped = bool(a.group_offsets)
    return Sig((
        ("op", "gemm"), ("kernel", _lib.GEMM_KERNELS[p.kernel]), ("epi", _lib.GEMM_EPILOGUES[p.epilogue]),
        ("dtype", DT_NAME[a.dtype]), ("c", DT_NAME[a.c_dtype]), ("grouped", int(grouped)),
        ("gatherA", _div_kind(a.a_row_idx, a.a_row_div)), ("scatterC", int(bool(a.c_row_idx))),
        ("rs", "none" if not a.row_scale else ("idx" if a.row_scale_idx else "div")),
        ("bias", int(bool(a.bias))),
        ("res", "none" if not a.residual else ("inplace" if a.residual == a.C else "separate")),
        ("pre", int(bool(a.pre_out))), ("gpre", int(bool(a.gelu_grad_pre))), ("vec8", p.vec8),
        ("ktail", int(a.K * es % ROWB != 0)),
        # a grouped call's groups end where the device-resident offsets say: every group may end in a partial row tile
        ("mtail", int(grouped or a.M % p.tile_m != 0)), ("ntail", int(a.N % p.tile_n != 0)),
    ))


def wgrad_signature(ops, a) -> Sig:
    from m3vit_amd import _lib
    k = ops.wgrad_kernel(a)
    return Sig((
        ("op", "wgrad"), ("kernel", _lib.WGRAD_KERNELS[k.kernel]), ("gc", k.gather_c), ("ga", k.gather_a), ("sc", k.scale_c),
        ("dtype", DT_NAME[a.dtype]), ("grouped", int(bool(a.group_offsets))),
        ("gatherC", _div_kind(a.c_row_idx, max(a.c_row_div, 1))), ("gatherA", _div_kind(a.a_row_idx, a.a_row_div)),
        ("mode", "direct" if a.direct_dW else ("balanced" if a.chunk_rows else "slabs")),
        ("bias", int(bool(a.bias_ws or a.direct_db))),
        ("ntail", int(a.N % k.tile_n != 0)), ("ktail", int(a.K % k.tile_k != 0)),
    ))


def wgrad_multi_signature(ops, a) -> Sig:
    """m3_wgrad_multi has one kernel per dtype (wgrad_multi.hip) and plain rows only: the dtype, whether bias column sums
    ride along and whether some problem has a partial 128 x 128 tile"""
    pr = [a.prob[j] for j in range(a.n)]
    return Sig((
        ("op", "wgrad_multi"), ("dtype", DT_NAME[a.dtype]), ("bias", int(any(q.db for q in pr))),
        ("tail", int(any(q.N % 128 or q.K % 128 for q in pr))),
    ))


def attention_signature(ops, which, dtype_code, N, dh) -> Sig:
    from m3vit_amd import _lib
    dtype = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}[dtype_code]
    p = ops.attention_plan(dtype, N, dh)
    tiles = (N + 15) // 16
    fam, inst = (p.fwd_family, p.fwd_key_tiles) if which == "fwd" else (p.bwd_family, p.bwd_tiles_per_wave)
    fields = [("op", "attention_" + which), ("family", _lib.ATTN_FAMILIES[fam]), ("instance", inst), ("dtype", DT_NAME[dtype_code]),
              ("dh", dh), ("partial_tile", int(N % 16 != 0))]
    if which == "fwd":            # wholly masked key tiles of the resident forward's instance (keys >= N in the last four tiles)
        fields.append(("masked_tiles", p.fwd_key_tiles - tiles if p.fwd_key_tiles else 0))
    else:
        fields.append(("key_blocks", "many" if p.bwd_key_blocks > 1 else "one"))
    return Sig(fields)


# ------------------------------------------------------------------------------------------------ recording
class _Proxy:
    """the loaded library with the five launching entry points wrapped: each call is noted, then made unchanged"""

    def __init__(self, real, rec):
        self._real, self._rec = real, rec

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in ("m3_gemm_nt", "m3_wgrad_tn", "m3_wgrad_multi", "m3_attention_fwd", "m3_attention_bwd"):
            return fn
        rec = self._rec

        def call(*args):
            rec.note(name, args)
            return fn(*args)
        return call


class Recorder:
    """with Recorder(ops) as rec: ... -> rec.calls, a list of (entry point, copy of the argument struct | argument tuple,
    the m3_wgrad_plan request ops made for the call | None).  The struct is copied as `ops` filled it, before the call; the
    call itself goes through with the very same arguments."""

    def __init__(self, ops):
        self.ops, self.calls, self._plan_req = ops, [], None

    def note(self, name, args):
        if name.startswith("m3_attention"):
            # (qkv, dtype, B, N, heads, dh, ..) / (qkv, o, d_o, lse, dtype, B, N, heads, dh, ..)
            dt, B, N, h, dh = args[1:6] if name == "m3_attention_fwd" else args[4:9]
            self.calls.append((name, (dt, B, N, h, dh), None))
        else:
            a = args[0]._obj                                  # byref(struct)
            self.calls.append((name, copy_struct(a), self._plan_req if name == "m3_wgrad_tn" else None))
        self._plan_req = None

    def __enter__(self):
        ops = self.ops
        self._lib, self._plan = ops.lib, ops.wgrad_launch_plan
        proxy = _Proxy(ops.lib(), self)
        ops.lib = lambda: proxy

        def plan(M, N, K, G, dtype, **kw):                    # what ops.wgrad_tn asks m3_wgrad_plan right before its launch
            self._plan_req = (M, N, K, G, dtype, dict(kw))
            return self._plan(M, N, K, G, dtype, **kw)
        ops.wgrad_launch_plan = plan
        return self

    def __exit__(self, *exc):
        self.ops.lib, self.ops.wgrad_launch_plan = self._lib, self._plan


def signature_of(ops, name, a):
    if name == "m3_gemm_nt":
        return gemm_signature(ops, a)
    if name == "m3_wgrad_tn":
        return wgrad_signature(ops, a)
    if name == "m3_wgrad_multi":
        return wgrad_multi_signature(ops, a)
    dt, B, N, h, dh = a
    return attention_signature(ops, "fwd" if name == "m3_attention_fwd" else "bwd", dt, N, dh)


def at_batch(ops, name, a, plan_req, num, den):
    """the same call with its rows scaled by num / den (the engine's row counts - tokens, routed rows, patches - are all
    proportional to the batch): for planning only.  A weight-gradient call is cut up again by m3_wgrad_plan for the new
    row count, from the request ops made for the recorded call, and the struct's mode fields follow the plan the way
    ops.wgrad_tn sets them."""
    if name.startswith("m3_attention") or num == den:
        return a
    assert a.M * num % den == 0, (name, a.M, num, den)
    M = a.M * num // den
    if name != "m3_wgrad_tn":
        return copy_struct(a, M=M)
    assert plan_req is not None and plan_req[0] == a.M, "a recorded m3_wgrad_tn call without its m3_wgrad_plan request"
    _, N, K, G, dtype, kw = plan_req
    p = ops.wgrad_launch_plan(M, N, K, G, dtype, **kw)
    bias = bool(a.bias_ws or a.direct_db)
    return copy_struct(a, M=M, splits=p.splits, chunk_rows=p.chunk_rows, units=p.units,
                       direct_dW=DUMMY if p.direct else None, direct_db=DUMMY if p.direct and bias else None,
                       bias_ws=DUMMY if bias and not p.direct else None, ws=DUMMY)


def census(ops, calls, num=1, den=1) -> Counter:
    """signature -> launch count of recorded calls, planned with their rows scaled by num / den"""
    out = Counter()
    for name, a, req in calls:
        out[signature_of(ops, name, at_batch(ops, name, a, req, num, den))] += 1
    return out
