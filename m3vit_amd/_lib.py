"""ctypes loader for libm3vit_hip.so (the C ABI declared in include/m3vit_hip.h).

There is deliberately NO fallback: if the HIP library is missing or a call fails the
error is raised, never papered over by a torch/CPU path.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("M3VIT_LIB") or os.path.join(_HERE, "libm3vit_hip.so")   # M3VIT_LIB: diagnostic builds


class M3Error(RuntimeError):
    pass


# ---- the bindings are READ from include/m3vit_hip.h at import (text only: the library is not needed for this) ----
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "m3vit_hip.h")
_SCALAR = {"int": c_int, "int32_t": c_int32, "int64_t": c_int64, "float": c_float, "double": c_double}
_DECL = r"(?:const\s+)?(\w+)(?:\s+|\s*(\*+)\s*)([A-Za-z_]\w*)"      # [const] type [*] name
_DIM = r"\s*(?:\[(\w+)\])?"


def read_header(text):
    """(constants, structs, signatures) of a header in the one style include/m3vit_hip.h is written in:
    `#define M3_X <integer>`, `typedef struct [tag] { fields } m3_x;` and `type m3_f(parameters);`.  Anything else - a
    declaration of another form, a type it does not know - raises M3Error naming the text; nothing is skipped."""
    consts, structs, sigs = {}, {}, {}

    def bad(what):
        raise M3Error(f"m3vit_hip.h: cannot read the declaration {' '.join(what.split())!r}")

    def ctype(base, stars, name, dim, what):
        stars = stars or ""
        if not stars and base in _SCALAR:
            t = _SCALAR[base]
        elif not stars and base in structs:
            t = structs[base]
        elif stars == "*" and base == "char":
            t = c_char_p
        elif stars == "*" and base == "int":
            t = POINTER(c_int)
        elif stars == "*" and base in structs and not name.endswith("_dev"):     # a struct the HOST fills
            t = POINTER(structs[base])
        elif stars == "*" and (base == "void" or base in _SCALAR or base in structs):   # a device address
            t = c_void_p
        else:
            bad(what)
        if dim is None:
            return t
        return t * (consts[dim] if dim in consts else int(dim) if dim.isdigit() else bad(what))

    def define(m):
        if m[1].startswith("M3_"):
            v = re.fullmatch(r"\(?(-?\d+)\)?", m[2].strip()) or bad(m[0])
            consts[m[1]] = int(v[1])
        return ""

    def struct(m):
        fields = []
        for stmt in filter(None, map(str.strip, m[1].split(";"))):                # `type a, *b, c[N]`
            first, *more = stmt.split(",")
            head = re.fullmatch(_DECL + _DIM, first.strip()) or bad(stmt)
            rest = [re.fullmatch(r"(\*+)?\s*([A-Za-z_]\w*)" + _DIM, s.strip()) or bad(stmt) for s in more]
            for stars, name, dim in [head.groups()[1:]] + [r.groups() for r in rest]:
                fields.append((name, ctype(head[1], stars, name, dim, stmt)))
        structs[m[2]] = type(m[2], (Structure,), {"_fields_": fields})
        return ""

    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(.*)$", define, text, flags=re.M)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)                            # include guard, <stdint.h>, __cplusplus
    text = re.sub(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    for stmt in filter(None, map(str.strip, text.split(";"))):                   # what is left: prototypes
        m = re.fullmatch(_DECL + r"\s*\((.*)\)", stmt, flags=re.S)
        if not m or not m[3].startswith("m3_"):
            bad(stmt)
        params = [] if m[4].strip() == "void" else [re.fullmatch(_DECL, p.strip()) or bad(stmt) for p in m[4].split(",")]
        sigs[m[3]] = (ctype(m[1], m[2], "", None, stmt), [ctype(p[1], p[2], p[3], None, stmt) for p in params])
    return consts, structs, sigs


with open(_HEADER) as _f:
    CONSTANTS, STRUCTS, SIGNATURES = read_header(_f.read())     # SIGNATURES: name -> (restype, argtypes)
globals().update(CONSTANTS)                                     # M3_F32, M3_OPTIM_CHUNK, ...: every #define M3_* of the header
globals().update({py: STRUCTS["m3_" + c] for py, c in {         # the Python names of the header's typedefs
    "GemmArgs": "gemm_args", "GemmPlan": "gemm_plan_out", "WgradArgs": "wgrad_args", "WgradReduceDesc": "wgrad_reduce_desc",
    "WgradKernelOut": "wgrad_kernel_out", "WgradShape": "wgrad_shape", "WgradPlan": "wgrad_plan_out",
    "WgradProblem": "wgrad_problem", "WgradMultiShape": "wgrad_multi_shape", "WgradMultiPlan": "wgrad_multi_plan_out",
    "WgradMultiArgs": "wgrad_multi_args", "AttentionPlan": "attention_plan_out", "CastDesc": "cast_desc",
    "OptimDesc": "optim_desc", "GateFwdArgs": "gate_fwd_args", "GateBwdArgs": "gate_bwd_args",
    "LnParamGrads": "ln_param_grads", "AugmentDesc": "augment_desc", "Conv3x3Plan": "conv3x3_plan_out",
    "ShareRows": "share_rows"}.items()})
WGRAD_MULTI_MAX = CONSTANTS["M3_WGRAD_MULTI_MAX"]


def _names(prefix, but=" "):
    """value -> lower-case name of the M3_<prefix>* constants (those of the sub-family `but` left out)"""
    return {v: k[len(prefix):].lower() for k, v in CONSTANTS.items() if k.startswith(prefix) and not k.startswith(but)}


GEMM_KERNELS, GEMM_EPILOGUES = _names("M3_GEMM_", but="M3_GEMM_EPI_"), _names("M3_GEMM_EPI_")
WGRAD_KERNELS, ATTN_FAMILIES = _names("M3_WGRAD_KERNEL_"), _names("M3_ATTN_")
CONV_REASONS = _names("M3_CONV_")                               # m3_conv3x3_plan_out.reason: ok, refuse_dtype, ...


def csrc_sha16() -> str:
    """first 16 hex digits of the sha256 over the kernel sources (csrc/*.hip, *.h and the C header, by name): stamps a
    PMC traffic file with the kernels it was measured on, so that bench.py can tell a stale replayed measurement
    (the GPU box has no .git to ask)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.h")))
    files.append(_HEADER)
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


_lib = None


def lib():
    """Load the library once.  Raises M3Error if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise M3Error(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C m3vit_amd/csrc` (hipcc, --offload-arch=gfx950). There is no CPU fallback.")
        # torch ships its own HIP runtime (libamdhip64): import it FIRST so that this library binds to the
        # same runtime instance (and therefore the same device context / streams) instead of a second copy
        # from /opt/rocm, which would see "no ROCm-capable device" for torch-allocated memory.
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)       # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().m3_last_error()
        raise M3Error(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")
