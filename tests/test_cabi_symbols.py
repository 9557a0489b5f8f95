"""CPU: the C-ABI library loads and exports every symbol include/m3vit_hip.h declares, and the ctypes bindings that
m3vit_amd._lib derives from the header's text agree with what a C++ compiler makes of the same header
(no compute calls without a GPU)."""
import ctypes
import os
import re
import shutil
import subprocess

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


def _header_text():
    txt = open(os.path.join(ROOT, "include", "m3vit_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _kind(t):
    """what the compiled probe prints for a type: p(ointer) / f(loat) / i(nteger) and the byte size"""
    if issubclass(t, (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)):
        return f"p{ctypes.sizeof(t)}"
    return ("f" if t in (ctypes.c_float, ctypes.c_double) else "i") + str(ctypes.sizeof(t))


def test_derived_bindings_match_the_compiler(tmp_path):
    """sizeof and every field's offset and size of every struct, the value of every M3_* constant, and the parameter count
    and each parameter's and the return type's kind and size of every entry point: as a host C++ compiler sees the header
    against the ctypes tables read from its text.  A dropped argument, an int for an int64_t, a float for an int, a field
    missing or out of order, a renumbered constant: each shows here, on the CPU, instead of as a stray device write."""
    from m3vit_amd import _lib
    txt = _header_text()                                      # the reader skipped nothing: independent counts
    assert len(_lib.CONSTANTS) == len(re.findall(r"^\s*#\s*define\s+M3_", txt, flags=re.M)) >= 83
    assert len(_lib.STRUCTS) == len(re.findall(r"\btypedef\s+struct\b", txt)) >= 17
    src = ["#include <cstddef>", "#include <cstdio>", "#include <type_traits>", '#include "m3vit_hip.h"',
           "template <class T> void k() { std::printf(\" %c%zu\", std::is_pointer<T>::value ? 'p' : "
           "std::is_floating_point<T>::value ? 'f' : 'i', sizeof(T)); }",
           "template <class F> struct sig;",               # over the function's TYPE: the probe links against nothing
           "template <class R, class... A> struct sig<R (*)(A...)> { static void print(const char *n) "
           "{ std::printf(\"F %s %zu\", n, sizeof...(A)); k<R>(); (k<A>(), ...); std::printf(\"\\n\"); } };",
           "int main() {"]
    want = []
    for name, val in _lib.CONSTANTS.items():
        src.append(f'  std::printf("C {name} %lld\\n", (long long)({name}));')
        want.append(f"C {name} {val}")
    for name, cls in _lib.STRUCTS.items():
        fields = [f for f, _ in cls._fields_]
        src.append(f'  std::printf("S {name} %zu' + " %zu:%zu" * len(fields) + f'\\n", sizeof({name})'
                   + "".join(f", offsetof({name}, {f}), sizeof({name}::{f})" for f in fields) + ");")
        want.append(f"S {name} {ctypes.sizeof(cls)}" + "".join(f" {getattr(cls, f).offset}:{getattr(cls, f).size}" for f in fields))
    for name, (res, args) in _lib.SIGNATURES.items():
        src.append(f'  sig<decltype(&{name})>::print("{name}");')
        want.append(f"F {name} {len(args)} " + " ".join(_kind(t) for t in [res] + args))
    src += ["  return 0;", "}"]
    (tmp_path / "probe.cpp").write_text("\n".join(src) + "\n")
    cxx = [shutil.which("c++")] if shutil.which("c++") else [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-x", "c++"]
    subprocess.check_call(cxx + ["-std=c++17", "-I", os.path.join(ROOT, "include"), str(tmp_path / "probe.cpp"),
                                 "-o", str(tmp_path / "probe")])      # host code only: nothing is compiled for a device
    got = subprocess.check_output([str(tmp_path / "probe")], text=True).splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, f"compiler: {g!r}  ctypes: {w!r}"


def test_reader_type_rules():
    """one entry point of each kind the header's reader has a rule for"""
    from ctypes import POINTER, c_char_p, c_double, c_int, c_int32, c_void_p
    from m3vit_amd import _lib
    S = _lib.SIGNATURES
    assert S["m3_last_error"] == (c_char_p, [])
    assert S["m3_loss_bce_fwd"][1][9] is c_double
    assert S["m3_ep_init"][1][3] is POINTER(c_int)
    assert S["m3_cast_batch"][1][0] is c_void_p                                    # descs_dev: a device address
    assert S["m3_wgrad_multi"][1][0] is POINTER(_lib.WgradMultiArgs)               # a struct the host fills
    assert S["m3_gemm_plan"][1] == [POINTER(_lib.GemmArgs), POINTER(_lib.GemmPlan)]
    N = dict(_lib.WgradMultiShape._fields_)["N"]
    assert issubclass(N, ctypes.Array) and N._type_ is c_int32 and N._length_ == _lib.M3_WGRAD_MULTI_MAX == _lib.WGRAD_MULTI_MAX
    assert _lib.WgradMultiArgs is _lib.STRUCTS["m3_wgrad_multi_args"] and _lib.LnParamGrads is _lib.STRUCTS["m3_ln_param_grads"]
    assert dict(_lib.WgradMultiArgs._fields_)["prob"]._type_ is _lib.WgradProblem  # nested struct array
    assert dict(_lib.WgradArgs._fields_)["prev"] is POINTER(_lib.WgradReduceDesc)  # pointer to another struct


@pytest.mark.parametrize("text, named", [
    ("int m3_ok(int a);\nint m3_broken(int a, float);\n", "m3_broken(int a, float)"),          # a parameter without a name
    ("int m3_ok(int a);\nint m3_odd(const uint8_t *p, int n);\n", "m3_odd(const uint8_t *p, int n)"),   # an unknown type
    ("typedef struct { int32_t a; unsigned b; } m3_t;\n", "unsigned b"),                       # ... in a struct
    ("#define M3_X 1u\n", "#define M3_X 1u"),                                                  # not a plain integer
    ("typedef struct { int32_t a[M3_NOPE]; } m3_t;\n", "int32_t a[M3_NOPE]"),                  # an unknown dimension
    ("int m3_a(int a)\nint m3_b(void);\n", "int m3_a(int a) int m3_b(void)"),                  # a lost semicolon
])
def test_reader_fails_loudly(text, named):
    """what the reader does not understand raises and names the text: nothing is skipped"""
    from m3vit_amd import _lib
    assert _lib.read_header("int m3_ok(int a);\n")[2] == {"m3_ok": (ctypes.c_int, [ctypes.c_int])}
    with pytest.raises(_lib.M3Error) as e:
        _lib.read_header(text)
    assert named in str(e.value)


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
