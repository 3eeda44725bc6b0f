"""The ctypes binding is derived from include/mdemi.h and include/mdemi_ext.h (mdemi/_cabi.py);
these CPU tests hold it to the headers: struct layouts and constants against what the host C
compiler reports, signatures against the prototypes, and the reader's refusal of anything it
does not understand."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

import pytest

from mdemi import _cabi, _lib as L

vp, i32, i64, u64, f32 = c_void_p, c_int32, c_int64, c_uint64, c_float


def _headers():
    return "".join(open(p).read() for p in L.HEADER_PATHS)


def _host_cc():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cc in (os.environ.get("CC"), "cc", os.path.join(rocm, "llvm", "bin", "clang")):
        if cc and shutil.which(cc):
            return shutil.which(cc)
    pytest.fail("no host C compiler: tried $CC, cc and ROCm's clang")


def test_layout_and_constants_match_the_c_compiler(tmp_path):
    """sizeof of every struct, offsetof / sizeof of every field and the value of every MDEMI_*
    constant, as a C99 compiler sees the two headers, against the ctypes classes and the Python
    constants.  Compiling them as C99 also pins that the headers stay valid C."""
    abi = _cabi.parse(_headers())
    assert len(abi.structs) >= 10 and len(abi.constants) >= 40
    lines, want = [], []
    for name, cls in abi.structs.items():
        lines.append(f'printf("sizeof {name} %zu\\n", sizeof({name}));')
        want.append(f"sizeof {name} {ctypes.sizeof(cls)}")
        for field, _ in cls._fields_:
            lines.append(f'printf("field {name}.{field} %zu %zu\\n", offsetof({name}, {field}), '
                         f"sizeof((({name}*)0)->{field}));")
            want.append(f"field {name}.{field} {getattr(cls, field).offset} {getattr(cls, field).size}")
    for name in abi.constants:
        lines.append(f'printf("const {name} %lld\\n", (long long)({name}));')
        want.append(f"const {name} {getattr(L, name[len('MDEMI_'):])}")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mdemi.h"\n#include "mdemi_ext.h"\n'
                   "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([_host_cc(), "-std=c99", "-I", os.path.dirname(L.HEADER_PATH), str(src),
                    "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(got) == len(want) >= 10 + 135 + 40  # structs, fields, constants
    assert [(g, w) for g, w in zip(got, want) if g != w] == []


def test_public_names_are_the_header_structs():
    abi_names = {"ConvGeom": "mdemi_conv_geom", "GemmDesc": "mdemi_gemm_desc", "WinAttnDesc": "mdemi_winattn_desc",
                 "TensorRef": "mdemi_tensor_ref", "AdamWGroup": "mdemi_adamw_group", "StepRecord": "mdemi_step_record",
                 "TelemetryState": "mdemi_telemetry_state", "GuardState": "mdemi_guard_state",
                 "EmaState": "mdemi_ema_state", "AugSample": "mdemi_aug_sample"}
    for alias, name in abi_names.items():
        assert getattr(L, alias).__name__ == name
    assert len(L.GemmDesc._fields_) == 48 and len(L.WinAttnDesc._fields_) == 35
    assert (L.OK, L.EINVAL, L.ELAUNCH, L.EUNSUP, L.EWORKSPACE) == (0, -1, -2, -3, -4)
    assert L.ACT_GRAD_OF == {L.ACT_GELU: L.ACT_GELU_GRAD, L.ACT_RELU: L.ACT_RELU_GRAD, L.ACT_SILU: L.ACT_SILU_GRAD}


def test_signatures_are_the_header_prototypes():
    header = _cabi._COMMENT.sub(" ", _headers())
    declared = dict(re.findall(r"\b(mdemi_\w+)\s*\(([^()]*)\)\s*;", header))
    lib = L.load()
    assert set(L.exported_symbols()) == set(declared) and len(declared) >= 129
    for name, params in declared.items():
        nargs = 0 if params.strip() == "void" else params.count(",") + 1
        assert len(getattr(lib, name).argtypes) == nargs, name
    gd = POINTER(L.GemmDesc)
    pinned = {
        "mdemi_bn_train_fwd16": (c_int, [vp] * 10 + [f32, i32, i64, i32, f32, i32, vp, vp]),
        "mdemi_dropout_dev16": (c_int, [vp, vp, vp, i64, f32, vp, u64, u64, vp]),
        "mdemi_gemm_pair_workspace_size": (c_size_t, [gd, gd]),
        "mdemi_last_error": (c_char_p, []),
    }
    for name, (restype, argtypes) in pinned.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_descriptor_pointers_are_type_checked():
    """A descriptor parameter takes byref() of its own struct only; ctypes stops the other one
    before the call reaches the library.  The workspace query is host code: no device needed."""
    fn = L.load().mdemi_gemm_workspace_size
    d = L.GemmDesc(M=64, N=64, K=64, batch=1, lda=64, ldb=64, ldc=64, alpha=1.0, split_k=1)
    assert isinstance(fn(ctypes.byref(d)), int)
    with pytest.raises(ctypes.ArgumentError):
        fn(ctypes.byref(L.WinAttnDesc()))


def test_a_missing_header_is_reported_by_path(monkeypatch, tmp_path):
    gone = str(tmp_path / "mdemi.h")
    monkeypatch.setattr(L, "HEADER_PATHS", [gone])
    with pytest.raises(L.MdemiLibraryError, match="mdemi.h"):
        L._read_headers()


@pytest.mark.parametrize("snippet, quoted", [
    ("typedef struct s { uint8_t x; } s;", "uint8_t x"),                          # unknown field type
    ("typedef struct s { int32_t x : 3; } s;", "int32_t x : 3"),                  # bit-field
    ("int mdemi_f(void (*cb)(int32_t), void* stream);", "(*cb)"),                 # function pointer
    ("#define MDEMI_X (1 << 3)", "(1 << 3)"),                                     # expression
    ("typedef struct s { int32_t x[MDEMI_N]; } s;", "MDEMI_N"),                   # unknown array bound
    ("int mdemi_f(void); stray", "stray"),                                        # text after a prototype
    ("int mdemi_f(void) stray;", "stray"),
    ("int mdemi_f(mdemi_thing x);", "mdemi_thing x"),                             # unknown parameter type
    ("float mdemi_f(void);", "float mdemi_f"),                                    # unknown return type
    ("int mdemi_f(void);\nint mdemi_f(void);", "mdemi_f"),                        # bound twice
    ("#if 1", "#if 1"),
])
def test_reader_refuses_what_it_cannot_read(snippet, quoted):
    with pytest.raises(_cabi.HeaderError) as e:
        _cabi.parse(snippet)
    assert quoted in str(e.value)


def _fields(cls):
    return [(n, t) for n, t in cls._fields_]


INNER = "typedef struct inner { int32_t a, b; float x, y; } inner;\n"
FORMS = {
    "multi-declarator": (INNER, lambda abi: (_fields(abi.structs["inner"]),
                                            [("a", i32), ("b", i32), ("x", f32), ("y", f32)])),
    "nested struct by value": (INNER + "typedef struct outer { int64_t n; inner in; const float* p; } outer;",
                               lambda abi: (_fields(abi.structs["outer"]),
                                            [("n", i64), ("in", abi.structs["inner"]), ("p", vp)])),
    "2-D array with a symbolic bound": (
        "#define MDEMI_SPANS 8\ntypedef struct s { double m[6]; int32_t rows[MDEMI_SPANS][2]; } s;",
        lambda abi: (_fields(abi.structs["s"]) + [len(abi.structs["s"]().rows), len(abi.structs["s"]().rows[0])],
                     [("m", ctypes.c_double * 6), ("rows", (i32 * 2) * 8), 8, 2])),
    "untagged typedef": ("typedef struct {\n  uint32_t f; uint64_t g;  /* flags */\n  size_t s; int k;\n} plain;",
                         lambda abi: (_fields(abi.structs["plain"]),
                                      [("f", c_uint32), ("g", u64), ("s", c_size_t), ("k", c_int)])),
    "void* const*": ("int mdemi_f(void* const* pp, float* const* e, const uint8_t* b, int flag, uint64_t seed);",
                     lambda abi: (abi.prototypes, {"mdemi_f": (c_int, [vp, vp, vp, c_int, u64])})),
    "(void)": ("const char* mdemi_s(void);\nsize_t mdemi_n( void );",
               lambda abi: (abi.prototypes, {"mdemi_s": (c_char_p, []), "mdemi_n": (c_size_t, [])})),
    "1u constant": ("#define MDEMI_ONE 1u  /* a flag */\n#define MDEMI_NEG (-4)  // an error\n#define MDEMI_TWO (2)",
                    lambda abi: (abi.constants, {"MDEMI_ONE": 1, "MDEMI_NEG": -4, "MDEMI_TWO": 2})),
    "descriptor pointer": ("typedef struct x_desc { int32_t v; } x_desc;\nint mdemi_f(const x_desc* d, x_desc** dd);",
                           lambda abi: (abi.prototypes, {"mdemi_f": (c_int, [POINTER(abi.structs["x_desc"]), vp])})),
    "guards and extern C": ('#ifndef X_H\n#define X_H\n#include <stdint.h>\n#include "mdemi.h"\n#ifdef __cplusplus\n'
                            'extern "C" {\n#endif\nint mdemi_f(void);\n#ifdef __cplusplus\n}\n#endif\n#endif /* X_H */\n',
                            lambda abi: (abi, _cabi.Abi({}, {}, {"mdemi_f": (c_int, [])}))),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_reader_reads_every_form_the_headers_use(form):
    snippet, result = FORMS[form]
    got, want = result(_cabi.parse(snippet))
    assert got == want
