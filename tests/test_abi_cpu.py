"""CPU tests (no GPU) of emernerf_amd/_abi.py, the reader of include/emernerf_hip.h that the ctypes binding is made from: the
struct layouts and constants it finds are held against the C compiler's, what it does not know it refuses, and it finds every
prototype that the regex of test_host_cpu finds."""
import ctypes
import os
import shutil
import subprocess

import pytest

from emernerf_amd import _abi, _build
from tests.test_host_cpu import _declared_functions


def _fields(cls, path="", offset=0):
    """(C member path, offset, size) of every field of a parsed struct, through nested structs, unions and (at element 0) arrays of
    structs."""
    for name, ctype in cls._fields_:
        off, p = offset + getattr(cls, name).offset, path + name
        yield p, off, ctypes.sizeof(ctype)
        elem, p = (ctype._type_, p + "[0]") if issubclass(ctype, ctypes.Array) else (ctype, p)
        if issubclass(elem, (ctypes.Structure, ctypes.Union)):
            yield from _fields(elem, p + ".", off)


def _cc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    bindir = os.path.dirname(os.path.realpath(hipcc))
    for exe in (os.path.join(bindir, "clang"), os.path.join(bindir, "amdclang"), os.path.join(bindir, "..", "lib", "llvm", "bin", "clang"),
                shutil.which("cc")):
        if exe and os.path.exists(exe):
            return exe
    raise RuntimeError("no C compiler: neither the clang of the ROCm toolchain nor cc")


def test_layouts_and_constants_agree_with_the_c_compiler(tmp_path):
    lines = ["#include <stddef.h>", f'#include "{_build.HEADER}"']
    n_fields = 0
    for name, cls in _abi.STRUCT.items():
        lines.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(cls)}, "sizeof({name})");')
        for path, off, size in _fields(cls):
            lines.append(f'_Static_assert(offsetof({name}, {path}) == {off} && sizeof((({name} *)0)->{path}) == {size}, "{name}.{path}");')
            n_fields += 1
    for name, value in _abi.CONST.items():
        lines.append(f'_Static_assert({name} == {value}, "{name}");')
    assert len(_abi.STRUCT) >= 21 and n_fields >= 300 and len(_abi.CONST) >= 50, (len(_abi.STRUCT), n_fields, len(_abi.CONST))
    src = tmp_path / "abi_layout.c"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([_cc(), "-std=c11", "-fsyntax-only", "-Werror", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.parametrize("text", [
    "typedef struct s { size_t n; } s;",                           # an unknown base type
    "typedef struct s { int32_t a : 3; } s;",                      # a bit-field
    "typedef struct s { int (*fn)(int); } s;",                     # a function-pointer field
    "typedef struct s { float v[EMER_N]; } s;",                    # an array bound that is no known constant
    "#define EMER_N 4\ntypedef struct s { float v[EMER_M]; } s;",
    "#define EMER_X 1.5\n",                                        # constants are integers
    "#define EMER_X (1 << 4)\n",
    "#define EMER_X\n",
    "#if 0\n#endif\n",                                             # any other preprocessor line
    "typedef struct s { void v; } s;",                             # void and char behind a pointer only
    "typedef struct s { struct t *next; } s;",                     # a struct is named by its typedef
    "int emer_f(float v[3]);",                                     # an array parameter
    "typedef struct s { int a; } s;\nint emer_f(s by_value);",
    "float emer_f(void);",                                         # return types: int, int64_t, const char *
    "int other_f(void);",
    "int emer_f(int a)",                                           # the text ends inside a declaration
])
def test_parser_refuses_what_it_does_not_know(text):
    with pytest.raises(_abi.EmerError):
        _abi.parse(text)


def test_parser_reads_the_subset_the_header_uses():
    consts, structs, funcs = _abi.parse(
        "/* c */ #define EMER_N (3) // c\n#define EMER_BIG 2147483647ll\n#define EMER_NEG (-2)\n"
        "typedef struct a { const float *p, *q; int32_t n[EMER_N], m; } a;\n"
        "typedef struct b { a first; union { a x; struct { const float *const *pp; double d; } y; } u; uint8_t tail[2]; } b;\n"
        "int64_t emer_size(void);\nconst char *emer_text(void);\nint emer_f(const b *host, const float *const *pp, uint64_t n, void *stream);\n")
    assert consts == {"EMER_N": 3, "EMER_BIG": 2 ** 31 - 1, "EMER_NEG": -2}
    assert [(n, t) for n, t in structs["a"]._fields_] == [("p", ctypes.c_void_p), ("q", ctypes.c_void_p), ("n", ctypes.c_int32 * 3), ("m", ctypes.c_int32)]
    assert ctypes.sizeof(structs["b"]) == 32 + 32 + 8 and structs["b"].u.offset == 32 and structs["b"].tail.offset == 64
    assert funcs == {"emer_size": (ctypes.c_int64, []), "emer_text": (ctypes.c_char_p, []),
                     "emer_f": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p])}


def test_every_declared_prototype_is_parsed():
    declared = _declared_functions()
    assert len(declared) >= 100 and declared == set(_abi.FUNC)
    assert _abi.FUNC["emer_last_error"] == (ctypes.c_char_p, [])
    queries = [n for n in declared if n.endswith(("_workspace", "_workspace_bytes", "_size", "_capacity"))]
    assert len(queries) >= 11
    for name, (restype, _) in _abi.FUNC.items():
        assert restype is (ctypes.c_int64 if name in queries else ctypes.c_char_p if name == "emer_last_error" else ctypes.c_int), name
