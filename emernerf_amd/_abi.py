"""include/emernerf_hip.h read as ctypes, once, at import: the header is the only copy of the C ABI.

  CONST   name -> int                       every ``#define EMER_X <int>``
  STRUCT  name -> ctypes.Structure class    every ``typedef struct name { ... } name;``
  FUNC    name -> (restype, [argtypes])     every ``emer_*`` prototype

The parser takes exactly the C the header is written in and raises on anything else: integer constants; structs of scalar,
pointer and array fields, earlier structs and nested anonymous structs / unions; prototypes over the same types.  Every pointer
is a c_void_p (it takes a tensor's address, ``ctypes.byref(...)`` and ctypes arrays alike); ``const char *`` returns c_char_p.
"""
from __future__ import annotations

import ctypes
import os
import re

from ._build import HEADER


class EmerError(RuntimeError):
    pass


BASE = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint8_t": ctypes.c_uint8,
        "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double,
        "void": None, "char": ctypes.c_char}   # the last two behind a pointer only
_KEPT_LINES = re.compile(r"#\s*((ifndef|define) EMERNERF_HIP_H|include <stdint\.h>|endif)")   # include guard and <stdint.h>
_RECORD = {"struct": ctypes.Structure, "union": ctypes.Union}


def parse(text: str):
    """(CONST, STRUCT, FUNC) of a header text."""
    consts, structs, funcs = {}, {}, {}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus\n.*?#endif", "", text, flags=re.S)   # extern "C" { and its }
    code = []
    for line in text.splitlines():
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        m = re.fullmatch(r"#\s*define\s+(EMER_\w+)\s+(.*?)", line.strip())
        if m:
            v = re.fullmatch(r"\(?\s*([-+]?\d+)(?:ll)?\s*\)?", m.group(2))
            if not v:
                raise EmerError(f"{m.group(1)}: not an integer constant: {m.group(2)!r}")
            consts[m.group(1)] = int(v.group(1))
        elif not _KEPT_LINES.fullmatch(line.strip()):
            raise EmerError(f"unsupported preprocessor line: {line.strip()!r}")
    toks = re.findall(r"\w+|\S", "\n".join(code))
    pos = 0

    def take(want=None):
        nonlocal pos
        t = toks[pos] if pos < len(toks) else "<end>"
        if want is not None and t != want:
            raise EmerError(f"expected {want!r}, got {t!r} after `{' '.join(toks[max(pos - 8, 0):pos])}`")
        pos += 1
        return t

    def peek(t):
        return pos < len(toks) and toks[pos] == t

    def base_type():
        while peek("const"):
            take()
        t = take()
        if t in _RECORD:
            return record(t)
        if t in BASE:
            return BASE[t]
        if t in structs:
            return structs[t]
        raise EmerError(f"unknown type {t!r}")

    def declarator(base, plain=False):
        """[*]... name [ [N] ] -> (name, ctype); plain: a parameter (no array, nothing by value but a scalar)."""
        stars = 0
        while peek("*") or peek("const"):
            stars += take() == "*"
        name = take()
        if not re.fullmatch(r"[A-Za-z_]\w*", name):
            raise EmerError(f"expected a name, got {name!r}")
        t = ctypes.c_void_p if stars else base
        if t is None or t is ctypes.c_char or (plain and issubclass(t, (ctypes.Structure, ctypes.Union))):
            raise EmerError(f"{name}: this type is taken behind a pointer only")
        if peek("["):
            take()
            n = take()
            if plain or not (n.isdigit() or n in consts):
                raise EmerError(f"{name}: array bound {n!r} is neither a literal nor an earlier constant")
            t = t * (int(n) if n.isdigit() else consts[n])
            take("]")
        return name, t

    def record(kind):
        take("{")
        fields = []
        while not peek("}"):
            base = base_type()
            fields.append(declarator(base))
            while peek(","):
                take()
                fields.append(declarator(base))
            take(";")
        take("}")
        return type("_anon", (_RECORD[kind],), {"_fields_": fields})

    while pos < len(toks):
        if peek("typedef"):
            take()
            take("struct")
            name = take()
            structs[name] = cls = record("struct")
            cls.__name__ = cls.__qualname__ = name
            take(name)
        else:
            base = base_type()
            stars = 0
            while peek("*"):
                stars += take() == "*"
            restype = (ctypes.c_char_p if base is ctypes.c_char else ctypes.c_void_p) if stars else base
            name = take()
            if not name.startswith("emer_") or restype not in (ctypes.c_int, ctypes.c_int64, ctypes.c_char_p):
                raise EmerError(f"unsupported declaration at {name!r}")
            take("(")
            args = []
            if peek("void") and toks[pos + 1:pos + 2] == [")"]:
                take()
            else:
                args.append(declarator(base_type(), plain=True)[1])
                while peek(","):
                    take()
                    args.append(declarator(base_type(), plain=True)[1])
            take(")")
            funcs[name] = (restype, args)
        take(";")
    return consts, structs, funcs


if not os.path.exists(HEADER):
    raise EmerError(f"{HEADER} not found: the ctypes binding of libemernerf_hip.so is read from it")
with open(HEADER) as _f:
    CONST, STRUCT, FUNC = parse(_f.read())
