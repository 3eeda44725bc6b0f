"""Reader of the C ABI headers (include/mdemi.h, include/mdemi_ext.h): turns their text into
integer constants, ``ctypes.Structure`` classes and (restype, argtypes) signatures, so the
binding in ``_lib.py`` restates nothing by hand.

It understands the C these headers use and nothing more.  Every directive, struct member,
parameter and statement has to be consumed by one of the rules below; anything else raises
``HeaderError`` quoting the declaration -- nothing is ever dropped or bound silently.
"""
from __future__ import annotations

import ctypes
import re
from collections import namedtuple

Abi = namedtuple("Abi", "constants structs prototypes")  # name -> int / Structure class / (restype, argtypes)

SCALARS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64, "int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double,
           "size_t": ctypes.c_size_t}
_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}  # and const char*: c_char_p

_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_CPP_GUARD = re.compile(r'#ifdef\s+__cplusplus\s*\n\s*(?:extern\s+"C"\s*\{|\})\s*\n\s*#endif\b')
_SKIPPED = re.compile(r"#\s*(?:include\s*[<\"][\w./]+[>\"]|ifn?def\s+\w+|endif|define\s+\w+)")
_DEFINE = re.compile(r"#\s*define\s+(MDEMI_\w+)\s+(?:\(\s*(-?\d+)[uU]?\s*\)|(-?\d+)[uU]?)")
_STRUCT = re.compile(r"typedef\s+struct\s*(\w+)?\s*\{([^{}]*)\}\s*(\w+)\s*;")
_MEMBER = re.compile(r"(?:const\s+)?(\w+)\b\s*(.*)", re.S)
_DECLARATOR = re.compile(r"(\*?)\s*(\w+)\s*((?:\[\s*\w+\s*\]\s*)*)")
_PROTO = re.compile(r"(const\s+char\s*\*|int\b|size_t\b)\s*(\w+)\s*\((.*)\)", re.S)
_PARAM = re.compile(r"(?:const\s+)?(\w+)\b\s*((?:\*\s*(?:const\b\s*)?)*)(\w+)")


class HeaderError(ValueError):
    pass


def _put(table, name, value, what):
    if name in table:
        raise HeaderError(f"{what} {name} is declared twice")
    table[name] = value


def _directive(line, constants):
    if _SKIPPED.fullmatch(line):
        return
    m = _DEFINE.fullmatch(line)
    if not m:
        raise HeaderError(f"cannot read the directive {line!r}")
    _put(constants, m.group(1), int(m.group(2) or m.group(3)), "constant")


def _member_fields(decl, abi):
    """One struct member declaration (no ';'), possibly with several declarators -> fields."""
    m = _MEMBER.fullmatch(decl)
    fields = []
    for piece in m.group(2).split(",") if m else ():
        d = _DECLARATOR.fullmatch(piece.strip())
        if not d:
            raise HeaderError(f"cannot read the struct member {decl!r}")
        base = m.group(1)
        if d.group(1):
            ctype = ctypes.c_void_p
        elif base in SCALARS or base in abi.structs:
            ctype = SCALARS.get(base) or abi.structs[base]
        else:
            raise HeaderError(f"unknown type {base!r} in the struct member {decl!r}")
        for bound in reversed(re.findall(r"\w+", d.group(3))):
            if not (bound.isdigit() or bound in abi.constants):
                raise HeaderError(f"unknown array bound {bound!r} in the struct member {decl!r}")
            ctype = ctype * (int(bound) if bound.isdigit() else abi.constants[bound])
        fields.append((d.group(2), ctype))
    if not fields:
        raise HeaderError(f"cannot read the struct member {decl!r}")
    return fields


def _struct(m, abi):
    tag, body, name = m.groups()
    if tag not in (None, name):
        raise HeaderError(f"struct tag {tag!r} differs from its typedef name {name!r}")
    fields = [f for decl in body.split(";") if decl.strip() for f in _member_fields(decl.strip(), abi)]
    _put(abi.structs, name, type(name, (ctypes.Structure,), {"_fields_": fields}), "struct")
    return ""


def _prototype(stmt, abi):
    m = _PROTO.fullmatch(stmt)
    if not m:
        raise HeaderError(f"cannot read the declaration {stmt!r}")
    argtypes = []
    for piece in [] if m.group(3).strip() == "void" else m.group(3).split(","):
        piece = " ".join(piece.split())
        p = _PARAM.fullmatch(piece)
        if not p:
            raise HeaderError(f"cannot read the parameter {piece!r} of {stmt!r}")
        base, stars = p.group(1), p.group(2).count("*")
        if stars == 1 and base.endswith("_desc") and base in abi.structs:
            argtypes.append(ctypes.POINTER(abi.structs[base]))  # a host-side descriptor: type-checked
        elif stars:
            argtypes.append(ctypes.c_void_p)
        elif base in SCALARS:
            argtypes.append(SCALARS[base])
        else:
            raise HeaderError(f"unknown type {base!r} of the parameter {piece!r} of {stmt!r}")
    _put(abi.prototypes, m.group(2), (_RETURNS.get(m.group(1), ctypes.c_char_p), argtypes), "function")


def parse(text):
    """Header text (several headers: concatenated in include order) -> Abi."""
    abi = Abi({}, {}, {})
    text = _CPP_GUARD.sub("", _COMMENT.sub(" ", text))
    code = []
    for line in text.split("\n"):
        if line.lstrip().startswith("#"):
            _directive(line.strip(), abi.constants)
        else:
            code.append(line)
    rest = _STRUCT.sub(lambda m: _struct(m, abi), "\n".join(code))
    *stmts, tail = rest.split(";")
    for stmt in stmts:
        _prototype(stmt.strip(), abi)
    if tail.strip():
        raise HeaderError(f"cannot read the text {tail.strip()!r}")
    return abi
