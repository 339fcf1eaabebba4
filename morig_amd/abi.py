"""The C ABI as ctypes objects, read from include/morig_hip.h when the package is imported: the header is the ONE statement of every
argument struct, prototype and constant; nothing here or in native.py repeats it.

    STRUCTS     header struct name -> ctypes.Structure subclass
    SIGNATURES  function name -> (restype, argtypes)
    CONSTANTS   every object-like `#define MORIG_X <integer>[u]` -> int

The grammar is tiny and strict (it is spelled out at the top of the header): once comments, preprocessor lines and the `extern "C"`
braces are gone, every statement is `typedef struct NAME { members } NAME;` or `RET morig_name(params);`, over the types of
``_ctype``. Anything else raises MorigNativeError quoting the text, so the header cannot grow syntax this reader would skip.
"""
from __future__ import annotations

import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "morig_hip.h")


class MorigNativeError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double}
_POINTEES = set(_SCALARS) | {"void", "char", "uint8_t"}          # what a plain pointer may point at
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTO = re.compile(r"([\w\s*]+?)\b(morig_\w+)\s*\(([^(){};]*)\)\s*;")
_SPACE = re.compile(r"\s*")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(MORIG_\w+)[ \t]+(-?\d+)[uU]?[ \t]*$", re.M)


def _ctype(text: str, structs: dict, member_of: str = None):
    """`const float*`, `void**`, `int32_t`, `const struct morig_x_args*` ... -> the ctypes type; member_of: the struct being declared
    (a pointer to a header struct is typed in a parameter list and opaque as a member, where it may name its own struct)"""
    words = [w for w in text.replace("*", " * ").split() if w not in ("const", "struct")]
    base, stars = (words[0] if words else ""), len(words) - 1
    if words[1:] != ["*"] * stars or base == "*":
        raise MorigNativeError(f"morig_hip.h: cannot read the type {text.strip()!r}")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1 and (base in structs or base == member_of):
        return C.c_void_p if member_of else C.POINTER(structs[base])
    if stars == 1 and base in _POINTEES:
        return C.c_char_p if base == "char" else C.c_void_p
    if stars == 2 and base == "void":
        return C.POINTER(C.c_void_p)
    raise MorigNativeError(f"morig_hip.h: type {text.strip()!r} is outside the binding's grammar")


def _declaration(text: str):
    """`const float* X` -> (`const float*`, `X`)"""
    m = re.fullmatch(r"\s*(.*?[\s*])(\w+)\s*", text, re.S)
    if not m:
        raise MorigNativeError(f"morig_hip.h: cannot read the declaration {text.strip()!r}")
    return m.group(1), m.group(2)


def _structure(name: str, body: str, structs: dict):
    fields = []
    for decl in filter(str.strip, body.split(";")):
        first, *more = decl.split(",")                           # int32_t M, N, K;
        typ, member = _declaration(first)
        ctype = _ctype(typ, structs, member_of=name)
        for extra in more:
            if not re.fullmatch(r"\s*\w+\s*", extra):
                raise MorigNativeError(f"morig_hip.h: cannot read the declarator {extra.strip()!r} of {decl.strip()!r}")
        fields += [(m.strip(), ctype) for m in [member] + more]
    return type(name, (C.Structure,), {"_fields_": fields})


def parse(text: str):
    """header text -> (STRUCTS, SIGNATURES, CONSTANTS)"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {name: int(value) for name, value in _DEFINE.findall(text)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    block = re.fullmatch(r'\s*extern\s+"C"\s*\{(.*)\}\s*', text, re.S)
    text = block.group(1) if block else text
    structs, signatures, pos = {}, {}, _SPACE.match(text).end()
    while pos < len(text):
        m = _STRUCT.match(text, pos) or _PROTO.match(text, pos)
        if not m:
            raise MorigNativeError(f"morig_hip.h: neither an argument struct nor a morig_ prototype: {text[pos:pos + 120].strip()!r}")
        if m.group(2 if m.re is _PROTO else 3) in {**structs, **signatures}:
            raise MorigNativeError(f"morig_hip.h: declared twice: {m.group(0)!r}")
        if m.re is _STRUCT:
            tag, body, name = m.groups()
            if tag != name:
                raise MorigNativeError(f"morig_hip.h: struct tag and typedef name differ: {tag!r} / {name!r}")
            structs[name] = _structure(name, body, structs)
        else:
            ret, name, params = m.groups()
            params = [] if params.strip() == "void" else params.split(",")
            signatures[name] = (_ctype(ret, structs), [_ctype(_declaration(p)[0], structs) for p in params])
        pos = _SPACE.match(text, m.end()).end()
    return structs, signatures, constants


with open(HEADER) as _f:
    STRUCTS, SIGNATURES, CONSTANTS = parse(_f.read())
