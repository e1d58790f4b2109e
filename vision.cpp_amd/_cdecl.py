"""Strict reader of the C declarations in include/visp_c_api.h and include/visp_hip_kernels.h, and their ctypes types.

The two headers are the only place where the C ABI is declared; _lib.py derives its structures, enumerators and
prototypes from what `parse` returns. The reader knows exactly the C those headers use -- typedef'd structs, opaque
struct typedefs, enums with integer values and VX_API / VISP_API function declarations -- and raises DeclError, quoting
the text, on anything else. It is no preprocessor: lines that start with `#` are dropped. It runs at every import of the
package, so it stays cheap: one pass over the text, one regular-expression call per parameter list, plain tuples for what it finds.
"""
from __future__ import annotations

import ctypes
import keyword
import re
from collections import namedtuple
from ctypes import POINTER, c_char, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint8, c_void_p

SCALARS = {"char": c_char, "int": c_int, "float": c_float, "double": c_double, "size_t": c_size_t,
           "int32_t": c_int32, "int64_t": c_int64, "uint8_t": c_uint8}

# A declared object (field, parameter, return type) is the tuple (text, base, stars, name, array) that _OBJECTS finds: its text,
# the base type, the run of `*` and `const` behind it, the name ("" for a return type) and "[n]" / "[]" / "".
# A function is (return type, [parameters]). Decls: structs {name: [fields]}, opaque {name}, enums {enum name, "" for the
# anonymous ones: {enumerator: value}}, functions {name: (return type, [parameters])}
Decls = namedtuple("Decls", "structs opaque enums functions")


class DeclError(ValueError):
    pass


_NOT_C = re.compile(r"/\*[^*]*\*+(?:[^/*][^*]*\*+)*/|//[^\n]*|^[ \t]*#[^\n]*", re.M)  # comments and preprocessor lines
_WS = re.compile(r"\s*")
_FUNC = re.compile(r"(?:VX_API|VISP_API)\s+([^;()]*?)\b(\w+)\s*\(([^;()]*)\)\s*;")
_STRUCT = re.compile(r"typedef\s+struct\s*(\w*)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_OPAQUE = re.compile(r"typedef\s+struct\s+(\w+)\s+(\w+)\s*;")
_ENUM = re.compile(r"enum\s*(\w*)\s*\{([^{}]*)\}\s*;")
_SKIP = re.compile(r'extern\s*"C"\s*\{|\}')
_ENUMERATOR = re.compile(r"\s*(\w+)\s*(?:=\s*(\d+)\s*)?")
# the declarators of a comma-separated list: `int64_t const ne[4]`, `visp_model* const* models`, `const void* A`, `char const*`
_OBJECTS = re.compile(r"(\s*(?:const\s+)?(\w+)((?:\s*\*|\s+const\b)*)\s*(\w+)?\s*(\[\d*\])?\s*)(?:,|$)")


def _quote(text: str) -> str:
    return " ".join(text.split())[:200]


def _objects(text: str, named: bool = True) -> list[tuple]:
    """`int a, int64_t const ne[4]` -> [(" int a", "int", "", "a", ""), (" int64_t const ne[4]", "int64_t", " const", "ne", "[4]")];
    everything in the text must have been read, every object has a name (or none has: a return type) and none is a plain void."""
    found = _OBJECTS.findall(text)
    if sum(len(v[0]) for v in found) + len(found) - 1 != len(text) or any(bool(v[3]) != named or (named and v[1] == "void" and "*" not in v[2]) for v in found):
        raise DeclError(f"cannot read the declarators of {_quote(text)!r}")
    return found


def _fields(text: str) -> list[tuple]:
    """One declaration of a struct: `int64_t lda`, or `int M, N` / `void *q, *k`, where the later declarators share the first one's base type."""
    first, *more = text.split(",")
    base = _objects(first)[0][1]
    return _objects(",".join([first] + [f"{base} {d}" for d in more]))


def parse(text: str) -> Decls:
    text = _NOT_C.sub(" ", text)
    decls = Decls({}, set(), {}, {})
    known = set(SCALARS) | {"void"}
    pos = _WS.match(text).end()
    while pos < len(text):
        m = _FUNC.match(text, pos) or _STRUCT.match(text, pos) or _OPAQUE.match(text, pos) or _ENUM.match(text, pos) or _SKIP.match(text, pos)
        if not m:
            raise DeclError(f"cannot read the declaration that starts {_quote(text[pos:pos + 400])!r}")
        try:
            used, declared = (), m[3] if m.re is _STRUCT else m[2] if m.re is _OPAQUE else "void"
            if m.re is _FUNC:
                ret, params = _objects(m[1], named=False), [] if m[3].strip() == "void" else _objects(m[3])
                if len(ret) != 1:
                    raise DeclError(f"cannot read the return type {_quote(m[1])!r}")
                decls.functions[m[2]] = (ret[0], params)
                used = ret + params
            elif m.re is _STRUCT:
                decls.structs[m[3]] = used = [v for d in m[2].split(";") if d.strip() for v in _fields(d)]
            elif m.re is _OPAQUE:
                if m[1] != m[2]:
                    raise DeclError("an opaque typedef must keep the tag's name")
                decls.opaque.add(m[2])
            elif m.re is _ENUM:
                values, nxt = decls.enums.setdefault(m[1], {}), 0
                for item in filter(None, (i.strip() for i in m[2].split(","))):
                    e = _ENUMERATOR.fullmatch(item)
                    if not e:
                        raise DeclError(f"cannot read the enumerator {item!r}")
                    values[e[1]] = nxt = int(e[2]) if e[2] else nxt
                    nxt += 1
            if unknown := {v[1] for v in used} - known:
                raise DeclError(f"unknown base type {', '.join(sorted(unknown))}")
            known.add(declared)
        except DeclError as e:
            raise DeclError(f"{e} in {_quote(m[0])!r}") from None
        pos = _WS.match(text, m.end()).end()
    return decls


def ctype(v: tuple, structs: dict):
    """The ctypes type of a parameter, a return value or a field that is no array; `structs` {C name: ctypes.Structure class}."""
    _, base, stars, name, array = v
    depth = stars.count("*") + bool(array)
    if depth == 0:
        if base not in SCALARS and base != "void":
            raise DeclError(f"{base} {name} is passed by value: only scalars are")
        return SCALARS.get(base)
    if depth == 1 and base == "char":
        return c_char_p
    if depth == 1 and base in structs:
        return POINTER(structs[base])
    return c_void_p  # any other pointer, pointer to pointer, opaque handle or array parameter


def structures(decls: Decls, names: dict) -> dict:
    """ctypes.Structure classes {C name: class} of the structs of `decls`, named by `names` {C name: Python name}."""
    out = {}
    for cname, fields in decls.structs.items():
        if cname not in names:
            raise DeclError(f"struct {cname} has no Python name")
        members = []
        for text, base, stars, name, array in fields:
            if array == "[]":
                raise DeclError(f"{cname}.{name} is an array without a size")
            t = ctype((text, base, stars, name, ""), out)
            members.append((name + "_" if keyword.iskeyword(name) else name, t * int(array[1:-1]) if array else t))
        out[cname] = type(names[cname], (ctypes.Structure,), {"_fields_": members, "__doc__": f"== {cname}"})
    return out


def prototype(function: tuple, structs: dict) -> tuple:
    """(argtypes, restype) of a parsed function (return type, [parameters])."""
    ret, params = function
    return [ctype(p, structs) for p in params], ctype(ret, structs)
