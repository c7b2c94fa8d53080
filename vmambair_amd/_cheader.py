"""Reads the C ABI out of include/vmambair_oss.h: constants, structs and prototypes as ctypes objects (for _capi.py).

Not a C parser.  The header keeps to the subset its opening comment lists, and every declaration between its ``extern "C"``
braces that is not of one of those forms is a ``RuntimeError`` naming the text -- nothing is skipped.  Needs neither the library
nor a GPU.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import NamedTuple

SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double,
           "long long": C.c_longlong}

_INT = re.compile(r"\(?\s*(-?\d+)\s*\)?")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S.*)$", re.M)   # a #define without a value is an include guard
#: one declaration: typedef struct / enum { body } name;  |  typedef void *name;  |  ret name(args);
_DECL = re.compile(r"\s*(?:typedef\s+(struct|enum)\s*\{([^{}]*)\}\s*(\w+)|typedef\s+void\s*\*\s*(\w+)|([\w\s*]+?)\s*\(([^()]*)\))\s*;")


class Header(NamedTuple):
    constants: dict    # name -> int: the #defines and the enumerators
    structs: dict      # name -> ctypes.Structure subclass, in header order
    prototypes: dict   # name -> (restype, argtypes), in header order


def _fail(what: str, text: str):
    raise RuntimeError(f"C header outside the subset _cheader.py reads, {what}: {' '.join(text.split())!r}")


def _declarator(text: str, types: dict):
    """``const float *a`` -> ("float", 1, "a");  ``int n`` -> ("int", 0, "n");  ``long long`` -> ("long long", 0, "")"""
    left, star, right = text.partition("*")
    words = [w for w in left.split() if w != "const"]
    if star:
        base, stars, name = " ".join(words), 1 + right.count("*"), right.replace("*", " ").strip()
    elif " ".join(words) in types:
        base, stars, name = " ".join(words), 0, ""
    else:
        base, stars, name = " ".join(words[:-1]), 0, words[-1] if words else ""
    if not re.fullmatch(r"\w*", name):
        _fail("cannot read the declarator", text)
    return base, stars, name


def parse(text: str) -> Header:
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants, structs, prototypes, types = {}, {}, {}, dict(SCALARS)

    def put(table, name, value, where):
        if name in constants or name in types or name in prototypes:
            _fail(f"duplicate name {name}", where)
        table[name] = value

    def scalar(base, where):
        if base not in types:
            _fail(f"unknown type {base!r}", where)
        return types[base]

    for m in _DEFINE.finditer(text):
        v = _INT.fullmatch(m[2].strip()) or _fail("#define that is not an integer", m[0])
        put(constants, m[1], int(v[1]), m[0])
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    m = re.search(r'extern\s+"C"\s*\{(.*)\}', text, re.S)
    body, pos = (m[1] if m else text), 0
    while body[pos:].strip():
        m = _DECL.match(body, pos) or _fail("cannot read the declaration", body[pos:].partition(";")[0])
        pos = m.end()
        kind, inner, name, handle, head, args = m.groups()
        if handle:                                        # typedef void *name;
            put(types, handle, C.c_void_p, m[0])
        elif kind == "enum":
            for item in filter(str.strip, inner.split(",")):
                e = re.fullmatch(r"\s*(\w+)\s*=\s*(-?\d+)\s*", item) or _fail("cannot read the enumerator", item)
                put(constants, e[1], int(e[2]), item)
            put(types, name, C.c_int, m[0])
        elif kind == "struct":
            fields = []
            for line in filter(str.strip, inner.split(";")):
                first, *more = line.split(",")
                base, stars, fname = _declarator(first, types)
                # the `*` belongs to the declarator, not to the base type: const void *u, *delta;
                for n_stars, fname in [(stars, fname)] + [(d.count("*"), d.replace("*", " ").strip()) for d in more]:
                    if not re.fullmatch(r"\w+", fname):
                        _fail("cannot read the field", line)
                    fields.append((fname, C.c_void_p if n_stars else scalar(base, line)))   # an earlier struct embeds its class
            cls = type(name, (C.Structure,), {"_fields_": fields})
            put(types, name, cls, m[0])
            structs[name] = cls
        else:                                             # ret name(args);
            base, stars, fname = _declarator(head, types)
            if not fname:
                _fail("cannot read the declaration", m[0])
            restype = (C.c_char_p if base == "char" and stars == 1 else C.c_void_p) if stars else \
                None if base == "void" else scalar(base, m[0])
            argtypes = []
            for arg in [] if args.strip() == "void" else args.split(","):
                base, stars, _ = _declarator(arg, types)
                if stars == 1 and base in structs and base.endswith("_params"):
                    argtypes.append(C.POINTER(structs[base]))   # callers pass the struct object itself
                else:
                    argtypes.append(C.c_void_p if stars else scalar(base, m[0]))
            put(prototypes, fname, (restype, argtypes), m[0])
    return Header(constants, structs, prototypes)


def read(path: str) -> Header:
    with open(path) as f:
        return parse(f.read())
