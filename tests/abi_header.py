"""include/mtvaf_hip.h as data: every prototype, both structs and the integer defines, parsed from the header with its comments
stripped, and the C-to-ctypes mapping the binding (mtvaf_amd/hip.py: _SIGS, LayerStruct, LayerGradsStruct) is checked against.
A statement the parser cannot read, or a C type outside the mapping, is an AssertionError: nothing is left out quietly."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mtvaf_hip.h")

CTYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
          "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}
_STRUCT = re.compile(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", re.S)


def raw():
    return open(HEADER).read()


def source():
    """The header without its comments."""
    return re.sub(r"/\*.*?\*/", " ", raw(), flags=re.S)


def comment_before(name):
    """The comment block that precedes the prototype of `name`."""
    src = raw()
    at = re.search(r"\b\w+\s+" + name + r"\s*\(", src)
    assert at, f"{name} is not declared in include/mtvaf_hip.h"
    return src[src.rfind("/*", 0, at.start()):at.start()]


def ctype(c_type):
    """ctypes type of a C type as the header spells it: any pointer and mtvaf_stream_t are c_void_p."""
    if "*" in c_type or c_type == "mtvaf_stream_t":
        return ctypes.c_void_p
    assert c_type in CTYPES, f"C type {c_type!r} has no ctypes mapping"
    return CTYPES[c_type]


def _declarator(text):
    """'const float* const* A' -> ('const float* const*', 'A')."""
    m = re.fullmatch(r"(.*?)(\w+)", " ".join(text.split()))
    assert m and m.group(1).strip(), f"cannot read the declarator {text!r}"
    return re.sub(r"\s*\*\s*", "*", m.group(1)).strip(), m.group(2)


def prototypes():
    """[(result type, name, [(C type, argument name)])] in header order: every statement of the header that is neither a
    preprocessor line, a typedef nor the extern "C" bracket must read as a prototype."""
    src = _STRUCT.sub(" ", source())
    src = re.sub(r"^\s*#.*$", " ", src, flags=re.M)
    src = re.sub(r'extern\s+"C"\s*\{|\}', " ", src)
    out = []
    for stmt in (" ".join(s.split()) for s in src.split(";")):
        if not stmt or stmt.startswith("typedef "):
            continue
        m = re.fullmatch(r"(.+?)\b(mtvaf_\w+)\s*\((.*)\)", stmt)
        assert m, f"not a prototype: {stmt!r}"
        args = [] if m.group(3).strip() == "void" else [_declarator(a) for a in m.group(3).split(",")]
        out.append((m.group(1).strip(), m.group(2), args))
    return out


def prototype(name):
    found = [p for p in prototypes() if p[1] == name]
    assert len(found) == 1, f"{name} is declared {len(found)} times in include/mtvaf_hip.h"
    return found[0]


def signature(name):
    """(restype, [argtypes]) of `name` as ctypes types, the form of hip._SIGS."""
    res, _, args = prototype(name)
    return ctype(res), [ctype(t) for t, _ in args]


def structs():
    """{struct name: [(field name, C type)]} in declaration order."""
    out = {}
    for body, name in _STRUCT.findall(source()):
        fields = []
        for decl in (" ".join(d.split()) for d in body.split(";")):
            if not decl:
                continue
            m = re.fullmatch(r"((?:const\s+)?\w+)\s*([\w\s,*]+)", decl)
            assert m, f"cannot read the field declaration {decl!r} of {name}"
            for d in m.group(2).split(","):
                stars, field = re.fullmatch(r"\s*([*\s]*)(\w+)\s*", d).groups()
                fields.append((field, m.group(1) + "*" * stars.count("*")))
        out[name] = fields
    return out


def defines():
    """{name: value} of every integer #define MTVAF_*."""
    return {n: int(v) for n, v in re.findall(r"^\s*#\s*define\s+(MTVAF_\w+)\s+\(?(-?\d+)\)?\s*$", source(), flags=re.M)}
