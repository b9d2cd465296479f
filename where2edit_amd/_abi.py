"""The C ABI of libw2e.so as ctypes needs it, read from include/*.h once at import: PROTOS {entry point: (restype, [argtypes])},
STRUCTS {C name: ctypes.Structure} and CONSTS {object-like integer #define: value}.  The headers are the only place a signature, a
struct layout or a constant is written down; nothing here (or anywhere else in Python) restates one.  Pure Python: no torch, no
library -- a declaration this reader cannot map is an error at import that names the header and the declaration, never a gap.

Every pointer is c_void_p -- the C type cannot tell a host `int*` from a device one, and c_void_p takes byref(), arrays, addresses and
None alike -- except `const char*` (c_char_p) and a pointer to one of the structs (POINTER of it)."""
import ctypes
import glob
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}
_POINTEES = {"float", "double", "int", "int16_t", "int32_t", "int64_t", "uint8_t", "uint32_t", "unsigned long long", "void"}
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+\(?[ \t]*(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*\)?[ \t]*$", re.M)
_STRUCT = re.compile(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", re.S)
_FUNCTION = re.compile(r"([\w\s*]+?)\b(w2e_\w+)\s*\(([^()]*)\)\s*;")


def _ctype(c_type, structs):
    """The ctypes type of one C type (no declarator name), or None where the fixed mapping has none."""
    words = c_type.replace("*", " * ").split()
    stars = words.count("*")
    base = " ".join(w for w in words if w not in ("*", "const"))
    if stars == 0:
        return _SCALARS.get(base)
    if stars == 1 and base == "char" and words[0] == "const":
        return ctypes.c_char_p
    if stars == 1 and base in structs:
        return ctypes.POINTER(structs[base])
    return ctypes.c_void_p if base in _POINTEES else None


def _declarator(text, structs, where):
    """`type name` (or a bare `type`) -> (ctypes type, name or None)."""
    t = _ctype(text, structs)
    if t is not None:
        return t, None
    m = re.fullmatch(r"(.*?)(\w+)", text.strip(), re.S)
    t = _ctype(m.group(1), structs) if m else None
    if t is None:
        raise ValueError(f"{where}: no ctypes type for `{' '.join(text.split())}`")
    return t, m.group(2)


def parse(text, where="<header>", structs=None):
    """(PROTOS, STRUCTS, CONSTS) of one header's text.  `structs`: the structs of headers read before it (extended in place)."""
    structs = {} if structs is None else structs
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = text.replace("\\\n", " ")
    consts = {name: int(value, 0) for name, value in _DEFINE.findall(text)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)

    def struct(m):
        fields = []
        for line in filter(None, (s.strip() for s in m.group(1).split(";"))):
            first, *more = line.split(",")
            ftype, name = _declarator(first, structs, f"{where}: struct {m.group(2)}")
            if name is None or any(not re.fullmatch(r"\s*\w+\s*", n) for n in more):
                raise ValueError(f"{where}: struct {m.group(2)}: cannot read the field `{line}`")
            fields += [(n.strip(), ftype) for n in [name] + more]
        structs[m.group(2)] = type(m.group(2), (ctypes.Structure,), {"_fields_": fields})
        return " "
    text = _STRUCT.sub(struct, text)

    protos = {}
    for m in _FUNCTION.finditer(text):
        decl = f"{where}: {m.group(2)}"
        res, _ = _declarator(m.group(1), structs, decl)
        args = [] if m.group(3).strip() in ("", "void") else [_declarator(a, structs, decl)[0] for a in m.group(3).split(",")]
        if m.group(2) in protos:
            raise ValueError(f"{decl}: declared twice")
        protos[m.group(2)] = (res, args)
    seen = re.findall(r"\b(w2e_\w+)\s*\(", text)
    if sorted(seen) != sorted(protos):
        raise ValueError(f"{where}: cannot read the declaration of {sorted(set(seen) - set(protos)) or sorted(seen)}")
    return protos, structs, consts


PROTOS, STRUCTS, CONSTS = {}, {}, {}
for _path in sorted(glob.glob(os.path.join(INCLUDE, "*.h"))):
    _p, _, _c = parse(open(_path).read(), os.path.relpath(_path, os.path.dirname(INCLUDE)), STRUCTS)
    if set(_p) & set(PROTOS) or set(_c) & set(CONSTS):
        raise ValueError(f"{_path}: declares again {sorted((set(_p) & set(PROTOS)) | (set(_c) & set(CONSTS)))}")
    PROTOS.update(_p)
    CONSTS.update(_c)
