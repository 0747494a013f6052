"""include/drqv2_hip.h as ctypes, for the tests that hold drqv2_amd._lib to it: every `drq_*` declaration, the DrqStep
descriptor, the enums and the integer #defines, read from the header once.  A type this reader does not understand is an
AssertionError that names it, never a guess."""
import ctypes as C
import functools
import os
import re

from drqv2_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "drqv2_hip.h")

SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
           "unsigned": C.c_uint, "unsigned int": C.c_uint, "unsigned long": C.c_uint64, "unsigned long long": C.c_uint64,
           "uint64_t": C.c_uint64, "drq_stream_t": C.c_void_p}
POINTEES = dict(SCALARS, DrqStep=_lib.DrqStep)


@functools.lru_cache(None)
def text():
    """the header as it is, comments included (the section titles and formulas the tests look for live in them)"""
    with open(HEADER) as f:
        return f.read()


@functools.lru_cache(None)
def code():
    """the header without its comments"""
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text(), flags=re.S))


def ctypes_of(ctype, where):
    """the ctypes types a prototype may give a C type (`const` and spacing ignored): one for a scalar; c_void_p for a
    pointer and, where the pointee is known, the typed pointer beside it"""
    words = ctype.replace("*", " * ").split()
    stars = words.count("*")
    base = " ".join(w for w in words if w not in ("*", "const"))
    if stars == 0:
        assert base in SCALARS, f"{where}: type {ctype!r} is not understood"
        return (SCALARS[base],)
    pointee = C.c_void_p if stars > 1 else POINTEES.get(base)     # a pointer to pointers: POINTER(c_void_p)
    return (C.c_void_p,) if pointee is None else (C.c_void_p, C.POINTER(pointee))


def _declarator(decl, where):
    """'const float* x' -> ('const float*', 'x')"""
    m = re.fullmatch(r"(.*?[\s*])([A-Za-z_]\w*)", " ".join(decl.split()))
    assert m and "[" not in decl, f"{where}: declaration {decl!r} is not understood"
    return m.group(1).strip(), m.group(2)


@functools.lru_cache(None)
def c_declarations():
    """{name: (return type, [parameter types])} as C text for every drq_* function declared"""
    out = {}
    for ret, name, params in re.findall(r"\b([A-Za-z_][\w ]*?[\s*]+)(drq_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code()):
        assert name not in out, f"{name} is declared twice"
        params = [] if params.strip() in ("", "void") else params.split(",")
        out[name] = (ret.strip(), [_declarator(p, name)[0] for p in params])
    return out


@functools.lru_cache(None)
def declarations():
    """{name: (the return type's ctypes types, [those of every parameter])} for every drq_* function declared"""
    return {name: (ctypes_of(ret, name), [ctypes_of(p, name) for p in params])
            for name, (ret, params) in c_declarations().items()}


def stream_entries():
    """the entries whose last parameter is the stream they launch on"""
    return {name for name, (_, params) in c_declarations().items() if params and params[-1] == "drq_stream_t"}


def assert_prototype(name):
    """_lib.PROTOTYPES[name] is the header's declaration of name: the return type and every argument type"""
    assert name in _lib.PROTOTYPES, f"{name} is missing from _lib.PROTOTYPES"
    assert name in declarations(), f"{name} is not declared in the header"
    (ret, params), (res, args) = declarations()[name], _lib.PROTOTYPES[name]
    assert res in ret, f"{name}: restype {res}, the header says {ret}"
    assert len(args) == len(params), f"{name}: {len(args)} argtypes, the header has {len(params)} parameters"
    for i, (a, p) in enumerate(zip(args, params)):
        assert a in p, f"{name}: argument {i} is {a}, the header says {p}"


@functools.lru_cache(None)
def struct_fields(name):
    """[(field, its ctypes types)] of `typedef struct { ... } name;`, in order"""
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + name + r"\s*;", code())
    assert m, f"struct {name} is not in the header"
    out = []
    for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
        first, *more = decl.split(",")
        ctype, field = _declarator(first, name)
        assert not more or "*" not in decl, f"{name}: declaration {decl!r} is not understood"
        out += [(f.strip(), ctypes_of(ctype, name)) for f in [field] + more]
    return out


@functools.lru_cache(None)
def enumerators():
    """{name: value} over every enum of the header"""
    out = {}
    for body in re.findall(r"\benum\s*\{([^}]*)\}", code()):
        value = -1
        for item in filter(None, (i.strip() for i in body.split(","))):
            name, _, given = (s.strip() for s in item.partition("="))
            value = int(given, 0) if given else value + 1
            out[name] = value
    return out


def define(name):
    """the integer a #define gives name"""
    m = re.search(r"^\s*#\s*define\s+" + name + r"\s+\(?(-?\w+)\)?\s*$", code(), re.M)
    assert m, f"{name} is not defined in the header"
    return int(m.group(1), 0)
