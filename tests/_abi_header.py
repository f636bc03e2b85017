"""include/dktstereo.h as ctypes sees it: the one reader of the header for the host-side ABI tests (test_host_abi_mirror.py
compares the whole of _ffi with it; the per-operator test_host_*_abi.py files take single facts from it).  The header is
read once and its comments are dropped; every function below returns the same parsed object on every call.

The rule that turns a C declaration into ctypes (functions() for arguments, structs() for fields):
    T *const *                 -> POINTER(c_void_p)      a host array of device pointers (_ffi.ptr_array)
    int *                      -> POINTER(c_int)         arguments only: a host array of ints
    dkt_<struct> *             -> POINTER(<its mirror>)  arguments only: the ctypes.Structure of _ffi whose docstring names it
    any other pointer          -> c_void_p               device addresses, void *stream
    int, long, float, double   -> c_int, c_long, c_float, c_double
    return long / const char * -> c_long / c_char_p, otherwise c_int
"""
import ctypes
import functools
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "dktstereo.h")

#: (entry, argument index): the exceptions to the rule, compared as c_void_p.  Each is a table that lives in DEVICE memory
#: (_flat_tables builds the pointer and length tables of dkt_ema_update / dkt_adamw_step on the device; the error word of
#: dkt_loop_status is a device counter), so Python passes its raw address, never a host array.
DEVICE_TABLES = {("dkt_loop_status", 4): "device error word", ("dkt_ema_update", 0): "device pointer table",
                 ("dkt_ema_update", 1): "device pointer table", ("dkt_adamw_step", 0): "device pointer table",
                 ("dkt_adamw_step", 1): "device pointer table", ("dkt_adamw_step", 2): "device pointer table",
                 ("dkt_adamw_step", 3): "device pointer table"}

_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double}
_PP = ctypes.POINTER(ctypes.c_void_p)
_STRUCT = r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;"


@functools.lru_cache(None)
def raw():
    """The header as written, comments included (for the tests that check what a comment cites)."""
    with open(HEADER) as f:
        return f.read()


@functools.lru_cache(None)
def text():
    """The header without its comments."""
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", raw(), flags=re.S)


@functools.lru_cache(None)
def defines():
    """{name: value} of the integer #defines and of the members of the status enum."""
    out = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$", text(), flags=re.M)}
    for body in re.findall(r"\benum\s*\{(.*?)\}", text(), flags=re.S):
        out.update((k, int(v)) for k, v in re.findall(r"(\w+)\s*=\s*(-?\d+)", body))
    return out


@functools.lru_cache(None)
def mirrors():
    """{struct name: the ctypes.Structure of _ffi whose docstring opens with that name}."""
    from dkt_stereo_amd import _ffi
    out = {}
    for cls in vars(_ffi).values():
        if isinstance(cls, type) and issubclass(cls, ctypes.Structure) and cls is not ctypes.Structure:
            m = re.match(r"(dkt_\w+) of include/dktstereo\.h", cls.__doc__ or "")
            assert m and m.group(1) not in out, cls
            out[m.group(1)] = cls
    return out


def _pointer(decl, argument):
    """ctype of the pointer declaration `decl` ("const float *const *pyr", "void *stream", "const dkt_x_desc *d")."""
    if re.search(r"\*\s*const\s*\*", decl):
        return _PP
    assert decl.count("*") == 1, decl
    base = " ".join(w for w in decl.split("*")[0].split() if w != "const")
    if argument and base == "int":
        return ctypes.POINTER(ctypes.c_int)
    if argument and base.startswith("dkt_"):
        return ctypes.POINTER(mirrors()[base])
    return ctypes.c_void_p


@functools.lru_cache(None)
def functions():
    """{name: (restype, [argtypes])} of every dkt_* prototype, by the rule above with DEVICE_TABLES applied."""
    out = {}
    flat = re.sub(_STRUCT, " ", text(), flags=re.S)
    for ret, name, args in re.findall(r"\b(const\s+char\s*\*|int|long)\s*(dkt_\w+)\s*\(([^;{}()]*)\)\s*;", flat):
        assert name not in out, name
        argtypes = []
        for i, a in enumerate([] if args.strip() == "void" else args.split(",")):
            a = " ".join(a.split())
            if (name, i) in DEVICE_TABLES:
                assert "*" in a, (name, i)
                argtypes.append(ctypes.c_void_p)
            elif "*" in a:
                argtypes.append(_pointer(a, True))
            else:
                assert re.match(r"(int|long|float|double) \w+$", a), (name, a)
                argtypes.append(_SCALARS[a.split()[0]])
        out[name] = (ctypes.c_long if ret == "long" else ctypes.c_int if ret == "int" else ctypes.c_char_p, argtypes)
    return out


@functools.lru_cache(None)
def structs():
    """{name: [(field, ctype, array length or 0)]} of every typedef struct, in declaration order; lengths are literals or
    #defines of the header."""
    out = {}
    for name, body in re.findall(_STRUCT, text(), flags=re.S):
        fields = out[name] = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            base = re.match(r"(?:const )?(void|float|double|int|long|unsigned char|unsigned)\b", decl)
            assert base, (name, decl)
            for item in decl[base.end():].split(","):
                m = re.match(r"\s*((?:\*\s*(?:const\s*)?)*)(\w+)\s*(?:\[(\w+)\])?\s*$", item)
                assert m, (name, decl)
                stars, field, dim = m.groups()
                ct = _pointer("%s %s" % (base.group(1), stars), False) if stars else _SCALARS[base.group(1)]
                length = 0 if dim is None else int(dim) if dim.isdigit() else defines()[dim]
                fields.append((field, ct, length))
    return out


def mirror_fields(cls):
    """The _fields_ of a ctypes.Structure in the form structs() gives."""
    return [(n, t._type_, t._length_) if issubclass(t, ctypes.Array) else (n, t, 0) for n, t in cls._fields_]
