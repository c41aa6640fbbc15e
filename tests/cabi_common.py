"""The tests' own reading of include/blsmi.h, independent of bls_amd._native.signatures(): the parameter spellings of one prototype and the
ctypes type each spelling stands for.  The ABI tests compare what bls_amd.engine binds against it."""
import ctypes as C
import re

from bls_amd import engine

CTYPES = {"const uint8_t *": C.POINTER(C.c_uint8), "uint8_t *": C.POINTER(C.c_uint8), "const uint64_t *": C.POINTER(C.c_uint64), "uint64_t *": C.POINTER(C.c_uint64),
          "const uint32_t *": C.POINTER(C.c_uint32), "size_t": C.c_size_t, "int": C.c_int, "int *": C.POINTER(C.c_int), "size_t *": C.POINTER(C.c_size_t),
          "const void *": C.c_void_p, "void *": C.c_void_p}


def strip_comments(header):
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", header, flags=re.S)


def _header_params(header, name, ret="int"):
    """the parameter types of one prototype, comments and names stripped: 'const uint8_t *', 'size_t', ...  (ret: the return type's spelling;
    any other than int needs a header without comments, where nothing but the prototype writes `name(`)"""
    m = re.search(r"\b%s\s*%s\s*\(([^;]*?)\);" % (re.escape(ret), name), header, flags=re.S)
    assert m, name
    out = []
    for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
        a = " ".join(a.split())
        arr = re.fullmatch(r"(.*?)\s*\w+\[\d*\]", a)
        if arr:                                                                  # `const uint8_t domain[8]` is a pointer
            out.append(arr.group(1) + " *")
        elif "*" in a:
            out.append(a[:a.rindex("*") + 1])
        else:
            out.append(a.rsplit(" ", 1)[0])
    return out


def bound_argtypes(name):
    """the argument types bls_amd.engine calls the entry point with (every one of these returns int)"""
    fn = engine._fn(name)
    assert fn.restype is C.c_int, name
    return list(fn.argtypes)
