"""bls_amd._native.signatures(): the one table bls_amd.engine binds every entry point from, read out of include/blsmi.h.  Held against the C
compiler for all of its prototypes, against the library's exports, and against literals for one entry point per spelling class."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from bls_amd import _native, engine
from cabi_common import _header_params, strip_comments

V, Z, I = C.c_void_p, C.c_size_t, C.c_int
u8p, u64p, i32p, intp, zp = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_int), C.POINTER(C.c_size_t)
# (fixed-width and plain names of one width are one ctypes class: uint64_t / size_t, uint32_t / unsigned, int32_t / int -- and one C type on this ABI)
SPELL = {C.c_int: "int", C.c_uint: "unsigned", C.c_size_t: "size_t", C.c_longlong: "long long", C.c_float: "float", C.c_uint8: "uint8_t",
         C.c_void_p: "void *", C.c_char_p: "char *", None: "void"}


def _spell(t):
    return SPELL[t] if t in SPELL else _spell(t._type_) + " *"


def test_table_against_the_compiler_and_the_exports(tmp_path):
    """`ret (*p_i)(types...) = name;` for every entry point, the types spelled back from the table: a wrong arity, width, signedness or pointer depth
    anywhere fails the build.  ctypes has no const, so that one qualifier comes from the tests' own reading of the header."""
    _native.build()
    sigs = _native.signatures()
    assert len(sigs) >= 206 and _native.declared_symbols() == sorted(sigs)
    exported = set(re.findall(r" T (blsmi_\w+)", subprocess.run(["nm", "-D", _native.SO_PATH], capture_output=True, text=True, check=True).stdout))
    assert exported == set(sigs)                                                 # nm -D exports equal the header's names
    header = strip_comments(open(_native.HEADER).read())
    lines = ['#include "blsmi.h"']
    for i, (name, (ret, args)) in enumerate(sorted(sigs.items())):
        spelled = [s for s in _header_params(header, name, ret="") if s != "void"]
        assert len(spelled) == len(args), name
        params = ", ".join(("const " if s.startswith("const ") else "") + _spell(t) for s, t in zip(spelled, args)) or "void"
        const_ret = re.search(r"^const\b[\w \*]*\b%s\s*\(" % name, header, flags=re.M)
        lines.append("%s%s (*p_%d)(%s) = %s;" % ("const " if const_ret else "", _spell(ret), i, params, name))
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "sigs.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(_native.HEADER), str(src)])


PINS = {
    "blsmi_host_alloc": (I, [Z, C.POINTER(V)]),                                  # void **
    "blsmi_set_option": (I, [C.c_char_p, C.c_longlong]),                         # const char *, long long
    "blsmi_version": (C.c_char_p, []),
    "blsmi_last_profile": (I, [C.c_char_p, Z]),                                  # char *
    "blsmi_debug_device_leases": (C.c_longlong, [I]),
    "blsmi_held_bytes": (Z, []),                                                 # a size_t return
    "blsmi_shutdown": (None, []),                                                # a void return
    "blsmi_last_kernel_ms": (I, [C.POINTER(C.c_float)] * 2),
    "blsmi_debug_lat_unit": (I, [I, i32p, Z, Z, i32p, u8p]),
    "blsmi_g1_msm_ex": (I, [u8p, u8p, Z, u8p, intp, C.c_uint]),                  # uint8_t out[96], unsigned
    "blsmi_trim": (I, [Z, zp]),
    "blsmi_groth16_verify_batch_jac_dev": (I, [V, V, Z, V, V, V, Z, u64p, Z, V, intp, zp, V]),
}


@pytest.mark.parametrize("name", sorted(PINS))
def test_pinned_signatures(name):
    assert _native.signatures()[name] == PINS[name]


def test_an_unknown_spelling_raises_and_names_the_prototype():
    for spelling in ("struct blsmi_ctx *", "double", "uint8_t * * *", "const"):
        with pytest.raises(_native.NativeError, match="int blsmi_x"):
            _native._ctype(spelling, "int blsmi_x(...)")


def test_the_binder_types_private_objects_and_leaves_the_library_alone():
    _native.build()
    fn = engine._fn("blsmi_held_bytes")
    assert fn is engine._fn("blsmi_held_bytes") and (fn.restype, list(fn.argtypes)) == (Z, [])
    raw = engine._lib().blsmi_held_bytes
    assert raw is not fn and raw.restype is C.c_int and raw.argtypes is None     # what every other user of the library sees
