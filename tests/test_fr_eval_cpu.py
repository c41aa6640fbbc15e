"""CPU side of the scalar field and the blob batches (blsmi 0.21: blsmi_fr_mul_batch[_dev], blsmi_fr_inv_batch[_dev], blsmi_fr_eval_batch[_dev],
blsmi_kzg_verify_blob_batch[_jac|_dev|_jac_dev]): the declarations against the exports and the types bls_amd.fr / bls_amd.kzg call them
with, the argument checks that come before any device work, the wrappers' own checks and marshalling, bls_amd/csrc/fr.h run natively under
the address and undefined-behaviour sanitizers against Python integers -- the field on a grid of edge operands, the constants, the domain
tables --, and the model of tests/fr_eval_cases.py held against Horner's rule."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from bls_amd import _native, engine, fr, kzg
from cabi_common import CTYPES, _header_params, bound_argtypes
from fr_eval_cases import EDGE_OPERANDS, MONT_ONE, R, TOP, BlobCase, bitrev, domain, evaluate, grid_pairs, horner, omega

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -3
FIELD = ["blsmi_fr_mul_batch", "blsmi_fr_mul_batch_dev", "blsmi_fr_inv_batch", "blsmi_fr_inv_batch_dev"]
EVAL = ["blsmi_fr_eval_batch", "blsmi_fr_eval_batch_dev"]
BLOB = ["blsmi_kzg_verify_blob_batch", "blsmi_kzg_verify_blob_batch_jac", "blsmi_kzg_verify_blob_batch_dev", "blsmi_kzg_verify_blob_batch_jac_dev"]
HEADING = "polynomial evaluation in Fr and KZG blob batches (blsmi 0.21)"
TYPES = dict(CTYPES, unsigned=C.c_uint)                                          # `unsigned log2n`: the one spelling 0.21 adds


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def test_declared_exported_and_typed(lib, tmp_path):
    declared = _native.declared_symbols()
    header = open(_native.HEADER).read()
    assert "0.21 adds" in header and "0.20 adds" in header and header.index("0.21 adds") > header.index("0.20 adds")
    assert header.index(HEADING) > header.index("the G1 lift and KZG batches (blsmi 0.20)")
    assert header.rindex("/* ----") == header.index("/* ---- " + HEADING)       # the new section is the last one
    exported = set(re.findall(r" T (blsmi_\w+)", subprocess.run(["nm", "-D", _native.SO_PATH], capture_output=True, text=True, check=True).stdout))
    assert exported == set(declared)                                             # nm -D exports equal the header's names
    sigs = _native.signatures()
    for s in FIELD + EVAL + BLOB:
        assert s in declared and s in exported and hasattr(lib, s) and s in sigs, s
        assert bound_argtypes(s) == [TYPES[t] for t in _header_params(header, s)], s
    twin = _header_params(header, "blsmi_kzg_verify_batch")                      # scalars / block / ok ... as the 0.20 call, noncanon behind ok
    mine = _header_params(header, BLOB[0])
    assert mine[-6:-3] + mine[-2:] == twin[-5:] and mine[-3] == "uint8_t *"
    twin, mine = _header_params(header, "blsmi_kzg_verify_batch_dev"), _header_params(header, BLOB[2])
    assert mine[-7:-4] + mine[-3:] == twin[-6:] and mine[-4] == "void *"
    for mod, names in ((fr, ["mul_batch", "mul_batch_dev", "inv_batch", "inv_batch_dev", "eval_batch", "eval_batch_dev"]),
                       (kzg, ["verify_blob_batch", "verify_blob_batch_jac", "verify_blob_batch_dev", "verify_blob_batch_jac_dev"])):
        for w in names:
            assert callable(getattr(mod, w)) and getattr(mod, w).__module__ == mod.__name__, w
            assert getattr(engine, w, None) is not getattr(mod, w) and not hasattr(engine, "fr_" + w) and not hasattr(engine, "kzg_" + w), w   # bls_amd.engine's inventory stays
    assert not [n for n, v in vars(engine).items() if callable(v) and getattr(v, "__module__", None) in ("bls_amd.fr", "bls_amd.kzg")]
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index(HEADING):])
    for phrase in ("ANY 256-bit value is taken mod r", "the inverse of 0 mod r (0, r, 2 r) is 0", "log2n <= 16", "w = 7^((r - 1) / N) mod r", "0x564c0a11...a5d36306",
                   "the layout of a blob", "noncanon (may be NULL)", "for the caller to reject", "ONE inversion per polynomial", "k_fr_bary_prod", "k_fr_inv",
                   "k_fr_bary_sum", "kept until blsmi_shutdown", "blsmi_trim does not release it", "blsmi_held_bytes does not count it", "BLSMI_E_ARG",
                   "order neither 0 nor 1", "m beyond 2^32 - 1", "m beyond 2^31 - 2", "beyond a size_t", "a zero caller scalar", "nothing is written",
                   "exactly as blsmi_kzg_verify_batch", "ok[j] is exactly its verdict on (C_j, pi_j, z_j, p_j(z_j))", "Fiat-Shamir", "stays the caller's",
                   "*rechecked = 0 on every early return", "No `block` value is refused", "buffers stay untouched", "one device", "request combiner",
                   "\"rlc_min\" does NOT apply", "What it does not change", "the floor of 0.17", "the lift of 0.20", "profiles/r21_blob_eval.log"):
        assert phrase in block, phrase
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "t.c"
    src.write_text('#include "blsmi.h"\nint main(void) { return blsmi_fr_mul_batch(0, 0, 0, 0) + blsmi_fr_mul_batch_dev(0, 0, 0, 0, 0) + blsmi_fr_inv_batch(0, 0, 0)'
                   ' + blsmi_fr_inv_batch_dev(0, 0, 0, 0) + blsmi_fr_eval_batch(0, 12u, 1, 0, 0, 0, 0) + blsmi_fr_eval_batch_dev(0, 12u, 1, 0, 0, 0, 0, 0)'
                   ' + blsmi_kzg_verify_blob_batch(0, 0, 0, 12u, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + blsmi_kzg_verify_blob_batch_jac(0, 0, 0, 12u, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_kzg_verify_blob_batch_dev(0, 0, 0, 12u, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_kzg_verify_blob_batch_jac_dev(0, 0, 0, 12u, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(_native.HEADER), str(src)])


def test_the_kernels_are_a_unit_of_the_build():
    assert "k_fr_eval.hip" in _native._UNITS and "k_fr_eval.hip" in _native._COST and "k_fr_eval.hip" not in _native._LIMBS28_UNITS
    kernels_h = open(os.path.join(_native.CSRC, "kernels.h")).read()
    unit = open(os.path.join(_native.CSRC, "k_fr_eval.hip")).read()
    for k in ("k_fr_mul", "k_fr_inv", "k_fr_bary_prod", "k_fr_bary_sum"):
        assert k + "(" in kernels_h and re.search(r"__launch_bounds__\(FR_WG\) %s\(" % k, unit), k
    code = re.sub(r"//[^\n]*", "", unit)
    assert "atomic" not in code.lower() and "asm" not in code                    # no atomics, no inline assembly: plain C++ stores only
    assert len(re.findall(r"__shared__ u32 lds\[8 \* 2 \* FR_WG\]", unit)) == 2  # two arrays of 256 elements, 16 KB, in either tree kernel


def test_argument_checks_come_before_any_device_work(lib):
    """this machine has no device: anything but BLSMI_E_ARG / BLSMI_OK here would be the sign of device work.  (m * N * 32 beyond a size_t
    cannot be reached where size_t has 64 bits: m <= 2^32 - 1 and N <= 2^16 bound the product by 2^53; the check is there for narrower ones.)"""
    buf = (C.c_uint8 * 4096)()
    w64 = (C.c_uint64 * 512)()
    u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    a, p8 = C.addressof(buf), C.cast(buf, u8p)
    mul, mul_dev, inv, inv_dev = (engine._fn(n) for n in FIELD)
    assert mul(None, p8, p8, 2) == mul(p8, None, p8, 2) == mul(p8, p8, None, 2) == mul(p8, p8, p8, 1 << 32) == E_ARG
    assert mul_dev(None, a, a, 2, None) == mul_dev(a, None, a, 2, None) == mul_dev(a, a, None, 2, None) == mul_dev(a, a, a, 1 << 32, None) == E_ARG
    assert inv(None, p8, 2) == inv(p8, None, 2) == inv(p8, p8, 1 << 32) == E_ARG
    assert inv_dev(None, a, 2, None) == inv_dev(a, None, 2, None) == inv_dev(a, a, 1 << 32, None) == E_ARG
    assert mul(None, None, None, 0) == mul_dev(None, None, None, 0, None) == inv(None, None, 0) == inv_dev(None, None, 0, None) == 0
    ev, ev_dev = (engine._fn(n) for n in EVAL)
    for f, x, tail in ((ev, p8, ()), (ev_dev, a, (None,))):
        for nc in (x, None):
            assert f(None, 4, 0, x, x, nc, 2, *tail) == f(x, 4, 0, None, x, nc, 2, *tail) == f(x, 4, 0, x, None, nc, 2, *tail) == E_ARG
            assert f(x, 17, 0, x, x, nc, 2, *tail) == f(x, 1 << 31, 1, x, x, nc, 2, *tail) == E_ARG     # log2n > 16
            assert f(x, 4, 2, x, x, nc, 2, *tail) == f(x, 4, -1, x, x, nc, 2, *tail) == E_ARG          # order is 0 or 1
            assert f(x, 0, 0, x, x, nc, 1 << 32, *tail) == E_ARG                                       # m beyond 2^32 - 1
            assert f(None, 99, 7, None, None, None, 0, *tail) == 0 and f(x, 4, 1, x, x, nc, 0, *tail) == 0
    assert all(b == 0 for b in buf)                                              # nothing was written
    for name in BLOB:
        fn = engine._fn(name)
        dev = name.endswith("_dev")
        pts = a if dev else (C.cast(w64, u64p) if name.endswith("_jac") else p8)
        sc8 = a if dev else p8

        def call(g=pts, h=pts, polys=sc8, log2n=4, order=1, c=pts, p=pts, z=sc8, m=2, scalars=None, block=0, ok=sc8, nc=sc8, want_nre=True):
            sc = (C.c_uint64 * len(scalars))(*scalars) if scalars else None
            comb, nre = C.c_int(7), C.c_size_t(7)
            tail = (None,) if dev else ()
            rc = fn(g, h, polys, log2n, order, c, p, z, m, sc, block, ok, nc, C.byref(comb), C.byref(nre) if want_nre else None, *tail)
            return rc, comb.value, nre.value if want_nre else 0
        for block in (0, 1, 1 << 40):
            for null in ("g", "h", "polys", "c", "p", "z", "ok"):
                assert call(block=block, **{null: None}) == (E_ARG, 0, 0), (name, null + " NULL")
                assert call(block=block, nc=None, **{null: None}) == (E_ARG, 0, 0), (name, null + " NULL")
            assert call(log2n=17, block=block) == (E_ARG, 0, 0) and call(log2n=0xffffffff, block=block) == (E_ARG, 0, 0), (name, "log2n > 16")
            assert call(order=2, block=block) == (E_ARG, 0, 0) and call(order=-1, block=block) == (E_ARG, 0, 0), (name, "order")
            assert call(scalars=[5, 0], block=block) == (E_ARG, 0, 0), (name, "a zero scalar")
            assert call(m=(1 << 31) - 1, block=block) == (E_ARG, 0, 0), (name, "m beyond 2^31 - 2")
            assert call(m=1 << 32, block=block) == (E_ARG, 0, 0), (name, "m beyond 2^32 - 1")
            assert call(m=0, block=block) == (0, 0, 0), (name, "m = 0")
            assert call(g=None, h=None, polys=None, log2n=99, order=9, c=None, p=None, z=None, ok=None, nc=None, m=0, block=block) == (0, 0, 0), (name, "m = 0, nothing else")
            assert call(ok=None, block=block, want_nre=False)[:2] == (E_ARG, 0), (name, "rechecked may be NULL")
    assert all(b == 0 for b in buf)


def _no_device_or(call, check):
    """a wrapper call on zero-filled input: it marshals (no ctypes.ArgumentError, no TypeError) and either finds no device or returns"""
    try:
        out = call()
    except engine.BlsmiError as e:
        assert "(-1)" in str(e), e
    else:
        assert check(out), out


def test_python_wrappers_validate_and_marshal():
    assert fr.mul_batch(b"", b"").shape == (0, 32) and fr.inv_batch(b"").shape == (0, 32)
    with pytest.raises(ValueError):
        fr.mul_batch(bytes(64), bytes(32))                                       # one b per a
    with pytest.raises(ValueError):
        fr.mul_batch(bytes(33), bytes(33))                                       # whole scalars
    with pytest.raises(ValueError):
        fr.inv_batch(bytes(31))
    _no_device_or(lambda: fr.mul_batch(bytes(64), bytes(64)), lambda o: (o.shape, o.dtype) == ((2, 32), np.uint8))
    _no_device_or(lambda: fr.inv_batch(np.zeros((3, 32), np.uint8)), lambda o: o.shape == (3, 32))
    fr.mul_batch_dev(0, 0, 0, 0); fr.inv_batch_dev(0, 0, 0)
    for call in (lambda: fr.mul_batch_dev(0, 0, 0, 2), lambda: fr.inv_batch_dev(0, 0, 2), lambda: fr.eval_batch_dev(0, 4, 1, 0, 0, 0, 2)):
        with pytest.raises(engine.BlsmiError) as ei:
            call()                                                               # null pointers with n > 0
        assert "(-3)" in str(ei.value)
    y, nc = fr.eval_batch(b"", 4, b"")
    assert y.shape == (0, 32) and nc.shape == (0,) and nc.dtype == bool and fr.eval_batch(b"", 4, b"", noncanon=False)[1] is None
    for bad in (lambda: fr.eval_batch(bytes(32 * 16), 17, bytes(32)), lambda: fr.eval_batch(bytes(32 * 16), -1, bytes(32)),   # log2n is 0 .. 16
                lambda: fr.eval_batch(bytes(32 * 16), 4, bytes(32), order=2),                                                # order is 0 or 1
                lambda: fr.eval_batch(bytes(32 * 15), 4, bytes(32)), lambda: fr.eval_batch(bytes(32 * 16), 4, bytes(64)),      # N values per point
                lambda: fr.eval_batch(bytes(32 * 16), 4, bytes(33)), lambda: fr.eval_batch_dev(0, 17, 0, 0, 0, 0, 0),
                lambda: fr.eval_batch_dev(0, 4, 3, 0, 0, 0, 0)):
        with pytest.raises(ValueError):
            bad()
    for kw in ({}, {"order": 1}, {"noncanon": False}):
        _no_device_or(lambda: fr.eval_batch(bytes(32 * 16 * 2), 4, bytes(64), **kw), lambda o: o[0].shape == (2, 32))
    fr.eval_batch_dev(0, 4, 1, 0, 0, 0, 0)
    f = kzg.verify_blob_batch
    g, h, blobs = bytes(96), bytes(192 * 2), bytes(32 * 16 * 2)
    for bad in (lambda: f(bytes(95), h, blobs, 4, bytes(192), bytes(192), bytes(64)),        # the key has one G1 record
                lambda: f(g, bytes(192 * 3), blobs, 4, bytes(192), bytes(192), bytes(64)),   # ... and two G2 records
                lambda: f(g, h, blobs, 4, bytes(192), bytes(288), bytes(64)),                # one proof per commitment
                lambda: f(g, h, blobs, 4, bytes(192), bytes(192), bytes(32)),                # one z per blob
                lambda: f(g, h, blobs[32:], 4, bytes(192), bytes(192), bytes(64)),           # N values per blob
                lambda: f(g, h, blobs, 3, bytes(192), bytes(192), bytes(64)),
                lambda: f(g, h, blobs, 17, bytes(192), bytes(192), bytes(64)),
                lambda: f(g, h, blobs, 4, bytes(192), bytes(192), bytes(64), order=2),
                lambda: f(g, h, blobs, 4, bytes(192), bytes(192), bytes(64), scalars=[1]),   # one scalar per blob
                lambda: f(g, h, blobs, 4, bytes(192), bytes(192), bytes(64), block=-1),
                lambda: kzg.verify_blob_batch_jac(g, h, blobs, 4, bytes(288), bytes(288), bytes(64))):   # in-memory records are 144 / 288 bytes
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(engine.BlsmiError) as ei:
        f(g, h, blobs, 4, bytes(192), bytes(192), bytes(64), scalars=[3, 0])     # a zero scalar: the library refuses
    assert "(-3)" in str(ei.value)
    for fn, pb, qb in ((kzg.verify_blob_batch, 96, 192), (kzg.verify_blob_batch_jac, 144, 288)):
        ok, nc, comb, nre = fn(bytes(pb), bytes(2 * qb), b"", 12, b"", b"", b"")  # m = 0
        assert ok.shape == (0,) and ok.dtype == np.uint8 and nc.shape == (0,) and nc.dtype == bool and (comb, nre) == (0, 0)
        for kw in ({}, {"scalars": [1, 2]}, {"block": 2}, {"noncanon": False}, {"order": 0}):
            _no_device_or(lambda: fn(bytes(pb), bytes(2 * qb), blobs, 4, bytes(pb * 2), bytes(pb * 2), bytes(64), **kw),
                          lambda out: (out[0].shape, out[0].dtype) == ((2,), np.uint8))
    for fn in (kzg.verify_blob_batch_dev, kzg.verify_blob_batch_jac_dev):
        assert fn(0, 0, 0, 12, 1, 0, 0, 0, 0, 0) == (0, 0)
        assert fn(0, 0, 0, 12, 1, 0, 0, 0, 0, 0, d_noncanon=0, scalars=[], block=2, stream=0) == (0, 0)
        with pytest.raises(engine.BlsmiError) as ei:
            fn(0, 0, 0, 12, 1, 0, 0, 0, 2, 0)                                    # null pointers with m > 0
        assert "(-3)" in str(ei.value)
        with pytest.raises(ValueError):
            fn(0, 0, 0, 17, 1, 0, 0, 0, 0, 0)


# ---- fr.h, natively --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fr_field(tmp_path_factory):
    gpp = shutil.which("g++") or shutil.which("c++")
    assert gpp, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("fr_field") / "fr_field")
    subprocess.check_call([gpp, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "fr_field.cc")])
    return exe


def _native_lines(exe, text):
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-400:], out.stderr[-2000:])
    return out.stdout.splitlines()


def test_fr_field_under_sanitizers(fr_field):
    pairs = grid_pairs(2000, 21)
    assert len(EDGE_OPERANDS) == 28 and len(pairs) == 28 * 28 + 2000 and {0, R, 2 * R, TOP, MONT_ONE - 1} <= set(EDGE_OPERANDS)
    lines = _native_lines(fr_field, "".join("ops %064x %064x\n" % p for p in pairs))
    assert len(lines) == len(pairs)
    for (a, b), line in zip(pairs, lines):
        t = line.split()
        x, y = a % R, b % R
        want = [x * y % R, x * x % R, (x + y) % R, (x - y) % R, -x % R, pow(x, R - 2, R), x]   # mul sqr add sub neg inv, from_be32 / to_be32 round trip
        assert [int(v, 16) for v in t[:7]] == want, (hex(a), hex(b))
        assert all(v < R for v in want) and (want[5] * x % R == 1 or x == 0 == want[5])
        assert [int(v) for v in t[7:]] == [x == 0, x == y, a < R], (hex(a), hex(b))   # is_zero, eq (on reduced representatives), is_canonical


def test_the_constants_against_big_integers(fr_field):
    lines = [int(v, 16) for v in _native_lines(fr_field, "consts\n")]
    w32 = pow(7, (R - 1) >> 32, R)
    assert (R - 1) % (1 << 32) == 0 and pow(7, (R - 1) // 2, R) == R - 1          # 2^32 divides r - 1; 7 is no square
    assert lines[:4] == [R, -pow(R, -1, 1 << 32) % (1 << 32), 2 ** 256 % R, 2 ** 512 % R]
    assert lines[4:] == [pow(w32, 1 << i, R) for i in range(33)] and lines[36] == 1 and lines[35] == R - 1
    # the committed table is what the generator writes
    gen = subprocess.run([sys.executable, os.path.join(_native.CSRC, "gen_fr_consts.py"), "--stdout"], capture_output=True, text=True, check=True).stdout
    assert gen == open(os.path.join(_native.CSRC, "fr_consts.h")).read()


def test_the_domain_tables_against_big_integers(fr_field):
    assert omega(12) == 0x564c0a11a0f704f4fc3e8acfe0f8245f0ad1347b378fbf96e206da11a5d36306   # the root of EIP-4844
    assert [bitrev(i, 3) for i in range(8)] == [0, 4, 2, 6, 1, 5, 3, 7] and bitrev(0, 0) == 0
    shapes = [(k, o) for k in (0, 1, 12, 16) for o in (0, 1)]
    lines = [int(v, 16) for v in _native_lines(fr_field, "".join("domain %d %d\n" % s for s in shapes))]
    at = 0
    for k, order in shapes:
        n = 1 << k
        w = pow(7, (R - 1) // n, R)
        got, at = lines[at:at + n + 1], at + n + 1
        want = [pow(w, bitrev(i, k) if order else i, R) for i in range(n)] if k <= 12 else list(domain(k, order))
        assert got[:n] == want and got[n] == pow(n, -1, R), (k, order)           # position order, then N^-1
        assert got[0] == 1 and len(set(got[:n])) == n and all(pow(v, n, R) == 1 for v in got[:min(n, 64)]), (k, order)
    assert at == len(lines)
    d = domain(16, 1)
    assert d[1] == R - 1 and d[2] == pow(7, (R - 1) // 4, R) and d[(1 << 16) - 1] == pow(omega(16), (1 << 16) - 1, R)   # the model's table, spot-checked by pow


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def test_the_model_against_horner():
    """the barycentric model equals Horner's rule on the coefficients: the values of a random coefficient vector over the domain, taken in
    either order, evaluate to the polynomial's value at random points, at 0, and at the roots themselves"""
    rng = random.Random(8)
    for k in range(0, 9):
        n = 1 << k
        coeffs = [rng.randrange(R) for _ in range(n)]
        for order in (0, 1):
            dom = domain(k, order)
            vals = [horner(coeffs, w) for w in dom]
            for z in [rng.randrange(R), rng.getrandbits(256), 0, R - 1, R, TOP, dom[0], dom[n - 1], dom[n // 2] + R]:
                assert evaluate(vals, k, order, z) == horner(coeffs, z % R), (k, order, hex(z))
            shifted = [v + R if v + R <= TOP and i % 3 == 0 else v for i, v in enumerate(vals)]   # values are taken mod r
            assert evaluate(shifted, k, order, 5) == horner(coeffs, 5)


def test_the_blob_corpus_by_big_integers():
    c = BlobCase(6, 4, 1, 3, spoil={1: "f", 2: "z", 3: "C", 4: "pi"}, edge={0: ("root", 5), 5: "const"})
    assert c.verdicts() == [1, 0, 0, 0, 0, 1] and c.noncanon == [False] * 6
    assert c.z[0] == domain(4, 1)[5] and c.y[0] == c.polys[0][5] and c.pi[5] == bytes(96) and c.C[5] != bytes(96)
    n = BlobCase(3, 4, 1, 3, edge={1: ("noncanon", 7)})
    assert n.verdicts() == [1, 1, 1] and n.noncanon == [False, True, False] and n.polys[1][7] >= R
    assert len(c.poly_bytes) == 6 * 16 * 32 and len(c.commitments) == len(c.proofs) == 6 * 96 and len(c.z_bytes) == 6 * 32
