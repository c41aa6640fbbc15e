"""CPU side of the coset interpolation and the cell batches (blsmi 0.22: blsmi_fr_coset_interp_batch[_dev],
blsmi_kzg_verify_cell_batch[_jac|_dev|_jac_dev]): the declarations against the exports and the types bls_amd.fr / bls_amd.kzg call them
with, the argument checks that come before any device work, the wrappers' own checks and marshalling, bls_amd/csrc/fr_ntt.h run natively
under the address and undefined-behaviour sanitizers against Python integers, and the model of tests/cell_cases.py held against the
remainder mod X^n - h^n and against Horner's rule."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from bls_amd import _native, engine, fr, kzg
from cabi_common import CTYPES, _header_params, bound_argtypes
from cell_cases import (EDGE_SHIFTS, EDGES, L, M, ORDER, SEED, SPOILS, TOP, CellCase, cell_shifts, coset, flags_of, interp, interp_fast,
                        poly_mod_coset)
from fr_eval_cases import EDGE_OPERANDS, R, bitrev, domain, horner, omega
from kzg_cases import INF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -3
INTERP = ["blsmi_fr_coset_interp_batch", "blsmi_fr_coset_interp_batch_dev"]
CELL = ["blsmi_kzg_verify_cell_batch", "blsmi_kzg_verify_cell_batch_jac", "blsmi_kzg_verify_cell_batch_dev", "blsmi_kzg_verify_cell_batch_jac_dev"]
HEADING = "==== coset interpolation in Fr and KZG cell batches (blsmi 0.22)"
TYPES = dict(CTYPES, unsigned=C.c_uint)


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def test_declared_exported_and_typed(lib, tmp_path):
    declared = _native.declared_symbols()
    header = open(_native.HEADER).read()
    assert "0.22 adds" in header and header.index("0.22 adds") > header.index("0.21 adds")
    assert header.index(HEADING) > header.index("polynomial evaluation in Fr and KZG blob batches (blsmi 0.21)")
    assert header.count(HEADING) == 1 and header.index(HEADING) > header.rindex("/* ----")   # behind the last section of that style
    exported = set(re.findall(r" T (blsmi_\w+)", subprocess.run(["nm", "-D", _native.SO_PATH], capture_output=True, text=True, check=True).stdout))
    assert exported == set(declared)                                             # nm -D exports equal the header's names
    sigs = _native.signatures()
    for s in INTERP + CELL:
        assert s in declared and s in exported and hasattr(lib, s) and s in sigs, s
        assert bound_argtypes(s) == [TYPES[t] for t in _header_params(header, s)], s
    twin, mine = _header_params(header, "blsmi_kzg_verify_blob_batch"), _header_params(header, CELL[0])
    assert mine[-7:] == twin[-7:] and mine[:2] == twin[:2]                       # the tail in the order of the blob call, flags where noncanon stands
    twin, mine = _header_params(header, "blsmi_kzg_verify_blob_batch_dev"), _header_params(header, CELL[2])
    assert mine[-8:] == twin[-8:]
    assert _header_params(header, INTERP[0]) == ["const uint8_t *", "unsigned", "int", "const uint8_t *", "uint8_t *", "uint8_t *", "uint8_t *", "size_t"]
    assert _header_params(header, INTERP[1]) == ["const void *", "unsigned", "int", "const void *", "void *", "void *", "void *", "size_t", "void *"]
    for mod, names in ((fr, ["coset_interp_batch", "coset_interp_batch_dev"]),
                       (kzg, ["verify_cell_batch", "verify_cell_batch_jac", "verify_cell_batch_dev", "verify_cell_batch_jac_dev", "cell_shifts"])):
        for w in names:
            assert callable(getattr(mod, w)) and getattr(mod, w).__module__ == mod.__name__ and not hasattr(engine, w), w
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index(HEADING):])
    for phrase in ("COSET h_j <w>", "ANY 256-bit value or shift is taken mod r", "natural order, fully reduced", "shift_pow (may be NULL)", "flags (may be NULL)",
                   "bit 0 of flags[j] is set when a value or the shift of item j was >= r", "bit 1 when h_j = 0 mod r", "is NOT refused", "0^-1 = 0", "0^0 = 1",
                   "the caller rejects by the flag", "c_ji = h_j^(-i) a_ji", "k_fr_inv", "k_fr_coset_interp", "log2n <= 10", "BLSMI_E_ARG", "log2n > 10",
                   "order neither 0 nor 1", "m beyond 2^32 - 1", "m beyond 2^31 - 2", "beyond a size_t", "nothing is written", "coeffs must not overlap vals",
                   "a zero caller scalar", "EIP-7594", "H and [tau^n] H", "exactly as blsmi_kzg_verify_batch", "ok[j] is exactly is_one[j] of blsmi_pairing_product_batch",
                   "P_j = C_j + (h_j^n mod r) pi_j - sum_i c_ji [tau^i] G", "ok[j] does not depend on them", "*rechecked = 0 on every early return",
                   "No `block` value is refused", "buffers stay untouched", "one device", "request combiner", "\"rlc_min\" does NOT apply", "What it does not change"):
        assert phrase in block, phrase
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "t.c"
    src.write_text('#include "blsmi.h"\nint main(void) { return blsmi_fr_coset_interp_batch(0, 6u, 1, 0, 0, 0, 0, 0) + blsmi_fr_coset_interp_batch_dev(0, 6u, 1, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_kzg_verify_cell_batch(0, 0, 0, 6u, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + blsmi_kzg_verify_cell_batch_jac(0, 0, 0, 6u, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_kzg_verify_cell_batch_dev(0, 0, 0, 6u, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_kzg_verify_cell_batch_jac_dev(0, 0, 0, 6u, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(_native.HEADER), str(src)])


def test_the_kernel_is_a_unit_of_the_build():
    assert "k_fr_ntt.hip" in _native._UNITS and "k_fr_ntt.hip" in _native._COST and "k_fr_ntt.hip" not in _native._LIMBS28_UNITS
    kernels_h = open(os.path.join(_native.CSRC, "kernels.h")).read()
    unit = open(os.path.join(_native.CSRC, "k_fr_ntt.hip")).read()
    assert "k_fr_coset_interp(" in kernels_h and len(re.findall(r"^__global__", unit, flags=re.M)) == 1   # one new kernel
    assert re.search(r"__launch_bounds__\(NTT_WG\) k_fr_coset_interp\(", unit) and '#include "fr_ntt.h"' in unit
    code = re.sub(r"//[^\n]*", "", unit)
    assert "atomic" not in code.lower() and "asm" not in code                    # no atomics, no inline assembly: plain C++ stores only
    gen = open(os.path.join(ROOT, "tools", "gen_kernel_decls.py")).read()
    assert '"k_fr_ntt.hip"' in gen and '"k_kzg.hip"' in gen                      # kernels.h is what the generator writes


def test_argument_checks_come_before_any_device_work(lib):
    """this machine has no device: anything but BLSMI_E_ARG / BLSMI_OK here would be the sign of device work.  (m * n * 32 beyond a size_t
    cannot be reached where size_t has 64 bits: m <= 2^32 - 1 and n <= 2^10 bound the product by 2^47; the check is there for narrower ones.)"""
    buf = (C.c_uint8 * 4096)()
    w64 = (C.c_uint64 * 512)()
    u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    a, p8 = C.addressof(buf), C.cast(buf, u8p)
    it, it_dev = (engine._fn(n) for n in INTERP)
    for f, x, tail in ((it, p8, ()), (it_dev, a, (None,))):
        for sp in (x, None):
            for fl in (x, None):
                assert f(None, 2, 0, x, x, sp, fl, 2, *tail) == f(x, 2, 0, None, x, sp, fl, 2, *tail) == f(x, 2, 0, x, None, sp, fl, 2, *tail) == E_ARG
                assert f(x, 11, 0, x, x, sp, fl, 2, *tail) == f(x, 16, 1, x, x, sp, fl, 2, *tail) == f(x, 1 << 31, 1, x, x, sp, fl, 2, *tail) == E_ARG   # log2n > 10
                assert f(x, 2, 2, x, x, sp, fl, 2, *tail) == f(x, 2, -1, x, x, sp, fl, 2, *tail) == E_ARG                                            # order is 0 or 1
                assert f(x, 0, 0, x, x, sp, fl, 1 << 32, *tail) == E_ARG                                                                             # m beyond 2^32 - 1
                assert f(None, 99, 7, None, None, None, None, 0, *tail) == 0 and f(x, 2, 1, x, x, sp, fl, 0, *tail) == 0
    assert all(b == 0 for b in buf)                                              # nothing was written
    for name in CELL:
        fn = engine._fn(name)
        dev = name.endswith("_dev")
        pts = a if dev else (C.cast(w64, u64p) if name.endswith("_jac") else p8)
        sc8 = a if dev else p8

        def call(g=pts, h=pts, vals=sc8, log2n=2, order=1, shifts=sc8, c=pts, p=pts, m=2, scalars=None, block=0, ok=sc8, fl=sc8, want_nre=True):
            sc = (C.c_uint64 * len(scalars))(*scalars) if scalars else None
            comb, nre = C.c_int(7), C.c_size_t(7)
            tail = (None,) if dev else ()
            rc = fn(g, h, vals, log2n, order, shifts, c, p, m, sc, block, ok, fl, C.byref(comb), C.byref(nre) if want_nre else None, *tail)
            return rc, comb.value, nre.value if want_nre else 0
        for block in (0, 1, 1 << 40):
            for null in ("g", "h", "vals", "shifts", "c", "p", "ok"):
                assert call(block=block, **{null: None}) == (E_ARG, 0, 0), (name, null + " NULL")
                assert call(block=block, fl=None, **{null: None}) == (E_ARG, 0, 0), (name, null + " NULL")
            assert call(log2n=11, block=block) == (E_ARG, 0, 0) and call(log2n=0xffffffff, block=block) == (E_ARG, 0, 0), (name, "log2n > 10")
            assert call(order=2, block=block) == (E_ARG, 0, 0) and call(order=-1, block=block) == (E_ARG, 0, 0), (name, "order")
            assert call(scalars=[5, 0], block=block) == (E_ARG, 0, 0), (name, "a zero scalar")
            assert call(m=(1 << 31) - 1, block=block) == (E_ARG, 0, 0), (name, "m beyond 2^31 - 2")
            assert call(m=1 << 32, block=block) == (E_ARG, 0, 0), (name, "m beyond 2^32 - 1")
            assert call(m=0, block=block) == (0, 0, 0), (name, "m = 0")
            assert call(g=None, h=None, vals=None, log2n=99, order=9, shifts=None, c=None, p=None, ok=None, fl=None, m=0, block=block) == (0, 0, 0), (name, "m = 0, nothing else")
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
    co, sp, fl = fr.coset_interp_batch(b"", 6, b"")
    assert co.shape == (0, 64, 32) and sp.shape == (0, 32) and fl.shape == (0,) and fl.dtype == np.uint8
    assert fr.coset_interp_batch(b"", 6, b"", shift_pow=False, flags=False)[1:] == (None, None)
    for bad in (lambda: fr.coset_interp_batch(bytes(32 * 4), 11, bytes(32)), lambda: fr.coset_interp_batch(bytes(32 * 4), -1, bytes(32)),   # log2n is 0 .. 10
                lambda: fr.coset_interp_batch(bytes(32 * 4), 2, bytes(32), order=2),                                                     # order is 0 or 1
                lambda: fr.coset_interp_batch(bytes(32 * 3), 2, bytes(32)), lambda: fr.coset_interp_batch(bytes(32 * 4), 2, bytes(64)),   # n values per shift
                lambda: fr.coset_interp_batch(bytes(32 * 4), 2, bytes(33)), lambda: fr.coset_interp_batch_dev(0, 11, 0, 0, 0, 0, 0, 0),
                lambda: fr.coset_interp_batch_dev(0, 2, 3, 0, 0, 0, 0, 0)):
        with pytest.raises(ValueError):
            bad()
    for kw in ({}, {"order": 1}, {"shift_pow": False}, {"flags": False}):
        _no_device_or(lambda: fr.coset_interp_batch(bytes(32 * 4 * 2), 2, bytes(64), **kw), lambda o: o[0].shape == (2, 4, 32))
    fr.coset_interp_batch_dev(0, 2, 1, 0, 0, 0, 0, 0)
    with pytest.raises(engine.BlsmiError) as ei:
        fr.coset_interp_batch_dev(0, 2, 1, 0, 0, 0, 0, 2)                        # null pointers with m > 0
    assert "(-3)" in str(ei.value)
    f = kzg.verify_cell_batch
    g, h, cells = bytes(96 * 4), bytes(192 * 2), bytes(32 * 4 * 2)
    for bad in (lambda: f(bytes(96 * 3), h, cells, 2, bytes(64), bytes(192), bytes(192)),       # the key has n G1 records
                lambda: f(g, bytes(192 * 3), cells, 2, bytes(64), bytes(192), bytes(192)),      # ... and two G2 records
                lambda: f(g, h, cells, 2, bytes(64), bytes(192), bytes(288)),                   # one proof per commitment
                lambda: f(g, h, cells, 2, bytes(32), bytes(192), bytes(192)),                   # one shift per cell
                lambda: f(g, h, cells[32:], 2, bytes(64), bytes(192), bytes(192)),              # n values per cell
                lambda: f(g, h, cells, 1, bytes(64), bytes(192), bytes(192)),
                lambda: f(g, h, cells, 11, bytes(64), bytes(192), bytes(192)),
                lambda: f(g, h, cells, 2, bytes(64), bytes(192), bytes(192), order=2),
                lambda: f(g, h, cells, 2, bytes(64), bytes(192), bytes(192), scalars=[1]),      # one scalar per cell
                lambda: f(g, h, cells, 2, bytes(64), bytes(192), bytes(192), block=-1),
                lambda: kzg.verify_cell_batch_jac(g, h, cells, 2, bytes(64), bytes(288), bytes(288))):   # in-memory records are 144 / 288 bytes
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(engine.BlsmiError) as ei:
        f(g, h, cells, 2, bytes(64), bytes(192), bytes(192), scalars=[3, 0])     # a zero scalar: the library refuses
    assert "(-3)" in str(ei.value)
    for fn, pb, qb in ((kzg.verify_cell_batch, 96, 192), (kzg.verify_cell_batch_jac, 144, 288)):
        ok, fl, comb, nre = fn(bytes(pb * 64), bytes(2 * qb), b"", 6, b"", b"", b"")   # m = 0
        assert ok.shape == (0,) and ok.dtype == np.uint8 and fl.shape == (0,) and fl.dtype == np.uint8 and (comb, nre) == (0, 0)
        for kw in ({}, {"scalars": [1, 2]}, {"block": 2}, {"flags": False}, {"order": 0}):
            _no_device_or(lambda: fn(bytes(pb * 4), bytes(2 * qb), cells, 2, bytes(64), bytes(pb * 2), bytes(pb * 2), **kw),
                          lambda out: (out[0].shape, out[0].dtype) == ((2,), np.uint8))
    for fn in (kzg.verify_cell_batch_dev, kzg.verify_cell_batch_jac_dev):
        assert fn(0, 0, 0, 6, 1, 0, 0, 0, 0, 0) == (0, 0)
        assert fn(0, 0, 0, 6, 1, 0, 0, 0, 0, 0, d_flags=0, scalars=[], block=2, stream=0) == (0, 0)
        with pytest.raises(engine.BlsmiError) as ei:
            fn(0, 0, 0, 6, 1, 0, 0, 0, 2, 0)                                     # null pointers with m > 0
        assert "(-3)" in str(ei.value)
        with pytest.raises(ValueError):
            fn(0, 0, 0, 11, 1, 0, 0, 0, 0, 0)
    with pytest.raises(ValueError):
        kzg.cell_shifts(-1, 6)
    with pytest.raises(ValueError):
        kzg.cell_shifts(27, 6)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def test_the_model_is_the_remainder_and_reproduces_the_values():
    """interp equals p mod (X^n - h^n) for a random p of degree 2 n + 2, and Horner's rule on its coefficients at the coset gives the values
    back, for l <= 8 in both orders; the fast form the GPU tests use for the large shapes equals it"""
    rng = random.Random(22)
    for l in range(0, 9):
        n = 1 << l
        for order in (0, 1):
            h = rng.randrange(1, R)
            p = [rng.randrange(R) for _ in range(2 * n + 3)]
            pts = coset(l, order, h)
            vals = [horner(p, x) for x in pts]
            c = interp(vals, l, order, h)
            assert c == poly_mod_coset(p, l, h) and c == interp_fast(vals, l, order, h), (l, order)
            assert [horner(c, x) for x in pts] == vals, (l, order)
            shifted = [v + R if i % 3 == 0 else v for i, v in enumerate(vals)]  # values and the shift are taken mod r
            assert interp(shifted, l, order, h + R) == c and interp_fast(shifted, l, order, h + R) == c
    for l in (0, 1, 2, 6):                                                       # h = 0 mod r: c_0 is the mean of the values, nothing else
        for order in (0, 1):
            vals = [rng.randrange(R) for _ in range(1 << l)]
            want = [sum(vals) * pow(1 << l, -1, R) % R] + [0] * ((1 << l) - 1)
            assert interp(vals, l, order, 0) == interp(vals, l, order, R) == interp_fast(vals, l, order, 0) == want
    assert flags_of([1, R - 1], 5) == 0 and flags_of([1, R], 5) == 1 and flags_of([1, 2], R + 5) == 1 and flags_of([1], 0) == 2 and flags_of([TOP], R) == 3


def test_cell_shifts_are_the_reversed_roots_of_an_extended_blob():
    """cell k of an EIP-7594 extended blob (8 192 values, 128 cells of 64) is the coset h_k w_64^bitrev_6(i) = roots_of_unity_brp[64 k + i]"""
    brp = domain(13, 1)
    hs = cell_shifts(7, 6)
    assert len(hs) == 128 and hs[0] == 1 and hs[1] == pow(omega(13), 64, R) and hs[2] == pow(omega(13), bitrev(2, 7), R)
    for k in (0, 1, 2, 77, 127):
        assert coset(6, 1, hs[k]) == list(brp[64 * k:64 * k + 64]), k
    lib_side = kzg.cell_shifts(7, 6)
    assert lib_side.shape == (128, 32) and lib_side.dtype == np.uint8
    assert [int.from_bytes(bytes(r), "big") for r in lib_side] == hs
    assert kzg.cell_shifts(0, 3).tolist() == [[0] * 31 + [1]]


def test_the_cell_corpus_by_big_integers():
    valid = CellCase(M, L, ORDER, SEED, edge=EDGES)
    assert valid.verdicts() == [1] * M
    for kind, spoil in SPOILS.items():
        c = CellCase(M, L, ORDER, SEED, spoil=spoil, edge=EDGES)
        assert c.verdicts() == [0 if j in spoil else 1 for j in range(M)], kind  # each spoil spoils its items only
        for j, how in spoil.items():                                             # ... and moves only what it names
            same = [c.vals[j] == valid.vals[j], c.h[j] == valid.h[j], c.C[j] == valid.C[j], c.pi[j] == valid.pi[j]]
            assert same == [how != "v", how != "h", how != "C", how != "pi"], (kind, j)
    assert [valid.h[j] for j in (0, 1, 2, 3, 4, 6)] == list(EDGE_SHIFTS) and [valid.flags[j] for j in (0, 1, 2, 3, 4, 6, 10)] == [0, 0, 1, 2, 3, 1, 1]
    assert sum(valid.flags) == 8 and valid.pi[8] == INF and valid.C[8] != INF and not any(valid.vals[9]) and not any(valid.coeffs[9]) and valid.pi[9] != INF
    assert valid.vals[10][2] >= R and valid.coeffs[3][1:] == [0, 0, 0] and valid.shift_pow[3] == 0
    tau = valid.key.tau
    assert pow(valid.h[11], 4, R) == pow(tau, 4, R) and valid.pi[11] != INF     # Z(tau) = 0: the item holds whatever its proof
    assert valid.h[15] == valid.h[12] and valid.C[15] != valid.C[12] and valid.C[16] == valid.C[13] and valid.h[16] != valid.h[13]
    assert len(valid.vals_bytes) == M * 4 * 32 and len(valid.srs_g1) == 4 * 96 and len(valid.srs_g2) == 2 * 192 and len(valid.shift_bytes) == M * 32


# ---- fr_ntt.h, natively ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fr_ntt(tmp_path_factory):
    gpp = shutil.which("g++") or shutil.which("c++")
    assert gpp, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("fr_ntt") / "fr_ntt")
    subprocess.check_call([gpp, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "fr_ntt.cc")])
    return exe


def _native_lines(exe, text):
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-400:], out.stderr[-2000:])
    return out.stdout.splitlines()


def test_the_index_arithmetic(fr_ntt):
    """every stage pairs every position exactly once, 2^s apart within blocks of 2^(s + 1), with the twiddle w^-(k << (l - 1 - s))"""
    for l in (0, 1, 2, 3, 6, 10):
        n = 1 << l
        lines = _native_lines(fr_ntt, "index %d\n" % l)
        assert len(lines) == l * (n // 2) + n
        for s in range(l):
            rows = [tuple(int(v) for v in x.split()) for x in lines[s * (n // 2):(s + 1) * (n // 2)]]
            assert sorted(v for lo, hi, _ in rows for v in (lo, hi)) == list(range(n)), (l, s)
            for t, (lo, hi, tw) in enumerate(rows):
                k = lo % (1 << s)
                assert hi == lo + (1 << s) and lo // (1 << s) % 2 == 0 and t == (lo >> (s + 1) << s) + k and tw == (n - (k << (l - 1 - s))) % n, (l, s, t)
        assert [int(x) for x in lines[l * (n // 2):]] == [bitrev(i, l) for i in range(n)]


def test_coset_interp_under_sanitizers(fr_ntt):
    """the serial coset_interp of fr_ntt.h -- the kernel's index arithmetic and butterfly -- against the model: l = 0, 1, 2, 6, 10, both orders,
    random, constant and edge-valued polynomials, a random shift and every edge shift"""
    rng = random.Random(23)
    jobs = []
    for l in (0, 1, 2, 6, 10):
        n = 1 << l
        for order in (0, 1):
            kinds = [[rng.randrange(R) for _ in range(n)], [rng.randrange(R)] * n, [EDGE_OPERANDS[(i * 7 + l) % len(EDGE_OPERANDS)] for i in range(n)]]
            shifts = [rng.randrange(1, R)] + (list(EDGE_SHIFTS) if l != 10 else [R + 1, 0])
            for h in shifts:
                jobs.append((l, order, h, kinds[len(jobs) % 3]))
            jobs.append((l, order, rng.getrandbits(256), kinds[2]))
    text = "".join("interp %d %d %064x %s\n" % (l, order, h, " ".join("%064x" % v for v in vals)) for l, order, h, vals in jobs)
    lines = _native_lines(fr_ntt, text)
    at = 0
    for l, order, h, vals in jobs:
        n = 1 << l
        got, at = lines[at:at + n + 2], at + n + 2
        want = interp_fast(vals, l, order, h) if l > 8 else interp(vals, l, order, h)
        assert [int(v, 16) for v in got[:n]] == want, (l, order, hex(h))
        assert int(got[n], 16) == pow(h % R, n, R) and int(got[n + 1]) == flags_of(vals, h), (l, order, hex(h))
    assert at == len(lines)
