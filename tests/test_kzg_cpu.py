"""CPU side of the G1 lift and the KZG batches (blsmi 0.20: blsmi_g1_mul_add_batch[_dev], blsmi_kzg_verify_batch[_jac|_dev|_jac_dev]): the
declarations against the exports and the types bls_amd.kzg calls them with, the argument checks that come before any device work, the
wrappers' own checks and marshalling, the corpus of tests/kzg_cases.py by the oracle alone, and the folded block equation composed from the
oracle's primitives and big integers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bls_amd import _native, engine, kzg
from cabi_common import CTYPES, _header_params, bound_argtypes
from kzg_cases import BAD_TWO, EDGE_SCALARS, EDGES, INF, M, R, SEED, SPOILS, KzgCase, is_one
from oracle import refcpu as RC
from pprod_rlc_locate_common import blocks_of, fq12_prod, rechecked_of
from test_pprod_rlc_locate_cpu import PINNED

E_ARG = -3
LIFT = ["blsmi_g1_mul_add_batch", "blsmi_g1_mul_add_batch_dev"]
FOUR = ["blsmi_kzg_verify_batch", "blsmi_kzg_verify_batch_jac", "blsmi_kzg_verify_batch_dev", "blsmi_kzg_verify_batch_jac_dev"]
WRAPPERS = ["verify_batch", "verify_batch_jac", "verify_batch_dev", "verify_batch_jac_dev", "g1_mul_add_batch", "g1_mul_add_batch_dev"]
HEADING = "the G1 lift and KZG batches (blsmi 0.20)"


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def test_declared_exported_and_typed(lib, tmp_path):
    declared = _native.declared_symbols()
    header = open(_native.HEADER).read()
    assert "0.20 adds" in header and "0.19 adds" in header
    assert header.index(HEADING) > header.index("scalar-field folds and Groth16 batches (blsmi 0.19)")   # the new section is the last
    exported = set(re.findall(r" T (blsmi_\w+)", subprocess.run(["nm", "-D", _native.SO_PATH], capture_output=True, text=True, check=True).stdout))
    assert exported == set(declared)                                             # nm -D exports equal the header's names
    sigs = _native.signatures()
    for s in LIFT + FOUR:
        assert s in declared and s in exported and hasattr(lib, s) and s in sigs, s
        assert bound_argtypes(s) == [CTYPES[t] for t in _header_params(header, s)], s
    twin = _header_params(header, "blsmi_groth16_verify_batch")                  # scalars / block / ok / combined / rechecked as the Groth16 call has them
    assert _header_params(header, FOUR[0])[-5:] == twin[-5:]
    assert _header_params(header, FOUR[2])[-6:] == _header_params(header, "blsmi_groth16_verify_batch_dev")[-6:]
    for w in WRAPPERS:
        assert callable(getattr(kzg, w)) and getattr(kzg, w).__module__ == "bls_amd.kzg", w
        assert getattr(engine, w, None) is not getattr(kzg, w) and not hasattr(engine, "kzg_" + w), w   # bls_amd.engine's inventory stays as it is
    assert not [n for n, v in vars(engine).items() if callable(v) and getattr(v, "__module__", None) == "bls_amd.kzg"]
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index(HEADING):])
    for phrase in ("ANY 256-bit value is taken mod r", "A_j may be any curve point", "every B_j lies in the prime-order subgroup", "the addition is a doubling",
                   "H, tau * H", "(P_j, H), (pi_j, -tau * H)", "P_j = C_j + (z_j mod r) * pi_j - (y_j mod r) * G", "the pair contributes 1",
                   "an all-zero srs_g2 entry drops its pairs", "three Miller loops", "no y_j * G exists", "and only those", "the lift never runs twice",
                   "prime-order subgroups", "at most 2^-64", "caller scalars carry 0.17's caveat", "BLSMI_E_ARG", "*rechecked = 0 on every early return",
                   "No `block` value is refused", "buffers stay untouched", "one device", "request combiner", "\"rlc_min\" does NOT apply"):
        assert phrase in block, phrase
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "t.c"
    src.write_text('#include "blsmi.h"\nint main(void) { return blsmi_g1_mul_add_batch(0, 0, 0, 0, 0, 0, 0, 0) + blsmi_g1_mul_add_batch_dev(0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_kzg_verify_batch(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + blsmi_kzg_verify_batch_jac(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_kzg_verify_batch_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + blsmi_kzg_verify_batch_jac_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(_native.HEADER), str(src)])


def test_the_kernel_is_a_unit_of_the_build():
    assert "k_kzg.hip" in _native._UNITS and "k_kzg.hip" in _native._COST
    kernels_h = open(os.path.join(_native.CSRC, "kernels.h")).read()
    assert "k_g1_mul_add_glv(" in kernels_h
    unit = open(os.path.join(_native.CSRC, "k_kzg.hip")).read()
    assert re.search(r"__launch_bounds__\(WG, BLSMI_GLV_WAVES\) k_g1_mul_add_glv\(", unit)   # launch bounds as k_g1_mul_glv


def test_argument_checks_come_before_any_device_work(lib):
    """this machine has no device: anything but BLSMI_E_ARG / BLSMI_OK here would be the sign of device work"""
    buf = (C.c_uint8 * 4096)()
    w64 = (C.c_uint64 * 512)()
    u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    a = C.addressof(buf)
    for name in FOUR:
        fn = engine._fn(name)
        dev = name.endswith("_dev")
        pts = a if dev else (C.cast(w64, u64p) if name.endswith("_jac") else C.cast(buf, u8p))
        sc8 = a if dev else C.cast(buf, u8p)

        def call(g=pts, h=pts, c=pts, p=pts, z=sc8, y=sc8, m=2, scalars=None, block=0, ok=sc8, want_nre=True):
            sc = (C.c_uint64 * len(scalars))(*scalars) if scalars else None
            comb, nre = C.c_int(7), C.c_size_t(7)
            tail = (None,) if dev else ()
            rc = fn(g, h, c, p, z, y, m, sc, block, ok, C.byref(comb), C.byref(nre) if want_nre else None, *tail)
            return rc, comb.value, nre.value if want_nre else 0
        for block in (0, 1, 1 << 40):
            for null in ("g", "h", "c", "p", "z", "y", "ok"):
                assert call(block=block, **{null: None}) == (E_ARG, 0, 0), (name, null + " NULL")
            assert call(scalars=[5, 0], block=block) == (E_ARG, 0, 0), (name, "a zero scalar")
            assert call(m=(1 << 31) - 1, block=block) == (E_ARG, 0, 0), (name, "m beyond 2^31 - 2")
            assert call(m=1 << 32, block=block) == (E_ARG, 0, 0), (name, "m beyond 2^32 - 1")
            assert call(m=0, block=block) == (0, 0, 0), (name, "m = 0")
            assert call(g=None, h=None, c=None, p=None, z=None, y=None, ok=None, m=0, block=block) == (0, 0, 0), (name, "m = 0, nothing else")
            assert call(ok=None, block=block, want_nre=False)[:2] == (E_ARG, 0), (name, "rechecked may be NULL")
    lift = engine._fn(LIFT[0])
    p8 = C.cast(buf, u8p)
    assert lift(None, 96, p8, 96, p8, p8, p8, 2) == E_ARG and lift(p8, 96, None, 96, p8, p8, p8, 2) == E_ARG and lift(p8, 96, p8, 96, None, p8, p8, 2) == E_ARG
    assert lift(p8, 96, p8, 96, p8, None, p8, 2) == E_ARG and lift(p8, 96, p8, 96, p8, p8, None, 2) == E_ARG
    for stride in (48, 95, 98, 1):
        assert lift(p8, stride, p8, 96, p8, p8, p8, 2) == E_ARG and lift(p8, 96, p8, stride, p8, p8, p8, 2) == E_ARG, stride
    assert lift(p8, 96, p8, 96, p8, p8, p8, 1 << 32) == E_ARG
    assert lift(None, 0, None, 0, None, None, None, 0) == 0
    lift_dev = engine._fn(LIFT[1])
    assert lift_dev(None, 96, a, 96, a, a, a, 2, None) == E_ARG and lift_dev(a, 96, a, 96, a, None, a, 2, None) == E_ARG and lift_dev(a, 100, a, 94, a, a, a, 2, None) == E_ARG
    assert lift_dev(None, 0, None, 0, None, None, None, 0, None) == 0


def _no_device_or(call, check):
    """a wrapper call on zero-filled input: it marshals (no ctypes.ArgumentError, no TypeError) and either finds no device or returns"""
    try:
        out = call()
    except engine.BlsmiError as e:
        assert "(-1)" in str(e), e
    else:
        assert check(out), out


def test_python_wrappers_validate_and_marshal():
    f = kzg.verify_batch
    g, h = bytes(96), bytes(192 * 2)
    with pytest.raises(ValueError):
        f(bytes(95), h, bytes(96 * 2), bytes(96 * 2), bytes(64), bytes(64))     # the key has one G1 record
    with pytest.raises(ValueError):
        f(g, bytes(192 * 3), bytes(96 * 2), bytes(96 * 2), bytes(64), bytes(64))   # ... and two G2 records
    with pytest.raises(ValueError):
        f(g, h, bytes(96 * 2), bytes(96 * 3), bytes(64), bytes(64))             # one proof per commitment
    with pytest.raises(ValueError):
        f(g, h, bytes(96 * 2), bytes(96 * 2), bytes(32), bytes(64))             # one z per opening
    with pytest.raises(ValueError):
        f(g, h, bytes(96 * 2), bytes(96 * 2), bytes(64), bytes(96))             # one y per opening
    with pytest.raises(ValueError):
        f(g, h, bytes(96 * 2), bytes(96 * 2), bytes(64), bytes(64), scalars=[1])   # one scalar per opening
    with pytest.raises(ValueError):
        f(g, h, bytes(96 * 2), bytes(96 * 2), bytes(64), bytes(64), block=-1)    # block is a size
    with pytest.raises(ValueError):
        kzg.verify_batch_jac(g, h, bytes(144 * 2), bytes(144 * 2), bytes(64), bytes(64))   # in-memory records are 144 / 288 bytes
    with pytest.raises(engine.BlsmiError) as ei:
        f(g, h, bytes(96 * 2), bytes(96 * 2), bytes(64), bytes(64), scalars=[3, 0])   # a zero scalar: the library refuses
    assert "(-3)" in str(ei.value)
    for fn, pb, qb in ((kzg.verify_batch, 96, 192), (kzg.verify_batch_jac, 144, 288)):
        ok, comb, nre = fn(bytes(pb), bytes(2 * qb), b"", b"", b"", b"")        # n = 0
        assert ok.shape == (0,) and ok.dtype == np.uint8 and (comb, nre) == (0, 0)
        for kw in ({}, {"scalars": [1, 2]}, {"block": 2}):                       # n = 2
            _no_device_or(lambda: fn(bytes(pb), bytes(2 * qb), bytes(pb * 2), bytes(pb * 2), bytes(64), bytes(64), **kw),
                          lambda out: (out[0].shape, out[0].dtype) == ((2,), np.uint8))
    for fn in (kzg.verify_batch_dev, kzg.verify_batch_jac_dev):
        assert fn(0, 0, 0, 0, 0, 0, 0, 0) == (0, 0)
        assert fn(0, 0, 0, 0, 0, 0, 0, 0, scalars=[], block=2, stream=0) == (0, 0)
        with pytest.raises(engine.BlsmiError) as ei:
            fn(0, 0, 0, 0, 0, 0, 2, 0)                                           # null pointers with m > 0
        assert "(-3)" in str(ei.value)
    ma = kzg.g1_mul_add_batch
    out, inf = ma(b"", b"", b"", 0)
    assert out.shape == (0, 96) and inf.shape == (0,) and inf.dtype == bool
    _no_device_or(lambda: ma(bytes(192), bytes(192), bytes(64), 2), lambda o: o[0].shape == (2, 96))
    _no_device_or(lambda: ma(bytes(96), bytes(96 + 128), bytes(64), 2, a_stride=0, b_stride=128), lambda o: o[0].shape == (2, 96))
    with pytest.raises(ValueError):
        ma(bytes(192), bytes(192), bytes(64), 2, a_stride=50)                    # a stride is 0 or a multiple of 4 from 96 up
    with pytest.raises(ValueError):
        ma(bytes(192), bytes(192), bytes(64), 2, b_stride=128)                   # the bytes are exactly what the records span
    with pytest.raises(ValueError):
        ma(bytes(192), bytes(192), bytes(32), 2)                                 # one scalar per item
    with pytest.raises(ValueError):
        ma(b"", b"", b"", -1)
    kzg.g1_mul_add_batch_dev(0, 96, 0, 96, 0, 0, 0, 0)
    with pytest.raises(ValueError):
        kzg.g1_mul_add_batch_dev(0, 96, 0, 7, 0, 0, 0, 0)


# ---- the corpus and the folded block equation on the oracle ---------------------------------------------------------------------------
def _scalars(m):
    return [PINNED[j % len(PINNED)] + (j // len(PINNED)) for j in range(m)]


@pytest.fixture(scope="module")
def cases():
    out = {"valid": KzgCase(M, SEED), "edges": KzgCase(M, SEED, edge=EDGES)}
    for kind, spoil in SPOILS.items():
        out[kind] = KzgCase(M, SEED, spoil=spoil)
    return out


def test_the_corpus_is_right_by_the_oracle_alone(cases):
    for kind, c in cases.items():
        bad = SPOILS.get(kind, {})
        assert c.verdicts() == [0 if j in bad else 1 for j in range(M)], kind      # every item comes out as constructed
    e = cases["edges"]
    assert [e.z[j] for j in (0, 1, 2, 3)] == list(EDGE_SCALARS) and [e.y[j] for j in (4, 6, 8, 9)] == list(EDGE_SCALARS)
    assert e.pi[10] == INF and e.C[10] != INF and e.y[10] % R != 0                 # pi at infinity: y = c
    assert e.C[11] == INF and e.pi[11] != INF
    assert e.W(12) == INF and e.C[12] != INF and e.pi[12] != INF                   # W at infinity, neither summand is
    assert e.C[13] == RC.g1_mul(e.pi[13], (e.z[13] % R).to_bytes(32, "big"))       # C = z pi: the lift's addition is a doubling
    assert e.y[4] % R == 0 and e.y[8] % R == 0                                     # s_b = 0 at block 1
    v = cases["valid"]
    assert all(p != INF for p in v.C + v.pi) and len(v.commitments) == len(v.proofs) == 96 * M and len(v.z_bytes) == len(v.y_bytes) == 32 * M
    # only the value moved / only the evaluation point moved: the points of the spoiled item are those of the valid batch
    assert (cases["y"].C[5], cases["y"].pi[5], cases["y"].z[5]) == (v.C[5], v.pi[5], v.z[5]) and cases["y"].y[5] == v.y[5] + 1
    assert (cases["z"].C[14], cases["z"].pi[14], cases["z"].y[14]) == (v.C[14], v.pi[14], v.y[14]) and cases["z"].z[14] == v.z[14] + 1
    # an all-zero tau H: the one-pair product (P_j, H), one exactly when P_j = [q tau] G is at infinity
    assert e.verdicts((e.H, bytes(192)))[:14] == [1 if j == 10 else 0 for j in range(14)]


@pytest.mark.parametrize("block", [1, 8, 33])
def test_the_folded_block_equation_from_the_oracle_alone(cases, block):
    """FE of a block's cells -- the s_b (-G) cell from the big-integer s_b, no P_j and no y_j G anywhere -- is prod_{j in b} (item value j)^(r_j):
    one exactly when every item of the block holds.  The spoiled value moves the block's value: only the fold sees it."""
    r = _scalars(M)
    for kind in ("two", "y", "z", "edges"):
        c, bad = cases[kind], SPOILS.get(kind, {})
        values = {j: c.item_value(j) for j in bad}
        for lo, hi in blocks_of(M, block):
            v = c.block_value(r, lo, hi)
            want = fq12_prod(RC.fq12_exp_u64(values[j], r[j]) for j in range(lo, hi) if j in bad)   # (the items that hold contribute 1^r = 1)
            assert np.array_equal(np.asarray(v, dtype=np.uint64), np.asarray(want, dtype=np.uint64)), (kind, block, lo)
            assert is_one(v) == (not any(lo <= j < hi for j in bad)), (kind, block, lo)
    assert rechecked_of(M, block, BAD_TWO) == {1: 2, 8: 16, 33: 33}[block]
