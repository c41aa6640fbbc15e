"""CPU side of the pairing products (blsmi 0.10: blsmi_pairing_product_batch[_jac|_dev|_jac_dev]): the declarations and exports, the
argument checks that return BLSMI_E_ARG before any device work, m = 0, the Python wrappers' flattening and validation, and the
construction the GPU tests (tests/test_gpu_pairing_product.py) use to make products that equal one: e(aP, Q) e(-P, aQ) = 1."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bls_amd import _native, engine
from oracle import pyref as P
from oracle import refcpu as RC

E_ARG = -3
SYMS = ["blsmi_pairing_product_batch", "blsmi_pairing_product_batch_jac", "blsmi_pairing_product_batch_dev", "blsmi_pairing_product_batch_jac_dev"]


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def test_declared_and_exported(lib, tmp_path):
    declared = _native.declared_symbols()
    for s in SYMS:
        assert s in declared, s
        assert hasattr(lib, s), s
    header = open(_native.HEADER).read()
    assert "0.10 adds" in header
    # the call's scope is stated where the committee batches state theirs
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index("pairing products (blsmi 0.10)"):])
    for phrase in ("ONE device", "not sharded", "request combiner", "\"segsum_chunk\"", "FQ12One", "BLSMI_E_ARG"):
        assert phrase in block, phrase
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "t.c"
    src.write_text('#include "blsmi.h"\nint main(void) { return blsmi_pairing_product_batch(0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_pairing_product_batch_jac(0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(_native.HEADER), str(src)])


def test_version_string_source():
    txt = open(os.path.join(_native.CSRC, "blsmi.hip")).read()
    assert re.search(r'"blsmi 0\.10 ', txt)


def _u64(vals):
    a = np.ascontiguousarray(vals, dtype=np.uint64)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint64))


def _buf(n):
    a = np.zeros(max(8, n), dtype=np.uint8)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint8))


def _host_calls(lib):
    """(name, call(np, seg_off or None, m, g1_null=False, g2_null=False, outs=(True, True))) for the two host forms"""
    def mk(fn, jac):
        def call(np_, seg_off, m, g1_null=False, g2_null=False, outs=(True, True)):
            a, pa = _buf((144 if jac else 96) * np_)
            b, pb = _buf((288 if jac else 192) * np_)
            out = np.zeros(max(1, 72 * m), dtype=np.uint64)
            one, pone = _buf(m)
            so = ps = None
            if seg_off is not None:
                so, ps = _u64(seg_off)
            if jac:
                pa, pb = a.ctypes.data_as(C.POINTER(C.c_uint64)), b.ctypes.data_as(C.POINTER(C.c_uint64))
            args = [None if g1_null else pa, None if g2_null else pb]
            if not jac:
                args.append(None)
            args += [C.c_size_t(np_), ps, C.c_size_t(m), out.ctypes.data_as(C.POINTER(C.c_uint64)) if outs[0] else None, pone if outs[1] else None]
            return fn(*args)
        return call
    return [("affine", mk(lib.blsmi_pairing_product_batch, False)), ("jac", mk(lib.blsmi_pairing_product_batch_jac, True))]


def test_host_argument_checks_come_before_any_device_work(lib):
    """this machine has no device: anything but BLSMI_E_ARG / BLSMI_OK here would be the sign of device work"""
    for name, call in _host_calls(lib):
        assert call(4, [1, 2, 4], 2) == E_ARG, (name, "seg_off[0] != 0")
        assert call(4, [0, 3, 2, 4], 3) == E_ARG, (name, "decreasing offsets")
        assert call(4, [0, 2, 3], 2) == E_ARG, (name, "seg_off[m] < np")
        assert call(4, [0, 2, 5], 2) == E_ARG, (name, "seg_off[m] > np")
        assert call(4, None, 2) == E_ARG, (name, "seg_off NULL")
        assert call(4, [0, 2, 4], 2, g1_null=True) == E_ARG, (name, "g1 NULL with np > 0")
        assert call(4, [0, 2, 4], 2, g2_null=True) == E_ARG, (name, "g2 NULL with np > 0")
        assert call(4, [0, 2, 4], 2, outs=(False, False)) == E_ARG, (name, "both outputs NULL")
        assert call(4, None, 0) == 0, (name, "m = 0")
        assert call(0, None, 0, g1_null=True, g2_null=True, outs=(False, False)) == 0, (name, "m = 0, nothing else")


def test_dev_forms_null_buffers_and_empty(lib):
    v = C.c_void_p
    z = C.c_size_t
    assert lib.blsmi_pairing_product_batch_dev(None, None, None, z(4), None, z(2), None, None, None) == E_ARG
    assert lib.blsmi_pairing_product_batch_jac_dev(None, None, z(4), None, z(2), None, None, None) == E_ARG
    assert lib.blsmi_pairing_product_batch_dev(v(0), v(0), v(0), z(0), v(0), z(0), v(0), v(0), v(0)) == 0
    assert lib.blsmi_pairing_product_batch_jac_dev(v(0), v(0), z(0), v(0), z(0), v(0), v(0), v(0)) == 0


def test_python_wrappers_flatten_and_validate():
    assert engine.seg_offsets([2, 0, 3]).tolist() == [0, 2, 2, 5]
    g1, g2 = bytes(96 * 5), bytes(192 * 5)
    with pytest.raises(ValueError):
        engine.pairing_product_batch(g1[:-1], g2, engine.seg_offsets([5]))                 # not whole records
    with pytest.raises(ValueError):
        engine.pairing_product_batch(g1, g2[:192 * 4], engine.seg_offsets([5]))            # the two sides differ in count
    with pytest.raises(ValueError):
        engine.pairing_product_batch(g1, g2, engine.seg_offsets([2, 2]))                   # offsets end short of np
    with pytest.raises(ValueError):
        engine.pairing_product_batch(g1, g2, engine.seg_offsets([5]), inf_flags=bytes(4))  # one flag per pair
    with pytest.raises(ValueError):
        engine.pairing_product_batch(g1, g2, [])                                           # m + 1 entries, at least the 0
    with pytest.raises(ValueError):
        engine.pairing_product_batch_jac(bytes(144 * 5), bytes(288 * 4), engine.seg_offsets([5]))
    with pytest.raises(ValueError):
        engine.pairing_product_batch_dev(8, 8, 1, 8, 1, 8, 8, d_inf_flags=8, jac=True)     # the in-memory form takes no flags
    # what the library itself refuses reaches the caller as an error, not as a result
    with pytest.raises(engine.BlsmiError):
        engine.pairing_product_batch(g1, g2, [1, 5])
    # m = 0: nothing to do, no device needed
    vals, one = engine.pairing_product_batch(b"", b"", [0])
    assert vals.shape == (0, 72) and vals.dtype == np.uint64 and one.shape == (0,) and one.dtype == np.uint8
    vals, one = engine.pairing_product_batch_jac(b"", b"", engine.seg_offsets([]))
    assert vals.shape == (0, 72) and one.shape == (0,)


def fq12_one():
    one = np.zeros(72, dtype=np.uint64)
    one[:6] = np.array(P.limbs64(P.to_mont(1)), dtype=np.uint64)
    return one


def neg_g1(p):
    return p[:48] + ((P.Q - int.from_bytes(p[48:], "big")) % P.Q).to_bytes(48, "big")


def test_product_that_equals_one_on_the_oracle():
    """e(aP, Q) e(-P, aQ) = 1: the two-pair equations of the GPU tests, confirmed on the oracle alone"""
    xs = P.XORShift(2024)
    p = RC.g1_mul(RC.g1_generator(), P.rand_fr(xs).to_bytes(32, "big"))
    q = RC.g2_mul(RC.g2_generator(), P.rand_fr(xs).to_bytes(32, "big"))
    a = P.rand_fr(xs)
    ap, aq = RC.g1_mul(p, a.to_bytes(32, "big")), RC.g2_mul(q, a.to_bytes(32, "big"))
    ok, v = RC.final_exponentiation(RC.miller_loop(ap + neg_g1(p), q + aq, 2))
    assert ok and np.array_equal(v, fq12_one())
    bq = RC.g2_mul(q, ((a + 1) % P.R_ORDER).to_bytes(32, "big"))                # a perturbed scalar
    ok, v = RC.final_exponentiation(RC.miller_loop(ap + neg_g1(p), q + bq, 2))
    assert ok and not np.array_equal(v, fq12_one())
    # FE is multiplicative: the long segments of the GPU tests are checked through the fold of single pairings
    e1, e2 = RC.pairing_batch(ap + p, q + bq, 2)
    ok, v = RC.final_exponentiation(RC.miller_loop(ap + p, q + bq, 2))
    assert ok and np.array_equal(v, RC.fq12_mul(e1, e2))
