"""CPU side of the randomised pairing-product batches (blsmi 0.17: blsmi_pairing_product_batch_rlc[_jac|_dev|_jac_dev],
blsmi_debug_pairing_product_batch_rlc_dev_nosplit): the declarations against the exports and the Python wrappers' argument types, the
argument checks that come before any device work, the host plan (bls_amd/csrc/pprod_rlc_plan.h) run natively under the address and
undefined-behaviour sanitizers, and the combined equation composed from the oracle's primitives on the corpus of
tests/pprod_rlc_corpus.py -- what tests/test_gpu_pprod_rlc.py expects of the device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bls_amd import _native, engine
from cabi_common import CTYPES, _header_params, bound_argtypes
from oracle import refcpu as RC
from pprod_rlc_corpus import ONE, QA, Corpus, g1, neg1, table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -3
FOUR = ["blsmi_pairing_product_batch_rlc", "blsmi_pairing_product_batch_rlc_jac", "blsmi_pairing_product_batch_rlc_dev", "blsmi_pairing_product_batch_rlc_jac_dev"]
SYMS = FOUR + ["blsmi_debug_pairing_product_batch_rlc_dev_nosplit"]


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def test_declared_exported_and_typed(lib, tmp_path):
    declared = _native.declared_symbols()
    header = open(_native.HEADER).read()
    assert "0.17 adds" in header and "0.16 adds" in header
    assert "pairing products, randomised (blsmi 0.17)" in header
    exported = set(re.findall(r" T (blsmi_\w+)", subprocess.run(["nm", "-D", _native.SO_PATH], capture_output=True, text=True, check=True).stdout))
    assert exported == set(declared)                                             # nm -D exports equal the header's names
    for s in SYMS:
        assert s in declared and s in exported and hasattr(lib, s), s
        want = [CTYPES[t] for t in _header_params(header, s)]
        assert bound_argtypes(s) == want, s
    for w in ("pairing_product_batch_rlc", "pairing_product_batch_rlc_jac", "pairing_product_batch_rlc_dev", "pairing_product_batch_rlc_jac_dev"):
        assert callable(getattr(engine, w)), w
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index("pairing products, randomised (blsmi 0.17)"):])
    for phrase in ("contributes 1", "one device", "request combiner", "BLSMI_E_ARG", "never touched", "not merged",
                   "is_one[j] is exactly what blsmi_pairing_product_batch gives item j", "at most 2^-64", "prime-order subgroups", "\"rlc_min\" does NOT apply"):
        assert phrase in block, phrase
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "t.c"
    src.write_text('#include "blsmi.h"\nint main(void) { return blsmi_pairing_product_batch_rlc(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_pairing_product_batch_rlc_jac(0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_pairing_product_batch_rlc_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_pairing_product_batch_rlc_jac_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_debug_pairing_product_batch_rlc_dev_nosplit(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(_native.HEADER), str(src)])


def test_argument_checks_come_before_any_device_work(lib):
    """this machine has no device: anything but BLSMI_E_ARG / BLSMI_OK here would be the sign of device work"""
    buf = (C.c_uint8 * 4096)()
    w64 = (C.c_uint64 * 512)()
    u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    for name in FOUR[:2]:
        fn = engine._fn(name)
        jac = name.endswith("_jac")
        pts = C.cast(w64, u64p) if jac else C.cast(buf, u8p)

        def call(q=(0, 1, 1, 0), nq=2, np_=4, seg=(0, 2, 4), scalars=None, m=2, g1p=pts, tab=pts, null_seg=False, want_one=True):
            qi = (C.c_uint32 * max(1, len(q)))(*q) if q is not None else None
            so = (C.c_uint64 * len(seg))(*seg)
            sc = (C.c_uint64 * len(scalars))(*scalars) if scalars else None
            one = (C.c_uint8 * 8)(*([7] * 8))
            comb = C.c_int(7)
            head = (g1p, tab) if jac else (g1p, None, tab)
            rc = fn(*head, nq, qi, np_, None if null_seg else so, m, sc, one if want_one else None, C.byref(comb))
            return rc, comb.value, list(one)[:m]
        assert call(seg=(1, 2, 4))[:2] == (E_ARG, 0), (name, "offsets that do not start at 0")
        assert call(seg=(0, 3, 2))[:2] == (E_ARG, 0), (name, "offsets that decrease")
        assert call(seg=(0, 2, 3))[:2] == (E_ARG, 0), (name, "offsets that do not end at np")
        assert call(q=(0, 1, 2, 0))[:2] == (E_ARG, 0), (name, "q_idx >= nq")
        assert call(q=(0, 0, 0, 0), nq=0)[:2] == (E_ARG, 0), (name, "nq = 0 with pairs")
        assert call(q=None, nq=3)[:2] == (E_ARG, 0), (name, "q_idx NULL with nq != np")
        assert call(scalars=[5, 0])[:2] == (E_ARG, 0), (name, "a zero scalar")
        assert call(g1p=None)[:2] == (E_ARG, 0), (name, "g1 NULL")
        assert call(tab=None)[:2] == (E_ARG, 0), (name, "table NULL")
        assert call(null_seg=True)[:2] == (E_ARG, 0), (name, "seg_off NULL")
        assert call(want_one=False)[:2] == (E_ARG, 0), (name, "is_one NULL")
        assert call(q=(), seg=(0,), np_=0, m=0) == (0, 0, []), (name, "m = 0")
        assert call(q=None, nq=0, seg=(0,), np_=0, m=0, g1p=None, tab=None, null_seg=True, want_one=False)[:2] == (0, 0), (name, "m = 0, nothing else")
        assert call(q=(), nq=2, seg=(0, 0, 0, 0), np_=0, m=3, g1p=None, tab=None) == (0, 1, [1, 1, 1]), (name, "np = 0 with m = 3: every item is one, no device")
    a = C.addressof(buf)
    for name in FOUR[2:] + SYMS[4:]:                                              # what the _dev forms can refuse without a device
        fn = engine._fn(name)
        head = (a, a) if name.endswith("_jac_dev") else (a, None, a)
        comb = C.c_int(7)
        assert fn(*head, 2, a, 4, a, 2, (C.c_uint64 * 2)(3, 0), a, C.byref(comb), None) == E_ARG and comb.value == 0, (name, "a zero scalar")
        comb = C.c_int(7)
        assert fn(*head, 3, None, 4, a, 2, None, a, C.byref(comb), None) == E_ARG and comb.value == 0, (name, "d_q_idx NULL with nq != np")
        comb = C.c_int(7)
        assert fn(*head, 2, a, 4, a, 2, None, None, C.byref(comb), None) == E_ARG and comb.value == 0, (name, "d_is_one NULL")
        comb = C.c_int(7)
        assert fn(*head, 2, a, 4, None, 2, None, a, C.byref(comb), None) == E_ARG and comb.value == 0, (name, "d_seg_off NULL")
        comb = C.c_int(7)
        assert fn(*((None,) * len(head)), 0, None, 0, None, 0, None, None, C.byref(comb), None) == 0 and comb.value == 0, (name, "m = 0")


def test_python_wrappers_validate():
    with pytest.raises(ValueError):
        engine.pairing_product_batch_rlc(bytes(96 * 2), bytes(192 * 3), None, [0, 2])                  # no q_idx: one entry per pair
    with pytest.raises(ValueError):
        engine.pairing_product_batch_rlc(bytes(96 * 2), bytes(192), [0], [0, 2])                       # one index per pair
    with pytest.raises(ValueError):
        engine.pairing_product_batch_rlc(bytes(96 * 2), bytes(192), [0, 0], [0, 1])                    # offsets end at np
    with pytest.raises(ValueError):
        engine.pairing_product_batch_rlc(bytes(96 * 2), bytes(192), [0, 0], [0, 2], scalars=[1, 2])    # one scalar per item
    with pytest.raises(ValueError):
        engine.pairing_product_batch_rlc_jac(bytes(96 * 2), bytes(288), [0, 0], [0, 2])                # in-memory records are 144 bytes
    with pytest.raises(engine.BlsmiError) as ei:
        engine.pairing_product_batch_rlc(bytes(96 * 2), bytes(192), [0, 1], [0, 2])                    # index >= nq: the library refuses
    assert "(-3)" in str(ei.value)
    one, comb = engine.pairing_product_batch_rlc(b"", bytes(192), [], [0, 0, 0])
    assert one.tolist() == [1, 1] and comb == 1
    one, comb = engine.pairing_product_batch_rlc(b"", b"", None, [0])
    assert one.shape == (0,) and comb == 0


def test_plan_under_sanitizers(tmp_path):
    gpp = shutil.which("g++") or shutil.which("c++")
    assert gpp, "no C++ compiler"
    exe = str(tmp_path / "pprod_rlc_plan")
    subprocess.check_call([gpp, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "pprod_rlc_plan.cc")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.fullmatch(r"PPROD_RLC_PLAN ok \d+\n", out.stdout), (out.stdout, out.stderr)
    # one plan read line by line: entries 8 and 5 shared (pairs 0, 2 and 3, 5, 6), entries 0, 2, 7 singletons; shared first, each in table order
    out = subprocess.run([exe, "9", "3", "0", "3", "3", "8", "8", "2", "8", "5", "0", "5", "5", "7"], capture_output=True, text=True, check=True).stdout.splitlines()
    assert out == ["item_of 0 0 0 2 2 2 2 2", "perm 3 5 6 0 2", "seg_off 0 3 5", "single 4 1 7", "entry_of 5 8 0 2 7", "group_of 1 3 1 0 2 0 0 4"]
    out = subprocess.run([exe, "3", "2", "0", "1", "3"], capture_output=True, text=True, check=True).stdout.splitlines()      # q_idx NULL
    assert out == ["item_of 0 1 1", "perm", "seg_off 0", "single 0 1 2", "entry_of 0 1 2", "group_of 0 1 2"]
    assert subprocess.run([exe, "2", "1", "0", "2", "0", "2"], capture_output=True, text=True, check=True).stdout == "invalid\n"


# ---- the equation on the oracle -------------------------------------------------------------------------------------------------------
PINNED = [1, 1 << 63, (1 << 64) - 1, 2, 0x123456789abcdef1, 77, 3, 0xfedcba9876543211]


def _scalars(m):
    return [PINNED[j % len(PINNED)] + (j // len(PINNED)) for j in range(m)]


@pytest.fixture(scope="module")
def base():
    c = Corpus()
    return c, c.verdicts()


@pytest.mark.parametrize("bad", [(), (2,), (0, 7), (14,)])
def test_the_equation_from_the_oracle_alone(base, bad):
    """FE(miller_loop over (sum r P per group, Q_g)) is one exactly when every item's FE(miller_loop(item)) is one, and equals
    prod_j (item value j)^(r_j)"""
    c0, v0 = base
    assert all(v0), "every item of the base corpus holds"
    c = Corpus(bad) if bad else c0
    values = [c.item_value(j) if j in bad else (ONE if v0[j] else None) for j in range(len(c.items))]
    assert all(v is not None for v in values)
    verdicts = [int(np.array_equal(v, ONE)) for v in values]
    assert verdicts == [0 if j in bad else 1 for j in range(len(c.items))]
    r = _scalars(len(c.items))
    got = c.combined_value(r)
    assert np.array_equal(got, ONE) == all(verdicts)
    want = ONE
    for j in bad:                                                                # (the items that hold contribute 1^r = 1)
        want = RC.fq12_mul(want, RC.fq12_exp_u64(values[j], r[j]))
    assert np.array_equal(np.asarray(got, dtype=np.uint64), np.asarray(want, dtype=np.uint64))


def test_the_cancelling_pair_on_the_oracle():
    """two failing items with values v and 1 / v: equal scalars let them through, scalars (5, 6) do not"""
    p = g1(99)
    c = Corpus(items=[])
    c.items = [[(p, QA, 0)], [(neg1(p), QA, 0)]]
    assert c.tab == table()
    v, w = c.item_value(0), c.item_value(1)
    assert not np.array_equal(v, ONE) and not np.array_equal(w, ONE) and np.array_equal(RC.fq12_mul(v, w), ONE)
    assert np.array_equal(c.combined_value([5, 5]), ONE)
    assert not np.array_equal(c.combined_value([5, 6]), ONE)
    assert np.array_equal(c.combined_value([5, 6]), RC.fq12_mul(RC.fq12_exp_u64(v, 5), RC.fq12_exp_u64(w, 6)))
