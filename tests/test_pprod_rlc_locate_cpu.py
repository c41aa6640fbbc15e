"""CPU side of the randomised pairing-product batches that find the bad items by blocks (blsmi 0.18:
blsmi_pairing_product_batch_rlc_locate[_jac|_dev|_jac_dev]): the declarations against the exports and the Python wrappers' argument types,
the argument checks that come before any device work (0.17's, on the new names, with `rechecked` written as 0), the host plan
(bls_amd/csrc/pprod_locate_plan.h) run natively under the address and undefined-behaviour sanitizers, and the block equations composed
from the oracle's primitives on the corpus of tests/pprod_rlc_corpus.py -- what tests/test_gpu_pprod_rlc_locate.py expects of the device."""
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
from pprod_rlc_corpus import ONE, Corpus
from pprod_rlc_locate_common import BAD2, block_value, blocks_of, fq12_prod, is_one, rechecked_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -3
FOUR = ["blsmi_pairing_product_batch_rlc_locate", "blsmi_pairing_product_batch_rlc_locate_jac", "blsmi_pairing_product_batch_rlc_locate_dev",
        "blsmi_pairing_product_batch_rlc_locate_jac_dev"]


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def test_declared_exported_and_typed(lib, tmp_path):
    declared = _native.declared_symbols()
    header = open(_native.HEADER).read()
    assert "0.18 adds" in header and "0.17 adds" in header
    assert "pairing products, randomised, that find the bad items by blocks (blsmi 0.18)" in header
    exported = set(re.findall(r" T (blsmi_\w+)", subprocess.run(["nm", "-D", _native.SO_PATH], capture_output=True, text=True, check=True).stdout))
    assert exported == set(declared)                                             # nm -D exports equal the header's names
    for s in FOUR:
        assert s in declared and s in exported and hasattr(lib, s), s
        want = [CTYPES[t] for t in _header_params(header, s)]
        assert bound_argtypes(s) == want, s
        twin = _header_params(header, s.replace("_locate", ""))                  # the 0.17 twin's arguments, `block` after scalars, `rechecked` after combined
        at = len(twin) - 1 - twin[::-1].index("const uint64_t *")              # scalars: the last u64 pointer
        grown = twin[:at + 1] + ["size_t"] + twin[at + 1:]
        grown.insert(grown.index("int *") + 1, "size_t *")
        assert _header_params(header, s) == grown, s
    for w in ("pairing_product_batch_rlc_locate", "pairing_product_batch_rlc_locate_jac", "pairing_product_batch_rlc_locate_dev", "pairing_product_batch_rlc_locate_jac_dev"):
        assert callable(getattr(engine, w)), w
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index("pairing products, randomised, that find the bad items by blocks (blsmi 0.18)"):])
    for phrase in ("B = ceil(m / block)", "block = 0 is automatic, max(64, ceil(m / 256))", "any value >= 1 is legal", "block >= m gives one block",
                   "and only those", "*rechecked is the number of those items", "*rechecked = 0", "no second ladder, no second Miller loop",
                   "at most 2^-64", "its weights are its own items'", "in one block or in two", "prime-order subgroups",
                   "an infinite P_k adds nothing to its cell", "an all-zero entry drops its cells", "contributes 1", "none of these sends anything to the per-item path",
                   "has value one", "BLSMI_E_ARG", "No `block` value is refused", "buffers stay untouched", "one device", "request combiner",
                   "\"rlc_min\" does NOT apply", "When to call it"):
        assert phrase in block, phrase
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "t.c"
    src.write_text('#include "blsmi.h"\nint main(void) { return blsmi_pairing_product_batch_rlc_locate(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_pairing_product_batch_rlc_locate_jac(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_pairing_product_batch_rlc_locate_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_pairing_product_batch_rlc_locate_jac_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
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

        def call(q=(0, 1, 1, 0), nq=2, np_=4, seg=(0, 2, 4), scalars=None, m=2, g1p=pts, tab=pts, null_seg=False, want_one=True, block=0, want_nre=True):
            qi = (C.c_uint32 * max(1, len(q)))(*q) if q is not None else None
            so = (C.c_uint64 * len(seg))(*seg)
            sc = (C.c_uint64 * len(scalars))(*scalars) if scalars else None
            one = (C.c_uint8 * 8)(*([7] * 8))
            comb, nre = C.c_int(7), C.c_size_t(7)
            head = (g1p, tab) if jac else (g1p, None, tab)
            rc = fn(*head, nq, qi, np_, None if null_seg else so, m, sc, block, one if want_one else None, C.byref(comb), C.byref(nre) if want_nre else None)
            return rc, comb.value, nre.value if want_nre else 0, list(one)[:m]
        for block in (0, 1, 1 << 40):                                             # no block value is refused, none lets a bad argument through
            assert call(seg=(1, 2, 4), block=block)[:3] == (E_ARG, 0, 0), (name, "offsets that do not start at 0")
            assert call(seg=(0, 3, 2), block=block)[:3] == (E_ARG, 0, 0), (name, "offsets that decrease")
            assert call(seg=(0, 2, 3), block=block)[:3] == (E_ARG, 0, 0), (name, "offsets that do not end at np")
            assert call(q=(0, 1, 2, 0), block=block)[:3] == (E_ARG, 0, 0), (name, "q_idx >= nq")
            assert call(q=(0, 0, 0, 0), nq=0, block=block)[:3] == (E_ARG, 0, 0), (name, "nq = 0 with pairs")
            assert call(q=None, nq=3, block=block)[:3] == (E_ARG, 0, 0), (name, "q_idx NULL with nq != np")
            assert call(scalars=[5, 0], block=block)[:3] == (E_ARG, 0, 0), (name, "a zero scalar")
            assert call(g1p=None, block=block)[:3] == (E_ARG, 0, 0), (name, "g1 NULL")
            assert call(tab=None, block=block)[:3] == (E_ARG, 0, 0), (name, "table NULL")
            assert call(null_seg=True, block=block)[:3] == (E_ARG, 0, 0), (name, "seg_off NULL")
            assert call(want_one=False, block=block)[:3] == (E_ARG, 0, 0), (name, "is_one NULL")
            assert call(q=(), seg=(0,), np_=0, m=0, block=block) == (0, 0, 0, []), (name, "m = 0")
            assert call(q=None, nq=0, seg=(0,), np_=0, m=0, g1p=None, tab=None, null_seg=True, want_one=False, block=block)[:3] == (0, 0, 0), (name, "m = 0, nothing else")
            assert call(q=(), nq=2, seg=(0, 0, 0, 0), np_=0, m=3, g1p=None, tab=None, block=block) == (0, 1, 0, [1, 1, 1]), (name, "np = 0 with m = 3: ones, on the host")
            assert call(q=(), nq=2, seg=(0, 0, 0, 0), np_=0, m=3, g1p=None, tab=None, block=block, want_nre=False)[:2] == (0, 1), (name, "rechecked may be NULL")
    a = C.addressof(buf)
    for name in FOUR[2:]:                                                         # what the _dev forms can refuse without a device
        fn = engine._fn(name)
        head = (a, a) if name.endswith("_jac_dev") else (a, None, a)
        for block in (0, 1, 1 << 40):
            def call(*mid):
                comb, nre = C.c_int(7), C.c_size_t(7)
                args = list(mid)
                rc = fn(*args[:-1], C.byref(comb), C.byref(nre), args[-1])
                return rc, comb.value, nre.value
            assert call(*head, 2, a, 4, a, 2, (C.c_uint64 * 2)(3, 0), block, a, None) == (E_ARG, 0, 0), (name, "a zero scalar")
            assert call(*head, 3, None, 4, a, 2, None, block, a, None) == (E_ARG, 0, 0), (name, "d_q_idx NULL with nq != np")
            assert call(*head, 2, a, 4, a, 2, None, block, None, None) == (E_ARG, 0, 0), (name, "d_is_one NULL")
            assert call(*head, 2, a, 4, None, 2, None, block, a, None) == (E_ARG, 0, 0), (name, "d_seg_off NULL")
            assert call(*((None,) * len(head)), 0, None, 0, None, 0, None, block, None, None) == (0, 0, 0), (name, "m = 0")


def test_python_wrappers_validate():
    f = engine.pairing_product_batch_rlc_locate
    with pytest.raises(ValueError):
        f(bytes(96 * 2), bytes(192 * 3), None, [0, 2])                            # no q_idx: one entry per pair
    with pytest.raises(ValueError):
        f(bytes(96 * 2), bytes(192), [0], [0, 2])                                 # one index per pair
    with pytest.raises(ValueError):
        f(bytes(96 * 2), bytes(192), [0, 0], [0, 1])                              # offsets end at np
    with pytest.raises(ValueError):
        f(bytes(96 * 2), bytes(192), [0, 0], [0, 2], scalars=[1, 2])              # one scalar per item
    with pytest.raises(ValueError):
        engine.pairing_product_batch_rlc_locate_jac(bytes(96 * 2), bytes(288), [0, 0], [0, 2])   # in-memory records are 144 bytes
    with pytest.raises(ValueError):
        f(b"", bytes(192), [], [0, 0, 0], block=-1)                               # block is a size
    with pytest.raises(engine.BlsmiError) as ei:
        f(bytes(96 * 2), bytes(192), [0, 1], [0, 2])                              # index >= nq: the library refuses
    assert "(-3)" in str(ei.value)
    for block in (0, 1, 1 << 40):
        one, comb, nre = f(b"", bytes(192), [], [0, 0, 0], block=block)
        assert one.tolist() == [1, 1] and comb == 1 and nre == 0
        one, comb, nre = f(b"", b"", None, [0], block=block)
        assert one.shape == (0,) and comb == 0 and nre == 0


def test_plan_under_sanitizers(tmp_path):
    gpp = shutil.which("g++") or shutil.which("c++")
    assert gpp, "no C++ compiler"
    exe = str(tmp_path / "pprod_locate_plan")
    subprocess.check_call([gpp, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "pprod_locate_plan.cc")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.fullmatch(r"PPROD_LOCATE_PLAN ok \d+\n", out.stdout), (out.stdout, out.stderr)
    # one plan read line by line (the table of tests/test_pprod_rlc_cpu.py's, items of 0, 3, 0, 5, 0 pairs, blocks of 2 items): block 0 has
    # entry 8 twice (a multi-pair cell) and entry 2 once; block 1 has entry 5 three times, entries 0 and 7 once; block 2 has no pairs
    args = ["9", "5", "0", "0", "3", "3", "8", "8", "8", "2", "8", "5", "0", "5", "5", "7"]
    out = subprocess.run([exe, "2"] + args, capture_output=True, text=True, check=True).stdout.splitlines()
    assert out == ["perm 0 2 3 5 6", "cell_off 0 2 5", "single 1 4 7", "entry_of 5 8 0 2 7", "sum_of 0 2 1 3 4", "entry_at 1 3 0 2 4", "slot_off 0 2 5 5"]
    # block >= m: 0.17's grouping (perm 3 5 6 0 2, single 4 1 7), the slots in 0.17's order
    out = subprocess.run([exe, "5"] + args, capture_output=True, text=True, check=True).stdout.splitlines()
    assert out == ["perm 3 5 6 0 2", "cell_off 0 3 5", "single 4 1 7", "entry_of 5 8 0 2 7", "sum_of 0 1 2 3 4", "entry_at 0 1 2 3 4", "slot_off 0 5"]
    # block 1: entry 5 in item 3 only, still one multi-pair cell; five blocks
    out = subprocess.run([exe, "1"] + args, capture_output=True, text=True, check=True).stdout.splitlines()
    assert out == ["perm 0 2 3 5 6", "cell_off 0 2 5", "single 1 4 7", "entry_of 5 8 0 2 7", "sum_of 0 2 1 3 4", "entry_at 1 3 0 2 4", "slot_off 0 0 2 2 5 5"]
    out = subprocess.run([exe, "2", "3", "2", "0", "1", "3"], capture_output=True, text=True, check=True).stdout.splitlines()      # q_idx NULL
    assert out == ["perm", "cell_off 0", "single 0 1 2", "entry_of 0 1 2", "sum_of 0 1 2", "entry_at 0 1 2", "slot_off 0 3"]
    assert subprocess.run([exe, "4", "2", "1", "0", "2", "0", "2"], capture_output=True, text=True, check=True).stdout == "invalid\n"


# ---- the block equations on the oracle ----------------------------------------------------------------------------------------------------
PINNED = [1, 1 << 63, (1 << 64) - 1, 2, 0x123456789abcdef1, 77, 3, 0xfedcba9876543211]


def _scalars(m):
    return [PINNED[j % len(PINNED)] + (j // len(PINNED)) for j in range(m)]


@pytest.fixture(scope="module")
def base():
    c0 = Corpus()
    v0 = c0.verdicts()
    assert all(v0), "every item of the base corpus holds"
    c = Corpus(BAD2)
    values = [c.item_value(j) if j in BAD2 else ONE for j in range(len(c.items))]
    assert [int(is_one(v)) for v in values] == [0 if j in BAD2 else 1 for j in range(len(c.items))]
    return c, values


@pytest.mark.parametrize("block", [1, 8, 33])
def test_the_block_equations_from_the_oracle_alone(base, block):
    """FE of each block's product over its cells' (S_c, Q) is prod_{j in b} (item value j)^(r_j): one exactly when every item of the block
    holds; the product of the block values is 0.17's combined value"""
    c, values = base
    m = len(c.items)
    r = _scalars(m)
    got = []
    for lo, hi in blocks_of(m, block):
        v = block_value(c, r, lo, hi)
        want = fq12_prod(RC.fq12_exp_u64(values[j], r[j]) for j in range(lo, hi) if j in BAD2)   # (the items that hold contribute 1^r = 1)
        assert np.array_equal(np.asarray(v, dtype=np.uint64), np.asarray(want, dtype=np.uint64)), (block, lo)
        assert is_one(v) == (not any(lo <= j < hi for j in BAD2)), (block, lo)
        got.append(v)
    assert len(got) == -(-m // block)
    assert np.array_equal(np.asarray(fq12_prod(got), dtype=np.uint64), np.asarray(c.combined_value(r), dtype=np.uint64))
    assert rechecked_of(m, block, BAD2) == {1: 2, 8: 16, 33: 33}[block]
