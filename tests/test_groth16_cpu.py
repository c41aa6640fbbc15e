"""CPU side of the scalar-field fold and the Groth16 batches (blsmi 0.19: blsmi_fr_wsum_segmented_u64[_dev],
blsmi_groth16_verify_batch[_jac|_dev|_jac_dev]): the declarations against the exports and the Python wrappers' argument types, the argument
checks that come before any device work, the wrappers' own checks, the corpus of tests/groth16_cases.py by the oracle alone, the folded
block equation composed from the oracle's primitives and big integers, and the arithmetic of bls_amd/csrc/fr_fold.h run natively under the
address and undefined-behaviour sanitizers against Python integers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bls_amd import _native, engine
from cabi_common import CTYPES, _header_params, bound_argtypes
from groth16_cases import BAD_INPUT, BAD_TWO, EDGE_INPUTS, M, R, Groth16Case, edges_for, is_one
from oracle import pyref as P
from oracle import refcpu as RC
from pprod_rlc_locate_common import blocks_of, fq12_prod, rechecked_of
from test_pprod_rlc_locate_cpu import PINNED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -3
FOLD = ["blsmi_fr_wsum_segmented_u64", "blsmi_fr_wsum_segmented_u64_dev"]
FOUR = ["blsmi_groth16_verify_batch", "blsmi_groth16_verify_batch_jac", "blsmi_groth16_verify_batch_dev", "blsmi_groth16_verify_batch_jac_dev"]
HEADING = "scalar-field folds and Groth16 batches (blsmi 0.19)"


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def test_declared_exported_and_typed(lib, tmp_path):
    declared = _native.declared_symbols()
    header = open(_native.HEADER).read()
    assert "0.19 adds" in header and "0.18 adds" in header
    assert header.index(HEADING) > header.index("pairing products, randomised, that find the bad items by blocks (blsmi 0.18)")   # the new section is the last
    exported = set(re.findall(r" T (blsmi_\w+)", subprocess.run(["nm", "-D", _native.SO_PATH], capture_output=True, text=True, check=True).stdout))
    assert exported == set(declared)                                             # nm -D exports equal the header's names
    for s in FOLD + FOUR:
        assert s in declared and s in exported and hasattr(lib, s), s
        assert bound_argtypes(s) == [CTYPES[t] for t in _header_params(header, s)], s
    twin = _header_params(header, "blsmi_pairing_product_batch_rlc_locate")     # scalars / block / ok / combined / rechecked as the 0.18 call has them
    assert _header_params(header, FOUR[0])[-5:] == twin[-5:]
    for w in ("fr_wsum_segmented_u64", "fr_wsum_segmented_u64_dev", "groth16_verify_batch", "groth16_verify_batch_jac", "groth16_verify_batch_dev", "groth16_verify_batch_jac_dev"):
        assert callable(getattr(engine, w)), w
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index(HEADING):])
    for phrase in ("ANY 256-bit value is taken mod r", "an empty segment gives zeros", "a zero weight is allowed", "fully reduced (< r)", "not one per row",
                   "alpha, IC_0 .. IC_nin", "beta, gamma, delta", "(A_j, B_j), (-alpha, beta), (-L_j, gamma), (-C_j, delta)", "the pair contributes 1",
                   "an all-zero vk_g2 entry drops its pairs", "no L_j exists", "no item pays a full-width ladder", "and only those", "only for IC_i of order r",
                   "prime-order subgroups", "at most 2^-64", "caller scalars carry 0.17's caveat", "BLSMI_E_ARG", "*rechecked = 0 on every early return",
                   "buffers stay untouched", "one device", "request combiner", "\"rlc_min\" does NOT apply"):
        assert phrase in block, phrase
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "t.c"
    src.write_text('#include "blsmi.h"\nint main(void) { return blsmi_fr_wsum_segmented_u64(0, 0, 0, 0, 0, 0) + blsmi_fr_wsum_segmented_u64_dev(0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_groth16_verify_batch(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + blsmi_groth16_verify_batch_jac(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_groth16_verify_batch_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + blsmi_groth16_verify_batch_jac_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(_native.HEADER), str(src)])


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
        inp = a if dev else C.cast(buf, u8p)

        def call(vk1=pts, vk2=pts, nin=2, pg1=pts, pg2=pts, inputs=inp, m=2, scalars=None, block=0, ok=inp, want_nre=True):
            sc = (C.c_uint64 * len(scalars))(*scalars) if scalars else None
            comb, nre = C.c_int(7), C.c_size_t(7)
            tail = (None,) if dev else ()
            rc = fn(vk1, vk2, nin, pg1, pg2, inputs, m, sc, block, ok, C.byref(comb), C.byref(nre) if want_nre else None, *tail)
            return rc, comb.value, nre.value if want_nre else 0
        for block in (0, 1, 1 << 40):
            assert call(vk1=None, block=block) == (E_ARG, 0, 0), (name, "vk_g1 NULL")
            assert call(vk2=None, block=block) == (E_ARG, 0, 0), (name, "vk_g2 NULL")
            assert call(pg1=None, block=block) == (E_ARG, 0, 0), (name, "proof_g1 NULL")
            assert call(pg2=None, block=block) == (E_ARG, 0, 0), (name, "proof_g2 NULL")
            assert call(inputs=None, block=block) == (E_ARG, 0, 0), (name, "inputs NULL with m * nin > 0")
            assert call(ok=None, block=block) == (E_ARG, 0, 0), (name, "ok NULL")
            assert call(scalars=[5, 0], block=block) == (E_ARG, 0, 0), (name, "a zero scalar")
            assert call(m=1 << 32, block=block) == (E_ARG, 0, 0), (name, "m beyond 2^32 - 1")
            assert call(m=0, block=block) == (0, 0, 0), (name, "m = 0")
            assert call(vk1=None, vk2=None, pg1=None, pg2=None, inputs=None, ok=None, m=0, block=block) == (0, 0, 0), (name, "m = 0, nothing else")
            assert call(ok=None, block=block, want_nre=False)[:2] == (E_ARG, 0), (name, "rechecked may be NULL")
    fold = engine._fn(FOLD[0])
    vals, w, out = C.cast(buf, u8p), C.cast(w64, u64p), C.cast(buf, u8p)
    off = lambda *o: (C.c_uint64 * len(o))(*o)                                    # noqa: E731
    assert fold(vals, 2, w, None, 1, out) == E_ARG                               # seg_off NULL
    assert fold(vals, 2, w, off(0, 3), 1, None) == E_ARG                         # out NULL
    assert fold(vals, 2, w, off(1, 3), 1, out) == E_ARG                          # offsets that do not start at 0
    assert fold(vals, 2, w, off(0, 3, 2), 2, out) == E_ARG                       # offsets that decrease
    assert fold(vals, 2, None, off(0, 3), 1, out) == E_ARG                       # weights NULL with rows
    assert fold(None, 2, w, off(0, 3), 1, out) == E_ARG                          # vals NULL with rows and columns
    assert fold(vals, 1, w, off(0, 1 << 32), 1, out) == E_ARG                    # more rows than the accumulator is sized for
    assert fold(None, 0, None, None, 0, None) == 0                               # nseg = 0
    fold_dev = engine._fn(FOLD[1])
    assert fold_dev(a, 2, a, None, 1, a, None) == E_ARG and fold_dev(a, 2, a, a, 1, None, None) == E_ARG and fold_dev(None, 0, None, None, 0, None, None) == 0


def test_python_wrappers_validate():
    f = engine.groth16_verify_batch
    vk1, vk2 = bytes(96 * 4), bytes(192 * 3)
    with pytest.raises(ValueError):
        f(bytes(96 * 3), vk2, bytes(96 * 2), bytes(192), bytes(64), 2)           # the key has nin + 2 G1 records
    with pytest.raises(ValueError):
        f(vk1, bytes(192 * 2), bytes(96 * 2), bytes(192), bytes(64), 2)          # ... and three G2 records
    with pytest.raises(ValueError):
        f(vk1, vk2, bytes(96 * 3), bytes(192), bytes(64), 2)                     # two G1 records per proof
    with pytest.raises(ValueError):
        f(vk1, vk2, bytes(96 * 2), bytes(192), bytes(32), 2)                     # nin scalars per proof
    with pytest.raises(ValueError):
        f(vk1, vk2, bytes(96 * 2), bytes(192), bytes(64), 2, scalars=[1, 2])     # one scalar per proof
    with pytest.raises(ValueError):
        f(vk1, vk2, bytes(96 * 2), bytes(192), bytes(64), 2, block=-1)           # block is a size
    with pytest.raises(ValueError):
        engine.groth16_verify_batch_jac(vk1, vk2, bytes(144 * 2), bytes(288), bytes(64), 2)   # in-memory records are 144 / 288 bytes
    with pytest.raises(engine.BlsmiError) as ei:
        f(vk1, vk2, bytes(96 * 2), bytes(192), bytes(64), 2, scalars=[0])        # a zero scalar: the library refuses
    assert "(-3)" in str(ei.value)
    ok, comb, nre = f(vk1, vk2, b"", b"", b"", 2)
    assert ok.shape == (0,) and comb == 0 and nre == 0
    ok, comb, nre = f(bytes(96 * 2), vk2, b"", b"", None, 0)
    assert ok.shape == (0,) and comb == 0 and nre == 0
    g = engine.fr_wsum_segmented_u64
    with pytest.raises(ValueError):
        g(bytes(32 * 3), 2, [1, 2], [0, 2])                                      # n * ncol scalars
    with pytest.raises(ValueError):
        g(bytes(32 * 4), 2, [1], [0, 2])                                         # one weight per row
    with pytest.raises(ValueError):
        g(bytes(32 * 4), 2, [1, 2], [1, 2])                                      # offsets from 0
    with pytest.raises(ValueError):
        g(bytes(32 * 4), 2, [1, 2], [0, 2, 1])                                   # ... that do not decrease
    with pytest.raises(ValueError):
        g(b"", -1, [], [0])
    assert g(b"", 3, [], [0]).shape == (0, 4, 32)


# ---- the corpus and the folded block equation on the oracle ---------------------------------------------------------------------------
def _scalars(m):
    return [PINNED[j % len(PINNED)] + (j // len(PINNED)) for j in range(m)]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for nin in (3, 1, 0):
        out[nin, "valid"] = Groth16Case(M, nin, 19)
        out[nin, "edges"] = Groth16Case(M, nin, 19, **edges_for(nin))
    out[3, "input"] = Groth16Case(M, 3, 19, spoil=BAD_INPUT)
    out[1, "input"] = Groth16Case(M, 1, 19, spoil=BAD_INPUT)
    out[3, "two"] = Groth16Case(M, 3, 19, spoil=BAD_TWO)
    out[3, "B"] = Groth16Case(M, 3, 19, spoil={30: "B"})
    return out


def test_the_corpus_is_right_by_the_oracle_alone(cases):
    for (nin, kind), c in cases.items():
        bad = {"input": BAD_INPUT, "two": BAD_TWO, "B": {30: "B"}}.get(kind, {})
        assert c.verdicts() == [0 if j in bad else 1 for j in range(M)], (nin, kind)
    e = cases[3, "edges"]
    assert e.A[3] == bytes(96) and e.C[11] == bytes(96) and e.C[3] != bytes(96)
    assert [e.inputs[0], e.inputs[1][:2]] == [[0, R - 1, R], [2 ** 256 - 1, R]] and set(EDGE_INPUTS) <= {v for x in e.inputs[:3] for v in x}
    assert cases[0, "valid"].input_bytes == b"" and len(cases[0, "valid"].vk_g1) == 2 * 96


@pytest.mark.parametrize("block", [1, 8, 33])
def test_the_folded_block_equation_from_the_oracle_alone(cases, block):
    """FE of a block's cells -- the gamma cell from the big-integer t_b and s_bi, no L_j anywhere -- is prod_{j in b} (item value j)^(r_j):
    one exactly when every item of the block holds.  The spoiled public input moves the block's value: only the fold sees it."""
    r = _scalars(M)
    for key, bad in (((3, "two"), BAD_TWO), ((3, "input"), BAD_INPUT), ((3, "edges"), {}), ((0, "valid"), {})):
        c = cases[key]
        values = {j: c.item_value(j) for j in bad}
        for lo, hi in blocks_of(M, block):
            v = c.block_value(r, lo, hi)
            want = fq12_prod(RC.fq12_exp_u64(values[j], r[j]) for j in range(lo, hi) if j in bad)   # (the items that hold contribute 1^r = 1)
            assert np.array_equal(np.asarray(v, dtype=np.uint64), np.asarray(want, dtype=np.uint64)), (key, block, lo)
            assert is_one(v) == (not any(lo <= j < hi for j in bad)), (key, block, lo)
    assert rechecked_of(M, block, BAD_TWO) == {1: 2, 8: 16, 33: 33}[block]


# ---- the plan's appended cells, natively ------------------------------------------------------------------------------------------------
def test_appended_cells_under_sanitizers(tmp_path):
    gpp = shutil.which("g++") or shutil.which("c++")
    assert gpp, "no C++ compiler"
    exe = str(tmp_path / "pprod_locate_append")
    subprocess.check_call([gpp, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "pprod_locate_append.cc")])
    # three proofs, blocks of two: block 0 has its delta cell (two pairs: sum 0) and the cells of B_0, B_1; block 1 a one-pair delta cell and
    # B_2; behind each block's own cells its alpha cell (sums 5, 6 against entry 4) and its gamma cell (sums 7, 8 against entry 5)
    out = subprocess.run([exe, "3", "2"], capture_output=True, text=True, check=True).stdout.splitlines()
    assert out == ["sum_of 0 1 2 5 7 3 4 6 8", "entry_at 0 1 2 4 5 0 3 4 5", "slot_off 0 5 9"]
    for m, block in ((37, 8), (37, 1), (37, 64), (1, 1), (64, 64), (65, 64)):     # the invariants, checked by the program itself
        out = subprocess.run([exe, str(m), str(block)], capture_output=True, text=True)
        assert out.returncode == 0, (m, block, out.stderr)
        B = -(-m // block)
        assert out.stdout.splitlines()[2].split()[-1] == str(m + 3 * B), (m, block)   # m cells of B_j; per block a delta, an alpha and a gamma cell


# ---- fr_fold.h, natively ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fr_fold(tmp_path_factory):
    gpp = shutil.which("g++") or shutil.which("c++")
    assert gpp, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("fr_fold") / "fr_fold")
    subprocess.check_call([gpp, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "fr_fold.cc")])
    return exe


def _fold_native(exe, rows, weights, ncol, parts):
    text = "%d %d\n" % (ncol, len(rows)) + "".join("%d %s\n" % (w, " ".join("%064x" % v for v in row)) for row, w in zip(rows, weights))
    out = subprocess.run([exe, str(parts)], input=text, capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    return [int(line, 16) for line in out.stdout.split()]


def _fold_python(rows, weights, ncol):
    return [sum(weights) % R] + [sum(w * row[i] for row, w in zip(rows, weights)) % R for i in range(ncol)]


def test_fr_fold_under_sanitizers(fr_fold):
    top = (1 << 64) - 1
    xs = P.XORShift(1919)
    random_rows = [[P.rand_int(xs, 1 << 256) for _ in range(3)] for _ in range(1000)]
    random_w = [P.rand_int(xs, 1 << 64) for _ in range(1000)]
    batches = [
        ("all r - 1", [[R - 1] * 2] * 300, [top] * 300, 2),                      # the longest carries
        ("all 2^256 - 1", [[2 ** 256 - 1] * 2] * 300, [top] * 300, 2),
        ("zeros", [[0, 0]] * 5, [top, 0, 1, 0, 7], 2),
        ("zero weights", [[R - 1, 5]] * 4, [0] * 4, 2),
        ("one row", [[R, 2 ** 256 - 1, 1, R + 1]], [top], 4),
        ("no column", [[]] * 9, [top] * 9, 0),
        ("no row", [], [], 3),
        ("random", random_rows, random_w, 3),
    ]
    for what, rows, weights, ncol in batches:
        want = _fold_python(rows, weights, ncol)
        assert all(v < R for v in want)
        for parts in (1, 2, 7, 64, 257):
            assert _fold_native(fr_fold, rows, weights, ncol, parts) == want, (what, parts)
