"""CPU side of the grouped randomised batch verification that finds the bad tuples by cells (blsmi 0.13:
blsmi_g?pubs_*verify*_batch_rlc_grouped_locate[_jac]): the declarations against the exports and the Python wrappers' argument types, the
argument checks that come before any device work, the cell plan (bls_amd/csrc/cell_plan.h) run natively as a stand-alone program under the
address and undefined-behaviour sanitizers and against a pure-Python mirror of the cut, and one cell equation composed from the oracle's
primitives -- what tests/test_gpu_rlc_grouped_locate.py expects of the device."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bls_amd import _native, engine, g1pubs, g2pubs
from cabi_common import CTYPES, _header_params, bound_argtypes
from oracle import refcpu as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -3
SYMS = ["blsmi_g2pubs_verify_batch_rlc_grouped_locate", "blsmi_g1pubs_verify_batch_rlc_grouped_locate", "blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_locate",
        "blsmi_g2pubs_verify_batch_rlc_grouped_locate_jac", "blsmi_g1pubs_verify_batch_rlc_grouped_locate_jac",
        "blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_locate_jac"]


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def test_declared_exported_and_typed(lib, tmp_path):
    declared = _native.declared_symbols()
    header = open(_native.HEADER).read()
    assert "0.13 adds" in header and "0.12 adds" in header
    exported = set(re.findall(r" T (blsmi_\w+)", subprocess.run(["nm", "-D", _native.SO_PATH], capture_output=True, text=True, check=True).stdout))
    for s in SYMS:
        assert s in declared and s in exported and hasattr(lib, s), s
        want = [CTYPES[t] for t in _header_params(header, s)]
        assert bound_argtypes(s) == want, s
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index("finds the bad tuples by cells (blsmi 0.13)"):])
    for phrase in ("\"rlc_min\" does NOT apply", "one device", "request combiner", "BLSMI_E_ARG", "2^-64", "rechecked", "OF ONE CELL", "no evenness rule",
                   "n > 2^32 - 1", "locates by message"):
        assert phrase in block, phrase
    assert engine._fn("blsmi_version")().startswith(b"blsmi 0.")                           # the pinned literal stays
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "t.c"
    src.write_text('#include "blsmi.h"\nint main(void) { return blsmi_g2pubs_verify_batch_rlc_grouped_locate(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_g1pubs_verify_batch_rlc_grouped_locate(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_locate_jac(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(_native.HEADER), str(src)])


def test_argument_checks_come_before_any_device_work(lib):
    """this machine has no device: anything but BLSMI_E_ARG / BLSMI_OK here would be the sign of device work"""
    z = C.c_size_t
    buf = (C.c_uint8 * 1024)()
    w64 = (C.c_uint64 * 128)()
    off = (C.c_uint64 * 3)(0, 4, 8)
    dom = (C.c_uint8 * 8)()
    u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    for name in SYMS:
        fn = engine._fn(name)
        a8, a64 = C.cast(buf, u8p), C.cast(w64, u64p)
        head = (a8, C.cast(dom, u8p)) if "with_domain" in name else (a8, C.cast(off, u64p))
        pts = (a64, a64) if name.endswith("_jac") else (a8, a8, None)

        def call(idx, d, n, block=4, scalars=None, head=head, pts=pts, null_idx=False):
            ix = (C.c_uint32 * max(1, len(idx)))(*idx)
            sc = (C.c_uint64 * len(scalars))(*scalars) if scalars else None
            comb, re_ = C.c_int(7), C.c_size_t(7)
            rc = fn(*head, z(d), None if null_idx else ix, *pts, sc, block, None, None, z(n), C.byref(comb), C.byref(re_))
            return rc, comb.value, re_.value
        assert call([0, 2], 2, 2) == (E_ARG, 0, 0), (name, "index >= d")
        assert call([0, 0], 0, 2) == (E_ARG, 0, 0), (name, "d = 0 with n > 0")
        for block in (0, 1, 3, 1024):
            assert call([0, 1], 2, 2, block=block, scalars=[5, 0]) == (E_ARG, 0, 0), (name, "a zero scalar", block)
        assert call([0, 1], 2, 2, null_idx=True) == (E_ARG, 0, 0), (name, "msg_idx NULL")
        assert call([0, 1], 2, 2, head=(None, head[1])) == (E_ARG, 0, 0), (name, "msgs NULL")
        assert call([0, 1], 2, 2, head=(head[0], None)) == (E_ARG, 0, 0), (name, "offsets / domain NULL")
        assert call([0, 1], 2, 2, pts=(None,) + tuple(pts[1:])) == (E_ARG, 0, 0), (name, "pks NULL")
        assert call([0, 1], 2, 2, pts=(pts[0], None) + tuple(pts[2:])) == (E_ARG, 0, 0), (name, "sigs NULL")
        assert call([0], 1, 1 << 32) == (E_ARG, 0, 0), (name, "n = 2^32")      # (refused before msg_idx is read)
        for block in (0, 1, 3, 8, 1024):                                         # odd blocks and block = 1 are values like any other
            assert call([], 2, 0, block=block) == (0, 0, 0), (name, "n = 0", block)
        assert call([], 0, 0, null_idx=True) == (0, 0, 0), (name, "n = 0, nothing else")
        assert fn(*head, z(2), (C.c_uint32 * 2)(0, 2), *pts, None, 4, None, None, z(2), None, None) == E_ARG, (name, "combined and rechecked NULL")


def test_python_wrappers_validate():
    with pytest.raises(ValueError):
        engine.g1pubs_verify_batch_rlc_grouped_locate([b"m"], [0, 0], bytes(96), bytes(192 * 2))     # one key per tuple
    with pytest.raises(ValueError):
        engine.g2pubs_verify_batch_rlc_grouped_locate([b"m"], [0, 0], bytes(192 * 2), bytes(96 * 2), scalars=[1])
    with pytest.raises(ValueError):
        engine.g2pubs_verify_batch_rlc_grouped_locate([b"m"], [0, 0], bytes(192 * 2), bytes(96 * 2), inf_flags=[0])
    with pytest.raises(ValueError):
        engine.g1pubs_verify_batch_rlc_grouped_locate_jac([b"m"], [0], bytes(96), bytes(288))        # in-memory keys are 144 bytes
    with pytest.raises(ValueError):
        engine.g1pubs_verify_with_domain_batch_rlc_grouped_locate([bytes(32)], bytes(7), [0], bytes(96), bytes(192))
    with pytest.raises(ValueError):
        engine.g2pubs_verify_batch_rlc_grouped_locate([b"m"], [0, 0], bytes(192 * 2), bytes(96 * 2), block=-2)
    with pytest.raises(engine.BlsmiError):
        engine.g2pubs_verify_batch_rlc_grouped_locate([b"m"], [0, 1], bytes(192 * 2), bytes(96 * 2), block=3)   # index >= d: the library refuses
    with pytest.raises(engine.BlsmiError):
        engine.g1pubs_verify_batch_rlc_grouped_locate_jac([b"m"], [0, 0], bytes(144 * 2), bytes(288 * 2), scalars=[3, 0], block=1)
    for fn in (engine.g1pubs_verify_batch_rlc_grouped_locate, engine.g2pubs_verify_batch_rlc_grouped_locate, engine.g1pubs_verify_batch_rlc_grouped_locate_jac):
        ok, bm, comb, rechecked = fn([b"m"], [], b"", b"")
        assert ok.shape == (0,) and bm.shape == (0,) and comb == 0 and rechecked == 0
    ok, bm, comb, rechecked = engine.g1pubs_verify_with_domain_batch_rlc_grouped_locate([bytes(32)], bytes(8), [], b"", b"", block=7)
    assert ok.shape == (0,) and comb == 0 and rechecked == 0
    for mod in (g1pubs, g2pubs):
        assert mod.VerifyBatchRandomizedGroupedLocate([b"m"], [], [], []) == []
        with pytest.raises(ValueError):
            mod.VerifyBatchRandomizedGroupedLocate([b"m"], [0], [], [])
    assert g1pubs.VerifyWithDomainBatchRandomizedGroupedLocate([bytes(32)], [], [], [], bytes(8)) == []
    with pytest.raises(ValueError):
        g1pubs.VerifyWithDomainBatchRandomizedGroupedLocate([bytes(32)], [0], [], [], bytes(8))


# ---- the cell plan, natively ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    gpp = shutil.which("g++")
    assert gpp, "no g++"
    exe = str(tmp_path_factory.mktemp("cplan") / "cell_plan")
    subprocess.check_call([gpp, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "cell_plan.cc")])
    return exe


def test_cell_plan_native_cases(plan_exe):
    """empty and unreferenced table entries, a single-tuple group, block of 1, of exactly a group's size and above it, the failing-position
    lists with none / all / some cells failing, n = 0, 2^16 tuples: checked inside the program"""
    r = subprocess.run([plan_exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    m = re.fullmatch(r"CELL_PLAN ok (\d+)\n", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) >= 60


def cells_mirror(msg_idx, block):
    """the cut in pure Python: -> (perm, [(lo, hi, group)] over perm).  Tuples sorted by message (stable), every non-empty group cut into
    cells of at most `block` consecutive positions.  tests/test_gpu_rlc_grouped_locate.py uses it for the expected `rechecked`."""
    n = len(msg_idx)
    block = block or max(64, -(-n // 256)) + (max(64, -(-n // 256)) & 1)
    perm = sorted(range(n), key=lambda i: msg_idx[i])                            # (sorted is stable)
    cells, lo, g = [], 0, 0
    while lo < n:
        end = lo
        while end < n and msg_idx[perm[end]] == msg_idx[perm[lo]]:
            end += 1
        for a in range(lo, end, block):
            cells.append((a, min(end, a + block), g))
        lo, g = end, g + 1
    return perm, cells


def _plan(plan_exe, d, block, idx, fail):
    out = subprocess.run([plan_exe, str(d), str(block), str(len(idx))] + [str(x) for x in idx] + [str(x) for x in fail], capture_output=True, text=True, check=True).stdout
    if out == "invalid\n":
        return None
    return {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out.splitlines()}


def test_cell_plan_against_the_python_mirror(plan_exe):
    rnd = np.random.RandomState(11)
    for d, n, block in ((1, 5, 2), (4, 4, 1), (7, 40, 3), (50, 20, 4), (6, 71, 4), (3, 300, 0), (5, 200, 1024), (9, 90, 10)):
        idx = rnd.randint(0, d, size=n).tolist()
        perm, cells = cells_mirror(idx, block)
        for fail in ([0] * len(cells), [1] * len(cells), rnd.randint(0, 2, size=len(cells)).tolist()):
            got = _plan(plan_exe, d, block, idx, fail)
            assert got["perm"] == perm
            assert got["cell_off"] == [0] + [hi for _, hi, _ in cells]
            assert got["group_of"] == [g for _, _, g in cells]
            want = [(perm[k], g) for c, (lo, hi, g) in enumerate(cells) if fail[c] for k in range(lo, hi)]
            assert got["pos"] == [p for p, _ in want] and got["grp"] == [g for _, g in want]
    assert _plan(plan_exe, 3, 4, [0, 3, 1], []) is None                          # an index outside the table
    # the base shape of the GPU tests: sizes 1, 2, 9, 25, 33 cut by block = 4
    idx = [0] + [1] * 2 + [3] * 9 + [4] * 25 + [5] * 33
    assert [hi - lo for lo, hi, _ in cells_mirror(idx, 4)[1]] == [1, 2, 4, 4, 1] + [4] * 6 + [1] + [4] * 8 + [1]


# ---- one cell equation on the oracle -------------------------------------------------------------------------------------------------
def _fe(f):
    return RC.final_exponentiation(f)[1]


def cell_holds(kind, msg, pks, sigs, r, members):
    """e(S_c, G2gen) == e(H(m), K_c)  /  e(G1gen, S_c) == e(K_c, H(m)) for the tuples `members` of ONE message: 64-bit multiples, the two
    sums, one Miller loop a side, the final exponentiation"""
    k32 = {i: int(r[i]).to_bytes(32, "big") for i in members}
    m = len(members)
    if kind == "g2pubs":
        S = RC.g1_sum(b"".join(RC.g1_mul(sigs[i], k32[i]) for i in members), m)
        K = RC.g2_sum(b"".join(RC.g2_mul(pks[i], k32[i]) for i in members), m)
        lhs = _fe(RC.miller_loop(S, RC.g2_generator(), 1))
        rhs = _fe(RC.miller_loop(RC.hash_g1(msg), K, 1))
    else:
        S = RC.g2_sum(b"".join(RC.g2_mul(sigs[i], k32[i]) for i in members), m)
        K = RC.g1_sum(b"".join(RC.g1_mul(pks[i], k32[i]) for i in members), m)
        lhs = _fe(RC.miller_loop(RC.g1_generator(), S, 1))
        rhs = _fe(RC.miller_loop(K, RC.hash_g2(msg), 1))
    return bool(np.array_equal(lhs, rhs))


@pytest.mark.parametrize("kind", ("g1pubs", "g2pubs"))
def test_cell_equation_on_the_oracle(kind):
    """one cell of 3 tuples: valid; a tampered signature; the same-cell pair sig_a + D / sig_c - D, unnoticed exactly when r_a == r_c"""
    mod = RC.g1pubs if kind == "g1pubs" else RC.g2pubs
    msg = b"slot 17 head"
    sks = [hashlib.sha256(b"cell-sk-%d" % i).digest()[:31].rjust(32, b"\0") for i in range(3)]
    pks = [mod.priv_to_pub(sk) for sk in sks]
    sigs = [mod.sign(msg, sk) for sk in sks]
    r = [1 << 63, (1 << 64) - 1, 0x123456789abcdef1]
    assert cell_holds(kind, msg, pks, sigs, r, [0, 1, 2])
    assert cell_holds(kind, msg, pks, sigs, [1, 1, 1], [0, 1, 2]) and cell_holds(kind, msg, pks, sigs, r, [1])
    D = (RC.g1_mul(RC.g1_generator(), (12345).to_bytes(32, "big")) if kind == "g2pubs" else RC.g2_mul(RC.g2_generator(), (12345).to_bytes(32, "big")))
    add = RC.g1_sum if kind == "g2pubs" else RC.g2_sum
    tampered = list(sigs); tampered[1] = add(sigs[1] + D, 2)
    assert not mod.verify(msg, pks[1], tampered[1])
    assert not cell_holds(kind, msg, pks, tampered, r, [0, 1, 2])
    order = 52435875175126190479447740508185965837690552500527637822603658699938581184513
    minus_d = (RC.g1_mul if kind == "g2pubs" else RC.g2_mul)(D, (order - 1).to_bytes(32, "big"))
    pair = list(sigs); pair[0] = add(sigs[0] + D, 2); pair[2] = add(sigs[2] + minus_d, 2)
    assert not mod.verify(msg, pks[0], pair[0]) and not mod.verify(msg, pks[2], pair[2])
    assert not cell_holds(kind, msg, pks, pair, r, [0, 1, 2])                    # r_a != r_c: caught
    req = list(r); req[2] = req[0]
    assert cell_holds(kind, msg, pks, pair, req, [0, 1, 2])                      # r_a == r_c: the documented caveat
