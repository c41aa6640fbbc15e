"""CPU side of the randomised batch verification that finds the bad tuples by blocks (blsmi 0.12:
blsmi_g?pubs_*verify*_batch_rlc_locate[_jac]): the declarations against the exports and the Python wrappers' argument types, the argument
checks that come before any device work, the host plan (bls_amd/csrc/locate_plan.h) run natively under the address and
undefined-behaviour sanitizers, and the block equations composed from the oracle's primitives -- what tests/test_gpu_rlc_locate.py
expects of the device."""
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
SYMS = ["blsmi_g2pubs_verify_batch_rlc_locate", "blsmi_g1pubs_verify_batch_rlc_locate", "blsmi_g1pubs_verify_with_domain_batch_rlc_locate",
        "blsmi_g2pubs_verify_batch_rlc_locate_jac", "blsmi_g1pubs_verify_batch_rlc_locate_jac", "blsmi_g1pubs_verify_with_domain_batch_rlc_locate_jac"]


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def test_declared_exported_and_typed(lib, tmp_path):
    declared = _native.declared_symbols()
    header = open(_native.HEADER).read()
    assert "0.12 adds" in header
    exported = set(re.findall(r" T (blsmi_\w+)", subprocess.run(["nm", "-D", _native.SO_PATH], capture_output=True, text=True, check=True).stdout))
    for s in SYMS:
        assert s in declared and s in exported and hasattr(lib, s), s
        want = [CTYPES[t] for t in _header_params(header, s)]
        assert bound_argtypes(s) == want, s
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index("finds the bad tuples by blocks (blsmi 0.12)"):])
    for phrase in ("\"rlc_min\" does NOT apply", "one device", "request combiner", "BLSMI_E_ARG", "2^-64", "rechecked", "even and at least 2"):
        assert phrase in block, phrase
    assert engine._fn("blsmi_version")().startswith(b"blsmi 0.")                           # the pinned literal stays
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "t.c"
    src.write_text('#include "blsmi.h"\nint main(void) { return blsmi_g2pubs_verify_batch_rlc_locate(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_g1pubs_verify_with_domain_batch_rlc_locate_jac(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(_native.HEADER), str(src)])


def test_argument_checks_come_before_any_device_work(lib):
    """this machine has no device: anything but BLSMI_E_ARG / BLSMI_OK here would be the sign of device work"""
    z = C.c_size_t
    buf = (C.c_uint8 * 1024)()
    w64 = (C.c_uint64 * 128)()
    off = (C.c_uint64 * 3)(0, 4, 8)
    dom = (C.c_uint8 * 8)()
    for name in SYMS:
        fn = engine._fn(name)
        u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
        a8, a64 = C.cast(buf, u8p), C.cast(w64, u64p)
        head = (a8, C.cast(dom, u8p)) if "with_domain" in name else (a8, C.cast(off, u64p))
        pts = (a64, a64) if name.endswith("_jac") else (a8, a8, None)

        def call(block, n, scalars=None, head=head, pts=pts):
            sc = (C.c_uint64 * len(scalars))(*scalars) if scalars else None
            comb, re_ = C.c_int(7), C.c_size_t(7)
            rc = fn(*head, *pts, sc, block, None, None, n, C.byref(comb), C.byref(re_))
            return rc, comb.value, re_.value
        assert call(3, 2) == (E_ARG, 0, 0), (name, "an odd block")
        assert call(1, 2) == (E_ARG, 0, 0), (name, "block = 1")
        assert call(71, 2) == (E_ARG, 0, 0), (name, "an odd block >= n")
        assert call(1, 0) == (E_ARG, 0, 0), (name, "block = 1 with n = 0")
        assert call(2, 2, scalars=[5, 0]) == (E_ARG, 0, 0), (name, "a zero scalar")
        assert call(0, 2, scalars=[0, 5]) == (E_ARG, 0, 0), (name, "a zero scalar, automatic block")
        assert call(2, 2, head=(None, head[1])) == (E_ARG, 0, 0), (name, "msgs NULL")
        assert call(2, 2, head=(head[0], None)) == (E_ARG, 0, 0), (name, "offsets / domain NULL")
        assert call(2, 2, pts=(None,) + tuple(pts[1:])) == (E_ARG, 0, 0), (name, "pks NULL")
        assert call(2, 2, pts=(pts[0], None) + tuple(pts[2:])) == (E_ARG, 0, 0), (name, "sigs NULL")
        for block in (0, 2, 8, 1024):
            assert call(block, 0) == (0, 0, 0), (name, "n = 0", block)
        assert fn(None, None, *([None] * len(pts)), None, 0, None, None, 0, None, None) == 0, (name, "n = 0, nothing else")
        assert fn(*head, *pts, None, 3, None, None, 2, None, None) == E_ARG, (name, "combined and rechecked NULL")


def test_python_wrappers_validate():
    with pytest.raises(ValueError):
        engine.g1pubs_verify_batch_rlc_locate([b"m", b"n"], bytes(96), bytes(192 * 2))             # one key per tuple
    with pytest.raises(ValueError):
        engine.g2pubs_verify_batch_rlc_locate([b"m", b"n"], bytes(192 * 2), bytes(96))             # one signature per tuple
    with pytest.raises(ValueError):
        engine.g2pubs_verify_batch_rlc_locate([b"m", b"n"], bytes(192 * 2), bytes(96 * 2), scalars=[1])
    with pytest.raises(ValueError):
        engine.g2pubs_verify_batch_rlc_locate([b"m", b"n"], bytes(192 * 2), bytes(96 * 2), inf_flags=[0])
    with pytest.raises(ValueError):
        engine.g1pubs_verify_batch_rlc_locate_jac([b"m"], bytes(96), bytes(288))                   # in-memory keys are 144 bytes
    with pytest.raises(ValueError):
        engine.g1pubs_verify_with_domain_batch_rlc_locate([bytes(32)], bytes(7), bytes(96), bytes(192))
    with pytest.raises(ValueError):
        engine.g2pubs_verify_batch_rlc_locate([b"m", b"n"], bytes(192 * 2), bytes(96 * 2), block=-2)
    with pytest.raises(engine.BlsmiError):
        engine.g2pubs_verify_batch_rlc_locate([b"m", b"n"], bytes(192 * 2), bytes(96 * 2), block=3)  # the library refuses an odd block
    with pytest.raises(engine.BlsmiError):
        engine.g1pubs_verify_batch_rlc_locate_jac([b"m", b"n"], bytes(144 * 2), bytes(288 * 2), scalars=[3, 0], block=2)
    for fn in (engine.g1pubs_verify_batch_rlc_locate, engine.g2pubs_verify_batch_rlc_locate, engine.g1pubs_verify_batch_rlc_locate_jac):
        ok, bm, comb, rechecked = fn([], b"", b"")
        assert ok.shape == (0,) and bm.shape == (0,) and comb == 0 and rechecked == 0
    ok, bm, comb, rechecked = engine.g1pubs_verify_with_domain_batch_rlc_locate([], bytes(8), b"", b"", block=8)
    assert ok.shape == (0,) and comb == 0 and rechecked == 0
    for mod in (g1pubs, g2pubs):
        assert mod.VerifyBatchRandomizedLocate([], [], []) == []
        with pytest.raises(ValueError):
            mod.VerifyBatchRandomizedLocate([b"m"], [], [])
    assert g1pubs.VerifyWithDomainBatchRandomizedLocate([], [], [], bytes(8)) == []
    with pytest.raises(ValueError):
        g1pubs.VerifyWithDomainBatchRandomizedLocate([bytes(32)], [], [], bytes(8))


# ---- the host plan, natively ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    gpp = shutil.which("g++")
    assert gpp, "no g++"
    exe = str(tmp_path_factory.mktemp("lplan") / "locate_plan")
    subprocess.check_call([gpp, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "locate_plan.cc")])
    return exe


def test_locate_plan_native_cases(plan_exe):
    """n = 1, n = block, n = block + 1, odd n with halved records, all / no blocks failing, block > n, the automatic rule from 1 to 2^20:
    checked inside the program"""
    r = subprocess.run([plan_exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    m = re.fullmatch(r"LOCATE_PLAN ok (\d+) sampled (\d+)\n", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) >= 40 and int(m.group(2)) >= 70000


def _plan(plan_exe, n, block, halved, fail):
    out = subprocess.run([plan_exe, str(n), str(block), str(int(halved))] + [str(x) for x in fail], capture_output=True, text=True, check=True).stdout
    if out == "invalid\n":
        return None
    return {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out.splitlines()}


def test_locate_plan_against_numpy(plan_exe):
    rnd = np.random.RandomState(5)
    for n, block in ((1, 2), (8, 8), (9, 8), (71, 8), (70, 2), (71, 1024), (300, 0), (20000, 0)):
        want_block = block or max(64, -(-n // 256)) + (max(64, -(-n // 256)) & 1)
        B = -(-n // want_block)
        for halved in (False, True):
            for fail in ([0] * B, [1] * B, rnd.randint(0, 2, size=B).tolist()):
                got = _plan(plan_exe, n, block, halved, fail)
                borders = [min(n, b * want_block) for b in range(B + 1)]
                assert got["block"] == [want_block]
                assert got["tup_off"] == borders
                assert got["rec_off"] == ([(x + 1) // 2 for x in borders] if halved else borders)
                assert got["pos"] == [i for i in range(n) if fail[i // want_block]]
    assert _plan(plan_exe, 10, 3, False, []) is None and _plan(plan_exe, 10, 1, True, []) is None


# ---- the block equations on the oracle -----------------------------------------------------------------------------------------------
def _fe(f):
    return RC.final_exponentiation(f)[1]


def block_holds(kind, msgs, pks, sigs, r, lo, hi):
    """e(S_b, G2gen) == prod_{i in b} e(r_i H(m_i), pk_i)  /  e(G1gen, S_b) == prod_{i in b} e(r_i pk_i, H(m_i)) for the tuples lo .. hi - 1:
    64-bit multiples, the sum, the Miller loop over the pair list, the final exponentiation"""
    idx = range(lo, hi)
    k32 = {i: int(r[i]).to_bytes(32, "big") for i in idx}
    if kind == "g2pubs":
        S = RC.g1_sum(b"".join(RC.g1_mul(sigs[i], k32[i]) for i in idx), hi - lo)
        lhs = _fe(RC.miller_loop(S, RC.g2_generator(), 1))
        rhs = _fe(RC.miller_loop(b"".join(RC.g1_mul(RC.hash_g1(msgs[i]), k32[i]) for i in idx), b"".join(pks[i] for i in idx), hi - lo))
    else:
        S = RC.g2_sum(b"".join(RC.g2_mul(sigs[i], k32[i]) for i in idx), hi - lo)
        lhs = _fe(RC.miller_loop(RC.g1_generator(), S, 1))
        rhs = _fe(RC.miller_loop(b"".join(RC.g1_mul(pks[i], k32[i]) for i in idx), b"".join(RC.hash_g2(msgs[i]) for i in idx), hi - lo))
    return bool(np.array_equal(lhs, rhs))


@pytest.mark.parametrize("kind", ("g1pubs", "g2pubs"))
def test_block_equations_on_the_oracle(kind):
    """n = 6, block = 2: the block equations hold exactly for the blocks without a corrupted tuple, and the total fails with any of them"""
    mod = RC.g1pubs if kind == "g1pubs" else RC.g2pubs
    msgs = [b"locate message %d" % i for i in range(6)]
    sks = [hashlib.sha256(b"locate-sk-%d" % i).digest()[:31].rjust(32, b"\0") for i in range(6)]
    pks = [mod.priv_to_pub(sk) for sk in sks]
    sigs = [mod.sign(msgs[i], sks[i]) for i in range(6)]
    r = [1, 1 << 63, (1 << 64) - 1, 2, 0x123456789abcdef1, 77]
    blocks = [(0, 2), (2, 4), (4, 6)]
    assert all(block_holds(kind, msgs, pks, sigs, r, lo, hi) for lo, hi in blocks) and block_holds(kind, msgs, pks, sigs, r, 0, 6)
    for bad in ([3], [0, 5], [0, 1, 2, 3, 4, 5]):
        cs = list(sigs)
        for i in bad:
            cs[i] = mod.sign(msgs[i] + b"!", sks[i])                              # a valid signature of another message
            assert not mod.verify(msgs[i], pks[i], cs[i])
        got = [block_holds(kind, msgs, pks, cs, r, lo, hi) for lo, hi in blocks]
        assert got == [not any(lo <= i < hi for i in bad) for lo, hi in blocks], (bad, got)
        assert not block_holds(kind, msgs, pks, cs, r, 0, 6)
