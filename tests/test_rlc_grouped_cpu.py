"""CPU side of the grouped randomised batch verification (blsmi 0.11: blsmi_g?pubs_*verify*_batch_rlc_grouped[_jac],
blsmi_g?_sum_segmented_u64): the declarations against the exports and the Python wrappers' argument types, the argument checks that come
before any device work, the host plan (bls_amd/csrc/group_plan.h) run natively under the address and undefined-behaviour sanitizers, and
the grouped equation composed from the oracle's primitives -- what tests/test_gpu_rlc_grouped.py expects of the device."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bls_amd import _native, engine
from cabi_common import CTYPES, _header_params, bound_argtypes
from oracle import refcpu as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -3
SYMS = ["blsmi_g2pubs_verify_batch_rlc_grouped", "blsmi_g1pubs_verify_batch_rlc_grouped", "blsmi_g1pubs_verify_with_domain_batch_rlc_grouped",
        "blsmi_g2pubs_verify_batch_rlc_grouped_jac", "blsmi_g1pubs_verify_batch_rlc_grouped_jac", "blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_jac",
        "blsmi_g1_sum_segmented_u64", "blsmi_g2_sum_segmented_u64"]


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def test_declared_exported_and_typed(lib, tmp_path):
    declared = _native.declared_symbols()
    header = open(_native.HEADER).read()
    assert "0.11 adds" in header
    exported = set(re.findall(r" T (blsmi_\w+)", subprocess.run(["nm", "-D", _native.SO_PATH], capture_output=True, text=True, check=True).stdout))
    for s in SYMS:
        assert s in declared and s in exported and hasattr(lib, s), s
        want = [CTYPES[t] for t in _header_params(header, s)]
        assert bound_argtypes(s) == want, s
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index("grouped randomised batch verification (blsmi 0.11)"):])
    for phrase in ("\"rlc_min\" does NOT apply", "one device", "request combiner", "BLSMI_E_ARG", "never hashed", "not merged"):
        assert phrase in block, phrase
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "t.c"
    src.write_text('#include "blsmi.h"\nint main(void) { return blsmi_g1pubs_verify_batch_rlc_grouped(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_jac(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) + blsmi_g2_sum_segmented_u64(0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(_native.HEADER), str(src)])


def test_argument_checks_come_before_any_device_work(lib):
    """this machine has no device: anything but BLSMI_E_ARG / BLSMI_OK here would be the sign of device work"""
    z = C.c_size_t
    buf = (C.c_uint8 * 1024)()
    w64 = (C.c_uint64 * 128)()
    off = (C.c_uint64 * 3)(0, 4, 8)
    dom = (C.c_uint8 * 8)()
    for name in SYMS[:6]:
        fn = getattr(lib, name)
        jac = name.endswith("_jac")
        head = (buf, dom) if "with_domain" in name else (buf, off)
        pts = (w64, w64) if jac else (buf, buf, None)

        def call(idx, d, n, scalars=None, head=head, pts=pts, null_idx=False):
            ix = (C.c_uint32 * max(1, len(idx)))(*idx)
            sc = (C.c_uint64 * len(scalars))(*scalars) if scalars else None
            comb = C.c_int(7)
            rc = fn(*head, z(d), None if null_idx else ix, *pts, sc, None, None, z(n), C.byref(comb))
            return rc, comb.value
        assert call([0, 2], 2, 2) == (E_ARG, 0), (name, "index >= d")
        assert call([0, 0], 0, 2) == (E_ARG, 0), (name, "d = 0 with n > 0")
        assert call([0, 1], 2, 2, scalars=[5, 0]) == (E_ARG, 0), (name, "a zero scalar")
        assert call([0, 1], 2, 2, null_idx=True) == (E_ARG, 0), (name, "msg_idx NULL")
        assert call([0, 1], 2, 2, head=(None, head[1])) == (E_ARG, 0), (name, "msgs NULL")
        assert call([0, 1], 2, 2, pts=(None,) + tuple(pts[1:])) == (E_ARG, 0), (name, "pks NULL")
        assert call([], 2, 0) == (0, 0), (name, "n = 0")
        assert call([], 0, 0, null_idx=True) == (0, 0), (name, "n = 0, nothing else")
    so = (C.c_uint64 * 3)(0, 2, 4)
    ix = (C.c_uint32 * 4)(0, 1, 2, 9)
    for name in SYMS[6:]:
        fn = getattr(lib, name)
        assert fn(buf, None, z(4), w64, ix, so, z(2), buf, buf) == E_ARG, (name, "index >= npk")
        assert fn(buf, None, z(4), None, None, so, z(2), buf, buf) == E_ARG, (name, "scalars NULL")
        assert fn(buf, None, z(4), w64, None, (C.c_uint64 * 3)(1, 2, 4), z(2), buf, buf) == E_ARG, (name, "seg_off[0] != 0")
        assert fn(buf, None, z(4), w64, None, so, z(2), None, buf) == E_ARG, (name, "out NULL")
        assert fn(None, None, z(0), None, None, None, z(0), None, None) == 0, (name, "m = 0")


def test_python_wrappers_validate():
    with pytest.raises(ValueError):
        engine.g1pubs_verify_batch_rlc_grouped([b"m"], [0, 0], bytes(96), bytes(192 * 2))        # one key per tuple
    with pytest.raises(ValueError):
        engine.g2pubs_verify_batch_rlc_grouped([b"m"], [0, 0], bytes(192 * 2), bytes(96 * 2), scalars=[1])
    with pytest.raises(engine.BlsmiError):
        engine.g2pubs_verify_batch_rlc_grouped([b"m"], [0, 1], bytes(192 * 2), bytes(96 * 2))    # index >= d: the library refuses
    ok, bm, comb = engine.g1pubs_verify_batch_rlc_grouped([b"m"], [], b"", b"")
    assert ok.shape == (0,) and comb == 0
    with pytest.raises(ValueError):
        engine.g1_sum_segmented_u64(bytes(96 * 2), 2, [1], None, [0, 2])                         # one scalar per point


# ---- the host plan, natively ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    gpp = shutil.which("g++")
    assert gpp, "no g++"
    exe = str(tmp_path_factory.mktemp("gplan") / "group_plan")
    subprocess.check_call([gpp, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "group_plan.cc")])
    return exe


def test_group_plan_native_cases(plan_exe):
    """d = 1, d = n, empty groups, an out-of-range index, n = 0, a group of 2^16 + 1: checked inside the program"""
    r = subprocess.run([plan_exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert re.fullmatch(r"GROUP_PLAN ok \d+\n", r.stdout), r.stdout
    assert int(r.stdout.split()[-1]) >= 10


def test_group_plan_against_a_stable_sort(plan_exe):
    rnd = np.random.RandomState(3)
    for d, n in ((1, 5), (4, 4), (7, 40), (50, 20)):
        idx = rnd.randint(0, d, size=n).astype(np.uint32)
        out = subprocess.run([plan_exe, str(d)] + [str(x) for x in idx], capture_output=True, text=True, check=True).stdout.splitlines()
        got = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out}
        assert got["perm"] == np.argsort(idx, kind="stable").tolist()
        used = sorted(set(idx.tolist()))
        assert got["msg_of"] == used
        assert got["seg_off"] == [0] + np.cumsum([int((idx == j).sum()) for j in used]).tolist()
        assert got["group_of"] == [used.index(j) for j in idx.tolist()]
    assert subprocess.run([plan_exe, "3", "0", "3"], capture_output=True, text=True, check=True).stdout == "range\n"


# ---- the grouped equation on the oracle ---------------------------------------------------------------------------------------------
def _fe(f):
    return RC.final_exponentiation(f)[1]


def grouped_holds(kind, table, msg_idx, pks, sigs, r):
    """e(sig side) == prod_g e(sum_{i in g} r_i pk_i, H(m_g)), composed from the oracle's primitives"""
    n = len(msg_idx)
    k32 = [int(x).to_bytes(32, "big") for x in r]
    groups = sorted(set(msg_idx))
    members = {g: [i for i in range(n) if msg_idx[i] == g] for g in groups}
    if kind == "g2pubs":
        S = RC.g1_sum(b"".join(RC.g1_mul(sigs[i], k32[i]) for i in range(n)), n)
        lhs = _fe(RC.miller_loop(S, RC.g2_generator(), 1))
        K = b"".join(RC.g2_sum(b"".join(RC.g2_mul(pks[i], k32[i]) for i in members[g]), len(members[g])) for g in groups)
        rhs = _fe(RC.miller_loop(b"".join(RC.hash_g1(table[g]) for g in groups), K, len(groups)))
    else:
        S = RC.g2_sum(b"".join(RC.g2_mul(sigs[i], k32[i]) for i in range(n)), n)
        lhs = _fe(RC.miller_loop(RC.g1_generator(), S, 1))
        K = b"".join(RC.g1_sum(b"".join(RC.g1_mul(pks[i], k32[i]) for i in members[g]), len(members[g])) for g in groups)
        rhs = _fe(RC.miller_loop(K, b"".join(RC.hash_g2(table[g]) for g in groups), len(groups)))
    return bool(np.array_equal(lhs, rhs))


@pytest.mark.parametrize("kind", ("g1pubs", "g2pubs"))
def test_grouped_equation_on_the_oracle(kind):
    """n = 6, d = 2: the equation holds for valid tuples; with two signatures of ONE group swapped it holds exactly when r_a == r_b"""
    mod = RC.g1pubs if kind == "g1pubs" else RC.g2pubs
    table = [b"slot 17 head", b"slot 17 target"]
    msg_idx = [0, 1, 0, 0, 1, 0]
    sks = [hashlib.sha256(b"grouped-sk-%d" % i).digest()[:31].rjust(32, b"\0") for i in range(6)]
    pks = [mod.priv_to_pub(sk) for sk in sks]
    sigs = [mod.sign(table[msg_idx[i]], sks[i]) for i in range(6)]
    assert all(mod.verify(table[msg_idx[i]], pks[i], sigs[i]) for i in range(6))
    r = [1, 1 << 63, (1 << 64) - 1, 2, 0x123456789abcdef1, 77]
    assert grouped_holds(kind, table, msg_idx, pks, sigs, r)
    a, b = 2, 5                                                                  # both in group 0
    sw = list(sigs); sw[a], sw[b] = sigs[b], sigs[a]
    assert not mod.verify(table[0], pks[a], sw[a]) and not mod.verify(table[0], pks[b], sw[b])
    assert not grouped_holds(kind, table, msg_idx, pks, sw, r)                   # r_a != r_b
    req = list(r); req[b] = req[a]
    assert grouped_holds(kind, table, msg_idx, pks, sw, req)                     # r_a == r_b: the swap goes unnoticed (the caller's responsibility)
    assert not grouped_holds(kind, table, [0, 1, 0, 1, 1, 0], pks, sigs, r)      # a tuple grouped under the other message
