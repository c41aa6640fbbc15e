"""CPU side of the randomised verification of many committee aggregates (blsmi 0.16: blsmi_g?pubs_verify_aggregate_common*_batch_rlc
[_jac|_dev], blsmi_debug_g2_sum_segmented_u64_pair): the declarations against the exports and the Python wrappers' argument types, the
argument checks that come before any device work, and the equation composed from the oracle's primitives -- tests/test_rlc_grouped_cpu.py's
grouped_holds with every key replaced by its committee's sum, which is what tests/test_gpu_agg_common_rlc.py expects of the device."""
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
from oracle import pyref as P
from oracle import refcpu as RC
from test_rlc_grouped_cpu import grouped_holds

E_ARG = -3
HOST = ["blsmi_g2pubs_verify_aggregate_common_batch_rlc", "blsmi_g1pubs_verify_aggregate_common_batch_rlc", "blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc"]
SYMS = HOST + [s + "_jac" for s in HOST] + [s + "_dev" for s in HOST] + ["blsmi_debug_g2_sum_segmented_u64_pair"]


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def test_declared_exported_and_typed(lib, tmp_path):
    declared = _native.declared_symbols()
    header = open(_native.HEADER).read()
    assert "0.16 adds" in header and "0.15 adds" in header
    exported = set(re.findall(r" T (blsmi_\w+)", subprocess.run(["nm", "-D", _native.SO_PATH], capture_output=True, text=True, check=True).stdout))
    assert exported == set(declared)                                             # nm -D exports equal the header's names
    assert len(SYMS) == 10
    for s in SYMS:
        assert s in declared and s in exported and hasattr(lib, s), s
        want = [CTYPES[t] for t in _header_params(header, s)]
        assert bound_argtypes(s) == want, s
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index("committee aggregates, randomised (blsmi 0.16)"):])
    for phrase in ("ok[j] is exactly what *_verify_aggregate_common*_batch gives for the same inputs", "\"rlc_min\" does NOT apply", "one device", "request combiner",
                   "BLSMI_E_ARG before any device work", "at most 2^-64 over the drawn scalars", "in the prime-order subgroups", "both outputs NULL"):
        assert phrase in block, phrase
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "t.c"
    src.write_text('#include "blsmi.h"\nint main(void) { return blsmi_g2pubs_verify_aggregate_common_batch_rlc(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc_jac(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_g1pubs_verify_aggregate_common_batch_rlc_dev(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_debug_g2_sum_segmented_u64_pair(0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(_native.HEADER), str(src)])


def test_argument_checks_come_before_any_device_work(lib):
    """this machine has no device: anything but BLSMI_E_ARG / BLSMI_OK here would be the sign of device work"""
    z = C.c_size_t
    buf = (C.c_uint8 * 4096)()
    w64 = (C.c_uint64 * 512)()
    moff = (C.c_uint64 * 3)(0, 4, 8)
    dom = (C.c_uint8 * 8)()
    for name in HOST + [s + "_jac" for s in HOST]:
        fn = engine._fn(name)
        jac = name.endswith("_jac")
        u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
        pts = C.cast(w64, u64p) if jac else C.cast(buf, u8p)
        head = (C.cast(buf, u8p), C.cast(dom, u8p)) if "with_domain" in name else (C.cast(buf, u8p), C.cast(moff, u64p))

        def call(msg_idx=(0, 1), d=2, npk=4, idx=(0, 1, 2, 3), seg=(0, 2, 4), scalars=None, m=2, head=head, pks=pts, sigs=pts, null_msg_idx=False, null_seg=False,
                 want_ok=True, want_bm=False):
            mi = (C.c_uint32 * max(1, len(msg_idx)))(*msg_idx)
            ix = (C.c_uint32 * len(idx))(*idx) if idx is not None else None
            so = (C.c_uint64 * len(seg))(*seg)
            sc = (C.c_uint64 * len(scalars))(*scalars) if scalars else None
            ok, bm = (C.c_uint8 * 8)(), (C.c_uint8 * 8)()
            comb = C.c_int(7)
            rc = fn(*head, d, None if null_msg_idx else mi, pks, npk, ix, None if null_seg else so, sigs, sc, ok if want_ok else None, bm if want_bm else None, m, C.byref(comb))
            return rc, comb.value
        assert call(seg=(1, 2, 4)) == (E_ARG, 0), (name, "offsets that do not start at 0")
        assert call(seg=(0, 3, 2)) == (E_ARG, 0), (name, "offsets that decrease")
        assert call(idx=(0, 1, 2, 4)) == (E_ARG, 0), (name, "an index >= npk")
        assert call(idx=None, npk=3) == (E_ARG, 0), (name, "positions past the registry")
        assert call(msg_idx=(0, 2)) == (E_ARG, 0), (name, "msg_idx >= d")
        assert call(msg_idx=(0, 0), d=0) == (E_ARG, 0), (name, "d = 0 with m > 0")
        assert call(scalars=[5, 0]) == (E_ARG, 0), (name, "a zero scalar")
        assert call(null_msg_idx=True) == (E_ARG, 0), (name, "msg_idx NULL")
        assert call(null_seg=True) == (E_ARG, 0), (name, "seg_off NULL")
        assert call(head=(None, head[1])) == (E_ARG, 0), (name, "msgs NULL")
        assert call(head=(head[0], None)) == (E_ARG, 0), (name, "msg_off / domain NULL")
        assert call(pks=None) == (E_ARG, 0), (name, "pks NULL")
        assert call(sigs=None) == (E_ARG, 0), (name, "sigs NULL")
        assert call(want_ok=False) == (E_ARG, 0), (name, "both outputs NULL")
        assert call(msg_idx=(), seg=(0,), idx=None, m=0) == (0, 0), (name, "m = 0")
        assert call(msg_idx=(), seg=(0,), idx=None, m=0, head=(None, None), pks=None, sigs=None, null_msg_idx=True, null_seg=True, want_ok=False, d=0, npk=0) == (0, 0), \
            (name, "m = 0, nothing else")
    for name in (s + "_dev" for s in HOST):                                      # what the _dev forms can refuse without a device
        fn = engine._fn(name)
        comb = C.c_int(7)
        a = C.addressof(buf)
        assert fn(a, a, 2, a, a, 4, a, a, a, (C.c_uint64 * 2)(3, 0), a, 2, C.byref(comb), None) == E_ARG and comb.value == 0, (name, "a zero scalar")
        comb = C.c_int(7)
        assert fn(a, a, 2, None, a, 4, a, a, a, None, a, 2, C.byref(comb), None) == E_ARG and comb.value == 0, (name, "d_msg_idx NULL")
        comb = C.c_int(7)
        assert fn(None, None, 0, None, None, 0, None, None, None, None, None, 0, C.byref(comb), None) == 0 and comb.value == 0, (name, "m = 0")
    fn = lib.blsmi_debug_g2_sum_segmented_u64_pair
    so = (C.c_uint64 * 3)(0, 2, 4)
    assert fn(buf, None, z(4), w64, (C.c_uint32 * 4)(0, 1, 2, 9), so, z(2), buf, buf) == E_ARG                # index >= npk
    assert fn(buf, None, z(4), None, None, so, z(2), buf, buf) == E_ARG                                       # scalars NULL
    assert fn(None, None, z(0), None, None, None, z(0), None, None) == 0                                      # m = 0


def test_python_wrappers_validate():
    seg = [0, 1, 3]
    with pytest.raises(ValueError):
        engine.g1pubs_verify_aggregate_common_batch_rlc([b"m"], [0, 0], bytes(96 * 3), 3, None, seg, bytes(192))          # one signature per item
    with pytest.raises(ValueError):
        engine.g2pubs_verify_aggregate_common_batch_rlc([b"m"], [0, 0], bytes(192 * 3), 3, None, seg, bytes(96 * 2), scalars=[1])
    with pytest.raises(ValueError):
        engine.g2pubs_verify_aggregate_common_batch_rlc([b"m"], [0], bytes(192 * 3), 3, None, seg, bytes(96 * 2))         # one message index per item
    with pytest.raises(ValueError):
        engine.g1pubs_verify_aggregate_common_with_domain_batch_rlc_jac([bytes(32)], bytes(8), [0, 0], bytes(144 * 3), 3, None, seg, bytes(288 * 3))
    with pytest.raises(engine.BlsmiError) as ei:
        engine.g2pubs_verify_aggregate_common_batch_rlc([b"m"], [0, 1], bytes(192 * 3), 3, None, seg, bytes(96 * 2))      # index >= d: the library refuses
    assert "(-3)" in str(ei.value)
    ok, bm, comb = engine.g1pubs_verify_aggregate_common_batch_rlc([b"m"], [], b"", 0, None, [0], b"")
    assert ok.shape == (0,) and bm.shape == (0,) and comb == 0
    from bls_amd import g1pubs, g2pubs
    for mod in (g1pubs, g2pubs):
        assert mod.VerifyAggregateCommonBatchRandomized([], [], []) == []
        with pytest.raises(ValueError):
            mod.VerifyAggregateCommonBatchRandomized([None, None], [[], []], [b"a"])
        with pytest.raises(ValueError):
            mod.VerifyAggregateCommonBatchRandomized([None, None], [[], []], [b"a", b"a"], scalars=[1])
    with pytest.raises(ValueError):
        g1pubs.VerifyAggregateCommonWithDomainBatchRandomized([None], [[]], [bytes(32)], bytes(8), scalars=[1, 2])
    assert g1pubs.VerifyAggregateCommonWithDomainBatchRandomized([], [], [], bytes(8)) == []
    from bls_amd._groups import message_table
    assert message_table([b"a", b"b", b"a", b"", b"b"]) == ([b"a", b"b", b""], [0, 1, 0, 2, 1])


# ---- the equation on the oracle -------------------------------------------------------------------------------------------------------
def committee_holds(kind, table, msg_idx, registry, committees, sigs, r):
    """grouped_holds over the committees' sums: e(sig side) == prod_g e(sum_{j in g} r_j apk_j, H(m_g)), apk_j = the sum of committee j"""
    add = RC.g2_sum if kind == "g2pubs" else RC.g1_sum
    apk = [add(b"".join(registry[i] for i in c), len(c)) for c in committees]
    assert all(a is not None for a in apk)
    return grouped_holds(kind, table, msg_idx, apk, sigs, r)


@pytest.mark.parametrize("kind", ("g1pubs", "g2pubs"))
def test_committee_equation_on_the_oracle(kind):
    """m = 6 items over a 10-key registry, d = 2, committee sizes 1, 2, 3, 3, 4, 5, one key twice in one committee"""
    mod = RC.g1pubs if kind == "g1pubs" else RC.g2pubs
    table = [b"slot 31 head", b"slot 31 target"]
    msg_idx = [0, 1, 0, 0, 1, 0]
    sks = [int.from_bytes(hashlib.sha256(b"committee-sk-%d" % i).digest()[:31], "big") for i in range(10)]
    registry = [mod.priv_to_pub(sk.to_bytes(32, "big")) for sk in sks]
    committees = [[4], [0, 9], [1, 2, 3], [5, 7, 5], [6, 8, 0, 2], [9, 1, 3, 4, 7]]                     # key 5 twice in committee 3
    assert [len(c) for c in committees] == [1, 2, 3, 3, 4, 5]

    def sign(j, comm):
        return mod.sign(table[msg_idx[j]], (sum(sks[i] for i in comm) % P.R_ORDER).to_bytes(32, "big"))
    sigs = [sign(j, c) for j, c in enumerate(committees)]
    assert all(mod.verify_aggregate_common(sigs[j], [registry[i] for i in committees[j]], table[msg_idx[j]]) for j in range(6))
    r = [1, 1 << 63, (1 << 64) - 1, 2, 0x123456789abcdef1, 77]
    assert committee_holds(kind, table, msg_idx, registry, committees, sigs, r)
    other = [list(c) for c in committees]; other[4][1] = 9                                             # one member replaced
    assert not mod.verify_aggregate_common(sigs[4], [registry[i] for i in other[4]], table[1])
    assert not committee_holds(kind, table, msg_idx, registry, other, sigs, r)
    assert not committee_holds(kind, table, [0, 1, 0, 1, 1, 0], registry, committees, sigs, r)        # an item under the other message
    a, b = 2, 5                                                                                       # two signatures of message 0 swapped
    sw = list(sigs); sw[a], sw[b] = sigs[b], sigs[a]
    assert not committee_holds(kind, table, msg_idx, registry, committees, sw, r)                     # r_a != r_b
    req = list(r); req[b] = req[a]
    assert committee_holds(kind, table, msg_idx, registry, committees, sw, req)                       # r_a == r_b: unnoticed (the caller's responsibility)
    assert np.array_equal(np.asarray(msg_idx)[[a, b]], [0, 0])
