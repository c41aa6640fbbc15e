"""CPU side of the committee batches (blsmi 0.9: blsmi_g?_sum_segmented[_jac|_dev], *_verify_aggregate_common*_batch[_jac|_dev]): the
argument checks that return BLSMI_E_ARG before any device work, m = 0, the Python flattening, and the oracle composition the GPU tests
(tests/test_gpu_agg_common_batch.py) use to make valid aggregates cheaply: sig = (sum sk mod r) H(m)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from bls_amd import _native, engine
from bls_amd._groups import Point, flatten_committees
from oracle import pyref as P
from oracle import refcpu as RC

E_ARG = -3


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def _u64(vals):
    a = np.ascontiguousarray(vals, dtype=np.uint64)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint64))


def _u32(vals):
    a = np.ascontiguousarray(vals, dtype=np.uint32)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint32))


def _buf(n):
    a = np.zeros(max(1, n), dtype=np.uint8)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint8))


def _sum_calls(lib):
    """(name, call(npk, idx, seg_off, m, out_null=False)) for the four host forms of the segmented sum"""
    def mk(fn, pb, jac):
        def call(npk, idx, seg_off, m, out_null=False):
            pts, pp = _buf((pb // 2 * 3 if jac else pb) * max(npk, 1))
            out, po = _buf(pb * m)
            inf, pi = _buf(m)
            args = [pts.ctypes.data_as(C.POINTER(C.c_uint64)) if jac else pp]
            if not jac:
                args.append(None)
            args += [C.c_size_t(npk), idx, seg_off, C.c_size_t(m), None if out_null else po, pi]
            return fn(*args)
        return call
    return [("g1", mk(lib.blsmi_g1_sum_segmented, 96, False)), ("g2", mk(lib.blsmi_g2_sum_segmented, 192, False)),
            ("g1_jac", mk(lib.blsmi_g1_sum_segmented_jac, 96, True)), ("g2_jac", mk(lib.blsmi_g2_sum_segmented_jac, 192, True))]


def _verify_calls(lib):
    """(name, call(npk, idx, seg_off, m, msg_off=None, sigs_null=False)) for the six host forms of the batch"""
    def mk(fn, pkb, sgb, kind, jac):
        def call(npk, idx, seg_off, m, msg_off=None, sigs_null=False):
            pks, pp = _buf(pkb * max(npk, 1))
            sigs, ps = _buf(sgb * max(m, 1))
            msgs, pm = _buf(64 * max(m, 1))
            ok, pok = _buf(m)
            if jac:
                pp, ps = pks.ctypes.data_as(C.POINTER(C.c_uint64)), sigs.ctypes.data_as(C.POINTER(C.c_uint64))
            if kind == 2:
                dom, pd = _buf(8)
                head = [pm, pd]
            else:
                if msg_off is None:
                    msg_off = list(range(0, m + 1))
                off, poff = _u64(msg_off)
                head = [pm, poff]
            return fn(*head, pp, C.c_size_t(npk), idx, seg_off, None if sigs_null else ps, pok, None, C.c_size_t(m))
        return call
    return [("g2pubs", mk(lib.blsmi_g2pubs_verify_aggregate_common_batch, 192, 96, 0, False)),
            ("g1pubs", mk(lib.blsmi_g1pubs_verify_aggregate_common_batch, 96, 192, 1, False)),
            ("g1pubs_domain", mk(lib.blsmi_g1pubs_verify_aggregate_common_with_domain_batch, 96, 192, 2, False)),
            ("g2pubs_jac", mk(lib.blsmi_g2pubs_verify_aggregate_common_batch_jac, 288, 144, 0, True)),
            ("g1pubs_jac", mk(lib.blsmi_g1pubs_verify_aggregate_common_batch_jac, 144, 288, 1, True)),
            ("g1pubs_domain_jac", mk(lib.blsmi_g1pubs_verify_aggregate_common_with_domain_batch_jac, 144, 288, 2, True))]


def _bad_segments():
    """(what, npk, idx or None, seg_off, m): each one is BLSMI_E_ARG"""
    return [("seg_off[0] != 0", 8, None, [1, 2, 3], 2),
            ("decreasing offsets", 8, None, [0, 3, 2, 4], 3),
            ("idx[k] >= npk", 8, [0, 1, 8, 2], [0, 2, 4], 2),
            ("idx == NULL, seg_off[m] > npk", 4, None, [0, 2, 5], 2),
            ("seg_off NULL", 4, None, None, 2)]


def _seg_ptrs(idx, seg_off):
    keep = []
    pi = ps = None
    if idx is not None:
        a, pi = _u32(idx); keep.append(a)
    if seg_off is not None:
        b, ps = _u64(seg_off); keep.append(b)
    return keep, pi, ps


def test_segmented_sum_argument_checks(lib):
    for name, call in _sum_calls(lib):
        for what, npk, idx, seg_off, m in _bad_segments():
            keep, pi, ps = _seg_ptrs(idx, seg_off)
            assert call(npk, pi, ps, m) == E_ARG, (name, what)
        keep, pi, ps = _seg_ptrs([0, 1, 2], [0, 1, 3])
        assert call(4, pi, ps, 2, out_null=True) == E_ARG, (name, "NULL out")
        assert call(4, pi, None, 0) == 0, (name, "m = 0")


def test_verify_batch_argument_checks(lib):
    for name, call in _verify_calls(lib):
        for what, npk, idx, seg_off, m in _bad_segments():
            keep, pi, ps = _seg_ptrs(idx, seg_off)
            assert call(npk, pi, ps, m) == E_ARG, (name, what)
        keep, pi, ps = _seg_ptrs([0, 1, 2], [0, 1, 3])
        assert call(4, pi, ps, 2, sigs_null=True) == E_ARG, (name, "NULL signatures")
        if "domain" not in name:
            assert call(4, pi, ps, 2, msg_off=[1, 2, 3]) == E_ARG, (name, "msg_off[0] != 0")
            assert call(4, pi, ps, 2, msg_off=[0, 3, 2]) == E_ARG, (name, "decreasing msg_off")
        assert call(4, pi, None, 0) == 0, (name, "m = 0")


def test_dev_forms_null_buffers_and_empty(lib):
    v = C.c_void_p
    for fn in (lib.blsmi_g1_sum_segmented_dev, lib.blsmi_g2_sum_segmented_dev):
        assert fn(None, None, C.c_size_t(4), None, None, C.c_size_t(2), None, None, None) == E_ARG
        assert fn(None, None, C.c_size_t(0), None, None, C.c_size_t(0), None, None, None) == 0
    for fn in (lib.blsmi_g2pubs_verify_aggregate_common_batch_dev, lib.blsmi_g1pubs_verify_aggregate_common_batch_dev,
               lib.blsmi_g1pubs_verify_aggregate_common_with_domain_batch_dev):
        assert fn(None, None, None, C.c_size_t(4), None, None, None, None, C.c_size_t(2), None) == E_ARG
        assert fn(v(0), v(0), v(0), C.c_size_t(0), v(0), v(0), v(0), v(0), C.c_size_t(0), v(0)) == 0


def test_flattening_gives_the_offsets():
    pts = [Point(None, 1) for _ in range(9)]
    committees = [pts[0:3], [], pts[3:4], pts[4:9], []]
    flat, off = flatten_committees(committees)
    assert off.dtype == np.uint64 and off.tolist() == [0, 3, 3, 4, 9, 9]
    assert flat == pts
    assert engine.seg_offsets([]).tolist() == [0]
    assert engine.seg_offsets([0, 0, 2]).tolist() == [0, 0, 0, 2]


def _sk(i):
    return hashlib.sha256(b"cpu-agg-common-%d" % i).digest()[:31].rjust(32, b"\0")


def _summed(sks):
    return (sum(int.from_bytes(s, "big") for s in sks) % P.R_ORDER).to_bytes(32, "big")


def test_summed_secret_key_composition():
    sks = [_sk(i) for i in range(5)]
    msg, msg32, dom = b"committee message", hashlib.sha256(b"m32").digest(), b"\x01\x00\x00\x00\x02\x00\x00\x00"
    pks2 = [RC.g2pubs.priv_to_pub(s) for s in sks]
    pks1 = [RC.g1pubs.priv_to_pub(s) for s in sks]
    sig2 = RC.g2pubs.sign(msg, _summed(sks))
    sig1 = RC.g1pubs.sign(msg, _summed(sks))
    sigd = RC.g1pubs.sign_with_domain(msg32, _summed(sks), dom)
    assert RC.g2pubs.verify_aggregate_common(sig2, pks2, msg)
    assert RC.g1pubs.verify_aggregate_common(sig1, pks1, msg)
    assert RC.g1pubs.verify_aggregate_common_with_domain(sigd, pks1, msg32, dom)
    # the same as aggregating the members' own signatures
    assert sig2 == RC.g1_sum(b"".join(RC.g2pubs.sign(msg, s) for s in sks), len(sks))
    # a repeated member counts twice; a dropped one breaks it
    assert RC.g2pubs.verify_aggregate_common(RC.g2pubs.sign(msg, _summed(sks + sks[:1])), pks2 + pks2[:1], msg)
    assert not RC.g2pubs.verify_aggregate_common(sig2, pks2[1:], msg)
    assert not RC.g1pubs.verify_aggregate_common_with_domain(sigd, pks1, msg32, dom[::-1])
    # the empty committee is never valid
    assert not RC.g2pubs.verify_aggregate_common(sig2, [], msg)
