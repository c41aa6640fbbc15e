"""CPU side of the wire format <-> in-memory point conversions (blsmi 0.15: blsmi_g?_decompress_batch_jac[_dev], blsmi_g?_compress_batch_jac[_dev]):
the eight declarations against the exports and the Python wrappers' argument types, the argument checks that come before any device work, the
five new functions of both Go shims, how many engine calls the Python mirrors make (counting stubs in the engine's place), the big-integer
model of "wire record -> in-memory record", and the corpora of tests/wire_jac_cases.py.  What tests/test_gpu_wire_jac.py expects of the device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import group_edges as G
import wire_jac_cases as W
from bls_amd import _groups, _native, engine, g1pubs, g2pubs
from cabi_common import CTYPES, _header_params, bound_argtypes
from gpu_common import P

E_ARG = -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["blsmi_g1_decompress_batch_jac", "blsmi_g2_decompress_batch_jac", "blsmi_g1_compress_batch_jac", "blsmi_g2_compress_batch_jac",
        "blsmi_g1_decompress_batch_jac_dev", "blsmi_g2_decompress_batch_jac_dev", "blsmi_g1_compress_batch_jac_dev", "blsmi_g2_compress_batch_jac_dev"]


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


# ---- the ABI surface -------------------------------------------------------------------------------------------------------------------
def test_declared_exported_and_typed(lib, tmp_path):
    declared = _native.declared_symbols()
    header = open(_native.HEADER).read()
    assert "0.15 adds" in header and "0.14 adds" in header
    exported = set(re.findall(r" T (blsmi_\w+)", subprocess.run(["nm", "-D", _native.SO_PATH], capture_output=True, text=True, check=True).stdout))
    for s in SYMS:
        assert s in declared and s in exported and hasattr(lib, s), s
        assert bound_argtypes(s) == [CTYPES[t] for t in _header_params(header, s)], s
    assert _header_params(header, "blsmi_g1_decompress_batch_jac") == ["const uint8_t *", "int", "uint64_t *", "uint8_t *", "uint8_t *", "size_t"]
    assert _header_params(header, "blsmi_g2_compress_batch_jac_dev") == ["const void *", "void *", "size_t", "void *"]
    assert header.index("in-memory points (blsmi 0.15)") > header.index("point validation (blsmi 0.14)")      # appended: the last section
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index("in-memory points (blsmi 0.15)"):])
    for phrase in ("ToProjective", "(0, 1, 0)", "err != 0", "0xc0", "reads as 0", "no curve test", "BLSMI_E_ARG", "ONE device", "request combiner", "must not overlap",
                   "untouched", "One kernel launch"):
        assert phrase in block, phrase
    assert engine.version.__name__ == "version" and "blsmi 0.10" in header    # the version string keeps its pinned beginning
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "t.c"
    src.write_text('#include "blsmi.h"\nint main(void) { return blsmi_g1_decompress_batch_jac(0, 1, 0, 0, 0, 0) + blsmi_g2_decompress_batch_jac(0, 2, 0, 0, 0, 0)'
                   ' + blsmi_g1_compress_batch_jac(0, 0, 0) + blsmi_g2_compress_batch_jac(0, 0, 0) + blsmi_g1_decompress_batch_jac_dev(0, 1, 0, 0, 0, 0, 0)'
                   ' + blsmi_g2_decompress_batch_jac_dev(0, 0, 0, 0, 0, 0, 0) + blsmi_g1_compress_batch_jac_dev(0, 0, 0, 0) + blsmi_g2_compress_batch_jac_dev(0, 0, 0, 0); }\n')
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(_native.HEADER), str(src)])


def test_argument_checks_come_before_any_device_work(lib):
    """this machine has no device: anything but BLSMI_E_ARG / BLSMI_OK here would be the sign of device work"""
    buf = (C.c_uint8 * 512)()
    out = (C.c_uint8 * 512)()
    a8, a64 = C.cast(buf, C.POINTER(C.c_uint8)), C.cast(buf, C.POINTER(C.c_uint64))
    o8, o64 = C.cast(out, C.POINTER(C.c_uint8)), C.cast(out, C.POINTER(C.c_uint64))
    v = C.c_void_p
    for name in SYMS:
        fn = engine._fn(name)
        dev = name.endswith("_dev")
        if "decompress" in name:
            def call(src, dst, err, n, check=1, inf=None, fn=fn, dev=dev):
                return fn(v(src), check, v(dst), v(inf), v(err), n, None) if dev else fn(src, check, dst, inf, err, n)
            src, dst, err = (C.addressof(buf), C.addressof(out), C.addressof(out) + 256) if dev else (a8, o64, o8)
            for check in (3, -1, 256):
                assert call(src, dst, err, 1, check=check) == E_ARG, (name, "check", check)
            for check in (0, 1, 2):
                assert call(None, dst, err, 1, check=check) == E_ARG, (name, "in NULL")
                assert call(src, None, err, 1, check=check) == E_ARG, (name, "out_jac NULL")
                assert call(src, dst, None, 1, check=check) == E_ARG, (name, "err NULL")
                assert call(src, dst, err, 0, check=check) == 0, (name, "n = 0")
                assert call(None, None, None, 0, check=check) == 0, (name, "n = 0, nothing else")
        else:
            def call(src, dst, n, fn=fn, dev=dev):
                return fn(v(src), v(dst), n, None) if dev else fn(src, dst, n)
            src, dst = (C.addressof(buf), C.addressof(out)) if dev else (a64, o8)
            assert call(None, dst, 1) == E_ARG, (name, "pts NULL")
            assert call(src, None, 1) == E_ARG, (name, "out NULL")
            assert call(src, dst, 0) == 0 and call(None, None, 0) == 0, (name, "n = 0")
    assert bytes(out) == bytes(512)


# ---- the Go shims ----------------------------------------------------------------------------------------------------------------------
def test_both_shims_declare_the_five_functions():
    want = {"g2pubs": (96, 48, "g2", "g1"), "g1pubs": (48, 96, "g1", "g2")}
    for pkg, (pkb, sgb, pkg_grp, sig_grp) in want.items():
        src = open(os.path.join(ROOT, "shim", pkg, "accel_cgo.go")).read()
        for sig in ("func DeserializePublicKeys(b [][%d]byte) ([]*PublicKey, []error) {" % pkb,
                    "func DeserializeSignatures(b [][%d]byte) ([]*Signature, []error) {" % sgb,
                    "func SerializePublicKeys(pubs []*PublicKey) [][%d]byte {" % pkb,
                    "func SerializeSignatures(sigs []*Signature) [][%d]byte {" % sgb,
                    "func VerifySerializedBatchRandomized(msgs [][]byte, pubs [][%d]byte, sigs [][%d]byte, block int) []bool {" % (pkb, sgb)):
            assert sig in src, (pkg, sig)
        for call in ("C.blsmi_%s_decompress_batch_jac(" % pkg_grp, "C.blsmi_%s_decompress_batch_jac(" % sig_grp, "C.blsmi_%s_compress_batch_jac(" % pkg_grp,
                     "C.blsmi_%s_compress_batch_jac(" % sig_grp, "C.blsmi_%s_verify_batch_rlc_locate_jac(" % pkg):
            assert call in src, (pkg, call)
        for code, text in _groups._DECODE_ERRORS.items():                       # the error codes map to the messages of the Python mirror
            m = re.search(r"var decodeErrors = \[5\]string\{([^}]*)\}", src)
            assert m and [t.strip().strip('"') for t in m.group(1).split(",")][code] == text, (pkg, code)
        body = src[src.index("func DeserializePublicKeys("):]
        assert "new(bls.G2Projective)" in body and "new(bls.G1Projective)" in body and "unsafe.Pointer(p)" in body   # built the way SumPublicKeys builds its result


# ---- the Python mirrors: how many library calls ----------------------------------------------------------------------------------------------
class Counting:
    """stands in for the engine functions of the mirrors: counts the calls and answers with well-formed arrays"""

    def __init__(self, monkeypatch):
        self.calls = []
        for group, wb, jb in ((1, 48, 144), (2, 96, 288)):
            monkeypatch.setattr(engine, "g%d_compress_batch_jac" % group, self._compress("g%d_compress_batch_jac" % group, wb))
            monkeypatch.setattr(engine, "g%d_decompress_batch_jac" % group, self._decompress("g%d_decompress_batch_jac" % group, jb))
            for other in ("g%d_jac_to_affine_batch", "g%d_compress_batch", "g%d_decompress_batch"):
                monkeypatch.setattr(engine, other % group, self._forbidden(other % group))

    def _compress(self, name, wb):
        def fn(jac, n):
            self.calls.append((name, n))
            return np.full((n, wb), 7, dtype=np.uint8)
        return fn

    def _decompress(self, name, jb):
        def fn(data, n, check_subgroup=True):
            self.calls.append((name, n))
            err = np.zeros(n, dtype=np.uint8)
            err[1::3] = 3
            return np.zeros((n, jb), dtype=np.uint8), np.zeros(n, dtype=bool), err
        return fn

    def _forbidden(self, name):
        def fn(*a, **k):
            self.calls.append((name, None))
            raise AssertionError("%s must not be called" % name)
        return fn


def test_serialize_of_an_in_memory_point_is_one_engine_call(monkeypatch):
    c = Counting(monkeypatch)
    for mod, pk_jb, sig_jb, pk_wb, sig_wb in ((g2pubs, 288, 144, 96, 48), (g1pubs, 144, 288, 48, 96)):
        pk_ctor = mod.NewPublicKeyFromG2Projective if pk_jb == 288 else mod.NewPublicKeyFromG1Projective
        sg_ctor = mod.NewSignatureFromG1Projective if sig_jb == 144 else mod.NewSignatureFromG2Projective
        one = (P.to_mont(1)).to_bytes(48, "little")
        pk = pk_ctor(bytes(pk_jb - 48 * (pk_jb // 144)) + one + bytes(48 * (pk_jb // 144 - 1)))     # some record with z = 1
        sg = sg_ctor(bytes(sig_jb - 48 * (sig_jb // 144)) + one + bytes(48 * (sig_jb // 144 - 1)))
        c.calls.clear()
        assert pk.Serialize() == bytes([7]) * pk_wb
        assert len(c.calls) == 1 and c.calls[0] == ("g%d_compress_batch_jac" % (2 if pk_jb == 288 else 1), 1), c.calls
        c.calls.clear()
        assert sg.Serialize() == bytes([7]) * sig_wb
        assert len(c.calls) == 1, c.calls
        c.calls.clear()
        assert mod.SerializePublicKeys([pk] * 9) == [bytes([7]) * pk_wb] * 9 and len(c.calls) == 1 and c.calls[0][1] == 9, c.calls
        c.calls.clear()
        assert mod.SerializeSignatures([sg] * 4) == [bytes([7]) * sig_wb] * 4 and len(c.calls) == 1, c.calls
        assert mod.SerializePublicKeys([]) == [] and len(c.calls) == 1


@pytest.mark.parametrize("n", (1, 2, 7, 130))
def test_deserialize_public_keys_is_one_engine_call_for_any_n(monkeypatch, n):
    c = Counting(monkeypatch)
    for mod, pk_group, pk_wb, sig_wb in ((g2pubs, 2, 96, 48), (g1pubs, 1, 48, 96)):
        c.calls.clear()
        keys, errs = mod.DeserializePublicKeys([bytes(pk_wb)] * n)
        assert c.calls == [("g%d_decompress_batch_jac" % pk_group, n)], c.calls
        assert errs == [3 if i % 3 == 1 else 0 for i in range(n)] and [k is None for k in keys] == [e != 0 for e in errs]
        assert all(k.p.jac is not None and len(k.p.jac) == 3 * pk_wb for k in keys if k is not None)   # in-memory points
        c.calls.clear()
        sigs, errs = mod.DeserializeSignatures([bytes(sig_wb)] * n)
        assert len(c.calls) == 1 and len(sigs) == len(errs) == n, c.calls
    c.calls.clear()
    assert g2pubs.DeserializePublicKeys([]) == ([], []) and c.calls == []
    pts, errs = _groups.Point.deserialize_many([bytes(48)] * n, 1)
    assert len(pts) == n and all(p.jac is not None for p in pts) and len(c.calls) == 1


def test_deserialize_of_one_point_stays_as_it_is(monkeypatch):
    seen = []

    def fake(data, n, check):
        seen.append((len(data), n, check))
        return np.ones((1, 96), dtype=np.uint8), np.zeros(1, dtype=bool), np.zeros(1, dtype=np.uint8)
    monkeypatch.setattr(engine, "g1_decompress_batch", fake)
    p = _groups.Point.deserialize(bytes(48), 1)
    assert seen == [(48, 1, True)] and p.jac is None and p.raw == bytes([1]) * 96   # the affine call, a wire-form point


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", (1, 2))
def test_wire_as_jac_agrees_with_the_big_integer_model(group):
    """_groups._wire_as_jac against oracle.pyref.to_mont, coordinate by coordinate: finite points, infinity (None and the all-zero record) and a
    coordinate that is not below q (read as 0)"""
    nfq = 2 if group == 1 else 4
    one = [1] + [0] * (nfq // 2 - 1)

    def model(vals):                                                           # vals: the raw coordinates of the wire record
        if vals is None or not any(vals):
            return bytes(48 * nfq * 3 // 2)
        return b"".join(P.to_mont(v if v < P.Q else 0).to_bytes(48, "little") for v in list(vals) + one)
    cases = [[c for xy in a for c in G.coeffs(group, xy)] for a in G.base_points(group)]
    cases += [[P.Q + 3] + c[1:] for c in cases[:2]] + [c[:-1] + [(1 << 384) - 1] for c in cases[:2]] + [[P.Q] * nfq]
    for vals in cases:
        raw = b"".join(v.to_bytes(48, "big") for v in vals)
        got = _groups._wire_as_jac(_groups.Point(raw, group))
        assert got == model(vals), vals
        if all(v < P.Q for v in vals):
            assert got == W.memory_record(group, G.unwire(group, raw)).tobytes()   # ... and with the GPU tests' expectation
    for p in (_groups.Point(None, group), _groups.Point(bytes(48 * nfq), group)):
        assert _groups._wire_as_jac(p) == model(None) and len(model(None)) == (144 if group == 1 else 288)
    z_one = _groups._wire_as_jac(_groups.Point(b"".join(v.to_bytes(48, "big") for v in cases[0]), group))[48 * nfq:]
    assert z_one == b"".join(P.to_mont(v).to_bytes(48, "little") for v in one)


# ---- the corpora -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", (1, 2))
def test_the_corpora_hold_what_they_claim(group):
    es = W.encodings(group)
    labels = {e.label for e in es}
    assert {"subgroup", "subgroup, -y", "infinity", "infinity with a stray bit", "compression bit missing", "no y", "curve point", "x >= q"} <= labels
    assert {e.err for e in es if e.label == "infinity with a stray bit"} == {2} and {e.err for e in es if e.label == "compression bit missing"} == {1}
    assert {e.err for e in es if e.label == "no y"} == {3} and all(e.outside for e in es if e.label == "curve point")
    assert any(e.point is not None for e in es if e.label == "x >= q")       # read as x = 0 (a coefficient of x for G2): a point, not an error
    assert {W.expect(group, e, 1)[0] for e in es} == {0, 1, 2, 3, 4} and 4 not in {W.expect(group, e, 0)[0] for e in es}
    for e in es:                                                               # the well-formed encodings are what Compress gives for their points
        if e.err == 0 and e.label != "x >= q":
            assert W.compress(group, e.point) == e.blob
    recs, want = W.compression_corpus(group)
    z = [W.read_record(group, r)[2] for r in recs]
    one = G.FIELD[group].one
    assert all(v == one for v in z[:64]) and all(v != one for v in z[64:128]) and [i for i in range(128, 192) if z[i] != one] == [165]
    assert z[-1] != one and all(v == one for v in z[-6:-1])
    assert {w[0] & 0xe0 for w in want} == {0x80, 0xa0, 0xc0}
    edges = W.edge_records(group)
    assert any(W.read_record(group, r)[2] == G.FIELD[group].zero and W.read_record(group, r)[0] != G.FIELD[group].zero for r in edges)
    half = [(W.HALF_LO, 0x80), (W.HALF_HI, 0xa0)]
    for r in edges:                                                            # the sign boundary: y = (q - 1) / 2 is not "greater", (q + 1) / 2 is
        jac = W.read_record(group, r)
        if jac[2] == G.FIELD[group].zero:
            continue
        y = W.K.jacobian_to_affine(group, jac)[1]
        for v, flag in half:
            if y == v or (group == 2 and (y[1] == v or (y[1] == 0 and y[0] == v))):
                assert W.oracle_compress(group, r)[0] & 0xe0 == flag
    ys = [W.K.jacobian_to_affine(group, W.read_record(group, r))[1] for r in edges if W.read_record(group, r)[2] != G.FIELD[group].zero]
    if group == 1:
        assert W.HALF_LO in ys and W.HALF_HI in ys
    else:
        assert {(W.HALF_LO, 0), (W.HALF_HI, 0)} <= set(ys) and {W.HALF_LO, W.HALF_HI} <= {y[1] for y in ys}
    for n in (1, 33, 63, 64, 65):
        recs, want = W.compression_cut(group, n)
        assert recs.shape == (n, W.JW[group]) and W.read_record(group, recs[-1])[2] != one and len(want) == n
