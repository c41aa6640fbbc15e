"""CPU side of the batch point validation (blsmi 0.14: blsmi_g?_check_batch[_jac|_dev]): the corpus of tests/point_check_cases.py holds every
class it claims, the identities the kernels of bls_amd/csrc/k_check.hip rest on -- the curve equation and the endomorphisms on Jacobian
coordinates -- hold with big integers against oracle.pyref, and the ABI surface: the declarations against the exports and the Python wrappers'
argument types, the header as C99, the argument checks that come before any device work.  What tests/test_gpu_point_check.py expects of the
device."""
import collections
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import group_edges as G
import point_check_cases as K
from bls_amd import _native, engine, g1pubs, g2pubs
from cabi_common import CTYPES, _header_params, bound_argtypes
from gpu_common import P

E_ARG = -3
GROUPS = (1, 2)
FORMS = ("affine", "jacobian")
SYMS = ["blsmi_g1_check_batch", "blsmi_g2_check_batch", "blsmi_g1_check_batch_jac", "blsmi_g2_check_batch_jac", "blsmi_g1_check_batch_dev", "blsmi_g2_check_batch_dev"]


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


# ---- the corpus ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("group", GROUPS)
def test_every_class_is_present(group, form):
    cs = K.cases(group, form)
    count = collections.Counter(c.status for c in cs)
    for st in K.STATUSES:
        assert count[st] >= 4, (group, form, st, dict(count))
    assert set(count) == set(K.STATUSES)
    outside = {c.src for c in cs if c.status == K.NOT_IN_SUBGROUP}
    assert "outside_points" in outside and "x_zero_points" in outside, outside
    good = {c.src for c in cs if c.status == K.OK}
    assert good == {"subgroup_points", "generator"}, good
    labels = {c.label for c in cs}
    assert {"y+1", "swapped"} <= labels and ("b=5" if group == 1 else "y.c1 negated") in labels
    if group == 1:                                                             # the record whose x is not below q, judged as the point (0, y)
        odd = [c for c in cs if c.src == "noncanonical"]
        assert odd and all(c.point[0] == 0 for c in odd) and {c.status for c in odd} == {K.NOT_ON_CURVE, K.NOT_IN_SUBGROUP}
    if form == "jacobian":
        assert len(cs) < 500
        per_point = collections.Counter((c.label, c.point) for c in cs if c.z is not None)
        assert min(per_point.values()) >= (3 if group == 1 else 4)
        assert any(c.z == G.FIELD[group].one for c in cs)
        if group == 2:
            assert any(c.z is not None and (c.z[0] == 0 or c.z[1] == 0) for c in cs)
        inf = [G.unrecord(group, c.rec) for c in cs if c.src == "infinity"]
        assert len(inf) == 6 and all(j[2] == G.FIELD[group].zero for j in inf)
        assert sum(1 for j in inf if j[0] != G.FIELD[group].zero and j[1] != G.FIELD[group].zero) == 4   # Z = 0 with arbitrary non-zero X and Y
        assert sum(1 for j in inf if j[0] == G.FIELD[group].zero and j[1] == G.FIELD[group].one) == 2    # and (0, 1, 0)
    else:
        flagged = [c for c in cs if c.inf]
        assert any(any(c.rec) for c in flagged) and any(not any(c.rec) and not c.inf for c in cs)        # a finite record with its flag; the bare all-zero record
        assert all(c.status == K.INFINITY for c in flagged)


@pytest.mark.parametrize("group", GROUPS)
def test_every_scaled_record_maps_back_and_satisfies_the_jacobian_curve_equation_exactly_when_its_point_is_on_the_curve(group):
    F = G.FIELD[group]
    b = P.B_COEFF if group == 1 else P.B_COEFF_FQ2
    on_curve = P.g1_on_curve if group == 1 else P.g2_on_curve
    n = 0
    for c in K.jacobian_cases(group):
        if c.z is None:
            continue
        X, Y, Z = G.unrecord(group, c.rec)
        assert Z == c.z and K.jacobian_to_affine(group, (X, Y, Z)) == c.point, c.label
        z2 = F.sqr(Z)
        z6 = F.mul(F.sqr(z2), z2)
        holds = F.sqr(Y) == F.add(F.mul(F.sqr(X), X), F.mul(b, z6))           # Y^2 == X^3 + b Z^6
        assert holds == on_curve(c.point), c.label
        assert holds == (c.status != K.NOT_ON_CURVE)
        n += 1
    assert n >= 100


def _beta():
    """the cube root of unity the G1 ladder's phi uses (consts: C_BETA), recovered from the generator: phi(G) = [-x^2] G"""
    g = P.G1_GEN
    want = P.jac_to_affine(P.F1, P.jac_neg(P.F1, P.affine_mul(P.F1, g, P.BLS_X * P.BLS_X)))
    beta = want[0] * P.fq_inv(g[0]) % P.Q
    assert pow(beta, 3, P.Q) == 1 and beta != 1 and want[1] == g[1]
    return beta


def _psi_constants():
    """psi(x, y) = (Cx conj x, Cy conj y): the two constants from the images of one point"""
    a = G.subgroup_points(2)[0]
    px, py = P.psi(a)
    return P.fq2_mul(px, P.fq2_inv(P.fq2_conj(a[0]))), P.fq2_mul(py, P.fq2_inv(P.fq2_conj(a[1])))


def test_the_jacobian_endomorphisms_are_the_affine_ones():
    """phi(X, Y, Z) = (beta X, Y, Z) and psi(X, Y, Z) = (Cx conj X, Cy conj Y, conj Z), taken to affine, are phi and psi of the point --
    inside and outside the subgroup, under every Z of the corpus"""
    beta = _beta()
    cx, cy = _psi_constants()
    seen = collections.Counter()
    for c in K.jacobian_cases(1):
        if c.z is None or c.status == K.NOT_ON_CURVE:
            continue
        X, Y, Z = G.unrecord(1, c.rec)
        assert K.jacobian_to_affine(1, (beta * X % P.Q, Y, Z)) == (beta * c.point[0] % P.Q, c.point[1]), c.label
        seen[(1, c.status)] += 1
    for c in K.jacobian_cases(2):
        if c.z is None or c.status == K.NOT_ON_CURVE:
            continue
        X, Y, Z = G.unrecord(2, c.rec)
        img = (P.fq2_mul(cx, P.fq2_conj(X)), P.fq2_mul(cy, P.fq2_conj(Y)), P.fq2_conj(Z))
        assert K.jacobian_to_affine(2, img) == P.psi(c.point), c.label
        seen[(2, c.status)] += 1
    assert all(seen[(g, st)] >= 12 for g in GROUPS for st in (K.OK, K.NOT_IN_SUBGROUP)), seen
    # ... and the predicates built from them say what the oracle's r * P says
    for group in GROUPS:
        for label, src, a in K.finite_points(group):
            if K.oracle_status(group, a) == K.NOT_ON_CURVE:
                continue
            F = G.FIELD[group]
            if group == 1:
                s = P.jac_add_affine(F, P.affine_mul(F, a, P.BLS_X * P.BLS_X), (beta * a[0] % P.Q, a[1]))
            else:
                s = P.jac_add_affine(F, P.affine_mul(F, a, P.BLS_X), P.psi(a))
            assert P.jac_is_zero(F, s) == (K.oracle_status(group, a) == K.OK), (group, label)


def test_cuts_hold_every_status_and_end_on_a_bad_record():
    for group in GROUPS:
        for form in FORMS:
            cs = K.cases(group, form)
            for n in K.SIZES:
                part = K.cut(cs, n)
                assert len(part) == n and part[-1].status != K.OK
                if n >= 4:
                    assert {c.status for c in part} == set(K.STATUSES), (group, form, n)


# ---- the ABI surface -------------------------------------------------------------------------------------------------------------------
def test_declared_exported_and_typed(lib, tmp_path):
    declared = _native.declared_symbols()
    header = open(_native.HEADER).read()
    assert "0.14 adds" in header and "0.13 adds" in header
    exported = set(re.findall(r" T (blsmi_\w+)", subprocess.run(["nm", "-D", _native.SO_PATH], capture_output=True, text=True, check=True).stdout))
    for s in SYMS:
        assert s in declared and s in exported and hasattr(lib, s), s
        assert bound_argtypes(s) == [CTYPES[t] for t in _header_params(header, s)], s
    assert header.index("point validation (blsmi 0.14)") > header.index("pairing products (blsmi 0.10)")      # appended: the last section
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index("point validation (blsmi 0.14)"):])
    for phrase in ("IsOnCurve", "IsInCorrectSubgroupAssumingOnCurve", "is read as 0", "AS THAT POINT", "z == 0", "in_inf", "not consulted", "BLSMI_E_ARG",
                   "no field inversion and no square root", "one kernel launch", "ONE device", "request combiner", "untouched", "BLSMI_LAYOUT=single"):
        assert phrase in block, phrase
    for name, value in (("BLSMI_POINT_OK", 0), ("BLSMI_POINT_INFINITY", 1), ("BLSMI_POINT_NOT_ON_CURVE", 3), ("BLSMI_POINT_NOT_IN_SUBGROUP", 4)):
        assert re.search(r"#define %s %d\b" % (name, value), block), name
    assert (engine.POINT_OK, engine.POINT_INFINITY, engine.POINT_NOT_ON_CURVE, engine.POINT_NOT_IN_SUBGROUP) == K.STATUSES
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "t.c"
    src.write_text('#include "blsmi.h"\nint main(void) { return blsmi_g1_check_batch(0, 0, 1, 0, 0) + blsmi_g2_check_batch(0, 0, 1, 0, 0)'
                   ' + blsmi_g1_check_batch_jac(0, 2, 0, 0) + blsmi_g2_check_batch_jac(0, 0, 0, 0) + blsmi_g1_check_batch_dev(0, 0, 0, 1, 0, 0, 0)'
                   ' + blsmi_g2_check_batch_dev(0, 0, 1, 1, 0, 0, 0) + BLSMI_POINT_OK + BLSMI_POINT_NOT_IN_SUBGROUP; }\n')
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(_native.HEADER), str(src)])


def test_argument_checks_come_before_any_device_work(lib):
    """this machine has no device: anything but BLSMI_E_ARG / BLSMI_OK here would be the sign of device work"""
    buf = (C.c_uint8 * 512)()
    st = (C.c_uint8 * 8)()
    a8, a64, s8 = C.cast(buf, C.POINTER(C.c_uint8)), C.cast(buf, C.POINTER(C.c_uint64)), C.cast(st, C.POINTER(C.c_uint8))
    v = C.c_void_p
    for name in SYMS:
        fn = engine._fn(name)
        if name.endswith("_dev"):
            def call(pts, status, check, n, fn=fn, jac=0, flags=None):
                return fn(v(pts), v(flags), jac, check, v(status), n, None)
            p, s = C.addressof(buf), C.addressof(st)
            assert call(p, s, 1, 1, jac=1, flags=p) == E_ARG, (name, "flags with the in-memory form")
        elif name.endswith("_jac"):
            def call(pts, status, check, n, fn=fn):
                return fn(pts, check, status, n)
            p, s = a64, s8
        else:
            def call(pts, status, check, n, fn=fn):
                return fn(pts, None, check, status, n)
            p, s = a8, s8
        for check in (3, -1, 256):
            assert call(p, s, check, 1) == E_ARG, (name, "check", check)
            assert call(p, s, check, 0) == E_ARG, (name, "check with n = 0", check)
        for check in (0, 1, 2):
            assert call(None, s, check, 1) == E_ARG, (name, "pts NULL")
            assert call(p, None, check, 1) == E_ARG, (name, "status NULL")
            assert call(p, s, check, 0) == 0, (name, "n = 0")
            assert call(None, None, check, 0) == 0, (name, "n = 0, nothing else")
    assert bytes(st) == bytes(8)


def test_python_wrappers_validate_and_raise_without_a_device():
    with pytest.raises(ValueError):
        engine.g1_check_batch(bytes(96 * 2), 3)
    with pytest.raises(ValueError):
        engine.g2_check_batch(bytes(192 * 2), 2, in_inf=[0])
    with pytest.raises(ValueError):
        engine.g1_check_batch_jac(bytes(96), 1)                               # in-memory G1 points are 144 bytes
    with pytest.raises(ValueError):
        engine.check_batch_dev("g2", 8, 8, 1, 8, jac=True)                    # the in-memory form takes no flags
    with pytest.raises(engine.BlsmiError):
        engine.g2_check_batch(bytes(192), 1, check=3)                         # what the library refuses reaches the caller as an error
    assert engine.g1_check_batch(b"", 0).shape == (0,) and engine.g2_check_batch_jac(b"", 0, check=2).shape == (0,)   # n = 0: no device needed
    import torch
    if torch.cuda.is_available():
        return
    g1 = K.affine_cases(1)[0]
    g2j = K.jacobian_cases(2)[0]
    for call in (lambda: engine.g1_check_batch(g1.rec, 1), lambda: engine.g2_check_batch_jac(g2j.rec.tobytes(), 1),
                 lambda: engine.check_batch_dev("g1", 4096, 0, 1, 8192),
                 lambda: g1pubs.ValidatePublicKeys([g1pubs.NewPublicKeyFromG1(g1.rec)]),
                 lambda: g2pubs.ValidatePublicKeys([g2pubs.NewPublicKeyFromG2Projective(g2j.rec.tobytes())]),
                 lambda: g2pubs.ValidateSignatures([g2pubs.NewSignatureFromG1(g1.rec)])):
        with pytest.raises(engine.BlsmiError):
            call()
    assert g1pubs.ValidateSignatures([]) == [] and g2pubs.ValidatePublicKeys([]) == []
