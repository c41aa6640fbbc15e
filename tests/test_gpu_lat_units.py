"""-m gpu: every job kind of the latency path (k_lat.hip) at the bounds its program generator admits, on worst-case limb patterns.

The unit programs (bls_amd/csrc/gen_lat.py: UNIT_PROGRAMS, run through blsmi_debug_lat_unit) hold single MUL / SQR / LIN / INV jobs with the
largest limb and value bounds, term counts and coefficients the builder emits; the tuples (tests/lat_units.py, tests/lat_operands.py) put every
limb of every operand at its bound -- all plus, x side against y side, alternating -- and values within eps of +-q, then walk the whole corpus
through every input.  One tuple is one wave; every n is odd.  Expected values are Python integers from the job table (lat_units.evaluate).

What an output must satisfy, by job kind (fp.cuh: fp_mul_body, fp_norm, fp_reduce, FpS):
  MUL / SQR         value = the formula mod q, limbs 0..13 in [0, 2^27), value strictly inside (-0.41 q, 1.41 q)
  un-reduced LIN    the INTEGER value sum c_i value(a_i), limbs 0..13 in [-16, 2^27 + 16)
  reduced LIN       value = the formula mod q, inside (-1.01 q, 2.01 q), limbs 0..13 in [0, 2^27)
  INV               value = x^-1 R^2 mod q (0 for 0), inside the storage contract: |limb| <= 2^27 + 64, |value| <= 256 q
  verdicts          1 exactly for the tuples that represent (1, 0, ..., 0) (check1; 1 = R mod q in this representation) / all zeros (iszero)"""
import numpy as np
import pytest

import lat_operands as O
import lat_units as U

pytestmark = pytest.mark.gpu

Q = U.Q
LIMB = 1 << 27


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    return engine


def _run(eng, name):
    t = U.tuples(name)
    assert len(t) % 2 == 1 and len(t) <= 513
    out, ok = eng.debug_lat_unit(U.which(name), np.array(t, dtype=np.int32), U.nout(name))
    return t, out, ok


@pytest.mark.parametrize("name", [n for n in U.G.UNIT_PROGRAMS if n not in ("unit_check1", "unit_iszero")])
def test_unit_program(eng, name):
    p = U.program(name)
    t, out, _ = _run(eng, name)
    assert out.shape == (len(t), len(p.out_nodes), 15)
    bad, seen = [], set()
    for ti, tup in enumerate(t):
        want = U.evaluate(p, [O.value(e) for e in tup])
        for e, (cls, mod, exact) in enumerate(want):
            limbs = [int(x) for x in out[ti, e]]
            v = O.value(limbs)
            seen.add(cls)
            if cls == "prod":
                good = v % Q == mod and all(0 <= l < LIMB for l in limbs[:14]) and -41 * Q < 100 * v < 141 * Q
            elif cls == "lin":
                assert exact is not None, "an un-reduced LIN output must have an exact expectation"
                good = v == exact and all(-16 <= l < LIMB + 16 for l in limbs[:14])
            elif cls == "red":
                good = v % Q == mod and -101 * Q < 100 * v < 201 * Q and all(0 <= l < LIMB for l in limbs[:14])
            else:
                assert cls == "inv"
                good = v % Q == mod and all(abs(l) <= O.BOUND for l in limbs) and abs(v) <= 256 * Q
            if not good:
                bad.append((ti, e, cls))
    assert not bad, (name, len(bad), bad[:12])
    assert seen == {"unit_lin4": {"lin"}, "unit_inv": {"inv"}}.get(name, {"prod"} if name.startswith(("unit_mul", "unit_sqr")) else {"red"})


@pytest.mark.parametrize("name", ["unit_check1", "unit_iszero"])
def test_verdict_program(eng, name):
    t, _, ok = _run(eng, name)
    vals = [[O.value(e) % Q for e in tup] for tup in t]
    if name == "unit_check1":
        want = [int(v[0] == O.ONE and not any(v[1:])) for v in vals]
    else:
        want = [int(not any(v)) for v in vals]
    assert 10 <= sum(want) <= len(want) - 10                               # both verdicts are well represented
    bad = [i for i, (g, w) in enumerate(zip(ok, want)) if int(g) != w]
    assert not bad, (name, bad[:12])


def test_argument_checks(eng):
    """unknown program, wrong input count, n == 0: the library's argument error, before any launch"""
    import ctypes as C
    lib = eng._lib()
    a = np.zeros((1, 16, 15), dtype=np.int32); o = np.zeros((12, 15, 1), dtype=np.int32); k = np.zeros(1, dtype=np.uint8)
    i32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    call = lambda w, nin, n: lib.blsmi_debug_lat_unit(C.c_int(w), a.ctypes.data_as(i32p), C.c_size_t(nin), C.c_size_t(n), o.ctypes.data_as(i32p), k.ctypes.data_as(u8p))
    assert call(len(U.G.UNIT_PROGRAMS), 16, 1) == -3 and call(-1, 16, 1) == -3
    assert call(0, 15, 1) == -3 and call(0, 16, 0) == -3
    assert call(0, 16, 1) == 0
