"""-m gpu: the tower, Miller-step and final-exponentiation code of every layout at its edges, bit-exact against the C oracle or the Python
statement of the homogeneous steps (tests/miller_steps.py).

Operands come from tests/edge_operands.py: extremes of the reference encoding and of the device residue in both limb builds, tower
elements with extreme, one-hot, monomial and Fq6-subfield coefficients, cyclotomic elements, then random ones.  Every n is odd, so the
last workgroup of each layout (64 / 32 / 16 / 4 tuples) is ragged."""
import numpy as np
import pytest

import edge_operands as E
import miller_steps as M
from gpu_common import P, RC

pytestmark = pytest.mark.gpu

LAYOUTS = ("plain", "pair", "quad", "row")
_KW = {"plain": {}, "pair": {"lane_pair": True}, "quad": {"lane_quad": True}, "row": {"lane_row": True}}
# which debug ops each layout runs (include/blsmi.h: BLSMI_OP_LANE_*)
FQ_OPS = {"plain": ("FQ_MUL", "FQ_SQR", "FQ_ADD", "FQ_SUB", "FQ_NEG", "FQ_DBL", "FQ_INV")}
FQ2_OPS = {"plain": ("FQ2_MUL", "FQ2_SQR", "FQ2_INV", "FQ2_MUL_NR"), "pair": ("FQ2_MUL", "FQ2_SQR", "FQ2_INV", "FQ2_MUL_NR")}
FQ6_OPS = {k: ("FQ6_MUL", "FQ6_SQR", "FQ6_INV", "FQ6_FROB1", "FQ6_MUL_BY_1", "FQ6_MUL_BY_01") for k in ("plain", "pair")}
_FQ12_BASE = ("FQ12_MUL", "FQ12_SQR", "FQ12_INV", "FQ12_FROB1", "FQ12_FROB2", "FQ12_FROB3", "FQ12_MUL_BY_014")
FQ12_OPS = {"plain": _FQ12_BASE + ("FQ12_MUL_BY_LINE_PAIR",), "pair": _FQ12_BASE + ("FQ12_MUL_BY_LINE_PAIR",), "quad": _FQ12_BASE, "row": _FQ12_BASE}
RUN16_LAYOUTS = ("plain", "pair", "quad")


def _fq2(fn):
    return lambda x, y: fn(x)


REF = {
    "FQ_MUL": RC.fq_mul, "FQ_SQR": _fq2(RC.fq_sqr), "FQ_ADD": RC.fq_add, "FQ_SUB": RC.fq_sub, "FQ_NEG": _fq2(RC.fq_neg), "FQ_DBL": _fq2(RC.fq_dbl),
    "FQ_INV": lambda x, y: RC.fq_inverse(x)[1],
    "FQ2_MUL": RC.fq2_mul, "FQ2_SQR": _fq2(RC.fq2_sqr), "FQ2_INV": lambda x, y: RC.fq2_inverse(x)[1], "FQ2_MUL_NR": _fq2(RC.fq2_mul_nr),
    "FQ6_MUL": RC.fq6_mul, "FQ6_SQR": _fq2(RC.fq6_sqr), "FQ6_INV": lambda x, y: RC.fq6_inverse(x)[1], "FQ6_FROB1": lambda x, y: RC.fq6_frobenius(x, 1),
    "FQ6_MUL_BY_1": lambda x, y: RC.fq6_mul_by_1(x, y[:12]), "FQ6_MUL_BY_01": lambda x, y: RC.fq6_mul_by_01(x, y[:12], y[12:24]),
    "FQ12_MUL": RC.fq12_mul, "FQ12_SQR": _fq2(RC.fq12_sqr), "FQ12_INV": lambda x, y: RC.fq12_inverse(x)[1],
    "FQ12_FROB1": lambda x, y: RC.fq12_frobenius(x, 1), "FQ12_FROB2": lambda x, y: RC.fq12_frobenius(x, 2), "FQ12_FROB3": lambda x, y: RC.fq12_frobenius(x, 3),
    "FQ12_MUL_BY_014": lambda x, y: RC.fq12_mul_by_014(x, y[0:12], y[12:24], y[24:36]),
    "FQ12_MUL_BY_LINE_PAIR": lambda x, y: RC.fq12_mul_by_014(RC.fq12_mul_by_014(x, y[0:12], y[12:24], y[24:36]), y[36:48], y[48:60], y[60:72]),
}
UNARY = {"FQ_SQR", "FQ_NEG", "FQ_DBL", "FQ_INV", "FQ2_SQR", "FQ2_INV", "FQ2_MUL_NR", "FQ6_SQR", "FQ6_INV", "FQ6_FROB1",
         "FQ12_SQR", "FQ12_INV", "FQ12_FROB1", "FQ12_FROB2", "FQ12_FROB3"}


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    yield engine
    engine.set_latency_threshold(8192); engine.set_quad_threshold(16384); engine.set_row_threshold(*engine.ROW_DEFAULT)


def _odd(a, xs, width):
    """the corpus, plus random records up to an odd count"""
    extra = 9 if len(a) % 2 == 0 else 8
    return np.concatenate([a, E.rand_records(xs, extra, width)])


def _check(eng, name, layout, a, b):
    out, _ = eng.debug_op(name, a, None if name in UNARY else b, **_KW[layout])
    want = np.stack([REF[name](x, y) for x, y in zip(a, b if b is not None else a)])
    bad = [i for i in range(len(a)) if not np.array_equal(out[i], want[i])]
    assert not bad, (name, layout, bad[:8], len(bad))


# ---- operands solved for with the oracle so that an op's RESULT is a chosen record (edge_operands.NEAR_Q_EPS: every value q - eps) ----
_INV = {2: lambda x: RC.fq2_inverse(x)[1], 6: lambda x: RC.fq6_inverse(x)[1], 12: lambda x: RC.fq12_inverse(x)[1]}
_MUL = {2: RC.fq2_mul, 6: RC.fq6_mul, 12: RC.fq12_mul}
_FROB_ORDER = {"FQ6_FROB1": (6, 1), "FQ12_FROB1": (12, 1), "FQ12_FROB2": (12, 2), "FQ12_FROB3": (12, 3)}
_XI = np.concatenate([E.rec([E.MONT_ONE]), E.rec([E.MONT_ONE])])      # 1 + u


def _sparse(name, y):
    """the operand b of a sparse product as a full element (what the op multiplies by)"""
    one = E.rec([E.MONT_ONE] + [0] * 11)
    z = np.zeros(12, dtype=np.uint64)
    if name == "FQ6_MUL_BY_1":
        return np.concatenate([z, y[:12], z])
    if name == "FQ6_MUL_BY_01":
        return np.concatenate([y[:24], z])
    l1 = RC.fq12_mul_by_014(one, y[0:12], y[12:24], y[24:36])
    return l1 if name == "FQ12_MUL_BY_014" else RC.fq12_mul_by_014(l1, y[36:48], y[48:60], y[60:72])


def targeted(name, width, xs, n):
    """(a, b) with op(a, b) = edge_operands.near_q_records(n, width), or None for ops that cannot be inverted this way (squarings)"""
    y = E.near_q_records(n, width)
    b = E.rand_records(xs, n, width)
    if name in ("FQ_MUL", "FQ2_MUL", "FQ6_MUL", "FQ12_MUL"):
        inv = (lambda x: RC.fq_inverse(x)[1]) if width == 1 else _INV[width]
        mul = RC.fq_mul if width == 1 else _MUL[width]
        a = np.stack([mul(t, inv(u)) for t, u in zip(y, b)])
    elif name in ("FQ_INV", "FQ2_INV", "FQ6_INV", "FQ12_INV"):
        a = np.stack([(RC.fq_inverse(t)[1] if width == 1 else _INV[width](t)) for t in y])
    elif name in _FROB_ORDER:
        order, k = _FROB_ORDER[name]
        fro = RC.fq6_frobenius if width == 6 else RC.fq12_frobenius
        a = np.stack([fro(t, order - k) for t in y])
    elif name == "FQ2_MUL_NR":
        a = np.stack([RC.fq2_mul(t, _INV[2](_XI)) for t in y])
    elif name in ("FQ6_MUL_BY_1", "FQ6_MUL_BY_01", "FQ12_MUL_BY_014", "FQ12_MUL_BY_LINE_PAIR"):
        a = np.stack([_MUL[width](t, _INV[width](_sparse(name, u))) for t, u in zip(y, b)])
    elif name == "FQ_ADD":
        a = np.stack([RC.fq_sub(t, u) for t, u in zip(y, b)])
    elif name == "FQ_SUB":
        a = np.stack([RC.fq_add(t, u) for t, u in zip(y, b)])
    elif name == "FQ_NEG":
        a = np.stack([RC.fq_neg(t) for t in y])
    elif name == "FQ_DBL":
        a = np.stack([RC.fq_mul(t, RC.fq_inverse(E.rec([P.to_mont(2)]))[1]) for t in y])
    else:
        return None
    return a, b


def test_fq_ops_on_every_edge_pair(eng):
    """the single-lane Fq ops (k_wire.hip, the 28-bit build) on every pair of corpus values, both orders"""
    vals = E.fq_values()
    a = E.recs([[x] for x in vals for _ in vals])
    b = E.recs([[y] for _ in vals for y in vals])
    a, b = np.concatenate([a, a[:1]]), np.concatenate([b, b[:1]])     # odd n
    for name in FQ_OPS["plain"]:
        _check(eng, name, "plain", a if name not in UNARY else a[::len(vals)], b if name not in UNARY else b[::len(vals)])
    _, flag = eng.debug_op("FQ_INV", a[::len(vals)])
    assert [bool(f) for f in flag] == [bool(RC.fq_inverse(x)[0]) for x in a[::len(vals)]]
    xs = P.XORShift(9001)
    for name in FQ_OPS["plain"]:
        t = targeted(name, 1, xs, 25)
        if t is not None:
            _check(eng, name, "plain", *t)


def test_fq_sqrt_cmp_parity_on_edge_values(eng):
    """the single-lane ops that answer with a flag: square roots, comparison and parity on the corpus values, their squares and their
    negations -- flags and roots as the oracle's (FQ2_SQRT_ANY: either root)"""
    vals = E.fq_values()
    sq = [RC.fq_sqr(E.rec([v])) for v in vals]
    a = np.concatenate([E.recs([[v] for v in vals]), np.stack(sq), E.recs([[(P.Q - v) % P.Q] for v in vals])])
    if len(a) % 2 == 0:
        a = np.concatenate([a, a[:1]])
    out, ok = eng.debug_op("FQ_SQRT", a)
    for i, x in enumerate(a):
        r, e = RC.fq_sqrt(x)
        assert bool(ok[i]) == bool(r), i
        if r:
            assert np.array_equal(out[i], e), i
    _, flag = eng.debug_op("FQ_PARITY", a, raw_flag=True)
    assert list(flag) == [int(RC.fq_parity(x)) for x in a]
    b = a[::-1].copy()
    b[::7] = a[::7]                                                    # equal operands too
    _, flag = eng.debug_op("FQ_CMP", a, b, raw_flag=True)
    assert [int(f) - 1 for f in flag] == [RC.fq_cmp(x, y) for x, y in zip(a, b)]
    xs = P.XORShift(9002)
    a2 = _odd(E.tower_records(2, xs), xs, 2)
    a2 = np.concatenate([a2, np.stack([RC.fq2_sqr(x) for x in a2])[:-1]])
    _, flag = eng.debug_op("FQ2_PARITY", a2)
    assert list(flag) == [RC.fq2_parity(x) for x in a2]
    out, ok = eng.debug_op("FQ2_SQRT", a2)
    for i, x in enumerate(a2):
        r, e = RC.fq2_sqrt(x)
        assert bool(ok[i]) == bool(r), i
        if r:
            assert np.array_equal(out[i], e), i
    out, ok = eng.debug_op("FQ2_SQRT_ANY", a2)
    for i, x in enumerate(a2):
        r, e = RC.fq2_sqrt(x)
        assert bool(ok[i]) == bool(r), i
        if r:
            assert np.array_equal(out[i], e) or np.array_equal(out[i], RC.fq2_neg(e)), i


TOWER_CASES = [(layout, width, table) for width, table in ((2, FQ2_OPS), (6, FQ6_OPS), (12, FQ12_OPS)) for layout in LAYOUTS if layout in table]


@pytest.mark.parametrize("layout,width,table", TOWER_CASES, ids=["%s-fq%d" % (c[0], c[1]) for c in TOWER_CASES])
def test_tower_ops_on_edge_operands(eng, layout, width, table):
    """every Fq2 / Fq6 / Fq12 debug op a layout runs, on the corpus against itself reversed and against random operands"""
    xs = P.XORShift(9100 + width)
    a = _odd(E.tower_records(width, xs), xs, width)
    r = E.rand_records(xs, len(a), width)
    for name in table[layout]:
        for b in (a[::-1].copy(), r):
            _check(eng, name, layout, a, b)
            if name not in UNARY:
                _check(eng, name, layout, b, a)                   # the edge operand on the other side
        t = targeted(name, width, xs, 25)                           # results at q - eps (edge_operands.NEAR_Q_EPS)
        if t is not None:
            _check(eng, name, layout, *t)


def test_cyclotomic_ops_on_edge_operands(eng):
    """CYCLO_SQR on every layout and the compressed 16-squaring run on the layouts that have it, on the unit and cyclotomic elements"""
    xs = P.XORShift(9201)
    cyc = E.cyclotomic_records(xs, 12)                             # 13: odd
    sq = np.stack([RC.fq12_sqr(x) for x in cyc])
    run = cyc
    for _ in range(16):
        run = np.stack([RC.fq12_sqr(x) for x in run])
    for layout in LAYOUTS:
        out, _ = eng.debug_op("FQ12_CYCLO_SQR", cyc, **_KW[layout])
        assert np.array_equal(out, sq), layout
    for layout in RUN16_LAYOUTS:
        out, _ = eng.debug_op("FQ12_CYCLO_RUN16", cyc, **_KW[layout])
        assert np.array_equal(out, run), layout


def test_inverse_of_zero_on_every_layout(eng):
    """zero has no inverse: the oracle reports it (flag 0) and leaves zero; every layout must give zero, and the single-lane Fq / Fq2
    ops, which report a flag, must report it"""
    for name, width, layouts in (("FQ_INV", 1, ("plain",)), ("FQ2_INV", 2, ("plain", "pair")), ("FQ6_INV", 6, ("plain", "pair")),
                                 ("FQ12_INV", 12, LAYOUTS)):
        z = np.zeros((3, 6 * width), dtype=np.uint64)
        ok, want = {1: RC.fq_inverse, 2: RC.fq2_inverse, 6: RC.fq6_inverse, 12: RC.fq12_inverse}[width](z[0])
        assert ok == 0 and not want.any()
        for layout in layouts:
            out, flag = eng.debug_op(name, z, **_KW[layout])
            assert not out.any(), (name, layout)
            if width <= 2 and layout == "plain":
                assert not flag.any(), name


# ---- Miller-loop steps -------------------------------------------------------------------------------------------------------
STEP_LAYOUTS = (("row", "", {"lane_row": True}), ("row", "_REF", {"lane_row": True}), ("pair", "", {"lane_pair": True}), ("quad", "", {"lane_quad": True}))


@pytest.mark.parametrize("layout,suffix,kw", STEP_LAYOUTS, ids=["row", "row_ref", "pair", "quad"])
def test_miller_steps_against_the_python_statement(eng, layout, suffix, kw):
    """one doubling and one mixed-addition step (X, Y, Z, xq, yq, xP, yP) -> (X3, Y3, Z3, c0, c1, c4) of each layout's own step routine,
    on corpus records (any field elements do: the formulas are polynomial) and random records"""
    xs = P.XORShift(9301)
    recs = _odd(E.tower_records(12, xs), xs, 12)
    for kind, op in (("dbl", "ROW_DBL_STEP"), ("add", "ROW_ADD_STEP")):
        got, _ = eng.debug_op(op + suffix, recs, **kw)
        want = M.step_records(kind, recs)
        bad = [i for i in range(len(recs)) if not np.array_equal(got[i], want[i])]
        assert not bad, (op + suffix, layout, bad[:8], len(bad))


def test_step_ops_outside_their_layouts_are_refused(eng):
    for name, kw in (("ROW_DBL_STEP", {}), ("ROW_DBL_STEP_REF", {"lane_pair": True}), ("ROW_ADD_STEP_REF", {"lane_quad": True}),
                     ("FQ12_FINAL_EXP", {}), ("FQ12_FINAL_EXP", {"lane_row": True}), ("FQ12_FINAL_EXP", {"lane_pair": True, "lane_quad": True}),
                     ("ROW_DBL_STEP", {"lane_pair": True, "lane_row": True})):
        with pytest.raises(eng.BlsmiError):
            eng.debug_op(name, np.zeros((1, 72), dtype=np.uint64), **kw)


# ---- final exponentiation ----------------------------------------------------------------------------------------------------
def _final_exp_all(eng, x):
    """the final exponentiation of every record on the five kernels: wave (k_lat), row, single lane, pair and quad"""
    out = {}
    try:
        eng.set_row_threshold(0, 0); eng.set_latency_threshold(1 << 20)
        out["wave"] = eng.final_exponentiation_batch(x)
        eng.set_row_threshold(1, 1 << 20)
        out["row"] = eng.final_exponentiation_batch(x)
        eng.set_row_threshold(0, 0); eng.set_latency_threshold(0)
        out["single"] = eng.final_exponentiation_batch(x)
    finally:
        eng.set_latency_threshold(8192); eng.set_quad_threshold(16384); eng.set_row_threshold(*eng.ROW_DEFAULT)
    out["pair"] = eng.debug_op("FQ12_FINAL_EXP", x, lane_pair=True)[0]
    out["quad"] = eng.debug_op("FQ12_FINAL_EXP", x, lane_quad=True)[0]
    return out


ONE = E.rec([E.MONT_ONE] + [0] * 11)


def test_final_exponentiation_on_edge_elements(eng):
    """one, monomials c w^k and Fq6-subfield elements map to exactly one; extreme-coefficient and random elements match the oracle;
    zero (no result in the reference: pairing.go:83) gives zero on all five kernels (include/blsmi.h)"""
    xs = P.XORShift(9401)
    trivial = E.recs([[E.MONT_ONE] + [0] * 11] + E.monomial_rows(xs) + E.subfield_rows(xs))
    extreme = E.recs([r for r in E.tower_rows(12) if any(r)])
    x = np.concatenate([np.zeros((1, 72), dtype=np.uint64), trivial, extreme, E.rand_records(xs, 6, 12)])
    if len(x) % 2 == 0:
        x = x[:-1]
    want = []
    for r in x:
        ok, f = RC.final_exponentiation(r)
        assert ok == (1 if r.any() else 0)
        want.append(f)
    want = np.stack(want)
    assert not want[0].any()
    assert all(np.array_equal(w, ONE) for w in want[1:1 + len(trivial)])
    for kernel, got in _final_exp_all(eng, x).items():
        bad = [i for i in range(len(x)) if not np.array_equal(got[i], want[i])]
        assert not bad, (kernel, bad[:8], len(bad))


def test_fq12_product_with_edge_factors(eng):
    """blsmi_fq12_product over corpus factors (odd count), and with a zero factor"""
    xs = P.XORShift(9501)
    f = _odd(E.recs([r for r in E.tower_rows(12, xs) if any(r)]), xs, 12)
    want = f[0]
    for y in f[1:]:
        want = RC.fq12_mul(want, y)
    assert np.array_equal(eng.fq12_product(f), want)
    g = f.copy(); g[len(g) // 2] = 0
    assert not eng.fq12_product(g).any()
