"""-m gpu: the lane-pair Fq2 inverse (fp2_pair.inc: fp_inv_pair_core, one safegcd split over the two lanes of a pair), bit-exact
against the C oracle, through the debug-op entry (FQ2_INV in the lane-pair layout), and the two places of the Karabina decompression
that feed the inversion from elsewhere (tower_body.inc: cyc_z1_fraction): z2 = 0 and the unit.

What the split can get wrong is an exchange between the lanes: a lane that steps the divsteps on another pair's low limbs, takes the
wrong column of the transition matrix, or applies it to the wrong half of the state.  The operands therefore differ from pair to pair
-- a small value beside a full-size one -- and the tuple counts put a lone pair, a ragged last wave, exactly one wave (32 pairs)
and one pair in a second workgroup on the device."""
import numpy as np
import pytest

from gpu_common import P, RC

pytestmark = pytest.mark.gpu

Q = P.Q
COUNTS = (1, 31, 32, 33, 65)
R28 = 1 << 392                                            # the lane-pair kernels hold x * 2^392 mod q in 14 x 28-bit limbs


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    return engine


def rec2(a):
    """the Fq2 value (c0, c1) as a debug-op record"""
    return np.array(P.limbs64(P.to_mont(a[0] % Q)) + P.limbs64(P.to_mont(a[1] % Q)), dtype=np.uint64)


def with_norm(n, xs):
    """an Fq2 element of norm n: a random c0, c1 a root of n - c0^2 (half of the c0 have one)"""
    while True:
        c0 = P.rand_int(xs, Q)
        c1 = P.fq_sqrt((n - c0 * c0) % Q)
        if c1 is not None and c1 * c1 % Q == (n - c0 * c0) % Q:
            return (c0, c1)


def special_values(xs):
    """the issue's list; the device inverts the NORM c0^2 + c1^2, as the residue g = norm * 2^392 mod q"""
    half = (Q + 1) // 2
    v = [(0, 0), (1, 0), (0, 1), (1, 1), (Q - 1, 0), (0, Q - 1), (2, 0), (half, 0)]
    v += [(0, P.rand_int(xs, Q)), (P.rand_int(xs, Q), 0), (0, 3), (5, 0)]              # c0 = 0 / c1 = 0: a wrong partner route shows
    v += [with_norm(1, xs), with_norm(Q - 1, xs)]
    # a sparse low word of g: the divsteps see long runs of even g (whole batches of them when the low limbs vanish)
    inv_r = pow(R28, -1, Q)
    for g in (1 << 28, 1 << 56, 1 << 200, 1 << 380, 3 << 84, (P.rand_int(xs, 1 << 300) | 1) << 64, ((1 << 28) - 1) << 28,
              (P.rand_int(xs, 1 << 350) << 29) | 1, (1 << 28) + 1):
        v.append(with_norm(g * inv_r % Q, xs))
    return v


@pytest.fixture(scope="module")
def corpus():
    """(records, expected): the specials, then 1 024 seeded random elements, ordered so that neighbouring pairs differ in size -- every
    other random element is a small integer (c0, c1 < 2^16 .. 2^64) -- with the oracle's inverse of each, computed once"""
    xs = P.XORShift(4201)
    vals = special_values(xs)
    for i in range(1024):
        if i % 2:
            bits = 16 + 8 * (i // 2 % 7)
            vals.append((P.rand_int(xs, 1 << bits), P.rand_int(xs, 1 << bits)))
        else:
            vals.append((P.rand_int(xs, Q), P.rand_int(xs, Q)))
    a = np.stack([rec2(x) for x in vals])
    want = np.stack([RC.fq2_inverse(x)[1] for x in a])
    assert not want[0].any() and np.array_equal(want[7], rec2((2, 0)))                 # inverse(0) = 0, inverse((q+1)/2) = 2
    a.setflags(write=False); want.setflags(write=False)
    return a, want, len(vals) - 1024


def _bad(got, want):
    return [i for i in range(len(want)) if not np.array_equal(got[i], want[i])]


def test_whole_corpus_in_one_call(eng, corpus):
    a, want, _ = corpus
    got, _ = eng.debug_op("FQ2_INV", a, lane_pair=True)
    bad = _bad(got, want)
    assert not bad, (bad[:8], len(bad))


@pytest.mark.parametrize("n", COUNTS)
def test_tuple_counts(eng, corpus, n):
    """n tuples from three places of the corpus: the specials first, specials running into random elements, random elements alone"""
    a, want, _ = corpus
    for start in (0, 12, 40 + n):
        got, _ = eng.debug_op("FQ2_INV", a[start:start + n], lane_pair=True)
        bad = _bad(got, want[start:start + n])
        assert not bad, (n, start, bad[:8], len(bad))


def test_each_special_beside_a_different_neighbour(eng, corpus):
    """every special value once on each side of a full-size random element: (x, r, x, r ...) and (r, x, r, x ...)"""
    a, want, ns = corpus
    r = ns + 2 * np.arange(ns)                            # the full-size random elements: even offsets after the specials
    for order in ((np.arange(ns), r), (r, np.arange(ns))):
        idx = np.stack(order, axis=1).reshape(-1)
        got, _ = eng.debug_op("FQ2_INV", a[idx], lane_pair=True)
        bad = _bad(got, want[idx])
        assert not bad, (bad[:8], len(bad))


# ---- the Karabina decompression's other two sources of a denominator -----------------------------------------------------------
# A cyclotomic element x (normal-form coefficients, record order c0.c0 .. c1.c2) whose 2^16-th power has z2 = c1.c0 = 0 and
# z3 = c0.c2 != 0: cyc_z1_fraction then takes z1 = 2 z4 z5 / z3 (n_alt) and inverts z3.  Found with tools/gen_cyc_z2_zero.py; the test
# checks the properties it relies on with the oracle before it uses the element.
from cyc_z2_zero import X_Z2_ZERO  # noqa: E402


def rec12(vals):
    return np.array([w for v in vals for w in P.limbs64(P.to_mont(v % Q))], dtype=np.uint64)


ONE12 = rec12([1] + [0] * 11)


def _run16(x):
    for _ in range(16):
        x = RC.fq12_sqr(x)
    return x


@pytest.fixture(scope="module")
def cyc_cases():
    """33 records: the z2 = 0 element and the unit alternating with random cyclotomic elements; what 16 squarings and the final
    exponentiation make of each, from the oracle"""
    import edge_operands as E
    x0 = rec12(X_Z2_ZERO)
    y0 = _run16(x0)
    assert not y0[36:48].any() and y0[24:36].any() and y0[60:72].any() and y0[12:24].any()          # z2 = 0; z3, z5, z4 != 0
    conj = x0.copy().reshape(12, 6)
    for k in range(6, 12):
        conj[k] = RC.fq_neg(conj[k])
    assert np.array_equal(RC.fq12_mul(x0, conj.reshape(-1)), ONE12)                                 # x^(q^6 + 1) = 1
    assert np.array_equal(RC.fq12_mul(RC.fq12_frobenius(x0, 4), x0), RC.fq12_frobenius(x0, 2))      # x^(q^4 - q^2 + 1) = 1
    rnd = E.cyclotomic_records(P.XORShift(4301), 16)[1:]
    x = np.stack([(x0, ONE12, rnd[i // 3])[i % 3] for i in range(33)])
    run = np.stack([_run16(r) for r in x])
    fe = np.stack([RC.final_exponentiation(r)[1] for r in x])
    return x, run, fe


@pytest.mark.parametrize("layout", ["pair", "quad"])
def test_decompression_with_z2_zero_and_on_the_unit(eng, cyc_cases, layout):
    """the compressed 16-squaring run (decompression: one inversion) at n = 33.  Inside the final exponentiation the runs start from
    whatever the easy part leaves, so only the unit can be steered into its special branch there: the final exponentiation of the same
    33 records covers that (one maps to one through five runs on the unit) and the z2 = 0 element as an ordinary operand."""
    x, run, fe = cyc_cases
    kw = {"lane_pair": True} if layout == "pair" else {"lane_quad": True}
    got, _ = eng.debug_op("FQ12_CYCLO_RUN16", x, **kw)
    bad = _bad(got, run)
    assert not bad, ("run16", layout, bad[:8], len(bad))
    got, _ = eng.debug_op("FQ12_FINAL_EXP", x, **kw)
    bad = _bad(got, fe)
    assert not bad, ("final_exp", layout, bad[:8], len(bad))
    assert all(np.array_equal(got[i], ONE12) for i in range(33) if i % 3 == 1)
