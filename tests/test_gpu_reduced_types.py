"""-m gpu: the pairing kernels after their Fq12 values moved to the reduced type (csrc/fp.cuh: FpR / FpW), and fp_reduce itself.

The lane-pair kernels (two lanes per tuple, 32 tuples per workgroup) are the ones the reduced type changes; the single-lane kernels share
the tower's source and keep the storage type (27-bit limbs).  Everything is compared bit for bit with the C oracle, the value-reduction
chain with Python integers.  References are computed once per module and sliced."""
import numpy as np
import pytest

import edge_operands as E
from gpu_common import P, RC, mont, rand_g1, rand_g2, sk_bytes, unmont

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 31, 32, 33, 65)            # 32: one workgroup's tile of the lane-pair kernels; 33 and 65 cross a tile with a partial tail
NMAX = max(SIZES)


def _defaults(engine):
    engine.set_latency_threshold(8192); engine.set_quad_threshold(16384); engine.set_row_threshold(*engine.ROW_DEFAULT)


def _pair_layout(engine):
    """every size through the lane-pair kernels (k_miller1h_pair / k_miller1_pair / k_final_exp_pair)"""
    engine.set_latency_threshold(0); engine.set_quad_threshold(0); engine.set_row_threshold(0, 0)


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    _pair_layout(engine)
    yield engine
    _defaults(engine)


@pytest.fixture(scope="module")
def pairs():
    """NMAX seeded (P, Q) pairs with the oracle's Miller values and pairings, computed once: a batch of n is the first n"""
    xs = P.XORShift(7100)
    g1 = [rand_g1(xs) for _ in range(NMAX)]
    g2 = [rand_g2(xs) for _ in range(NMAX)]
    want = RC.pairing_batch(b"".join(g1), b"".join(g2), NMAX)
    ml = np.stack([RC.miller_loop(a, b, 1) for a, b in zip(g1[:33], g2[:33])])
    return g1, g2, want, ml


@pytest.mark.parametrize("n", SIZES)
def test_pairing_batch_lane_pair_sizes(eng, pairs, n):
    g1, g2, want, _ = pairs
    got = eng.pairing_batch(b"".join(g1[:n]), b"".join(g2[:n]), n)
    bad = [i for i in range(n) if not np.array_equal(got[i], want[i])]
    assert not bad, (n, bad[:8], len(bad))


def test_miller_loop_and_final_exponentiation_at_33(eng, pairs):
    """MillerLoop runs the reference's own steps (k_miller1_pair) and must give the reference's Miller value itself; the final
    exponentiation of those values must give the pairings"""
    g1, g2, want, ml = pairs
    n = 33
    got = eng.miller_loop_batch(b"".join(g1[:n]), b"".join(g2[:n]), n)
    bad = [i for i in range(n) if not np.array_equal(got[i], ml[i])]
    assert not bad, ("miller_loop", bad[:8], len(bad))
    fe = eng.final_exponentiation_batch(ml)
    bad = [i for i in range(n) if not np.array_equal(fe[i], want[i])]
    assert not bad, ("final_exponentiation", bad[:8], len(bad))


@pytest.mark.parametrize("group", ["g2pubs", "g1pubs"])
def test_verify_batch_at_33(eng, group):
    """33 tuples per package, every third one spoiled (wrong message / wrong key in turn): verdicts as constructed and as the oracle's"""
    import bls_amd.g1pubs as g1p
    import bls_amd.g2pubs as g2p
    n = 33
    xs = P.XORShift(7200 if group == "g2pubs" else 7201)
    o = RC.g2pubs if group == "g2pubs" else RC.g1pubs
    mod = g2p if group == "g2pubs" else g1p
    mk_pk = mod.NewPublicKeyFromG2 if group == "g2pubs" else mod.NewPublicKeyFromG1
    mk_sig = mod.NewSignatureFromG1 if group == "g2pubs" else mod.NewSignatureFromG2
    msgs, pks, sigs, expect = [], [], [], []
    for i in range(n):
        sk = sk_bytes(xs)
        m = b"reduced types %d" % i
        pk, sig = o.priv_to_pub(sk), o.sign(m, sk)
        if i % 3 == 2:
            if (i // 3) % 2:
                m += b"!"
            else:
                pk = o.priv_to_pub(sk_bytes(xs))
        msgs.append(m); pks.append(pk); sigs.append(sig); expect.append(i % 3 != 2)
    assert [o.verify(m, p, s) for m, p, s in zip(msgs, pks, sigs)] == expect
    assert mod.VerifyBatch(msgs, [mk_pk(p) for p in pks], [mk_sig(s) for s in sigs]) == expect


# ---- the debug field ops on edge coefficients -------------------------------------------------------------------------------------
EDGE_COEFFS = (1, E.Q - 1, (E.Q - 1) // 2)


@pytest.fixture(scope="module")
def fq12_edges(kats):
    """Fq12 records: zero, then one non-zero coefficient at a time -- 1, q - 1, (q - 1) / 2 at each of the twelve places -- the same
    values at all twelve places, and the reference's pairing KAT; odd count"""
    rows = [[0] * 12]
    for v in EDGE_COEFFS:
        rows += [[v if j == k else 0 for j in range(12)] for k in range(12)]
        rows.append([v] * 12)
    rows.append([P.to_mont(int(v)) for v in kats["pairing_g1gen_g2gen"]])
    assert len(rows) % 2 == 1
    return E.recs(rows)


@pytest.fixture(scope="module")
def fq12_refs(fq12_edges):
    x = fq12_edges
    y = x[::-1].copy()
    inv = np.stack([RC.fq12_inverse(r)[1] for r in x])
    nz = x[[i for i in range(len(x)) if RC.fq12_inverse(x[i])[0]]]
    cyc = np.concatenate([E.cyclotomic(nz), x[-1:]])                     # the cyclotomic image of every invertible edge element, and the KAT (a pairing)
    if len(cyc) % 2 == 0:
        cyc = cyc[1:]
    fe = []
    for r in x:
        ok, f = RC.final_exponentiation(r)
        fe.append(f if ok else np.zeros(72, dtype=np.uint64))
    return {"y": y, "mul": np.stack([RC.fq12_mul(a, b) for a, b in zip(x, y)]), "sqr": np.stack([RC.fq12_sqr(a) for a in x]), "inv": inv,
            "cyc": cyc, "cyc_sqr": np.stack([RC.fq12_sqr(a) for a in cyc]), "fe": np.stack(fe)}


def _same(got, want, what):
    bad = [i for i in range(len(want)) if not np.array_equal(got[i], want[i])]
    assert not bad, (what, bad[:8], len(bad))


@pytest.mark.parametrize("layout", ["pair", "single"])
def test_fq12_debug_ops_on_edge_coefficients(eng, fq12_edges, fq12_refs, layout):
    kw = {"lane_pair": True} if layout == "pair" else {}
    x, r = fq12_edges, fq12_refs
    _same(eng.debug_op("FQ12_MUL", x, r["y"], **kw)[0], r["mul"], ("mul", layout))
    _same(eng.debug_op("FQ12_MUL", r["y"], x, **kw)[0], r["mul"], ("mul swapped", layout))
    _same(eng.debug_op("FQ12_SQR", x, **kw)[0], r["sqr"], ("sqr", layout))
    _same(eng.debug_op("FQ12_INV", x, **kw)[0], r["inv"], ("inv", layout))
    _same(eng.debug_op("FQ12_CYCLO_SQR", r["cyc"], **kw)[0], r["cyc_sqr"], ("cyclotomic sqr", layout))
    if layout == "pair":
        _same(eng.debug_op("FQ12_FINAL_EXP", x, lane_pair=True)[0], r["fe"], ("final exp", layout))
    else:
        try:
            eng.set_row_threshold(0, 0); eng.set_latency_threshold(0); eng.set_quad_threshold(16384)   # k_final_exp (one tuple per lane)
            _same(eng.final_exponentiation_batch(x), r["fe"], ("final exp", layout))
        finally:
            _pair_layout(eng)


# ---- fp_reduce at the bounds of the lazy type ------------------------------------------------------------------------------------
def test_value_reduction_chain_against_python_integers(eng):
    """FQ_LAZY builds 1029 ab + 4a and 4b - 1029 ab out of un-normalised multiples (limbs at seven times the limb size, values near
    +-1 500 q: three quarters of what the type admits), value-reduces both and multiplies them.  Operands: every pair of the edge
    corpus, then small multiples of q - 1 and of (q - 1) / 2 as 384-bit words (a record may exceed q), which push the Montgomery
    products to both ends of their range."""
    vals = E.fq_values()
    big = [k * (E.Q - 1) for k in range(2, 10)] + [k * ((E.Q - 1) // 2) for k in (3, 5, 19)] + [(1 << 384) - 1]
    assert all(v < 1 << 384 for v in big)
    av = [x for x in vals for _ in vals] + [x for x in big for _ in big] + [vals[i % len(vals)] for i in range(len(big))] + [0]
    bv = [y for _ in vals for y in vals] + [y for _ in big for y in big] + big + [0]
    if len(av) % 2 == 0:
        av, bv = av[:-1], bv[:-1]

    def raw(v):
        return np.array([(v >> (64 * i)) & ((1 << 64) - 1) for i in range(6)], dtype=np.uint64)
    a, b = np.stack([raw(v) for v in av]), np.stack([raw(v) for v in bv])
    got, _ = eng.debug_op("FQ_LAZY", a, b)
    bad = []
    for i, (x, y) in enumerate(zip(av, bv)):
        X, Y = P.from_mont(x % E.Q), P.from_mont(y % E.Q)
        p = X * Y % E.Q
        want = (1029 * p + 4 * X) * (4 * Y - 1029 * p) % E.Q
        if unmont(got[i]) != want or not np.array_equal(got[i], mont(want)):
            bad.append(i)
    assert not bad, (bad[:8], len(bad))
