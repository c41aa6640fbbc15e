"""CPU only: the Python statement of the homogeneous Miller-loop steps (tests/miller_steps.py), which the GPU edge tests hold the
kernels to, anchored to oracle.pyref's group law and pairing."""
from oracle import pyref as P

import miller_steps as M


def _affine(r):
    zi = P.fq2_inv(r[2])
    return P.fq2_mul(r[0], zi), P.fq2_mul(r[1], zi)


def _g2_points(xs, n):
    return [P.jac_to_affine(P.F2, P.affine_mul(P.F2, P.G2_GEN, P.rand_fr(xs))) for _ in range(n)]


def _scaled(a, xs):
    """affine point -> homogeneous (l x, l y, l) with a random l in Fq2*"""
    lam = (P.rand_int(xs, P.Q - 1) + 1, P.rand_int(xs, P.Q))
    return P.fq2_mul(a[0], lam), P.fq2_mul(a[1], lam), lam


def test_steps_follow_the_group_law_on_the_twist():
    """(X3/Z3, Y3/Z3) is 2T for a doubling and T+Q for an addition, from any homogeneous representative of T"""
    xs = P.XORShift(8801)
    pts = _g2_points(xs, 4)
    for a, b in zip(pts, pts[1:] + pts[:1]):
        t = _scaled(a, xs)
        two = P.jac_to_affine(P.F2, P.jac_double(P.F2, P.to_jac(P.F2, a)))
        nr, _ = M.doubling_step(t)
        assert P.g2_on_curve(_affine(nr)) and _affine(nr) == two
        tq = P.jac_to_affine(P.F2, P.jac_add_affine(P.F2, P.to_jac(P.F2, a), b))
        nr, _ = M.addition_step(t, b)
        assert _affine(nr) == tq


def test_homogeneous_miller_loop_gives_the_reference_pairing():
    """a Miller loop built from the statement's lines, then the reference's final exponentiation, equals pyref.pairing (the
    generators, and one random pair)"""
    xs = P.XORShift(8802)
    p = P.jac_to_affine(P.F1, P.affine_mul(P.F1, P.G1_GEN, P.rand_fr(xs)))
    q = P.jac_to_affine(P.F2, P.affine_mul(P.F2, P.G2_GEN, P.rand_fr(xs)))
    for a, b in ((P.G1_GEN, P.G2_GEN), (p, q)):
        assert P.final_exponentiation(M.miller_loop(a, b)) == P.pairing(a, b)
