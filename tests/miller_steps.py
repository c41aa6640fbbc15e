"""The homogeneous Miller-loop steps of the device (bls_amd/csrc/pairing_body.inc: doubling_step_h_i, addition_step_h), restated on
oracle.pyref's Fq2 arithmetic.  An independent statement for the tests: written from the formulas, not from the level-program generator.

On E': y^2 = x^3 + b', b' = 4 xi (xi = 1 + u), a point (X, Y, Z) stands for (X/Z, Y/Z).
  doubling:  A = XY, B = Y^2, E = 3 b' Z^2 = 12 xi Z^2, H = 2YZ, F = 3E, G = B + F
             X3 = 2A (B - F), Y3 = G^2 - 12 E^2, Z3 = 4BH;           line (o0, o1, o2) = (H, -3X^2, B - E)
  addition of the affine Q = (xq, yq):  th = Y - yq Z, la = X - xq Z, C = th^2, D = la^2, E = la D, F = Z C, G = X D, Hh = E + F - 2G
             X3 = la Hh, Y3 = th (G - Hh) - E Y, Z3 = Z E;           line (o0, o1, o2) = (la, -th, th xq - la yq)
The line at P = (xP, yP) is the sparse Fq12 element (c0, c1, c4) = (o2, o1 xP, o0 yP) (pairing.go:28-39)."""
import numpy as np

from oracle import pyref as P

add, sub, mul, sqr, neg, dbl = P.fq2_add, P.fq2_sub, P.fq2_mul, P.fq2_sqr, P.fq2_neg, P.fq2_dbl


def _muls(a, k):
    return (a[0] * k % P.Q, a[1] * k % P.Q)


def doubling_step(r):
    X, Y, Z = r
    A, B, X2 = mul(X, Y), sqr(Y), sqr(X)
    H = dbl(mul(Y, Z))
    E = _muls(P.fq2_mul_nr(sqr(Z)), 12)
    F = _muls(E, 3)
    G = add(B, F)
    nr = (dbl(mul(A, sub(B, F))), sub(sqr(G), _muls(sqr(E), 12)), _muls(mul(B, H), 4))
    return nr, (H, neg(_muls(X2, 3)), sub(B, E))


def addition_step(r, q):
    X, Y, Z = r
    xq, yq = q
    th, la = sub(Y, mul(yq, Z)), sub(X, mul(xq, Z))
    C, D = sqr(th), sqr(la)
    E = mul(la, D)
    F, G = mul(Z, C), mul(X, D)
    Hh = sub(add(E, F), dbl(G))
    nr = (mul(la, Hh), sub(mul(th, sub(G, Hh)), mul(E, Y)), mul(Z, E))
    return nr, (la, neg(th), sub(mul(th, xq), mul(la, yq)))


def line_at(o, p):
    """(c0, c1, c4) of the line o at P"""
    return o[2], P.fq2_mul_fq(o[1], p[0]), P.fq2_mul_fq(o[0], p[1])


def step_record(kind, vals):
    """kind "dbl" / "add" on a 12-value record (X, Y, Z, xq, yq: Fq2 each; xP, yP) of field elements -> the 12 output values
    (X3, Y3, Z3, c0, c1, c4), in k_debug_row's record layout"""
    f2 = [(vals[2 * j], vals[2 * j + 1]) for j in range(5)]
    r, q, p = f2[0:3], (f2[3], f2[4]), (vals[10], vals[11])
    nr, o = doubling_step(r) if kind == "dbl" else addition_step(r, q)
    return [c for e in tuple(nr) + line_at(o, p) for c in e]


def step_records(kind, recs):
    """step_record on an array of 12-Fq device records (6 x u64 Montgomery(2^384) limbs per Fq) -> the expected output records"""
    rows = []
    for r in recs:
        vals = [P.from_mont(P.from_limbs64(r[6 * i:6 * i + 6])) for i in range(12)]
        rows.append([w for v in step_record(kind, vals) for w in P.limbs64(P.to_mont(v))])
    return np.array(rows, dtype=np.uint64)


def miller_loop(p, q):
    """one (P, Q) pair through the homogeneous steps in the device's order (quad_body.inc: miller_loop_q): a Miller value with the
    reference's final exponentiation"""
    r = (q[0], q[1], P.FQ2_ONE)
    f = P.FQ12_ONE
    xr = P.BLS_X >> 1
    for i in range(61, -1, -1):
        r, o = doubling_step(r)
        f = P.fq12_mul_by_014(f, *line_at(o, p))
        if (xr >> i) & 1:
            r, o = addition_step(r, q)
            f = P.fq12_mul_by_014(f, *line_at(o, p))
        f = P.fq12_sqr(f)
    r, o = doubling_step(r)
    f = P.fq12_mul_by_014(f, *line_at(o, p))
    return P.fq12_conj(f)
