#!/usr/bin/env python3
"""Find a cyclotomic element of Fq12 whose compressed form has z2 = 0 and z3 != 0, and its 2^16-th root: the operand with which
tests/test_gpu_inv_pair.py sends the Karabina decompression (tower_body.inc: cyc_z1_fraction) down its z2 = 0 branch after a run of
sixteen compressed squarings.  Prints tests/cyc_z2_zero.py.

Write f = A + B s + C s^2 over Fq4 = Fq2[t] / (t^2 - xi), s^3 = t, with A = (z0, z1), B = (z2, z3), C = (z4, z5) (the record holds them
as c0 = (z0, z4, z3), c1 = (z2, z1, z5)).  The elements of order dividing q^4 - q^2 + 1 satisfy (Granger-Scott; bar = conjugation of
Fq4 over Fq2)
    t B C = A^2 - bar A        A B = t C^2 + bar B        A C = B^2 - bar C
(which is what turns f^2 into 3 A^2 - 2 bar A, 3 t C^2 + 2 bar B, 3 B^2 - 2 bar C).  With z2 = 0, B = z3 t and bar B = -B; eliminating
A = (B^2 - bar C) / C from the second relation leaves  B^3 + B (C - bar C) = t C^3, i.e. for z5 != 0
    z3 = (3 z4^2 + xi z5^2) / 2        xi z3^3 = z4^3 + 3 xi z4 z5^2,
a sextic in z4 for a chosen z5.  Its roots in Fq2 are found by gcd with X^(q^2) - X and equal-degree splitting."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pyref as P  # noqa: E402

Q = P.Q
XI = (1, 1)
mul, add, sub, sqr, inv = P.fq2_mul, P.fq2_add, P.fq2_sub, P.fq2_sqr, P.fq2_inv
ZERO, ONE = (0, 0), (1, 0)


def k(n):
    return (n % Q, 0)


# ---- polynomials over Fq2, lowest degree first -----------------------------------------------------------------------------------
def trim(p):
    while p and p[-1] == ZERO:
        p = p[:-1]
    return p


def pmul(a, b):
    r = [ZERO] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            r[i + j] = add(r[i + j], mul(x, y))
    return trim(r)


def pmod(a, f):
    a = list(a)
    li = inv(f[-1])
    while len(a) >= len(f):
        c = mul(a[-1], li)
        off = len(a) - len(f)
        for i, y in enumerate(f):
            a[off + i] = sub(a[off + i], mul(c, y))
        a = trim(a[:-1])
    return trim(a)


def psub(a, b):
    n = max(len(a), len(b))
    a, b = list(a) + [ZERO] * (n - len(a)), list(b) + [ZERO] * (n - len(b))
    return trim([sub(x, y) for x, y in zip(a, b)])


def ppow(a, e, f):
    r = [ONE]
    for bit in bin(e)[2:]:
        r = pmod(pmul(r, r), f)
        if bit == "1":
            r = pmod(pmul(r, a), f)
    return r


def pgcd(a, b):
    while b:
        a, b = b, pmod(a, b)
    return [mul(x, inv(a[-1])) for x in a]


def roots(f, xs):
    """the roots of f in Fq2"""
    g = pgcd(f, psub(ppow([ZERO, ONE], Q * Q, f), [ZERO, ONE]))
    out, todo = [], [g]
    while todo:
        h = todo.pop()
        if len(h) == 1:
            continue
        if len(h) == 2:
            out.append(P.fq2_neg(h[0]))
            continue
        d = (P.rand_int(xs, Q), P.rand_int(xs, Q))
        w = pgcd(h, psub(ppow([d, ONE], (Q * Q - 1) // 2, h), [ONE]))
        if 1 < len(w) < len(h):
            quo, rem = [], list(h)
            while len(rem) >= len(w):                                   # h / w
                c = rem[-1]; quo.insert(0, c)
                off = len(rem) - len(w)
                for i, y in enumerate(w):
                    rem[off + i] = sub(rem[off + i], mul(c, y))
                rem = rem[:-1]
            todo += [w, trim(quo)]
        else:
            todo.append(h)
    return out


# ---- Fq4 = Fq2[t] / (t^2 - xi) ----------------------------------------------------------------------------------------------------
def mul4(a, b):
    return (add(mul(a[0], b[0]), mul(XI, mul(a[1], b[1]))), add(mul(a[0], b[1]), mul(a[1], b[0])))


def inv4(a):
    n = inv(sub(sqr(a[0]), mul(XI, sqr(a[1]))))
    return (mul(a[0], n), P.fq2_neg(mul(a[1], n)))


def bar4(a):
    return (a[0], P.fq2_neg(a[1]))


def main():
    xs = P.XORShift(20260)
    while True:
        z5 = (P.rand_int(xs, Q), P.rand_int(xs, Q))
        e = mul(XI, sqr(z5))                                             # xi z5^2
        half = inv(k(2))
        z3p = [mul(e, half), ZERO, mul(k(3), half)]                      # z3 as a polynomial in z4
        f = psub(pmul([XI], pmul(z3p, pmul(z3p, z3p))), [ZERO, mul(k(3), e), ZERO, ONE])
        for z4 in roots(f, xs):
            z3 = mul(add(mul(k(3), sqr(z4)), e), half)
            if z3 == ZERO:
                continue
            B, C = (ZERO, z3), (z4, z5)
            A = mul4(sub4(mul4(B, B), bar4(C)), inv4(C))
            if mul4((ZERO, ONE), mul4(B, C)) != sub4(mul4(A, A), bar4(A)):
                continue
            g = ((A[0], z4, z3), (ZERO, A[1], z5))
            n = Q ** 4 - Q ** 2 + 1
            if P.fq12_pow(g, n) != P.FQ12_ONE:
                continue
            x = P.fq12_pow(g, pow(1 << 16, -1, n))
            y = x
            for _ in range(16):
                y = P.fq12_sqr(y)
            assert y == g
            print('"""A cyclotomic element of Fq12 whose 2^16-th power has z2 = c1.c0 = 0 and z3 = c0.c2 != 0 (tools/gen_cyc_z2_zero.py): normal-form\n'
                  'coefficients in record order c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1."""')
            print("X_Z2_ZERO = (")
            for v in P.fq12_flat(x):
                print("    0x%096x," % v)
            print(")")
            return


def sub4(a, b):
    return (sub(a[0], b[0]), sub(a[1], b[1]))


if __name__ == "__main__":
    main()
