"""A limb-exact model of the latency path's multiply cores (bls_amd/csrc/gen_lat_mul.py -> lat_mul.inc: lat_mul, lat_sqr3) and operand gather.

Python integers do not overflow, so every intermediate the hardware holds in a 32- or 64-bit register is range-checked here and `Overflow`
is raised the moment one leaves its type: a gathered limb and the 3a / 6a operands of the squaring (int32), the column accumulator after
every multiply-add (int64, v_mad_i64_i32).  Columns and terms run in the order gen_lat_mul.py emits them.  No GPU."""
from oracle import pyref as P

Q = P.Q
NL, LB = 15, 27
MASK = (1 << LB) - 1
QL = [(Q >> (LB * i)) & MASK for i in range(NL)]
QINV = (-pow(Q, -1, 1 << LB)) % (1 << LB)        # m = acc * QINV mod 2^27 makes acc + m q_0 divisible by 2^27 (BLSMI_QINV, low 27 bits)
R = 1 << (NL * LB)


class Overflow(ArithmeticError):
    pass


def _fit(v, bits, what):
    if not -(1 << (bits - 1)) <= v < (1 << (bits - 1)):
        raise Overflow("%s = %d leaves int%d" % (what, v, bits))
    return v


def value(limbs):
    return sum(int(l) << (LB * i) for i, l in enumerate(limbs))


def gather(terms):
    """sum c * S over [(c, limbs)]: k_lat.hip's gather keeps the low 32 bits of every limb sum"""
    return [_fit(sum(c * s[i] for c, s in terms), 32, "gathered limb %d" % i) for i in range(NL)]


class _Acc:
    def __init__(self, exact_operands=False):
        self.v = 0
        self.peak = 0
        self.exact_operands = exact_operands

    def mad(self, x, y, what):
        if not self.exact_operands:
            _fit(x, 32, what + " operand"); _fit(y, 32, what + " operand")
        self.v = _fit(self.v + x * y, 64, "accumulator after " + what)
        self.peak = max(self.peak, abs(self.v))


def _columns(a_terms, exact_operands=False):
    """the Montgomery columns: a_terms(k) = the operand products of column k, in order"""
    acc, m, r = _Acc(exact_operands), [0] * NL, [0] * NL
    for k in range(2 * NL - 1):
        for x, y, what in a_terms(k):
            acc.mad(x, y, "%s (column %d)" % (what, k))
        if k < NL:
            for i in range(k):
                acc.mad(m[i], QL[k - i], "m[%d] q[%d]" % (i, k - i))
            m[k] = ((acc.v & 0xffffffff) * QINV) & MASK
            acc.mad(m[k], QL[0], "m[%d] q[0]" % k)
            assert acc.v & MASK == 0
        else:
            for i in range(k - NL + 1, NL):
                acc.mad(m[i], QL[k - i], "m[%d] q[%d]" % (i, k - i))
            r[k - NL] = acc.v & MASK
        acc.v >>= LB
    r[NL - 1] = _fit(acc.v, 32, "top limb")
    return r, acc.peak


def lat_mul(a, b):
    """-> (the 15 result limbs, the accumulator's peak magnitude); value(result) = a b / 2^405 mod q"""
    def terms(k):
        lo, hi = (0, k) if k < NL else (k - NL + 1, NL - 1)
        return [(a[i], b[k - i], "a[%d] b[%d]" % (i, k - i)) for i in range(lo, hi + 1)]
    return _columns(terms)


def lat_sqr3(a, wrap6=True):
    """3 a^2 / 2^405 mod q as lat_sqr3 computes it: cross products once against 6a, the diagonal against 3a; 3a and 6a are int32.
    wrap6=False: 6a kept exact -- the product without the int32 store of 6a (the accumulator is still checked)"""
    a3 = [_fit(3 * x, 32, "3 a[%d]" % i) for i, x in enumerate(a)]
    a6 = [_fit(6 * x, 32, "6 a[%d]" % i) if wrap6 else 6 * x for i, x in enumerate(a)]

    def terms(k):
        lo, hi = (0, k) if k < NL else (k - NL + 1, NL - 1)
        t = [(a[i], a6[k - i], "a[%d] 6a[%d]" % (i, k - i)) for i in range(lo, hi + 1) if 2 * i < k]
        if k % 2 == 0:
            t.append((a[k // 2], a3[k // 2], "a[%d] 3a[%d]" % (k // 2, k // 2)))
        return t
    return _columns(terms, exact_operands=not wrap6)
