"""Edge operands for the group law: pairs of Jacobian points that send jac_add / jac_add_affine (curve.cuh) down their rare branches.

The additions branch on h = U2 - U1 and rr0 = S2 - S1 (U = X Z'^2, S = Y Z'^3, Z' the OTHER operand's Z): h == 0 and rr0 == 0 is the same
point (doubling), h == 0 alone is a pair of opposite points (infinity), Z == 0 an infinite operand.  Over Fq2 "zero" is a statement about
two coefficients, which the lane-pair layout holds on two lanes: a pair of G2 points whose x agree in ONE coefficient, or whose h is zero
and whose rr0 is zero in one coefficient, is where a wrong vote between the lanes shows.  Random points never get there.  The classes:

  same / opposite   (P z1, +-P z2), z1 != z2, over many z: the forms of zero a lazily reduced h can take depend on the operands
  inf_*             Z = 0 on the left, on the right, on both sides: (X, Y, 0) with X, Y non-zero, and (0, 1, 0)
  d_c0 / d_c1       G2: two points of E' whose x agree in c0 (c1) only; affine, and under Z1, Z2 with (Z1 Z2)^2 in Fq, so that h itself is
                    zero in exactly that coefficient;  d_c0_x / d_c1_x: the same points under unrelated Z (h is then full; the x are what agree)
  e_y_c0 / e_y_c1   G2, crafted records (not curve points: the formulas are polynomial): h == 0 and rr0 zero in c0 (c1) only
  e_x_c0 / e_x_c1   G2, crafted records: h zero in c0 (c1) only
  generic           no special case at all (padding to an odd count)

Points are tuples of integers, (X, Y, Z) with each coordinate an integer (G1) or a pair (G2); record() makes the 18 / 36 x u64 Montgomery
limbs blsmi_debug_op and the *_jac entry points read.  Everything is seeded with P.XORShift: the same corpus in every process.  No GPU."""
import functools
from collections import namedtuple

import numpy as np

import edge_operands as E
from gpu_common import P, RC, rand_g1, rand_g2

Q = P.Q
FIELD = {1: P.F1, 2: P.F2}
WIDTH = {1: 18, 2: 36}
PB = {1: 96, 2: 192}
SAME_OPPOSITE_MIN = 200                  # pairs of each of the two classes, at least
PARTIAL_MIN = 16                         # pairs / records of each partial-zero kind, at least

# p, q: Jacobian operands; pa, qa: the affine points they stand for (None: infinity), or NOT_A_POINT for the crafted records
Pair = namedtuple("Pair", "label p q pa qa")
NOT_A_POINT = "crafted"


# ---- representation ------------------------------------------------------------------------------------------------------------------
def coeffs(group, v):
    return (v,) if group == 1 else tuple(v)


def record(group, jac):
    """(X, Y, Z) -> one uint64 record of Montgomery limbs"""
    return np.array([w for c in jac for v in coeffs(group, c) for w in P.limbs64(P.to_mont(v % Q))], dtype=np.uint64)


def unrecord(group, rec):
    v = [P.from_mont(P.from_limbs64([int(w) for w in rec[6 * i:6 * i + 6]])) for i in range(WIDTH[group] // 6)]
    return tuple(v) if group == 1 else ((v[0], v[1]), (v[2], v[3]), (v[4], v[5]))


def records(group, jacs):
    return np.stack([record(group, j) for j in jacs])


def wire(group, a):
    """affine point -> wire bytes (None stays None)"""
    return None if a is None else (P.g1_serialize(a) if group == 1 else P.g2_serialize(a))


def unwire(group, w):
    if w is None:
        return None
    c = [int.from_bytes(w[48 * i:48 * i + 48], "big") for i in range(len(w) // 48)]
    return (c[0], c[1]) if group == 1 else ((c[0], c[1]), (c[2], c[3]))


def scale(group, a, z):
    """the representative (x z^2, y z^3, z) of the affine point a"""
    F = FIELD[group]
    z2 = F.sqr(z)
    return (F.mul(a[0], z2), F.mul(a[1], F.mul(z2, z)), z)


def neg(group, a):
    return P.affine_neg(FIELD[group], a)


def on_curve(group, a):
    return P.g1_on_curve(a) if group == 1 else P.g2_on_curve(a)


def h_rr0(group, p, q):
    """(h, rr0) of the addition p + q, with big integers"""
    F = FIELD[group]
    z1z1, z2z2 = F.sqr(p[2]), F.sqr(q[2])
    u1, u2 = F.mul(p[0], z2z2), F.mul(q[0], z1z1)
    s1, s2 = F.mul(F.mul(p[1], q[2]), z2z2), F.mul(F.mul(q[1], p[2]), z1z1)
    return F.sub(u2, u1), F.sub(s2, s1)


# ---- Z values ------------------------------------------------------------------------------------------------------------------------
def fq_z_values():
    """non-zero z: the extremes, then every z whose RECORD is an edge value of edge_operands.fq_values() (the reference encoding's extremes and
    the device-residue edges of both limb builds)"""
    vals = [1, 2, Q - 1, (Q - 1) // 2, (Q + 1) // 2] + [P.from_mont(v) for v in E.fq_values() if v % Q]
    seen, out = set(), []
    for v in vals:
        if v not in seen:
            seen.add(v); out.append(v)
    return out


def z_values(group, xs, n):
    """at least n z values of the group's field, every special value among them; G2: pairs of the Fq set, some with one coefficient zero"""
    base = fq_z_values()
    if group == 1:
        return base + [P.rand_int(xs, Q - 1) + 1 for _ in range(max(0, n - len(base)))]
    m = len(base)
    out = [(base[i], base[(5 * i + 2) % m]) for i in range(m)]
    out += [(v, 0) for v in base[:12]] + [(0, v) for v in base[:12]]
    return out + [(P.rand_int(xs, Q - 1) + 1, P.rand_int(xs, Q)) for _ in range(max(0, n - len(out)))]


def rand_z(group, xs):
    return P.rand_int(xs, Q - 1) + 1 if group == 1 else (P.rand_int(xs, Q - 1) + 1, P.rand_int(xs, Q))


# ---- points --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def subgroup_points(group, n=8, seed=7001):
    xs = P.XORShift(seed + group)
    return tuple(unwire(group, (rand_g1 if group == 1 else rand_g2)(xs)) for _ in range(n))


@functools.lru_cache(maxsize=None)
def outside_points(group, n=6):
    """curve points outside the prime-order subgroup, by the scan of tests/test_gpu_round3.py::_torsion_points"""
    out, x = [], 0
    while len(out) < n:
        pt = P.g1_from_x(x, bool(x & 1)) if group == 1 else P.g2_from_x((x % 7, x // 7 + 1), bool(x & 1))
        if pt is not None and not (P.g1_in_subgroup(pt) if group == 1 else P.g2_in_subgroup(pt)):
            out.append(pt)
        x += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def x_zero_points(group):
    """G1: (0, 2) and (0, -2).  G2: points with x.c0 == 0 and with x.c1 == 0"""
    if group == 1:
        return (P.g1_from_x(0, False), P.g1_from_x(0, True))
    return g2_scan(0, None, 3) + g2_scan(None, 0, 3)


CURVE_ORDER = {1: P.G1_COFACTOR * P.R_ORDER, 2: P.G2_COFACTOR * P.R_ORDER}          # #E(Fq), #E'(Fq2)
LOW_ORDERS = {1: (3, 11), 2: (13, 23)}                                             # small primes that divide the cofactors (11^2, 13^2, 23^2 do too)


@functools.lru_cache(maxsize=None)
def low_order_point(group, ell, seed=7100):
    """a curve point of order exactly ell (a prime factor of the cofactor), by the Python oracle's double-and-add: a seeded curve point
    times #E / ell^v (ell^v the whole power of ell in #E) has order ell^j; while its multiple by ell is finite, take that instead.  The
    seed's stream is drawn from until the first multiple is finite.  (Not [#E / ell] Q: the 11-part of E(Fq) is Z/11 x Z/11 -- the curve
    has all of E[11] over Fq -- so #E / 11 = 11 (...) kills every point.)"""
    assert CURVE_ORDER[group] % ell == 0
    xs = P.XORShift(seed + 100 * group + ell)
    F = FIELD[group]
    m = CURVE_ORDER[group]
    while m % ell == 0:
        m //= ell
    while True:
        x = P.rand_int(xs, Q) if group == 1 else (P.rand_int(xs, Q), P.rand_int(xs, Q))
        pt = P.g1_from_x(x, False) if group == 1 else P.g2_from_x(x, False)
        low = None if pt is None else P.jac_to_affine(F, P.affine_mul(F, pt, m))
        while low is not None:
            up = P.jac_to_affine(F, P.affine_mul(F, low, ell))
            if up is None:
                return low
            low = up


def g2_scan(a, b, n, start=1):
    """n points of E' with x = (a, t) (b None) or x = (t, b) (a None), t scanned upwards from `start`"""
    out, t = [], start
    while len(out) < n:
        pt = P.g2_from_x((a, t) if b is None else (t, b), bool(len(out) & 1))
        if pt is not None:
            out.append(pt)
        t += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def partial_pools():
    """{"c0": points of E' with the same x.c0 (12345, and 0), "c1": points with the same x.c1 (777, and 0)}: every two of one pool are a class-d pair"""
    return {"c0": (g2_scan(12345, None, 7), g2_scan(0, None, 3)), "c1": (g2_scan(None, 777, 7), g2_scan(None, 0, 3))}


def partial_pairs(kind):
    return [(pool[i], pool[j]) for pool in partial_pools()[kind] for i in range(len(pool)) for j in range(i + 1, len(pool))]


def base_points(group):
    return subgroup_points(group) + outside_points(group) + x_zero_points(group)


def infinities(group, xs):
    """Z = 0 records: X, Y arbitrary and non-zero (twice), and (0, 1, 0)"""
    F = FIELD[group]
    return [(rand_z(group, xs), rand_z(group, xs), F.zero) for _ in range(2)] + [(F.zero, F.one, F.zero)]


# ---- the classes ---------------------------------------------------------------------------------------------------------------------
def same_and_opposite(group, xs):
    pts = base_points(group)
    zs = z_values(group, xs, SAME_OPPOSITE_MIN + 1)
    out = []
    for i in range(max(SAME_OPPOSITE_MIN + 1, len(zs))):
        a = pts[i % len(pts)]
        z1, z2 = zs[i % len(zs)], zs[(3 * i + 1) % len(zs)]
        if z1 == z2:
            z2 = rand_z(group, xs)
        out.append(Pair("same", scale(group, a, z1), scale(group, a, z2), a, a))
        out.append(Pair("opposite", scale(group, a, z1), scale(group, neg(group, a), z2), a, neg(group, a)))
    return out


def infinite_operands(group, xs):
    pts = base_points(group)
    out = []
    for k, inf in enumerate(infinities(group, xs)):
        for j in range(3):
            a = pts[(3 * k + j) % len(pts)]
            fin = scale(group, a, FIELD[group].one if j == 0 else rand_z(group, xs))
            out += [Pair("inf_left", inf, fin, None, a), Pair("inf_right", fin, inf, a, None)]
        for other in infinities(group, xs):
            out.append(Pair("inf_both", inf, other, None, None))
    return out


def partial_zero_points(xs):
    """class d (G2): each pair affine, under Z1, Z2 = conj(Z1) t (t in Fq: (Z1 Z2)^2 lies in Fq and h keeps its zero coefficient), under real Z,
    and under unrelated Z"""
    out = []
    one = P.FQ2_ONE
    for kind in ("c0", "c1"):
        for k, (a, b) in enumerate(partial_pairs(kind)):
            if k & 1:
                b = neg(2, b)                                            # the y of either sign: x is what the class is about
            z1 = rand_z(2, xs); t = P.rand_int(xs, Q - 1) + 1
            z2 = P.fq2_mul_fq(P.fq2_conj(z1), t)
            r1, r2 = (P.rand_int(xs, Q - 1) + 1, 0), ((0, P.rand_int(xs, Q - 1) + 1) if k & 2 else (P.rand_int(xs, Q - 1) + 1, 0))
            out.append(Pair("d_" + kind, scale(2, a, one), scale(2, b, one), a, b))
            out.append(Pair("d_" + kind, scale(2, a, z1), scale(2, b, z2), a, b))
            out.append(Pair("d_" + kind, scale(2, a, r1), scale(2, b, r2), a, b))
            out.append(Pair("d_" + kind + "_x", scale(2, a, rand_z(2, xs)), scale(2, b, rand_z(2, xs)), a, b))
    return out


def crafted_records(xs):
    """class e (G2): with U1 = X1 Z2^2 and S1 = Y1 Z2^3, the second operand is X2 = (U1 + dx) / Z1^2, Y2 = (S1 + dy) / Z1^3 (Y2 arbitrary for
    the e_x kinds): h = dx and rr0 = dy exactly, for Z1 = Z2 = 1 and for general Z1, Z2"""
    F = P.F2
    out = []
    cs = [1, Q - 1, 2, (Q - 1) // 2]
    for kind in ("e_y_c0", "e_y_c1", "e_x_c0", "e_x_c1"):
        for i in range(2 * PARTIAL_MIN):
            c = cs[i % 8] if i % 8 < len(cs) else P.rand_int(xs, Q - 1) + 1
            d = (0, c) if kind.endswith("c0") else (c, 0)               # zero in c0 only / in c1 only
            z1, z2 = (P.FQ2_ONE, P.FQ2_ONE) if i < PARTIAL_MIN else (rand_z(2, xs), rand_z(2, xs))
            x1, y1 = (P.rand_int(xs, Q), P.rand_int(xs, Q)), (P.rand_int(xs, Q), P.rand_int(xs, Q))
            z1z1, z2z2 = F.sqr(z1), F.sqr(z2)
            u1, s1 = F.mul(x1, z2z2), F.mul(y1, F.mul(z2z2, z2))
            iz2, iz3 = F.inv(z1z1), F.inv(F.mul(z1z1, z1))
            if kind.startswith("e_y"):
                x2, y2 = F.mul(u1, iz2), F.mul(F.add(s1, d), iz3)
            else:
                x2, y2 = F.mul(F.add(u1, d), iz2), (P.rand_int(xs, Q), P.rand_int(xs, Q))
            out.append(Pair(kind, (x1, y1, z1), (x2, y2, z2), NOT_A_POINT, NOT_A_POINT))
    return out


def generic_pairs(group, xs, n):
    pts = base_points(group)
    out = []
    for i in range(n):
        a, b = pts[(len(pts) - 1 - i) % len(pts)], pts[(i + 3) % len(pts)]     # (the x = 0 points first)
        if a == b or a == neg(group, b):
            b = pts[(i + 4) % len(pts)]
        out.append(Pair("generic", scale(group, a, rand_z(group, xs)), scale(group, b, rand_z(group, xs)), a, b))
    return out


@functools.lru_cache(maxsize=None)
def corpus(group):
    """every pair of the group, an odd number of them"""
    xs = P.XORShift(9100 + group)
    out = same_and_opposite(group, xs) + infinite_operands(group, xs)
    if group == 2:
        out += partial_zero_points(xs) + crafted_records(xs)
    out += generic_pairs(group, xs, 9 if len(out) % 2 == 0 else 8)
    assert len(out) % 2 == 1 and len(out) > 64
    return tuple(out)


@functools.lru_cache(maxsize=None)
def doubling_operands(group):
    """(labels, points): every first operand of the same-point, class-d and class-e pairs (the x = 0 points are among the first), every
    infinity, padded to an odd count"""
    xs = P.XORShift(9200 + group)
    ops = [(c.label, c.p) for c in corpus(group) if c.label == "same" or c.label.startswith(("d_", "e_"))]
    ops += [("inf", p) for p in infinities(group, xs)]
    if len(ops) % 2 == 0:
        ops.append(("generic", scale(group, base_points(group)[0], rand_z(group, xs))))
    assert len(ops) % 2 == 1 and len(ops) > 64
    return tuple(l for l, _ in ops), tuple(p for _, p in ops)


# ---- tables and segments for the segmented sums --------------------------------------------------------------------------------------
SumCase = namedtuple("SumCase", "table inf jtab segs labels")


@functools.lru_cache(maxsize=None)
def sum_case(group):
    """One point table and the segments over it.  table: wire records (an infinite entry is a real point's record with its flag set, or the
    all-zero record, flag set as well: the oracle reads flags only); jtab: the same points as in-memory records under differing Z, infinity
    as Z = 0.  Segments: [P, Q] for every corpus pair that has affine operands; [P, -P, R], [P, P, R], [R, P, -P], [inf, P, P]; and long
    ones in which the exceptional pair arises between PARTIAL sums: A ++ A, A ++ -A, A ++ -A ++ [R], A and a rotation of A (of -A) interleaved
    (the wave tree's last level then adds equal / opposite sums of 32), A ++ [sum A] and A ++ [-sum A] (++ [R]) (a running sum meets its own
    value: the mixed addition with Z != 1), |A| in {2, 32, 33}."""
    xs = P.XORShift(9300 + group)
    F = FIELD[group]
    table, inf, jtab, index = [], [], [], {}
    zs = z_values(group, xs, 0)

    def entry(a, flagged=False):
        """index of the table entry for the affine point a (None: the all-zero record; flagged: a's record with the infinity flag)"""
        key = (a, flagged)
        if key not in index:
            k = len(table)
            index[key] = k
            table.append(bytes(PB[group]) if a is None else wire(group, a))
            inf.append(1 if a is None or flagged else 0)
            z = zs[(7 * k + 1) % len(zs)]
            j = (rand_z(group, xs), rand_z(group, xs), F.zero) if a is None or flagged else scale(group, a, z)
            jtab.append(record(group, j).tobytes())
        return index[key]

    segs, labels = [], []
    for c in corpus(group):
        if c.pa is NOT_A_POINT:
            continue
        segs.append([entry(c.pa), entry(c.qa)]); labels.append(c.label)
    pts = list(base_points(group)) + ([p for pools in partial_pools().values() for pool in pools for p in pool] if group == 2 else [])
    for i, a in enumerate(pts):
        r = pts[(i + 5) % len(pts)]
        na = neg(group, a)
        segs += [[entry(a), entry(na), entry(r)], [entry(a), entry(a), entry(r)], [entry(r), entry(a), entry(na)],
                 [entry(None) if i & 1 else entry(r, True), entry(a), entry(a)]]
        labels += ["P,-P,R", "P,P,R", "R,P,-P", "inf,P,P"]
    chain = [unwire(group, RC.g1_sum(wire(group, pts[0]) + wire(group, pts[1]), 2) if group == 1 else RC.g2_sum(wire(group, pts[0]) + wire(group, pts[1]), 2))]
    osum = RC.g1_sum if group == 1 else RC.g2_sum
    while len(chain) < 33:                                                     # distinct points by repeated addition: no multiplication needed
        chain.append(unwire(group, osum(wire(group, chain[-1]) + wire(group, pts[len(chain) % 5]), 2)))
    if group == 2:                                                             # the partial-zero points take part in the long segments too
        chain[1], chain[30] = partial_pools()["c0"][0][0], partial_pools()["c0"][0][1]
    r = entry(pts[2])
    for L in (2, 32, 33):
        A = [entry(a) for a in chain[:L]]
        nA = [entry(neg(group, a)) for a in chain[:L]]
        s = unwire(group, osum(b"".join(table[i] for i in A), L))
        rot, nrot = A[1:] + A[:1], nA[1:] + nA[:1]
        segs += [A + A, A + nA, A + nA + [r], [x for t in zip(A, rot) for x in t], [x for t in zip(A, nrot) for x in t],
                 [x for t in zip(A, nrot) for x in t] + [r], A + [entry(s)], A + [entry(neg(group, s))], A + [entry(neg(group, s)), r]]
        labels += ["%s |A|=%d" % (n, L) for n in ("A++A", "A++-A", "A++-A++R", "A/rot A", "A/rot -A", "A/rot -A++R", "A++sum", "A++-sum", "A++-sum++R")]
    if len(table) % 2 == 0:                                                    # an odd table and an odd number of segments
        entry(chain[32], True)
    if len(segs) % 2 == 0:
        segs.append([r]); labels.append("R")
    return SumCase(tuple(table), np.array(inf, dtype=np.uint8), tuple(jtab), tuple(tuple(s) for s in segs), tuple(labels))


def oracle_segment_sum(group, case, seg):
    """the C oracle's sum of one segment: wire bytes, or None for infinity"""
    if not seg:
        return None
    return (RC.g1_sum if group == 1 else RC.g2_sum)(b"".join(case.table[i] for i in seg), len(seg), bytes(int(case.inf[i]) for i in seg))
