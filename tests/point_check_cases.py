"""The corpus of the point-validation tests (blsmi 0.14: blsmi_g?_check_batch[_jac|_dev]), built from the helpers of tests/group_edges.py and
judged by oracle.pyref alone (g?_on_curve, g?_in_subgroup).  Per group:

  (a) subgroup   the seeded subgroup points and the generator
  (b) outside    curve points outside the prime-order subgroup (group_edges.outside_points) and the x == 0 points
  (c) off-curve  made from (a) and (b): y + 1; x and y swapped; G1: points of y^2 = x^3 + 5 (b = 4 replaced); G2: one coefficient of y negated alone
  (d) infinity   affine: the all-zero record, a finite record with its in_inf byte set; Jacobian: the three shapes of group_edges.infinities
                 (Z = 0 with arbitrary non-zero X and Y among them)
  (e) x >= q     G1, both forms: a coordinate that is not below q, expected as the point every loader reads -- that coordinate as 0
  (f) Jacobian   every finite point of (a) to (c) under Z = 1, a special value of group_edges.z_values, a random Z and, for G2, a Z with a zero
                 coefficient

Statuses: 0 good, 1 infinity, 3 not on the curve, 4 on the curve but outside the subgroup (include/blsmi.h: BLSMI_POINT_*).  Everything is seeded:
the same corpus in every process.  No GPU."""
import functools
import itertools
from collections import namedtuple

import numpy as np

import group_edges as G
from gpu_common import P

Q = P.Q
OK, INFINITY, NOT_ON_CURVE, NOT_IN_SUBGROUP = 0, 1, 3, 4
STATUSES = (OK, INFINITY, NOT_ON_CURVE, NOT_IN_SUBGROUP)
GENERATOR = {1: P.G1_GEN, 2: P.G2_GEN}
SIZES = (1, 31, 32, 33, 63, 64, 65, 129)

# affine: the wire record (bytes), its in_inf byte; jac: the uint64 record.  `point`: the affine point the record stands for (None: infinity),
# `z`: the Z a Jacobian record was scaled by (None where it was not scaled from `point`), `status`: the oracle's verdict
Affine = namedtuple("Affine", "label src rec inf point status")
Jacobian = namedtuple("Jacobian", "label src rec point z status")


@functools.lru_cache(maxsize=None)
def oracle_status(group, a):
    """infinity, then the curve equation, then -- only for a curve point -- the subgroup"""
    if a is None:
        return INFINITY
    if not (P.g1_on_curve(a) if group == 1 else P.g2_on_curve(a)):
        return NOT_ON_CURVE
    return OK if (P.g1_in_subgroup(a) if group == 1 else P.g2_in_subgroup(a)) else NOT_IN_SUBGROUP


def _other_curve_points(n):
    """points of y^2 = x^3 + 5 over Fq: on a curve, not on G1's"""
    out, x = [], 1
    while len(out) < n:
        y = P.fq_sqrt((x * x * x + 5) % Q)
        if y is not None:
            out.append((x, y))
        x += 1
    return out


@functools.lru_cache(maxsize=None)
def finite_points(group):
    """[(label, src, affine point)] of (a), (b), (c)"""
    F = G.FIELD[group]
    good = [("subgroup", "subgroup_points", a) for a in G.subgroup_points(group)] + [("generator", "generator", GENERATOR[group])]
    outside = [("outside", "outside_points", a) for a in G.outside_points(group)] + [("x_zero", "x_zero_points", a) for a in G.x_zero_points(group)]
    off = []
    for label, src, a in good + outside:
        off.append(("y+1", src, (a[0], F.add(a[1], F.one))))
        off.append(("swapped", src, (a[1], a[0])))
        if group == 2:
            off.append(("y.c1 negated", src, (a[0], (a[1][0], (-a[1][1]) % Q))))
    if group == 1:
        off += [("b=5", "other curve", a) for a in _other_curve_points(4)]
    return tuple(good + outside + off)


def _be(v):
    return int(v).to_bytes(48, "big")


@functools.lru_cache(maxsize=None)
def affine_cases(group):
    pb = G.PB[group]
    out = [Affine(label, src, G.wire(group, a), 0, a, oracle_status(group, a)) for label, src, a in finite_points(group)]
    # (d) every infinity form of the affine records
    out.append(Affine("all-zero record", "infinity", bytes(pb), 0, None, INFINITY))
    out.append(Affine("all-zero record, flagged", "infinity", bytes(pb), 1, None, INFINITY))
    for k in (0, 9, len(finite_points(group)) - 1, 12):                      # a subgroup point, an outside point, off-curve points: the flag wins
        label, src, a = finite_points(group)[k]
        out.append(Affine("flagged " + label, "infinity", G.wire(group, a), 1, None, INFINITY))
    if group == 1:                                                            # (e) x >= q is read as x = 0: (0, 2) is on the curve, (0, 3) is not
        for xraw, y in ((Q + 5, 2), (Q, 3), ((1 << 384) - 1, Q - 2)):
            a = (0, y)
            out.append(Affine("x >= q", "noncanonical", _be(xraw) + _be(y), 0, a, oracle_status(1, a)))
    return tuple(out)


def _raw_fq_words(v):
    """a 384-bit integer as the six words of a limb image, NOT reduced: what a coordinate >= q looks like in memory"""
    return [(v >> (64 * i)) & P.MASK64 for i in range(6)]


@functools.lru_cache(maxsize=None)
def jacobian_cases(group):
    xs = P.XORShift(9400 + group)
    F = G.FIELD[group]
    special = G.z_values(group, xs, 0)
    nbase = len(G.fq_z_values())
    out = []
    for k, (label, src, a) in enumerate(finite_points(group)):              # (f)
        zs = [F.one, special[(7 * k + 1) % nbase], G.rand_z(group, xs)]
        if group == 2:
            zs.append(special[nbase + k % 24])                               # (v, 0) and (0, v): a Z with a zero coefficient
        for z in zs:
            out.append(Jacobian(label, src, G.record(group, G.scale(group, a, z)), a, z, oracle_status(group, a)))
    for j in G.infinities(group, xs) + G.infinities(group, xs):               # (d): the three shapes, twice (the oracle must meet each status four times)
        out.append(Jacobian("Z = 0", "infinity", G.record(group, j), None, None, INFINITY))
    if group == 1:                                                            # (e) the limb image of X is not below q: read as X = 0
        for xraw, y in ((Q + 1, 2), ((1 << 384) - 1, 3)):
            rec = G.record(1, (0, y, 1))
            rec[:6] = _raw_fq_words(xraw)
            a = (0, y)
            out.append(Jacobian("X >= q", "noncanonical", rec, a, None, oracle_status(1, a)))
    return tuple(out)


def cases(group, form):
    return affine_cases(group) if form == "affine" else jacobian_cases(group)


def jacobian_to_affine(group, jac):
    """big integers: (X / Z^2, Y / Z^3)"""
    F = G.FIELD[group]
    zi = F.inv(jac[2])
    zi2 = F.sqr(zi)
    return (F.mul(jac[0], zi2), F.mul(jac[1], F.mul(zi2, zi)))


# ---- buffers ---------------------------------------------------------------------------------------------------------------------------
def affine_buffers(group, cs):
    return b"".join(c.rec for c in cs), np.array([c.inf for c in cs], dtype=np.uint8)


def jacobian_buffer(cs):
    return np.concatenate([c.rec for c in cs]).tobytes()


def statuses(cs, check=1):
    """the oracle's statuses; check == 0: the curve equation only, so every status 4 reads 0"""
    st = np.array([c.status for c in cs], dtype=np.uint8)
    if check == 0:
        st[st == NOT_IN_SUBGROUP] = OK
    return st


def cut(cs, n):
    """n cases cut from cs (in order, wrapping round where cs is shorter): all four statuses where n >= 4, and a non-zero status LAST, so that the
    lane after it -- a clamped tail lane -- recomputes a record whose status differs from the poison and from 0"""
    by = {s: [i for i, c in enumerate(cs) if c.status == s] for s in STATUSES}
    last = by[NOT_ON_CURVE][n % len(by[NOT_ON_CURVE])] if n % 2 else by[NOT_IN_SUBGROUP][n % len(by[NOT_IN_SUBGROUP])]
    head = [by[s][0] for s in (OK, INFINITY, NOT_IN_SUBGROUP, NOT_ON_CURVE)] if n >= 5 else [by[s][0] for s in STATUSES if cs[by[s][0]].status != cs[last].status][:n - 1]
    fill = itertools.cycle(range(len(cs)))
    idx = head + [next(fill) for _ in range(max(0, n - 1 - len(head)))]
    return [cs[i] for i in idx[:n - 1]] + [cs[last]]
