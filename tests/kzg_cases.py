"""The corpus of the KZG batch tests (blsmi 0.20: blsmi_kzg_verify_batch*, blsmi_g1_mul_add_batch*), built with big integers and the oracle's
G1 operations from pinned seeds, tau known, so that tests/test_kzg_cpu.py and tests/test_gpu_kzg.py speak about the same openings.
A key G = [g0] G1, H = [h0] G2, tau H; item j from random c, z, q with
    y = c - q (tau - z) mod r,        C = [c] G,        pi = [q] G
so that e(C - y G + z pi, H) e(pi, -tau H) = 1 holds by construction (C - y G + z pi = [q tau] G).  Ways to spoil an item, one at a time:
    "y"  y + 1 -- only the fold sees it        "z"  z + 1 -- only the lift sees it        "C"  C replaced        "pi"  pi negated
Edge items: ("z", v) / ("y", v) for v in 0, r - 1, r, 2^256 - 1 (taken mod r), the other scalars solved for; "piinf": pi at infinity (q = 0,
y = c); "Cinf": C at infinity; "Winf": W = C + z pi at infinity (c = -z q, y = -q tau); "dbl": C = z pi, the lift's final addition is a
doubling; ("y", 0) and ("y", r) are items with y = 0 mod r, so that at block 1 their block's s_b is 0."""
import numpy as np

from oracle import pyref as P
from oracle import refcpu as RC
from pprod_rlc_corpus import ONE, neg1

R = P.R_ORDER
G1, G2 = RC.g1_generator(), RC.g2_generator()
EDGE_SCALARS = (0, R - 1, R, 2 ** 256 - 1)
INF = bytes(96)


def g1_mul(p, k):
    """[k mod r] p as a wire record, the all-zero record for infinity"""
    if p == INF or k % R == 0:
        return INF
    return RC.g1_mul(p, (k % R).to_bytes(32, "big")) or INF


def g2(k):
    return RC.g2_mul(G2, (k % R).to_bytes(32, "big")) or bytes(192)


def g1_neg(p):
    return p if p == INF else neg1(p)


def g1_sum(pts):
    pts = [p for p in pts if p != INF]
    if not pts:
        return INF
    return RC.g1_sum(b"".join(pts), len(pts)) or INF


def fe_of_pairs(pairs):
    """FinalExponentiation(MillerLoop(pairs)) by the oracle; a pair with a point at infinity or an all-zero G2 record contributes 1"""
    keep = [(p, q) for p, q in pairs if p != INF and q != bytes(192)]
    if not keep:
        return ONE
    ok, v = RC.final_exponentiation(RC.miller_loop(b"".join(p for p, _ in keep), b"".join(q for _, q in keep), len(keep)))
    assert ok
    return v


def is_one(v):
    return bool(np.array_equal(np.asarray(v, dtype=np.uint64), ONE))


def scalar_bytes(vals):
    return b"".join(int(v).to_bytes(32, "big") for v in vals)


class KzgCase:
    """m openings under one key.  spoil: {item: "y" | "z" | "C" | "pi"}; edge: {item: ("z", v) | ("y", v) | "piinf" | "Cinf" | "Winf" | "dbl"}"""

    def __init__(self, m, seed, spoil=None, edge=None):
        xs = P.XORShift(seed)
        spoil, edge = spoil or {}, edge or {}
        self.m = m
        self.g0, self.h0, self.tau = (P.rand_fr(xs) for _ in range(3))
        tau = self.tau
        self.G = g1_mul(G1, self.g0)
        self.H, self.tauH, self.neg_tauH = g2(self.h0), g2(self.h0 * tau), g2(-self.h0 * tau)
        self.srs_g1, self.srs_g2 = self.G, self.H + self.tauH
        self.C, self.pi, self.z, self.y, self.q = [], [], [], [], []
        for j in range(m):
            c, z, q = (P.rand_fr(xs) for _ in range(3))
            y = None
            e = edge.get(j)
            if isinstance(e, tuple) and e[0] == "z":
                z = e[1]
            elif isinstance(e, tuple) and e[0] == "y":
                y = e[1]
                c = (y + q * (tau - z)) % R
            elif e == "piinf":
                q = 0
            elif e == "Cinf":
                c = 0
            elif e == "Winf":
                c = (-z * q) % R
            elif e == "dbl":
                c = (z * q) % R
            else:
                assert e is None, e
            if y is None:
                y = (c - q * (tau - z)) % R
            assert (c - y + z * q - q * tau) % R == 0
            pc, pp = self.gmul(c), self.gmul(q)
            kind = spoil.get(j)
            if kind == "y":
                y = (y + 1) % 2 ** 256
            elif kind == "z":
                z = (z + 1) % 2 ** 256
            elif kind == "C":
                pc = self.gmul(c + 1)
            elif kind == "pi":
                pp = g1_neg(pp)
            else:
                assert kind is None, kind
            self.C.append(pc); self.pi.append(pp); self.z.append(z); self.y.append(y); self.q.append(q)
        self.commitments, self.proofs = b"".join(self.C), b"".join(self.pi)
        self.z_bytes, self.y_bytes = scalar_bytes(self.z), scalar_bytes(self.y)

    def gmul(self, k):
        return g1_mul(self.G, k)

    def W(self, j):
        """C_j + (z_j mod r) pi_j by the oracle's ladder and sum"""
        return g1_sum([self.C[j], g1_mul(self.pi[j], self.z[j])])

    def point(self, j):
        """P_j = C_j + (z_j mod r) pi_j - (y_j mod r) G"""
        return g1_sum([self.W(j), g1_neg(self.gmul(self.y[j]))])

    def two_pairs(self, j, srs_g2=None):
        h, nth = (self.H, self.neg_tauH) if srs_g2 is None else srs_g2
        return [(self.point(j), h), (self.pi[j], nth)]

    def item_value(self, j, srs_g2=None):
        return fe_of_pairs(self.two_pairs(j, srs_g2))

    def verdicts(self, srs_g2=None):
        return [int(is_one(self.item_value(j, srs_g2))) for j in range(self.m)]

    def block_value(self, r, lo, hi):
        """FE of the cells of the block of items [lo, hi) as the call's holding path forms them: (sum r_j W_j, H), (s_b (-G), H) with the
        big-integer s_b = sum r_j y_j mod r (never from a P_j, never a y_j G), (sum r_j pi_j, -tau H)"""
        s = sum(r[j] * (self.y[j] % R) for j in range(lo, hi)) % R
        wsum = g1_sum([g1_mul(self.W(j), r[j]) for j in range(lo, hi)])
        psum = g1_sum([g1_mul(self.pi[j], r[j]) for j in range(lo, hi)])
        return fe_of_pairs([(wsum, self.H), (g1_mul(g1_neg(self.G), s), self.H), (psum, self.neg_tauH)])


# the batch both test files use: 37 openings
M = 37
SEED = 20
BAD_Y, BAD_Z, BAD_C, BAD_PI = {5: "y"}, {14: "z"}, {30: "C"}, {33: "pi"}
BAD_TWO = {7: "C", 21: "y"}                                                      # different blocks at block 8 (0 and 2) and at block 1
SPOILS = {"y": BAD_Y, "z": BAD_Z, "C": BAD_C, "pi": BAD_PI, "two": BAD_TWO}
EDGES = {0: ("z", 0), 1: ("z", R - 1), 2: ("z", R), 3: ("z", 2 ** 256 - 1), 4: ("y", 0), 6: ("y", R - 1), 8: ("y", R), 9: ("y", 2 ** 256 - 1),
         10: "piinf", 11: "Cinf", 12: "Winf", 13: "dbl"}
