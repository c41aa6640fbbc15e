"""The corpus of the Groth16 batch tests (blsmi 0.19: blsmi_groth16_verify_batch*), built with big integers and the oracle's group
operations from pinned seeds, so that tests/test_groth16_cpu.py and tests/test_gpu_groth16.py speak about the same proofs.
A verifying key from secret scalars (alpha, beta, gamma, delta, ic_0 .. ic_nin); proof j from random a, b with
    c = (a b - alpha beta - gamma (ic_0 + sum_i a_ji ic_i)) / delta mod r,        A = [a]G1, B = [b]G2, C = [c]G1
so that e(A, B) = e(alpha, beta) e(L_j, gamma) e(C, delta) holds by construction.  Ways to spoil an item (the proof stays, something else moves):
    "input"  its first public input is off by one -- the case only the fold sees        "A"  A replaced        "C"  C negated        "B"  B replaced
Edge items: public inputs 0, r - 1, r, 2^256 - 1 (taken mod r); "Ainf": A at infinity (c absorbs the rest); "Cinf": C at infinity with the
matching b."""
import numpy as np

from oracle import pyref as P
from oracle import refcpu as RC
from pprod_rlc_corpus import ONE, neg1

R = P.R_ORDER
G1, G2 = RC.g1_generator(), RC.g2_generator()
EDGE_INPUTS = (0, R - 1, R, 2 ** 256 - 1)


def g1(k):
    return RC.g1_mul(G1, (k % R).to_bytes(32, "big")) or bytes(96)


def g2(k):
    return RC.g2_mul(G2, (k % R).to_bytes(32, "big")) or bytes(192)


def g1_mul(p, k):
    """[k mod r] p as a wire record, the all-zero record for infinity"""
    if p == bytes(96) or k % R == 0:
        return bytes(96)
    return RC.g1_mul(p, (k % R).to_bytes(32, "big")) or bytes(96)


def g1_sum(pts):
    pts = [p for p in pts if p != bytes(96)]
    if not pts:
        return bytes(96)
    return RC.g1_sum(b"".join(pts), len(pts)) or bytes(96)


def fe_of_pairs(pairs):
    """FinalExponentiation(MillerLoop(pairs)) by the oracle; a pair with a point at infinity contributes 1"""
    keep = [(p, q) for p, q in pairs if p != bytes(96) and q != bytes(192)]
    if not keep:
        return ONE
    ok, v = RC.final_exponentiation(RC.miller_loop(b"".join(p for p, _ in keep), b"".join(q for _, q in keep), len(keep)))
    assert ok
    return v


def is_one(v):
    return bool(np.array_equal(np.asarray(v, dtype=np.uint64), ONE))


class Groth16Case:
    """m proofs of one circuit with nin public inputs.  spoil: {item: "input" | "A" | "C" | "B"}; edge: {item: "Ainf" | "Cinf"};
    inputs_of: {item: [nin integers below 2^256]} for chosen public inputs (the others are random below r)"""

    def __init__(self, m, nin, seed, spoil=None, edge=None, inputs_of=None):
        xs = P.XORShift(seed)
        spoil, edge, inputs_of = spoil or {}, edge or {}, inputs_of or {}
        self.m, self.nin = m, nin
        self.alpha, self.beta, self.gamma, self.delta = (P.rand_fr(xs) for _ in range(4))
        self.ic = [P.rand_fr(xs) for _ in range(nin + 1)]
        self.alpha_g1, self.ic_g1 = g1(self.alpha), [g1(k) for k in self.ic]
        self.vk_g1 = self.alpha_g1 + b"".join(self.ic_g1)
        self.beta_g2, self.gamma_g2, self.delta_g2 = g2(self.beta), g2(self.gamma), g2(self.delta)
        self.vk_g2 = self.beta_g2 + self.gamma_g2 + self.delta_g2
        self.A, self.B, self.C, self.inputs = [], [], [], []
        dinv = pow(self.delta, -1, R)
        for j in range(m):
            a, b = P.rand_fr(xs), P.rand_fr(xs)
            x = list(inputs_of.get(j, [P.rand_fr(xs) for _ in range(nin)]))
            assert len(x) == nin
            lsc = (self.ic[0] + sum(v * k for v, k in zip(x, self.ic[1:]))) % R
            rest = (self.alpha * self.beta + self.gamma * lsc) % R
            if edge.get(j) == "Ainf":
                pa, pb, c = bytes(96), g2(b), (-rest * dinv) % R
            elif edge.get(j) == "Cinf":
                pa, pb, c = g1(a), g2(rest * pow(a, -1, R)), 0
            else:
                pa, pb, c = g1(a), g2(b), ((a * b - rest) * dinv) % R
            pc = g1(c)
            kind = spoil.get(j)
            if kind == "input":
                x[0] = (x[0] + 1) % 2 ** 256
            elif kind == "A":
                pa = g1(a + 1)
            elif kind == "C":
                pc = neg1(pc)
            elif kind == "B":
                pb = g2(b + 1)
            else:
                assert kind is None, kind
            self.A.append(pa); self.B.append(pb); self.C.append(pc); self.inputs.append(x)
        self.proof_g1 = b"".join(a + c for a, c in zip(self.A, self.C))
        self.proof_g2 = b"".join(self.B)
        self.input_bytes = b"".join(v.to_bytes(32, "big") for x in self.inputs for v in x)

    def L(self, j):
        """IC_0 + sum_i (a_ji mod r) IC_i by the oracle's ladders and sum"""
        return g1_sum([self.ic_g1[0]] + [g1_mul(p, v) for p, v in zip(self.ic_g1[1:], self.inputs[j])])

    def four_pairs(self, j):
        return [(self.A[j], self.B[j]), (neg1(self.alpha_g1), self.beta_g2), (neg1(self.L(j)) if self.L(j) != bytes(96) else bytes(96), self.gamma_g2),
                (neg1(self.C[j]) if self.C[j] != bytes(96) else bytes(96), self.delta_g2)]

    def item_value(self, j):
        return fe_of_pairs(self.four_pairs(j))

    def verdicts(self):
        return [int(is_one(self.item_value(j))) for j in range(self.m)]

    def block_value(self, r, lo, hi):
        """FE of the cells of the block of items [lo, hi) as the call's holding path forms them: (r_j A_j, B_j) per item, (-t alpha, beta),
        the gamma cell from the big-integer t and s_i (never from an L_j), (-sum r_j C_j, delta)"""
        t = sum(r[lo:hi])
        s = [sum(r[j] * (self.inputs[j][i] % R) for j in range(lo, hi)) % R for i in range(self.nin)]
        folded = g1_sum([g1_mul(self.ic_g1[0], t)] + [g1_mul(p, v) for p, v in zip(self.ic_g1[1:], s)])
        csum = g1_sum([g1_mul(self.C[j], r[j]) for j in range(lo, hi)])
        neg = lambda p: neg1(p) if p != bytes(96) else p                          # noqa: E731
        cells = [(g1_mul(self.A[j], r[j]), self.B[j]) for j in range(lo, hi)]
        cells += [(neg(g1_mul(self.alpha_g1, t)), self.beta_g2), (neg(folded), self.gamma_g2), (neg(csum), self.delta_g2)]
        return fe_of_pairs(cells)


# the batches both test files use: 37 proofs, three public inputs / one
M = 37
BAD_INPUT = {5: "input"}
BAD_TWO = {7: "A", 21: "C"}                                                      # different blocks at block 8 (0 and 2) and at block 1
EDGES = dict(edge={3: "Ainf", 11: "Cinf"}, inputs_of={0: [0, R - 1, R], 1: [2 ** 256 - 1, R, 0], 2: [R - 1, 2 ** 256 - 1, 1]})


def edges_for(nin):
    e = dict(EDGES)
    e["inputs_of"] = {j: (x * nin)[:nin] for j, x in EDGES["inputs_of"].items()} if nin else {}
    return e
