"""The corpus of the randomised pairing-product tests (blsmi 0.17), built from the oracle alone so that tests/test_pprod_rlc_cpu.py and
tests/test_gpu_pprod_rlc.py speak about the same items.  A table of 9 G2 entries --
    0 Q_A = [x]G2 and 2 Q_B = [y]G2, shared by most items;  1, 4, 7 private (one pair each);  6 Q_C = [c]G2, used by exactly two items;
    5 unreferenced;  3 the all-zero record;  8 the bytes of Q_A once more, used by one item (equal bytes are not merged)
-- and items of 0 to 5 pairs in mixed order.  Item kinds (each holds, or fails with one scalar off by one):
    two      ([s y]G1, Q_A), (-[s x]G1, Q_B)
    groth    (A = [a]G1, B = [b]G2 private), (-[(a b + t y) / x]G1, Q_A), ([t]G1, Q_B)
    qc       ([u]G1, Q_C), (-[u c / x]G1, Q_A)
    dup      ([s y]G1, entry 8), (-[s x]G1, Q_B)
    cancel   (P, Q_A), (-P, Q_A)                                    always holds: its group's share cancels whatever the weights
    inf      (P flagged infinite, Q_A)                              a pair that contributes 1
    zero     (P, the all-zero entry)                                a pair that contributes 1
    lone     (P, Q_B)                                               a single finite pair: never one
and concatenations of those."""
import numpy as np

from oracle import pyref as P
from oracle import refcpu as RC

R = P.R_ORDER
G1, G2 = RC.g1_generator(), RC.g2_generator()
X, Y, CC = 0x1234567 + 3 * 2 ** 70, 0x7654321 + 5 * 2 ** 90, 0xabcdef + 7 * 2 ** 60
QA, QB, QC, UNREF, DUP, ZERO = 0, 2, 6, 5, 8, 3
PRIVATE = (1, 4, 7)


def _one():
    one = np.zeros(72, dtype=np.uint64)
    one[:6] = np.array(P.limbs64(P.to_mont(1)), dtype=np.uint64)
    return one


ONE = _one()


def g1(k):
    return RC.g1_mul(G1, (k % R).to_bytes(32, "big"))


def g2(k):
    return RC.g2_mul(G2, (k % R).to_bytes(32, "big"))


def neg1(p):
    return p[:48] + ((P.Q - int.from_bytes(p[48:], "big")) % P.Q).to_bytes(48, "big")


def table():
    priv = {e: g2(1000 + 17 * e) for e in PRIVATE}
    t = [None] * 9
    t[QA], t[QB], t[QC], t[UNREF], t[DUP], t[ZERO] = g2(X), g2(Y), g2(CC), g2(424242), g2(X), bytes(192)
    for e in PRIVATE:
        t[e] = priv[e]
    return t


def pairs_of(kind, seed, bad=False):
    """-> list of (P bytes, table entry, flag)"""
    xs = P.XORShift(1000 + seed)
    off = 1 if bad else 0
    s, t, a, u = (P.rand_fr(xs) for _ in range(4))
    if kind == "two":
        return [(g1(s * Y + off), QA, 0), (neg1(g1(s * X)), QB, 0)]
    if kind == "dup":
        return [(g1(s * Y + off), DUP, 0), (neg1(g1(s * X)), QB, 0)]
    if kind.startswith("groth"):
        e = PRIVATE[int(kind[-1])]
        b = 1000 + 17 * e
        return [(g1(a), e, 0), (neg1(g1((a * b + t * Y + off) * pow(X, -1, R))), QA, 0), (g1(t), QB, 0)]
    if kind == "qc":
        return [(g1(u), QC, 0), (neg1(g1((u * CC + off) * pow(X, -1, R))), QA, 0)]
    if kind == "cancel":
        return [(g1(s), QA, 0), (neg1(g1(s)), QA, 0)]
    if kind == "inf":
        return [(g1(s), QA, 1)]
    if kind == "zero":
        return [(g1(s), ZERO, 0)]
    if kind == "lone":
        return [(g1(s), QB, 0)]
    raise ValueError(kind)


# (kinds concatenated into one item); sizes 2 0 3 1 4 5 2 2 3 1 2 0 4 5 3 2 ... -- every size from 0 to 5, mixed
ITEMS = [("two",), (), ("groth0",), ("inf",), ("groth1", "zero"), ("two", "groth2"), ("cancel",), ("qc",), ("two", "inf"), ("zero",), ("qc",), (),
         ("two", "two"), ("two", "two", "zero"), ("dup", "inf"), ("two",), ("two", "cancel"), ("two", "two", "inf"), ("two",), ("two", "two"),
         ("cancel", "two", "zero"), ("two",), ("two", "two"), ("two",), ("two", "cancel", "inf"), ("two",), ("two", "two"), ("two",), ("two", "zero"),
         ("two", "two"), ("two",), ("two", "inf", "two"), ("two",)]
assert sorted(set(sum(len(pairs_of(k, 0)) for k in it) for it in ITEMS)) == [0, 1, 2, 3, 4, 5]


class Corpus:
    """g1s / q_idx / flags per pair, sizes per item; `bad`: the items built with a scalar off by one"""

    def __init__(self, bad=(), items=ITEMS):
        self.tab = table()
        self.items = []
        for j, kinds in enumerate(items):
            ps, first = [], True
            for i, k in enumerate(kinds):
                spoil = j in bad and first and k not in ("cancel", "inf", "zero")
                ps += pairs_of(k, 10 * j + i, spoil)
                first = first and not spoil
            self.items.append(ps)
        self.sizes = [len(it) for it in self.items]
        flat = [p for it in self.items for p in it]
        self.g1s = [p[0] for p in flat]
        self.q_idx = np.array([p[1] for p in flat], dtype=np.uint32)
        self.flags = np.array([p[2] for p in flat], dtype=np.uint8)
        self.np = len(flat)
        self.seg_off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.uint64)

    def item_value(self, j):
        """FinalExponentiation(MillerLoop(item j)) by the oracle, infinite pairs left out"""
        keep = [(p, self.tab[e]) for p, e, f in self.items[j] if not f and p != bytes(96) and self.tab[e] != bytes(192)]
        if not keep:
            return ONE
        ok, v = RC.final_exponentiation(RC.miller_loop(b"".join(p for p, _ in keep), b"".join(q for _, q in keep), len(keep)))
        assert ok
        return v

    def verdicts(self, known=None):
        """the oracle's per-item verdicts; known: {item: verdict} already computed for items this corpus shares with another"""
        return [known[j] if known and j in known else int(np.array_equal(self.item_value(j), ONE)) for j in range(len(self.items))]

    def combined_value(self, r):
        """FE(MillerLoop over (sum_{k in g} r_item(k) P_k, Q_g)) for the table entries g some pair refers to, from the oracle's primitives:
        infinite pairs add nothing, an all-zero entry drops its group, a group whose sum is infinity contributes 1"""
        groups = {}
        for j, it in enumerate(self.items):
            for p, e, f in it:
                groups.setdefault(int(e), [])
                if not f and p != bytes(96):
                    groups[int(e)].append(RC.g1_mul(p, int(r[j]).to_bytes(32, "big")))
        s, q = [], []
        for e in sorted(groups):
            pts = [p for p in groups[e] if p is not None]
            if self.tab[e] == bytes(192) or not pts:
                continue
            sg = RC.g1_sum(b"".join(pts), len(pts))
            if sg is None:
                continue
            s.append(sg); q.append(self.tab[e])
        if not s:
            return ONE
        ok, v = RC.final_exponentiation(RC.miller_loop(b"".join(s), b"".join(q), len(s)))
        assert ok
        return v
