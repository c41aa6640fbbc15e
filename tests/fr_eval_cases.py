"""The model and the corpus of the scalar-field tests (blsmi 0.21: blsmi_fr_mul_batch*, blsmi_fr_inv_batch*, blsmi_fr_eval_batch*,
blsmi_kzg_verify_blob_batch*), in Python big integers: the evaluation domains from pow(7, (r - 1) // N, r), the barycentric formula with
pow(x, -1, r), Horner's rule to hold it against, the grid of edge operands of the field, and blob batches built on tests/kzg_cases.py --
tau is known there, so C_j = [p_j(tau)] G and pi_j = [(p_j(tau) - y_j) / (tau - z_j)] G hold by construction, also when z_j is a root."""
import functools
import random

from kzg_cases import INF, R, KzgCase, g1_neg, scalar_bytes

TOP = 2 ** 256 - 1
MONT_ONE = 2 ** 256 % R
# the field's edge operands: around 0, r and 2 r, the top of 256 bits, around the Montgomery one, and a single nonzero word at each position
EDGE_OPERANDS = ([0, 1, 2, R - 1, R, R + 1, 2 * R, 2 * R + 1, 2 ** 255, TOP, MONT_ONE, MONT_ONE - 1]
                 + [1 << (32 * i) for i in range(8)] + [0xffffffff << (32 * i) for i in range(8)])


def grid_pairs(nrandom, seed):
    """the edge operands crossed with each other, and nrandom random pairs of 256-bit values"""
    rng = random.Random(seed)
    return [(a, b) for a in EDGE_OPERANDS for b in EDGE_OPERANDS] + [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(nrandom)]


def bitrev(i, k):
    return int(format(i, "0%db" % k)[::-1], 2) if k else 0


def omega(k):
    return pow(7, (R - 1) >> k, R)


@functools.lru_cache(maxsize=None)
def domain(k, order):
    """the roots in position order: position i holds w^i (order 0) or w^bitrev_k(i) (order 1)"""
    w, n = omega(k), 1 << k
    nat = [1] * n
    for i in range(1, n):
        nat[i] = nat[i - 1] * w % R
    return tuple(nat[bitrev(i, k)] for i in range(n)) if order else tuple(nat)


def evaluate(vals, k, order, z):
    """p(z) for the polynomial with the N = 2^k values vals (any integers, taken mod r) over domain(k, order): the value itself where z is
    a root, else the barycentric formula with pow(x, -1, r)"""
    dom, n, z = domain(k, order), 1 << k, z % R
    assert len(vals) == n
    for i, w in enumerate(dom):
        if w == z:
            return vals[i] % R
    s = sum(f * w % R * pow(z - w, -1, R) for f, w in zip(vals, dom)) % R
    return (pow(z, n, R) - 1) * pow(n, -1, R) % R * s % R


def horner(coeffs, z):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * z + c) % R
    return acc


def poly_bytes(polys):
    """m polynomials (lists of integers below 2^256) as the bytes the library reads"""
    return b"".join(scalar_bytes(p) for p in polys)


def is_noncanon(vals):
    return any(v >= R for v in vals)


def second_representatives(v):
    """the other 256-bit integers that are v mod r (v below r)"""
    return [v + t * R for t in (1, 2) if v + t * R <= TOP]


class BlobCase:
    """m blob proofs under the key of KzgCase(0, seed).  Item j: N = 2^k values f (below r unless an edge says otherwise), a point z, and
    y = p(z), c = p(tau), q = (c - y) / (tau - z) by big integers; C = [c] G, pi = [q] G.
    edge: {item: ("root", position) | ("noncanon", position) | "const"} -- z the root at that position; the value at that position written as
    v + r (the same polynomial mod r); a constant blob, so that q = 0 and pi is at infinity.
    spoil: {item: "f" | "z" | "C" | "pi"} -- one value of the blob incremented (only the evaluation sees it), z incremented, C replaced, pi
    negated, each AFTER C and pi were made."""

    def __init__(self, m, k, order, seed, spoil=None, edge=None):
        rng = random.Random(seed)
        srng = random.Random(seed + 1)                                           # where a spoiled value sits: its own stream, so that the batch is the same but for it
        spoil, edge = spoil or {}, edge or {}
        key = KzgCase(0, seed)
        self.m, self.k, self.order, self.key = m, k, order, key
        self.srs_g1, self.srs_g2, tau = key.srs_g1, key.srs_g2, key.tau
        n, dom = 1 << k, domain(k, order)
        self.polys, self.z, self.C, self.pi, self.c, self.q = [], [], [], [], [], []
        for j in range(m):
            f = [rng.randrange(R) for _ in range(n)]
            z = rng.randrange(R)
            e = edge.get(j)
            if e == "const":
                f = [f[0]] * n
            elif isinstance(e, tuple) and e[0] == "root":
                z = dom[e[1]]
            elif isinstance(e, tuple) and e[0] == "noncanon":
                f[e[1]] = rng.randrange(TOP - R + 1)                              # so that v + r fits 256 bits
            else:
                assert e is None, e
            y, c = evaluate(f, k, order, z), evaluate(f, k, order, tau)
            q = (c - y) * pow(tau - z, -1, R) % R
            assert (c - y + z * q - q * tau) % R == 0 and (e != "const" or (q == 0 and y == f[0]))
            if isinstance(e, tuple) and e[0] == "noncanon":
                f[e[1]] += R
            pc, pp = key.gmul(c), key.gmul(q)
            assert e != "const" or pp == INF                                    # pi at infinity with a constant blob
            kind = spoil.get(j)
            if kind == "f":
                at = e[1] if isinstance(e, tuple) and e[0] == "root" else srng.randrange(n)   # (where z is a root only that value counts)
                f[at] = (f[at] + 1) % 2 ** 256
            elif kind == "z":
                z = (z + 1) % 2 ** 256
            elif kind == "C":
                c = (c + 1) % R
                pc = key.gmul(c)
            elif kind == "pi":
                q = (-q) % R
                pp = g1_neg(pp)
            else:
                assert kind is None, kind
            self.polys.append(f); self.z.append(z); self.C.append(pc); self.pi.append(pp); self.c.append(c); self.q.append(q)
        self.y = [evaluate(f, k, order, z) for f, z in zip(self.polys, self.z)]   # of the blobs and points as they are handed over
        self.poly_bytes, self.z_bytes, self.y_bytes = poly_bytes(self.polys), scalar_bytes(self.z), scalar_bytes(self.y)
        self.commitments, self.proofs = b"".join(self.C), b"".join(self.pi)
        self.noncanon = [is_noncanon(f) for f in self.polys]

    def verdicts(self):
        """by big integers alone: G and H generate groups of order r, so e(C - y G + z pi, H) = e(pi, tau H) exactly when
        c - y + z q = q tau mod r for the discrete logarithms c, q of the C and pi handed over"""
        tau = self.key.tau
        return [int((c - y + z * q - q * tau) % R == 0) for c, y, z, q in zip(self.c, self.y, self.z, self.q)]

