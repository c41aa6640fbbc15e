"""The model and the corpus of the coset interpolation and the KZG cell batches (blsmi 0.22: blsmi_fr_coset_interp_batch*,
blsmi_kzg_verify_cell_batch*), in Python big integers plus the oracle's G1 / G2 operations, built on tests/kzg_cases.py -- tau is known
there.  A cell is the n = 2^l values of a polynomial p over the coset h <w>; its interpolant I (deg I < n, I = p on the coset) is
p mod (X^n - h^n), and with c = p(tau), q = (c - I(tau)) / (tau^n - h^n), C = [c] G, pi = [q] G the cell holds:
    e(C - [I(tau)] G, H) = e(pi, [tau^n - h^n] H)        exactly when        c - I(tau) + h^n q - q tau^n = 0 mod r."""
import random

import numpy as np

from fr_eval_cases import bitrev, horner, omega
from kzg_cases import INF, R, KzgCase, g1_neg, g2, scalar_bytes

TOP = 2 ** 256 - 1
EDGE_SHIFTS = (1, R - 1, R + 1, 0, R, TOP)


def coset(l, order, h):
    """the points of the coset in position order: h w^i (order 0) or h w^bitrev(i) (order 1)"""
    w, n = omega(l), 1 << l
    return [h % R * pow(w, bitrev(i, l) if order else i, R) % R for i in range(n)]


def interp(vals, l, order, h):
    """the n coefficients of the interpolant of vals (any integers, taken mod r) over the coset of h (taken mod r), by the naive inverse DFT
    and pow(h, -1, r); h = 0 mod r: h^-1 counts as 0 and 0^0 as 1 -- c_0 = a_0 and every other coefficient 0"""
    n, w, h = 1 << l, omega(l), h % R
    assert len(vals) == n
    nat = [0] * n                                                                # nat[k]: the value at h w^k
    for i, v in enumerate(vals):
        nat[bitrev(i, l) if order else i] = v % R
    ninv, winv = pow(n, -1, R), pow(w, -1, R)
    a = [ninv * sum(nat[k] * pow(winv, i * k, R) for k in range(n)) % R for i in range(n)]
    hinv = pow(h, -1, R) if h else 0
    return [a[i] * (pow(hinv, i, R) if i else 1) % R for i in range(n)]


def _dft(a, w):
    n = len(a)
    if n == 1:
        return list(a)
    ev, od, out, t = _dft(a[0::2], w * w % R), _dft(a[1::2], w * w % R), [0] * n, 1
    for k in range(n // 2):
        x = t * od[k] % R
        out[k], out[k + n // 2], t = (ev[k] + x) % R, (ev[k] - x) % R, t * w % R
    return out


def interp_fast(vals, l, order, h):
    """interp by a radix-2 recursion, for the shapes the naive sum is too slow for; tests/test_cell_cpu.py holds it against interp"""
    n, h = 1 << l, h % R
    nat = [0] * n
    for i, v in enumerate(vals):
        nat[bitrev(i, l) if order else i] = v % R
    ninv, hinv, t, out = pow(n, -1, R), (pow(h, -1, R) if h else 0), 1, []
    for x in _dft(nat, pow(omega(l), -1, R)):
        out.append(x * ninv % R * t % R)
        t = t * hinv % R
    return out


def flags_of(vals, h):
    return (1 if h >= R or any(v >= R for v in vals) else 0) | (2 if h % R == 0 else 0)


def cell_shifts(log2_cells, l):
    """h_k = w_N^bitrev(k) for the N / n cells of an extended blob of N = 2^(log2_cells + l) values"""
    w = omega(log2_cells + l)
    return [pow(w, bitrev(k, log2_cells), R) for k in range(1 << log2_cells)]


def poly_mod_coset(p, l, h):
    """p mod (X^n - h^n): X^(n k + i) = h^(n k) X^i"""
    n, hn = 1 << l, pow(h % R, 1 << l, R)
    out = [0] * n
    for d, c in enumerate(p):
        out[d % n] = (out[d % n] + c * pow(hn, d // n, R)) % R
    return out


def vals_bytes(cells):
    return b"".join(scalar_bytes(c) for c in cells)


class CellCase:
    """m cells under the key of KzgCase(0, seed): srs_g1 = [tau^i] G for i < n, srs_g2 = H, [tau^n] H.  Item j: a random p with 2 n + 3
    coefficients, a shift h, the values of p on the coset, c = p(tau), q = (c - I(tau)) / (tau^n - h^n); C = [c] G, pi = [q] G.
    edge: {item: "low" | "zero" | ("shift", v) | ("noncanon", i) | "tau" | ("coset_of", j0) | ("poly_of", j0)} -- deg p < n, so that q = 0 and
    pi is at infinity; p a multiple of X^n - h^n, so that every value is 0; the shift v as it is written (the polynomial solved for: q from
    the interpolant of the values at h mod r, whatever v); value i written as v + r; h = tau w^k with deg p < n, so that tau^n - h^n = 0 and
    the item holds with any pi; the shift of item j0 (same coset, another polynomial); the polynomial of item j0 (same C, another coset).
    spoil: {item: "v" | "h" | "C" | "pi"} -- one value incremented, the shift multiplied by w_2n, C replaced, pi negated, each AFTER C and
    pi were made."""

    def __init__(self, m, l, order, seed, spoil=None, edge=None, shifts=None):
        rng = random.Random(seed)
        srng = random.Random(seed + 1)                                           # where a spoiled value sits: its own stream
        spoil, edge = spoil or {}, edge or {}
        key = KzgCase(0, seed)
        n, tau = 1 << l, key.tau
        self.m, self.l, self.n, self.order, self.key = m, l, n, order, key
        self.srs_g1 = b"".join(key.gmul(pow(tau, i, R)) for i in range(n))
        self.srs_g2 = key.H + g2(key.h0 * pow(tau, n, R))
        self.neg_taunH = g2(-key.h0 * pow(tau, n, R))
        self.polys, self.vals, self.h, self.C, self.pi, self.c, self.q = [], [], [], [], [], [], []
        for j in range(m):
            p = [rng.randrange(R) for _ in range(2 * n + 3)]
            h = shifts[j] if shifts is not None else rng.randrange(1, R)
            q = None
            e = edge.get(j)
            if e == "low":
                p = p[:n]
            elif e == "zero":
                qq = p[:n + 3]
                hn = pow(h, n, R)
                p = [(-hn * qq[i] if i < n + 3 else 0) % R for i in range(2 * n + 3)]
                for i, v in enumerate(qq):
                    p[n + i] = (p[n + i] + v) % R
            elif isinstance(e, tuple) and e[0] == "shift":
                h = e[1]
            elif e == "tau":
                p, h, q = p[:n], tau * pow(omega(l), rng.randrange(n), R) % R, rng.randrange(1, R)
            elif isinstance(e, tuple) and e[0] == "coset_of":
                h = self.h[e[1]]
            elif isinstance(e, tuple) and e[0] == "poly_of":
                p = self.polys[e[1]]
            else:
                assert e is None or (isinstance(e, tuple) and e[0] == "noncanon"), e
            vals = [horner(p, x) for x in coset(l, order, h)]
            c = horner(p, tau)
            it = horner(interp(vals, l, order, h), tau)
            z = (pow(tau, n, R) - pow(h % R, n, R)) % R
            if q is None:
                q = (c - it) * pow(z, -1, R) % R
            assert (c - it + pow(h % R, n, R) * q - q * pow(tau, n, R)) % R == 0
            assert e != "low" or q == 0
            assert e != "zero" or not any(vals)
            if isinstance(e, tuple) and e[0] == "noncanon":
                vals[e[1]] += R                                                  # (r < 2^255: v + r fits 256 bits)
            pc, pp = key.gmul(c), key.gmul(q)
            kind = spoil.get(j)
            if kind == "v":
                at = srng.randrange(n)
                vals[at] = (vals[at] + 1) % 2 ** 256
            elif kind == "h":
                h = h % R * omega(l + 1) % R
            elif kind == "C":
                c = (c + 1) % R
                pc = key.gmul(c)
            elif kind == "pi":
                q = (-q) % R
                pp = g1_neg(pp)
            else:
                assert kind is None, kind
            self.polys.append(p); self.vals.append(vals); self.h.append(h); self.C.append(pc); self.pi.append(pp); self.c.append(c); self.q.append(q)
        self.coeffs = [interp(v, l, order, h) for v, h in zip(self.vals, self.h)]   # of the values and shifts as they are handed over
        self.shift_pow = [pow(h % R, n, R) for h in self.h]
        self.flags = [flags_of(v, h) for v, h in zip(self.vals, self.h)]
        self.vals_bytes, self.shift_bytes = vals_bytes(self.vals), scalar_bytes(self.h)
        self.commitments, self.proofs = b"".join(self.C), b"".join(self.pi)

    def verdicts(self):
        """by big integers alone, from the interpolant of the values and shifts as handed over: G and H generate groups of order r"""
        tau, n = self.key.tau, self.n
        return [int((c - horner(co, tau) + hn * q - q * pow(tau, n, R)) % R == 0)
                for c, co, hn, q in zip(self.c, self.coeffs, self.shift_pow, self.q)]


def ints(rows):
    return [int.from_bytes(bytes(row), "big") for row in np.asarray(rows).reshape(-1, 32)]


# the batch both test files use: 37 cells of 4 values
M, L, ORDER, SEED = 37, 2, 1, 22
EDGES = {0: ("shift", 1), 1: ("shift", R - 1), 2: ("shift", R + 1), 3: ("shift", 0), 4: ("shift", R), 6: ("shift", TOP), 8: "low", 9: "zero",
         10: ("noncanon", 2), 11: "tau", 15: ("coset_of", 12), 16: ("poly_of", 13)}
BAD_V, BAD_H, BAD_C, BAD_PI = {5: "v"}, {14: "h"}, {30: "C"}, {33: "pi"}
BAD_TWO = {7: "C", 21: "v"}                                                      # different blocks at block 8 (0 and 2) and at block 1
SPOILS = {"v": BAD_V, "h": BAD_H, "C": BAD_C, "pi": BAD_PI, "two": BAD_TWO}
assert INF == bytes(96)
