"""Edge operands for the tower and pairing kernels: records of 6 x u64 Montgomery(2^384) limbs per Fq, as blsmi_debug_op reads them.

Random operands almost never land where limb arithmetic is fragile: a result just below a multiple of q (fp_reduce's fp32 quotient
estimate then leaves it negative and only fp_canon's "+q if negative" step repairs it: see NEAR_Q_EPS), a value on a limb boundary
of the device's own residue, or a degenerate tower element that sends an inversion or the final exponentiation down a special path.
This module builds such operands.  The device holds x * R_dev mod q with R_dev = 2^405 (15 x 27-bit limbs) or 2^392 (14 x 28-bit limbs); both are covered
for every layout, whichever build a unit uses.

Values here are RECORD values: the integer the six limbs hold (x * 2^384 mod q for the field element x), not x itself.  A plain module,
imported by the tests that need it."""
import numpy as np

from oracle import pyref as P
from oracle import refcpu as RC

Q = P.Q
BUILDS = ((27, 15, 405), (28, 14, 392))                   # (bits per limb, limbs, log2 R_dev) of the two limb builds


def record_of_residue(d, log_r):
    """the record whose device residue (x * 2^log_r mod q) is d"""
    return d * pow(2, 384 - log_r, Q) % Q if log_r <= 384 else d * pow(pow(2, log_r - 384, Q), -1, Q) % Q


def _extremes():
    return [0, 1, 2, Q - 1, Q - 2, (Q - 1) // 2, (Q + 1) // 2]


def device_residues(lb, nl):
    """device residues at the edges of one limb build: the extremes, 2^(lb k) and 2^(lb k) - 1 at every limb boundary, alternating-limb masks"""
    out = [0, 1, Q - 1, Q - 2, (Q - 1) // 2, (Q + 1) // 2]
    for k in range(1, nl):
        if (1 << (lb * k)) < Q:
            out += [1 << (lb * k), (1 << (lb * k)) - 1]
    full = (1 << lb) - 1
    for start in (0, 1):
        m = sum(full << (lb * i) for i in range(start, nl, 2))
        out.append(m & ((1 << (Q.bit_length() - 1)) - 1))  # cut to 380 bits: below q
    return out


def fq_values():
    """record values: the reference encoding's extremes, then the device-residue edges of both builds (deduplicated, order kept)"""
    vals = list(_extremes())
    for lb, nl, log_r in BUILDS:
        vals += [record_of_residue(d, log_r) for d in device_residues(lb, nl)]
    seen, out = set(), []
    for v in vals:
        if v not in seen:
            seen.add(v); out.append(v)
    return out


def rec(vals):
    """record values -> one uint64 record (6 limbs per value)"""
    return np.array([w for v in vals for w in P.limbs64(v % Q)], dtype=np.uint64)


def recs(rows):
    return np.stack([rec(r) for r in rows])


# q - eps for small eps: as a RESULT, such a record is where fp_canon needs its "+q if negative" step.  The store path converts a result a
# (any representation) to the record by one Montgomery product with C = 2^384 mod q; when a lies below -q that product is exactly -eps,
# whose two top limbs round to 0 in fp_reduce's fp32 estimate for eps < 2^339 (28-bit limbs; 2^353 with 27-bit limbs): k = 0, and only
# the "+q" step brings -eps back to q - eps.  Random results land there with probability ~2^-40; results TARGETED at these records
# (tests/test_gpu_edges.py: operands solved for with the oracle so that the op's output is one) reach it whenever the layout's own
# arithmetic leaves the value below -q, as negations and differences of products do.
NEAR_Q_EPS = (1, 2, 3, 7, 255, 256, 1 << 20, (1 << 64) + 1, 1 << 128, (1 << 250) + 3, 1 << 330, (1 << 338) + 1)


def near_q_records(n, width):
    """n records whose every value is q - eps, eps cycling through NEAR_Q_EPS"""
    k = len(NEAR_Q_EPS)
    return recs([[Q - NEAR_Q_EPS[(r * 5 + i) % k] for i in range(width)] for r in range(n)])


def rand_records(xs, n, width):
    return recs([[P.rand_int(xs, Q) for _ in range(width)] for _ in range(n)])


MONT_ONE = P.to_mont(1)
MONT_NEG_ONE = P.to_mont(Q - 1)


def tower_rows(width, xs=None):
    """tower elements of `width` Fq (2, 6 or 12), as lists of record values"""
    one, m1 = MONT_ONE, MONT_NEG_ONE
    rows = [[0] * width, [one] + [0] * (width - 1)]                 # zero and one
    rows += [[Q - 1] * width, [m1] * width]                          # every coefficient q-1: as a record, and as the element -1
    rows += [[Q - 1 if i % 2 == 0 else 1 for i in range(width)], [1 if i % 2 == 0 else Q - 1 for i in range(width)]]   # Karatsuba sums at their bounds
    rows += [[m1 if i % 2 == 0 else one for i in range(width)]]
    for j in range(width // 2):                                     # one-hot at every Fq2 position, and (0, 1) / (1, 0) in each slot
        for c in ((Q - 1, Q - 1), (0, one), (one, 0), (0, 1), (1, 0)):
            r = [0] * width; r[2 * j], r[2 * j + 1] = c; rows.append(r)
    vals = fq_values()
    for k in range(0, len(vals), width):                            # the edge values themselves, packed width at a time
        chunk = vals[k:k + width]
        rows.append(chunk + [vals[(k + 3 * i) % len(vals)] for i in range(width - len(chunk))])
    if width == 12:                                                 # monomials c w^k and Fq6-subfield elements (c1 = 0)
        rows += monomial_rows(xs) + subfield_rows(xs)
    return rows


W_SLOT = (0, 3, 1, 4, 2, 5)                                         # Fq2 slot of w^k in the record: w^2 = v


def monomial_rows(xs=None):
    rows = []
    for k in range(6):
        for c in ((MONT_ONE, 0), (0, MONT_ONE), (Q - 1, Q - 1), (MONT_NEG_ONE, 0)) + (((P.rand_int(xs, Q), P.rand_int(xs, Q)),) if xs else ()):
            r = [0] * 12; r[2 * W_SLOT[k]], r[2 * W_SLOT[k] + 1] = c; rows.append(r)
    return rows


def subfield_rows(xs=None):
    rows = [[Q - 1] * 6 + [0] * 6, [MONT_ONE, 0, 0, 0, Q - 1, 1] + [0] * 6, [0, 0, MONT_ONE, 0, 0, 0] + [0] * 6]
    if xs is not None:
        rows += [[P.rand_int(xs, Q) for _ in range(6)] + [0] * 6 for _ in range(3)]
    return rows


def tower_records(width, xs=None):
    return recs(tower_rows(width, xs))


def cyclotomic(records):
    """x^((q^6-1)(q^2+1)) of every record, from the oracle: elements of the cyclotomic subgroup"""
    cyc = []
    for x in records:
        inv = RC.fq12_inverse(x)[1]
        conj = x.copy().reshape(12, 6)
        for k in range(6, 12):
            conj[k] = RC.fq_neg(conj[k])
        t = RC.fq12_mul(conj.reshape(-1), inv)
        cyc.append(RC.fq12_mul(RC.fq12_frobenius(t, 2), t))
    return np.stack(cyc)


def cyclotomic_records(xs, n):
    """the unit, then n random cyclotomic elements"""
    one = rec([MONT_ONE] + [0] * 11)
    return np.concatenate([one[None], cyclotomic(rand_records(xs, n, 12))])
