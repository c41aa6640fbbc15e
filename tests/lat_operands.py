"""Raw representatives for the unit programs of the latency path (bls_amd/csrc/gen_lat.py: UNIT_PROGRAMS; tests/test_gpu_lat_units.py).

An entry is a list of 15 int32 limbs, taken by the kernel as they are: value = sum limb_i 2^(27 i).  The contract is that of an `in` node of the
program generator (L = 1, V = 1): |limb| <= 2^27 + 64 and |value| <= q -- checked at the bottom of this module.  Real curve data gives uniformly
distributed canonical limbs; the entries here sit where the limb arithmetic has the least room: every limb at its bound with equal or alternating
signs, the corners of the normalised range, the representatives of 0 and 1 that are not canonical, values within eps of +-q.  A plain module; no GPU."""
import edge_operands as E
from oracle import pyref as P

Q = P.Q
NL, LB = 15, 27
BOUND = (1 << LB) + 64                     # |limb| of an L = 1 element (fp.cuh: Fp<1, V>)
TOP = LB * (NL - 1)
R = 1 << (NL * LB)                         # Montgomery R of the device representation


def value(limbs):
    return sum(int(l) << (LB * i) for i, l in enumerate(limbs))


def canon(v):
    """the canonical limbs of 0 <= v < 2^405"""
    assert 0 <= v < R
    return [(v >> (LB * i)) & ((1 << LB) - 1) for i in range(NL)]


def neg(limbs):
    return [-l for l in limbs]


def with_top(low14, largest=True):
    """low14 and the largest (smallest) top limb that keeps |value| <= q"""
    low = value(low14)
    t = (Q - low) >> TOP if largest else -((Q + low) >> TOP)
    return list(low14) + [t]


QL = canon(Q)
ALL_PLUS = with_top([BOUND] * 14)                                          # top limb 5
ALL_MINUS = with_top([-BOUND] * 14)
ALT0 = with_top([BOUND if i % 2 == 0 else -BOUND for i in range(14)])       # top limb 7
ALT1 = with_top([-BOUND if i % 2 == 0 else BOUND for i in range(14)])
assert ALL_PLUS[14] == 5 and ALT0[14] == 7


def _one_hot(i, s):
    return with_top([s * BOUND if j == i else 0 for j in range(14)])


EXTREME = [ALL_PLUS, ALL_MINUS, ALT0, ALT1] + [_one_hot(i, s) for i in range(14) for s in (1, -1)]
EXTREME += [with_top(e[:14], largest=False) for e in (ALL_PLUS, ALL_MINUS, ALT0, ALT1)]      # the same lower limbs under the most negative top limb
EXTREME += [neg(e) for e in EXTREME]

# the corners of the range a limb normalisation leaves (fp_norm: limbs 0..13 in [-16, 2^27 + 16))
_LO, _HI = -16, (1 << LB) + 15
CORNERS = [with_top([_LO] * 14), with_top([_HI] * 14), with_top([_HI if i % 2 else _LO for i in range(14)]), with_top([_LO if i % 2 else _HI for i in range(14)]),
           [_LO] * 14 + [0], [_HI] * 14 + [0], with_top([_HI] * 14, largest=False)]


def _minus_q(limbs):
    return [a - b for a, b in zip(limbs, QL)]


ONE = R % Q                                # the field element 1 in the device representation
ZERO_REPS = [[0] * NL, list(QL), neg(QL), [1 << LB, -1] + [0] * 13, [-(1 << LB), 1] + [0] * 13]
ONE_REPS = [canon(ONE), _minus_q(canon(ONE)), [canon(ONE)[0] - (1 << LB), canon(ONE)[1] + 1] + canon(ONE)[2:]]
# the raw values 1 and -1 (NOT the field element 1: check1 compares with R mod q) and their other representatives
SPECIAL = ZERO_REPS + ONE_REPS + [canon(1), _minus_q(canon(1)), neg(canon(1)), neg(_minus_q(canon(1))), neg(canon(ONE)), canon(Q - ONE)]
NEAR_Q = [canon(Q - eps) for eps in E.NEAR_Q_EPS]
NEAR_Q_NEG = [neg(x) for x in NEAR_Q]

RESIDUES = [canon(d) for d in E.device_residues(LB, NL)]


def _random(xs, n):
    out = []
    for k in range(n):
        if k % 2 == 0:                                                      # a random value, canonical
            out.append(canon(P.rand_int(xs, Q)))
        else:                                                               # a random representative: any lower limbs inside the bound, a top limb that keeps |value| <= q
            low14 = [P.rand_int(xs, 2 * BOUND + 1) - BOUND for _ in range(14)]
            lo, hi = with_top(low14, largest=False)[14], with_top(low14)[14]
            out.append(low14 + [lo + P.rand_int(xs, hi - lo + 1)])
    return out


RANDOM = _random(P.XORShift(2027), 48)

CORPUS = RESIDUES + EXTREME + CORNERS + SPECIAL + NEAR_Q + NEAR_Q_NEG + RANDOM

for _e in CORPUS:                                                           # the input contract
    assert len(_e) == NL and all(abs(l) <= BOUND for l in _e) and abs(value(_e)) <= Q, _e
assert all(value(z) % Q == 0 for z in ZERO_REPS) and all(value(o) % Q == ONE for o in ONE_REPS)
