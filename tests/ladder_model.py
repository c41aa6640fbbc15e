"""Integer model of the ADDITIONS every scalar-multiplication ladder performs, and the scalars for which one of them is exceptional.

For a point P of the prime-order subgroup every value a ladder holds is [a] P with a known residue a mod r, so the whole ladder can be
traced with plain integers: trace(k) lists its additions as (step, accumulator mod r, addend mod r).  Residue 0 is the point at infinity.
An addition whose two residues are equal and non-zero is the "same point, so double" branch of jac_add_affine_i / jac_add_i
(bls_amd/csrc/curve.cuh:52-107); residues that add up to r are the "opposite points, so infinity" branch.  An infinite accumulator or a
zero digit is no event: those go through the selects at the end of the addition.

The schedules restated here (the decompositions and the Booth recoding are glv_model's, imported):

  glv_g1, glv_g2   glv_mul, bls_amd/csrc/glv.cuh:171-188 -- windows w = NWIN - 1 .. 0 of signed 5-bit digits, five doublings before every
                   window but the first, inside a window the streams s = 0 .. NS - 1 in order; the addend of stream s is digit * mult[s]
                   with mult = (1, z^2) for G1 (glv_endo_s: -phi = [z^2]) and (1, z, z^2, z^3) for G2 (the signs of psi folded in).
                   step = (w, s).  The table 2 P .. 16 P is built by doublings and by (j - 1) P + P for odd j: never exceptional.
  plain4           mul_batch_body, bls_amd/csrc/k_curve.hip:71-91 -- 64 nibbles, most significant first, four doublings before every
                   nibble but the first, res + tab[nibble] with the GENERAL addition (both operands under their own Z).  step = the index
                   of the nibble, 0 .. 63.  plain4_table() is the construction tab[j] = tab[j - 1] + P (k_curve.hip:78-80), which doubles
                   at j = 2 for every point of order above 2 and holds infinity for a point of order below 16.
  fixed_lane       mul_fixed_body, k_curve.hip:208-218 -- sum over w = 0 .. 31 of T[w][byte w], least significant byte first, no
                   doublings.  step = w.
  fixed_wave       mul_fixed_wave_body, k_curve.hip:232-244 -- lane t < 32 holds T[t][byte t], lanes 32 .. 63 infinity; for off = 16, 8,
                   4, 2, 1 EVERY lane adds the value of lane t + off to its own (a lane whose partner lies beyond the wave reads itself:
                   __shfl_down; those lanes are infinite).  step = (off, t) for t < 32; lane 0 of the last level is the result, the lanes
                   t >= off of a level compute sums nobody reads.
  lat_mul1/2       build_mul_program, bls_amd/csrc/gen_lat.py:1137-1146 -- windows w = NWIN - 1 .. 0 of UNSIGNED 4-bit digits of each
                   sub-scalar, four doublings of R, U = S0 + S1 (G2: (S0 + S1) + (S2 + S3)), R = R + U.  step = (w, "S0+S1" | "S2+S3" |
                   "U+V" | "R+U").  These are the complete projective formulas: an event there takes no branch at all.

Where an event can be.  A collision needs  sum_i prefix_i mult_i = +-addend (mod r)  with a non-zero left side.  As an INTEGER the left
side is about k / 2^(bits still to come), and k < 2^256 < 3 r: it reaches r or 2 r only in the last window (glv, plain4, lat_mul), in the top
window (fixed_lane) and, for fixed_wave, in the last level, where lane 0 adds the bytes at odd places to the bytes at even places.  corpus()
therefore enumerates, for m = 1, 2, every stream / window / level, every digit and both kinds, the k = m r + (what the remaining additions
contribute), keeps what is below 2^256, and lets the TRACE decide: an entry is in the corpus only if its trace shows the event.  Below r the
sub-scalars are the canonical ones and no event occurs (tests/test_ladder_collisions_cpu.py samples that)."""
import functools
import os
import sys
from collections import namedtuple

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bls_amd", "csrc"))
import glv_model as M  # noqa: E402

R = M.R_ORDER
Z = M.Z
TOP = 1 << 256
LADDERS = ("glv_g1", "glv_g2", "plain4", "fixed_lane", "fixed_wave", "lat_mul1", "lat_mul2")

Trace = namedtuple("Trace", "adds events result")          # adds: (step, acc, addend); events: (kind, step); result: the last value mod r
Entry = namedtuple("Entry", "ladder kind step k")


def events_of(adds, order=R):
    out = []
    for step, acc, add in adds:
        if acc == 0 or add == 0:
            continue
        if acc == add:
            out.append(("same", step))
        elif (acc + add) % order == 0:
            out.append(("opposite", step))
    return out


def _trace(adds, result, order=R):
    return Trace(adds, events_of(adds, order), result)


# ---- the endomorphism ladders ----------------------------------------------------------------------------------------------------------
GLV = {1: (M.G1_NWIN, (1, M.Z2 % R), lambda k: list(M.decompose_g1(k))),
       2: (M.G2_NWIN, (1, Z, Z**2 % R, Z**3 % R), M.decompose_g2)}
GLV_INT = {1: (1, M.Z2), 2: (1, Z, Z**2, Z**3)}              # the streams' multipliers as integers


def glv(group, k):
    nwin, mult, decompose = GLV[group]
    digs = [M.booth_digits(v, 5, nwin) for v in decompose(k)]
    adds, acc = [], 0
    for w in range(nwin - 1, -1, -1):
        if w != nwin - 1:
            acc = acc * 32 % R
        for s, dig in enumerate(digs):
            add = dig[w] * mult[s] % R
            adds.append(((w, s), acc, add))
            acc = (acc + add) % R
    return _trace(adds, acc)


# ---- the plain 4-bit ladder ------------------------------------------------------------------------------------------------------------
def plain4(k, order=R):
    """order: the order of the point (a point outside the subgroup: the residues are taken modulo ITS order)"""
    adds, acc = [], 0
    for i in range(64):
        if i:
            acc = acc * 16 % order
        add = ((k >> (4 * (63 - i))) & 15) % order
        adds.append((i, acc, add))
        acc = (acc + add) % order
    return _trace(adds, acc, order)


def plain4_table(order=R):
    """tab[j] = tab[j - 1] + P for j = 2 .. 15 -> the trace; step = j"""
    adds = [(j, (j - 1) % order, 1 % order) for j in range(2, 16)]
    return _trace(adds, 15 % order, order)


# ---- the fixed-base forms --------------------------------------------------------------------------------------------------------------
def _byte(k, w):
    return (k >> (8 * w)) & 255


def fixed_lane(k):
    adds, acc = [], 0
    for w in range(32):
        add = (_byte(k, w) << (8 * w)) % R
        adds.append((w, acc, add))
        acc = (acc + add) % R
    return _trace(adds, acc)


def fixed_wave(k):
    v = [(_byte(k, t) << (8 * t)) % R for t in range(32)] + [0] * 32
    adds = []
    for off in (16, 8, 4, 2, 1):
        other = [v[t + off] if t + off < 64 else v[t] for t in range(64)]      # every lane reads before any lane writes
        adds += [((off, t), v[t], other[t]) for t in range(32)]
        v = [(a + b) % R for a, b in zip(v, other)]
    return _trace(adds, v[0])


# ---- the level programs ----------------------------------------------------------------------------------------------------------------
LAT_NWIN = {1: M.G1_LAT_NWIN, 2: M.G2_LAT_NWIN}


def lat_mul(group, k):
    nwin, (_, mult, decompose) = LAT_NWIN[group], GLV[group]
    subs = decompose(k)
    assert all(v < 1 << (4 * nwin) for v in subs)
    adds, acc = [], None
    for w in range(nwin - 1, -1, -1):
        s = [((v >> (4 * w)) & 15) * m % R for v, m in zip(subs, mult)]
        adds.append(((w, "S0+S1"), s[0], s[1]))
        u = (s[0] + s[1]) % R
        if group == 2:
            adds.append(((w, "S2+S3"), s[2], s[3]))
            v = (s[2] + s[3]) % R
            adds.append(((w, "U+V"), u, v))
            u = (u + v) % R
        if acc is None:
            acc = u
        else:
            acc = acc * 16 % R
            adds.append(((w, "R+U"), acc, u))
            acc = (acc + u) % R
    return _trace(adds, acc)


TRACE = {"glv_g1": lambda k: glv(1, k), "glv_g2": lambda k: glv(2, k), "plain4": plain4, "fixed_lane": fixed_lane, "fixed_wave": fixed_wave,
         "lat_mul1": lambda k: lat_mul(1, k), "lat_mul2": lambda k: lat_mul(2, k)}


# ---- candidates, by construction -------------------------------------------------------------------------------------------------------
def _digit_walk(group, k0, first, digit0, choices, scale=1):
    """Every k = k0 + scale sum_{j >= first} c_j mult_j (c_j from choices) in which c_j is what digit0 reads from stream j of k itself.
    mult_j = z^(2 j) (G1) / z^j (G2) and sub-scalar i is a base-mult digit of k, so adding a multiple of mult_j leaves the sub-scalars of
    the streams below j as they are: the condition on stream j is final once c_j is in, and the walk prunes there."""
    mult, decompose = GLV_INT[group], GLV[group][2]
    out = []

    def walk(j, k):
        if j == len(mult):
            out.append(k)
            return
        for c in choices:
            kk = k + scale * c * mult[j]
            if 0 < kk < TOP and digit0(decompose(kk)[j]) == c:
                walk(j + 1, kk)
    walk(first, k0)
    return out


def _glv_candidates(group):
    """last window (w = 0), the addition of stream s: the accumulator is k - d mult_s - sum_{j > s} e_j mult_j with d, e_j the streams' last
    Booth digits.  Same point: that is d mult_s (mod r), so k = m r + 2 d mult_s + sum e_j mult_j; opposite: k = m r + sum e_j mult_j."""
    nwin, _, decompose = GLV[group]
    mult = GLV_INT[group]
    booth0 = lambda v: M.booth_digits(v, 5, nwin)[0]          # noqa: E731
    out = set()
    for m in (1, 2):
        for s in range(len(mult)):
            for d in range(-16, 17):                          # d = 0 stands for the opposite-points form: the digit is then free
                k0 = m * R + 2 * d * mult[s]
                if not 0 < k0 < TOP:
                    continue
                d0 = booth0(decompose(k0)[s])
                if d0 == 0 or (d and d0 != d):
                    continue
                out.update(_digit_walk(group, k0, s + 1, booth0, range(-16, 17)))
    return out


def _lat_candidates(group):
    """last window, R + U: R = k - U with U = sum c_j mult_j over the streams' last nibbles.  Same: k = m r + 2 U; opposite: k = m r."""
    out = {R, 2 * R}
    for m in (1, 2):
        out.update(_digit_walk(group, m * R, 0, lambda v: v & 15, range(16), 2))
    return out


def _plain4_candidates():
    """last nibble: 16 prefix = k - nib.  Same: k = m r + 2 nib; opposite: k = m r"""
    return {m * R + 2 * nib for m in (1, 2) for nib in range(16)}


def _fixed_lane_candidates():
    """window w: the accumulator is L = k mod 256^w, an integer below 256^w <= 2^248 < r; the addend is d 256^w.  Same: L = d 256^w - m r,
    the bytes above w free (none are left where that is positive); opposite: L + d 256^w = m r"""
    out = {R, 2 * R}
    for m in (1, 2):
        for w in range(32):
            for d in range(1, 256):
                low = (d << (8 * w)) - m * R
                if 0 < low < 1 << (8 * w):
                    out.add(low + (d << (8 * w)))
    return out


def _solve_supported(m, sx, sy):
    """X = Y + m r with the bytes of X confined to the places sx and those of Y to sy (disjoint) -> (X, Y) or None.  From the lowest byte up:
    at a place of sy the byte of Y is the one that zeroes the sum, at a place of sx the sum is X's byte, anywhere else it has to be zero."""
    x = y = carry = 0
    for p in range(32):
        t = _byte(m * R, p) + carry
        if p in sy:
            b = -t % 256
            y |= b << (8 * p)
            t += b
        if p in sx:
            x |= (t & 255) << (8 * p)
        elif t & 255:
            return None
        carry = t >> 8
    return None if carry else (x, y)


def _fixed_wave_candidates():
    """level off, lane t < off: A = the bytes at the places t mod 2 off, B = those at t + off mod 2 off.  Same: A - B = +- m r, solved byte by
    byte; opposite: A + B = m r, which needs m r to have no other bytes (off = 1: k = m r).  Bytes at other places belong to other lanes."""
    out = {R, 2 * R}
    for off in (16, 8, 4, 2, 1):
        for t in range(off):
            sa = {p for p in range(32) if p % (2 * off) == t}
            sb = {p for p in range(32) if p % (2 * off) == t + off}
            for m in (1, 2):
                for sx, sy in ((sa, sb), (sb, sa)):
                    xy = _solve_supported(m, sx, sy)
                    if xy and xy[0] + xy[1] < TOP:
                        out.add(xy[0] + xy[1])
                if all(_byte(m * R, p) == 0 for p in range(32) if p not in sa | sb):
                    out.add(m * R)
    return out


CANDIDATES = {"glv_g1": lambda: _glv_candidates(1), "glv_g2": lambda: _glv_candidates(2), "plain4": _plain4_candidates,
              "fixed_lane": _fixed_lane_candidates, "fixed_wave": _fixed_wave_candidates,
              "lat_mul1": lambda: _lat_candidates(1), "lat_mul2": lambda: _lat_candidates(2)}


@functools.lru_cache(maxsize=None)
def corpus(ladder):
    """every constructed scalar below 2^256 whose trace has an event, one Entry per event, sorted by (k, step)"""
    out = []
    for k in sorted(CANDIDATES[ladder]()):
        if 0 < k < TOP:
            out += [Entry(ladder, kind, step, k) for kind, step in TRACE[ladder](k).events]
    return tuple(out)


def scalars(ladder, kind=None):
    """the distinct scalars of a ladder's corpus, ascending"""
    return sorted({e.k for e in corpus(ladder) if kind in (None, e.kind)})
