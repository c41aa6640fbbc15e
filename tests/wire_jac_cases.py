"""The corpora of the wire-format <-> in-memory-point tests (blsmi 0.15: blsmi_g?_decompress_batch_jac[_dev], blsmi_g?_compress_batch_jac[_dev]),
judged by oracle.pyref alone.  Per group:

  decompression   compressed encodings and what DecompressG? + the subgroup test + ToProjective make of them: subgroup points with both signs of
                  y, the infinity encoding, 0xc0 with a stray bit (err 2), the compression bit missing (err 1), an x with no y on the curve (err 3),
                  curve points outside the subgroup (err 4 under check 1 / 2, a usable point under check 0), an x field whose value is not below q
                  (read as 0, as FQReprToFQ reads it)
  compression     in-memory records and the bytes of Compress(ToAffine): runs of z == 1 and of z != 1 laid out against the 64-lane wave, z == 0 with
                  non-zero x and y, limb images that are not below q, and y on either side of the sign boundary under z != 1 (no curve test, so these
                  need not be curve points)

Everything is seeded: the same corpus in every process.  No GPU."""
import functools
from collections import namedtuple

import numpy as np

import group_edges as G
import point_check_cases as K
from gpu_common import P

Q = P.Q
WB = {1: 48, 2: 96}                       # bytes of a compressed point
JW = {1: 18, 2: 36}                       # words of an in-memory point
HALF_LO, HALF_HI = (Q - 1) // 2, (Q + 1) // 2
_CODES = (("compression mode", 1), ("unexpected information", 2), ("not on curve", 3))

# blob: the encoding; err / inf / point: DecompressG? of it WITHOUT a subgroup test (point None unless err == inf == 0); outside: the point is on
# the curve but not in the subgroup, so check 1 / 2 turn it into err 4
Encoding = namedtuple("Encoding", "label blob err inf point outside")


def compress(group, a):
    return P.g1_compress(a) if group == 1 else P.g2_compress(a)


def _decode(group, blob):
    try:
        a = (P.g1_decompress_unchecked if group == 1 else P.g2_decompress_unchecked)(blob)
    except P.DecodeError as e:
        return next(code for text, code in _CODES if text in str(e)), 0, None
    return 0, 1 if a is None else 0, a


def _encoding(group, label, blob):
    err, inf, a = _decode(group, bytes(blob))
    outside = a is not None and K.oracle_status(group, a) == K.NOT_IN_SUBGROUP
    return Encoding(label, bytes(blob), err, inf, a, outside)


def _no_y(group, n):
    """x values (small integers; G2: (k, 1)) for which x^3 + b is no square"""
    out, k = [], 1
    while len(out) < n:
        x = k if group == 1 else (k, 1)
        if (P.g1_from_x if group == 1 else P.g2_from_x)(x, False) is None:
            out.append(x)
        k += 1
    return out


def _raw_x(group, x, flags=0x80):
    """an encoding from raw 48-byte x fields (G2: (c0, c1), c1 first on the wire), which may hold values that are not below q"""
    b = bytearray(x.to_bytes(48, "big") if group == 1 else x[1].to_bytes(48, "big") + x[0].to_bytes(48, "big"))
    b[0] |= flags
    return b


@functools.lru_cache(maxsize=None)
def encodings(group):
    wb = WB[group]
    out = []
    for a in G.subgroup_points(group) + (K.GENERATOR[group],):              # both signs of y: the point and its negative
        out.append(_encoding(group, "subgroup", compress(group, a)))
        out.append(_encoding(group, "subgroup, -y", compress(group, G.neg(group, a))))
    assert {e.blob[0] & 0x20 for e in out} == {0, 0x20}
    inf = bytes([0xc0]) + bytes(wb - 1)
    out.append(_encoding(group, "infinity", inf))
    for pos, bit in ((0, 0x20), (0, 0x01), (1, 0x80), (wb - 1, 0x01), (wb // 2, 0x10)):
        b = bytearray(inf); b[pos] |= bit
        out.append(_encoding(group, "infinity with a stray bit", b))
    for a in G.subgroup_points(group)[:2]:
        b = bytearray(compress(group, a)); b[0] &= 0x7f
        out.append(_encoding(group, "compression bit missing", b))
    out.append(_encoding(group, "compression bit missing", bytes([0x40]) + bytes(wb - 1)))
    out.append(_encoding(group, "compression bit missing", bytes(wb)))
    for x in _no_y(group, 3):
        out.append(_encoding(group, "no y", _raw_x(group, x)))
        out.append(_encoding(group, "no y", _raw_x(group, x, 0xa0)))
    for a in G.outside_points(group) + G.x_zero_points(group):
        out.append(_encoding(group, "curve point", compress(group, a)))
    big = (Q, Q + 5, (1 << 381) - 1)                                          # x fields that are not below q (381 bits: the flag bits stay free)
    zero_c0, zero_c1 = ([a[0] for a in G.x_zero_points(2) if a[0][k] == 0][0] for k in (0, 1))   # G2: x = (0, t) and (t, 0) with a y on the curve
    for v in big:
        for flags in (0x80, 0xa0):
            out.append(_encoding(group, "x >= q", _raw_x(group, v if group == 1 else (zero_c1[0], v), flags)))
            if group == 2:
                out.append(_encoding(group, "x >= q", _raw_x(group, (v, zero_c0[1]), flags)))
                out.append(_encoding(group, "x >= q", _raw_x(group, (v, 2), flags)))
    want = {(1, 0), (2, 0), (3, 0), (0, 1), (0, 0)}
    assert {(e.err, e.inf) for e in out} == want and any(e.outside for e in out) and any(e.point and not e.outside for e in out)
    return tuple(out)


def expect(group, e, check):
    """(err, inf, point) of blsmi_g?_decompress_batch for the encoding under check 0 / 1 / 2"""
    if e.outside and check:
        return 4, 0, None
    return e.err, e.inf, e.point


def memory_record(group, a):
    """G?Affine.ToProjective as it lies in memory: (x, y, 1), and the reference's zero point (0, 1, 0) for None"""
    F = G.FIELD[group]
    return G.record(group, (F.zero, F.one, F.zero) if a is None else (a[0], a[1], F.one))


def wire_record_as_memory(group, rec, unusable):
    """big integers: the in-memory form of an affine wire record as blsmi_g?_decompress_batch hands it back"""
    if unusable or not any(rec):
        return memory_record(group, None)
    return memory_record(group, G.unwire(group, bytes(rec)))


def take(cs, n, start=0):
    """n cases in corpus order from `start`, wrapping round"""
    return [cs[(start + i) % len(cs)] for i in range(n)]


# ---- compression -------------------------------------------------------------------------------------------------------------------------
def read_record(group, rec):
    """the (X, Y, Z) a loader reads from an in-memory record: a limb image that is not below q is 0"""
    v = []
    for i in range(JW[group] // 6):
        raw = P.from_limbs64([int(w) for w in rec[6 * i:6 * i + 6]])
        v.append(P.from_mont(raw) if raw < Q else 0)
    return tuple(v) if group == 1 else ((v[0], v[1]), (v[2], v[3]), (v[4], v[5]))


def oracle_compress(group, rec):
    """Compress(ToAffine(record)) with big integers; z == 0 is infinity whatever x and y hold"""
    jac = read_record(group, rec)
    if jac[2] == G.FIELD[group].zero:
        return compress(group, None)
    return compress(group, K.jacobian_to_affine(group, jac))


def _rand_fq(xs):
    return P.rand_int(xs, Q)


def _rand_xy(group, xs):
    """coordinates of no curve in particular"""
    return (_rand_fq(xs), _rand_fq(xs)) if group == 1 else ((_rand_fq(xs), _rand_fq(xs)), (_rand_fq(xs), _rand_fq(xs)))


def _pool(group, xs, n):
    pts = list(G.base_points(group))
    return [pts[i % len(pts)] if i % 3 else _rand_xy(group, xs) for i in range(n)]


def _z1(group, a):
    return G.record(group, (a[0], a[1], G.FIELD[group].one))


def _zr(group, xs, a):
    return G.record(group, G.scale(group, a, G.rand_z(group, xs)))


def _raw(v):
    return [(v >> (64 * i)) & P.MASK64 for i in range(6)]


@functools.lru_cache(maxsize=None)
def edge_records(group):
    """z == 0 with non-zero x and y, limb images that are not below q, y on either side of the sign boundary under z != 1"""
    xs = P.XORShift(9520 + group)
    F = G.FIELD[group]
    out = [G.record(group, j) for j in G.infinities(group, xs)]
    x = _rand_xy(group, xs)[0]
    if group == 1:
        ys = [HALF_LO, HALF_HI, 0, 1, Q - 1]
    else:
        ys = [(HALF_LO, 0), (HALF_HI, 0), (HALF_LO, HALF_LO), (HALF_HI, HALF_LO), (3, HALF_LO), (3, HALF_HI), (Q - 1, HALF_LO), (Q - 1, HALF_HI), (0, 0), (1, 0), (Q - 1, 0)]
    for y in ys:
        out.append(_zr(group, xs, (x, y)))
        out.append(G.record(group, G.scale(group, (x, y), 2 if group == 1 else (0, 5))))
    for word in range(JW[group] // 6):                                         # every coordinate in turn holds a limb image >= q
        rec = _zr(group, xs, _rand_xy(group, xs))
        rec[6 * word:6 * word + 6] = _raw(Q + word) if word % 2 else _raw((1 << 384) - 1 - word)
        out.append(rec)
    rec = _z1(group, _rand_xy(group, xs)); rec[0:6] = _raw(Q)                  # ... and under z == 1
    out.append(rec)
    assert len({bytes(oracle_compress(group, r))[0] & 0xe0 for r in out}) == 3  # infinity, both signs
    return tuple(out)


@functools.lru_cache(maxsize=None)
def compression_corpus(group):
    """the records laid out against the wave: [0, 64) all z == 1; [64, 128) no z == 1; [128, 192) one z != 1 among 63 (at 165, so that the first
    32 -- a wave of the lane-pair form -- are all z == 1); then the edge records; then z == 1 records with a z != 1 record LAST"""
    xs = P.XORShift(9500 + group)
    pool = _pool(group, xs, 64)
    recs = [_z1(group, a) for a in pool]
    recs += [_zr(group, xs, a) for a in pool]
    recs += [_zr(group, xs, a) if i == 37 else _z1(group, a) for i, a in enumerate(pool)]
    recs += list(edge_records(group))
    recs += [_z1(group, a) for a in pool[:5]] + [_zr(group, xs, pool[5])]
    return np.stack(recs), [oracle_compress(group, r) for r in recs]


@functools.lru_cache(maxsize=None)
def compression_cut(group, n):
    """n records for the ragged sizes: z == 1 records, the edge records among them where there is room, and a z != 1 record LAST -- the clamped
    tail lanes behind it recompute a record that needs the inversion"""
    xs = P.XORShift(9540 + 7 * group + n)
    pool = _pool(group, xs, max(1, n))
    edges = edge_records(group)
    recs = [edges[i // 2 % len(edges)] if i % 2 and n > 8 else _z1(group, pool[i]) for i in range(n - 1)] + [_zr(group, xs, pool[n - 1])]
    return np.stack(recs), [oracle_compress(group, r) for r in recs]
