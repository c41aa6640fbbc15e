"""The model and the corpus of the wire-byte blob tests (blsmi 0.23: blsmi_kzg_blob_challenge_batch*, blsmi_kzg_verify_blob_batch_wire*), in
Python big integers and hashlib: the Fiat-Shamir challenge z = SHA-256("FSBLOBVERIFY_V1_" || N as 16 bytes || blob || commitment) mod r, stated
twice -- through hashlib over the whole message, and through the N / 2 + 2 padded blocks built by hand and a pure-Python compression
function, which pins the block layout bls_amd/csrc/sha256_fs.h encodes --, and blob batches from compressed points on the key of
tests/kzg_cases.py: tau is known there, so C = [p(tau)] G and pi = [(p(tau) - y) / (tau - z)] G hold by construction for the z the bytes give.
The rule of the call for an item with status != 0 is in WireCase.expect."""
import hashlib
import random

from fr_eval_cases import TOP, evaluate
from kzg_cases import INF, R, KzgCase, g1_neg
from oracle import pyref as P
from pprod_rlc_locate_common import rechecked_of

PREFIX = b"FSBLOBVERIFY_V1_"
ORDER = 1                                                                        # a blob's values lie in bit-reversed order
INF48 = bytes([0xc0]) + bytes(47)
# (value 0 of a blob of four values, the rest zero, with the infinity commitment) -> floor(digest / r): the three branches of the reduction
QUOTIENT_CASES = ((0, 0), (3, 1), (13, 2))


# the batch both test files use: 37 items of 16 values.  Every spoiled item is an item without an edge; 7 and 21 lie in different blocks at
# block 8 (0 and 2) and at block 1; item 5 shares block 0 with the rejected items 0 .. 4's v + r item.
M, K, SEED = 37, 4, 23
EDGES = {0: "zero", 2: "const", 4: ("noncanon", 5), 9: ("errC", 1), 10: ("errC", 2), 11: ("errC", 3), 12: ("errC", 4),
         17: ("errPi", 1), 18: ("errPi", 2), 19: ("errPi", 3), 20: ("errPi", 4), 26: "ff"}
STATUS_OF_EDGE = {4: 0x40, 9: 1, 10: 2, 11: 3, 12: 4, 17: 1 << 3, 18: 2 << 3, 19: 3 << 3, 20: 4 << 3, 26: 2 | 2 << 3}
SPOILS = {"f": {5: "f"}, "C": {30: "C"}, "pi": {33: "pi"}, "two": {7: "C", 21: "f"}}


def message(blob_bytes, k, c48):
    n = 1 << k
    assert len(blob_bytes) == 32 * n and len(c48) == 48
    return PREFIX + n.to_bytes(16, "big") + bytes(blob_bytes) + bytes(c48)


def digest(blob_bytes, k, c48):
    return int.from_bytes(hashlib.sha256(message(blob_bytes, k, c48)).digest(), "big")


def challenge(blob_bytes, k, c48):
    """z as an integer below r"""
    return digest(blob_bytes, k, c48) % R


# ---- the same by blocks ------------------------------------------------------------------------------------------------------------------
_K = [0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3,
      0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
      0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
      0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
      0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
      0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
_H0 = (0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19)
_M = 0xffffffff


def _rotr(x, n):
    return (x >> n | x << (32 - n)) & _M


def compress(h, block):
    """one application of SHA-256's compression function (FIPS 180-4, 6.2.2) to the 64-byte block"""
    assert len(block) == 64
    w = [int.from_bytes(block[4 * i:4 * i + 4], "big") for i in range(16)]
    for i in range(16, 64):
        s0 = _rotr(w[i - 15], 7) ^ _rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)
        s1 = _rotr(w[i - 2], 17) ^ _rotr(w[i - 2], 19) ^ (w[i - 2] >> 10)
        w.append((w[i - 16] + s0 + w[i - 7] + s1) & _M)
    a, b, c, d, e, f, g, hh = h
    for i in range(64):
        t1 = (hh + (_rotr(e, 6) ^ _rotr(e, 11) ^ _rotr(e, 25)) + ((e & f) ^ (~e & _M & g)) + _K[i] + w[i]) & _M
        t2 = ((_rotr(a, 2) ^ _rotr(a, 13) ^ _rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & _M
        a, b, c, d, e, f, g, hh = (t1 + t2) & _M, a, b, c, (d + t1) & _M, e, f, g
    return tuple((x + y) & _M for x, y in zip(h, (a, b, c, d, e, f, g, hh)))


def padded_blocks(blob_bytes, k, c48):
    """the N / 2 + 2 blocks (N = 1: 2) of the padded message, each put together from its sources by hand -- no concatenated message exists"""
    n = 1 << k
    blob, c48 = bytes(blob_bytes), bytes(c48)
    assert len(blob) == 32 * n and len(c48) == 48
    head = PREFIX + bytes(12) + n.to_bytes(4, "big")                             # 16 + 16 bytes
    bits = ((32 * n + 80) * 8).to_bytes(8, "big")
    if n == 1:
        return [head + blob, c48 + b"\x80" + bytes(7) + bits]                   # its own tail: the whole commitment and the padding share block 1
    out = [head + blob[:32]]                                                     # block 0: the prefix and value 0
    out += [blob[64 * i - 32:64 * i + 32] for i in range(1, n // 2)]             # 32 bytes off the block grid
    out.append(blob[32 * n - 32:] + c48[:32])                                    # block N / 2: the last value and 32 bytes of the commitment
    out.append(c48[32:] + b"\x80" + bytes(39) + bits)                            # the commitment's last 16 bytes, 0x80, zeros, the bit length
    assert len(out) == n // 2 + 2
    return out


def digest_by_blocks(blob_bytes, k, c48):
    h = _H0
    for b in padded_blocks(blob_bytes, k, c48):
        h = compress(h, b)
    return int.from_bytes(b"".join(x.to_bytes(4, "big") for x in h), "big")


def challenge_by_blocks(blob_bytes, k, c48):
    return digest_by_blocks(blob_bytes, k, c48) % R


def quotient_blob(v0):
    """the blob of four values whose value 0 is the integer v0, the rest zero"""
    return v0.to_bytes(32, "big") + bytes(96)


# ---- compressed points ---------------------------------------------------------------------------------------------------------------------
def compress_record(rec):
    """a 96-byte affine record (all zero: infinity) as the 48 compressed bytes"""
    return P.g1_compress(None if rec == INF else (int.from_bytes(rec[:48], "big"), int.from_bytes(rec[48:], "big")))


_ERRORS = {"unexpected compression mode": 1, "unexpected information in compressed infinity": 2, "point not on curve": 3, "not in correct subgroup": 4}


def decode(c48):
    """(error code of blsmi_g1_decompress_batch with check = 1, the affine record -- all zero for infinity and for an error) by the oracle"""
    try:
        a = P.g1_decompress(bytes(c48))
    except P.DecodeError as e:
        return _ERRORS[str(e)], INF
    return 0, (INF if a is None else P.g1_serialize(a))


def outside_point48():
    """a curve point outside the subgroup (tests/point_check_cases.py), compressed; its x is not 0"""
    import point_check_cases as PC
    a = next(a for label, _, a in PC.finite_points(1) if label == "outside" and a[0] != 0)
    assert P.g1_on_curve(a) and not P.g1_in_subgroup(a)
    return P.g1_compress(a)


def off_curve48():
    """x = 1: 1 + 4 = 5 is no square mod q"""
    assert P.g1_from_x(1, False) is None
    return bytes([0x80]) + bytes(46) + b"\x01"


def bad_point48(code, good48):
    """48 bytes that decode with error `code`; code 1 keeps the bytes of a good point but for the compression bit"""
    if code == 1:
        return bytes([good48[0] & 0x7f]) + good48[1:]
    if code == 2:
        return bytes([0xc0]) + bytes(46) + b"\x01"                               # the infinity bit with information behind it
    return {3: off_curve48, 4: outside_point48}[code]()


class WireCase:
    """m blob proofs from wire bytes under the key of KzgCase(0, seed).  Item j: N = 2^k values f below r (unless an edge says otherwise),
    c = p(tau), C = [c] G, c48 its compression; z = challenge(blob, c48); y = p(z), q = (c - y) / (tau - z), pi = [q] G, p48.
    edge: {item: "zero" | "const" | ("noncanon", position) | ("errC", code) | ("errPi", code) | "ff"}
        zero: the zero blob, C = pi = infinity, valid; const: a constant blob, pi at infinity; noncanon: the value at that position written as
        v + r -- z moves with the bytes and pi is made for that z, so the item holds mod r, and is rejected; errC / errPi: the commitment /
        the proof replaced by bytes that decode with that error code (a replaced commitment moves z: pi is made for that z and the true c);
        ff: the zero blob with 48 bytes of 0xff for both points.
    spoil: {item: "f" | "C" | "pi"} -- one blob byte flipped, C replaced by another valid commitment (z moves with it), pi negated, each AFTER
        everything was made."""

    def __init__(self, m, k, seed, edge=None, spoil=None):
        rng = random.Random(seed)
        srng = random.Random(seed + 1)
        edge, spoil = edge or {}, spoil or {}
        key = KzgCase(0, seed)
        self.m, self.k, self.key = m, k, key
        self.srs_g1, self.srs_g2, tau = key.srs_g1, key.srs_g2, key.tau
        n = 1 << k
        self.blobs, self.c48, self.p48, self.c, self.q = [], [], [], [], []
        for j in range(m):
            f = [rng.randrange(R) for _ in range(n)]
            e = edge.get(j)
            if e in ("zero", "ff"):
                f = [0] * n
            elif e == "const":
                f = [f[0]] * n
            elif isinstance(e, tuple) and e[0] == "noncanon":
                f[e[1]] = rng.randrange(TOP - R + 1)                             # so that v + r fits 256 bits
            else:
                assert e is None or (isinstance(e, tuple) and e[0] in ("errC", "errPi")), e
            c = evaluate(f, k, ORDER, tau)
            if isinstance(e, tuple) and e[0] == "noncanon":
                f[e[1]] += R                                                     # the same polynomial mod r
            blob = b"".join(v.to_bytes(32, "big") for v in f)
            c48 = compress_record(key.gmul(c))
            if e == "ff":
                c48 = b"\xff" * 48
            elif isinstance(e, tuple) and e[0] == "errC":
                c48 = bad_point48(e[1], c48)
            z = challenge(blob, k, c48)
            y = evaluate(f, k, ORDER, z)
            q = (c - y) * pow(tau - z, -1, R) % R
            assert (c - y + z * q - q * tau) % R == 0
            p48 = compress_record(key.gmul(q))
            assert e not in ("zero", "const") or p48 == INF48
            assert e != "zero" or c48 == INF48
            if e == "ff":
                p48 = b"\xff" * 48
            elif isinstance(e, tuple) and e[0] == "errPi":
                p48 = bad_point48(e[1], p48 if p48 != INF48 else compress_record(key.gmul(1)))
            kind = spoil.get(j)
            if kind == "f":
                at = srng.randrange(32 * n)
                blob = blob[:at] + bytes([blob[at] ^ (1 << srng.randrange(8))]) + blob[at + 1:]
            elif kind == "C":
                c = (c + 1) % R
                c48 = compress_record(key.gmul(c))
            elif kind == "pi":
                q = (-q) % R
                p48 = compress_record(g1_neg(key.gmul(-q)))
            else:
                assert kind is None, kind
            self.blobs.append(blob); self.c48.append(c48); self.p48.append(p48); self.c.append(c); self.q.append(q)
        # of the bytes as they are handed over
        self.z = [challenge(b, k, c) for b, c in zip(self.blobs, self.c48)]
        self.polys = [[int.from_bytes(b[32 * i:32 * i + 32], "big") for i in range(n)] for b in self.blobs]
        self.y = [evaluate(f, k, ORDER, z) for f, z in zip(self.polys, self.z)]
        self.noncanon = [any(v >= R for v in f) for f in self.polys]
        dc, dp = [decode(c) for c in self.c48], [decode(p) for p in self.p48]
        self.status = [ec | ep << 3 | int(nc) << 6 for (ec, _), (ep, _), nc in zip(dc, dp, self.noncanon)]
        self.C, self.pi = [r for _, r in dc], [r for _, r in dp]                 # the oracle's affine records (all zero for an error)
        self.poly_bytes, self.commitments48, self.proofs48 = b"".join(self.blobs), b"".join(self.c48), b"".join(self.p48)
        self.z_bytes = b"".join(z.to_bytes(32, "big") for z in self.z)

    def equation(self):
        """by big integers alone, for the items both of whose points decode: c - y + z q = q tau mod r for the discrete logarithms handed over"""
        tau = self.key.tau
        return [int((c - y + z * q - q * tau) % R == 0) if st & 0x3f == 0 else None for c, y, z, q, st in zip(self.c, self.y, self.z, self.q, self.status)]

    def verdicts(self):
        """ok[j] = 1 exactly when status[j] == 0 and the equation holds"""
        return [int(st == 0 and eq == 1) for st, eq in zip(self.status, self.equation())]

    def expect(self, block):
        """(ok, status, combined, rechecked) of the call at `block`.  An item with status != 0 is cleared to (infinity, infinity, 0) before the
        combined check and so fails no block: combined = 1 exactly when every item with status 0 holds; rechecked: the summed sizes of the
        blocks in which an item with status 0 fails, cleared items counted as their blocks' items."""
        bad = tuple(j for j, (st, eq) in enumerate(zip(self.status, self.equation())) if st == 0 and eq == 0)
        return self.verdicts(), list(self.status), 0 if bad else 1, rechecked_of(self.m, block, bad)
