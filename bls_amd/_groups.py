"""Shared implementation of the g1pubs / g2pubs host mirrors (see g1pubs.py, g2pubs.py)."""
from . import engine


class DeserializeError(ValueError):
    """Mirrors the (nil, error) returns of DeserializePublicKey / DeserializeSignature."""


_DECODE_ERRORS = {1: "unexpected compression mode", 2: "unexpected information in compressed infinity",
                  3: "point not on curve", 4: "not in correct subgroup"}


_Q = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab


def _jac_is_infinity(jac, group):
    """z.IsZero() of an in-memory record (g1.go:287-289, g2.go:325-327); a coordinate not below q reads as 0, as in the library"""
    nc = 1 if group == 1 else 2
    z = jac[48 * 2 * nc:]
    vals = [int.from_bytes(z[48 * e:48 * e + 48], "little") for e in range(nc)]
    return not any(v for v in vals if v < _Q)


class Point:
    """A group element as the library takes it: the affine wire form (96 bytes for G1, 192 for G2; None = infinity) or -- what the
    reference's own types hold, g2pubs/bls.go:13-15, 53-55 -- the in-memory Jacobian record `jac` (bls.G?Projective: 144 / 288 bytes of
    little-endian Montgomery limbs), converted to the wire form by the library only when somebody asks for .raw."""
    __slots__ = ("_raw", "group", "jac", "_inf")

    def __init__(self, raw, group, jac=None):
        self.group = group
        self.jac = None if jac is None else bytes(jac)
        if self.jac is not None:
            if len(self.jac) != (144 if group == 1 else 288):
                raise ValueError("in-memory G%d point: %d bytes" % (group, len(self.jac)))
            self._inf = _jac_is_infinity(self.jac, group)
            self._raw = None
        else:
            self._raw = None if raw is None else bytes(raw)
            self._inf = raw is None

    @property
    def raw(self):
        """ToAffine().SerializeBytes() (None for infinity); for a point held in memory form: one call into the library, cached"""
        if self._raw is None and self.jac is not None and not self._inf:
            fn = engine.g1_jac_to_affine_batch if self.group == 1 else engine.g2_jac_to_affine_batch
            self._raw = fn(self.jac, 1)[0]
        return self._raw

    @property
    def infinity(self):
        return self._inf

    def copy(self):
        return Point(self._raw, self.group, jac=self.jac)

    def bytes_or_zero(self):
        return self.raw if self.raw is not None else bytes(96 if self.group == 1 else 192)

    def __eq__(self, other):
        return isinstance(other, Point) and self.group == other.group and self.raw == other.raw

    def serialize(self):
        """CompressG1 / CompressG2 (g1.go:230-249, g2.go:269-289)."""
        if self.jac is not None:                                              # an in-memory point: ToAffine + Compress in one library call
            fn = engine.g1_compress_batch_jac if self.group == 1 else engine.g2_compress_batch_jac
            return fn(self.jac, 1)[0].tobytes()
        fn = engine.g1_compress_batch if self.group == 1 else engine.g2_compress_batch
        return fn(self.bytes_or_zero(), 1, [1 if self.infinity else 0])[0].tobytes()

    @staticmethod
    def deserialize(data, group):
        """DecompressG1 / DecompressG2 with the subgroup check (g1.go:185-198, g2.go:219-230)."""
        fn = engine.g1_decompress_batch if group == 1 else engine.g2_decompress_batch
        out, inf, err = fn(bytes(data), 1, True)
        if err[0]:
            raise DeserializeError(_DECODE_ERRORS.get(int(err[0]), "decode error"))
        return Point(None if inf[0] else out[0].tobytes(), group)

    @staticmethod
    def deserialize_many(blobs, group):
        """DecompressG? with the subgroup check + ToProjective of every blob in ONE library call -> (in-memory Points, error codes).  The
        point of a blob with an error code is the reference's zero point, as the library hands it back."""
        n = len(blobs)
        if n == 0:
            return [], []
        fn = engine.g1_decompress_batch_jac if group == 1 else engine.g2_decompress_batch_jac
        jac, _, err = fn(b"".join(bytes(b) for b in blobs), n, True)
        return [Point(None, group, jac=jac[i].tobytes()) for i in range(n)], [int(e) for e in err]


def point_sum(points, group):
    """Sequential Add from the zero point in the reference (g2pubs/bls.go:165-192); a tree on the device.  Points that are all held in
    memory form are added as the Jacobian points they are and the sum comes back the same way (blsmi_g?_sum_jac)."""
    n = len(points)
    if n == 0:
        return Point(None, group)
    if all(p.jac is not None for p in points):
        out, inf = (engine.g1_sum_jac if group == 1 else engine.g2_sum_jac)(b"".join(p.jac for p in points), n)
        return Point(None, group, jac=out)
    buf = b"".join(p.bytes_or_zero() for p in points)
    inf = [1 if p.infinity else 0 for p in points]
    fn = engine.g1_sum if group == 1 else engine.g2_sum
    return Point(fn(buf, n, inf), group)


def deserialize_objects(blobs, group, wrap):
    """the batch Deserialize* of the packages: (objects, errors) from one library call; objects[i] is None where errors[i] != 0"""
    pts, err = Point.deserialize_many(blobs, group)
    return [None if e else wrap(p) for p, e in zip(pts, err)], err


def serialize_points(points, group):
    """[p.serialize() for p in points] in one library call where every point is held in memory form (else one call too: the wire-form
    points become z = 1 records on the host, as in point_statuses)"""
    n = len(points)
    if n == 0:
        return []
    fn = engine.g1_compress_batch_jac if group == 1 else engine.g2_compress_batch_jac
    out = fn(b"".join(p.jac if p.jac is not None else _wire_as_jac(p) for p in points), n)
    return [out[i].tobytes() for i in range(n)]


def verify_serialized_randomized(pkg, pk_group, sig_group, msgs, pub_bytes, sig_bytes, block):
    """VerifySerializedBatchRandomized of both packages: two decompressions with the subgroup check into flat in-memory buffers, then the
    package's *_verify_batch_rlc_locate_jac, whose (ok, bitmap, combined, rechecked) comes back.  An undecodable element is the zero point
    there (z == 0): its tuple gets False."""
    n = len(msgs)
    if not (len(pub_bytes) == len(sig_bytes) == n):
        raise ValueError("length mismatch")
    if n == 0:
        return [], b"", 1, 0
    dec = {1: engine.g1_decompress_batch_jac, 2: engine.g2_decompress_batch_jac}
    pk, _, _ = dec[pk_group](b"".join(bytes(b) for b in pub_bytes), n, True)
    sg, _, _ = dec[sig_group](b"".join(bytes(b) for b in sig_bytes), n, True)
    fn = getattr(engine, pkg + "_verify_batch_rlc_locate_jac")
    return fn(msgs, pk.reshape(-1), sg.reshape(-1), None, block)


def all_in_memory(points):
    """True when every point of a call is held as an in-memory Jacobian record: the call takes the *_jac entry point"""
    return len(points) > 0 and all(p.jac is not None for p in points)


def _wire_as_jac(p):
    """the in-memory record of a point held in wire form, read as the library reads the wire record: z = 1 (G?Affine.ToProjective), the
    all-zero record and None as z = 0, a coordinate not below q as 0.  Host big integers: a multiplication by 2^384 per coordinate."""
    nfq = 2 if p.group == 1 else 4
    raw = p._raw
    if raw is None or not any(raw):
        return bytes(48 * nfq * 3 // 2)
    vals = [int.from_bytes(raw[48 * e:48 * e + 48], "big") for e in range(nfq)]
    mont = [((v if v < _Q else 0) << 384) % _Q for v in vals] + [(1 << 384) % _Q] + [0] * (nfq // 2 - 1)
    return b"".join(v.to_bytes(48, "little") for v in mont)


def point_statuses(points, group, check=1):
    """blsmi_g?_check_batch of a list of Points in ONE engine call: the affine form when every point is held in wire form, else the
    in-memory form (the wire-form points of a mixed list become z = 1 records on the host) -> (n,) uint8 of engine.POINT_*"""
    n = len(points)
    if n == 0:
        return []
    if any(p.jac is not None for p in points):
        fn = engine.g1_check_batch_jac if group == 1 else engine.g2_check_batch_jac
        return fn(b"".join(p.jac if p.jac is not None else _wire_as_jac(p) for p in points), n, check)
    fn = engine.g1_check_batch if group == 1 else engine.g2_check_batch
    return fn(b"".join(p.bytes_or_zero() for p in points), n, [1 if p.infinity else 0 for p in points], check)


def points_valid(points, group):
    """[IsOnCurve() && IsInCorrectSubgroupAssumingOnCurve()] (g1.go:93-105, 137-141; g2.go:118-130, 293-295; both true for infinity)"""
    return [int(st) in (engine.POINT_OK, engine.POINT_INFINITY) for st in point_statuses(points, group)]


def flatten_committees(committees):
    """committees (lists of Points) -> (every point in order, the m + 1 segment offsets): the idx = NULL form of the committee entry points
    (blsmi_g?_sum_segmented, *_verify_aggregate_common*_batch)"""
    pts = [p for c in committees for p in c]
    return pts, engine.seg_offsets([len(c) for c in committees])


def committee_sums(committees, group):
    """[point_sum(c, group) for c in committees] as one segmented sum on the device"""
    if not committees:
        return []
    pts, off = flatten_committees(committees)
    if all_in_memory(pts):
        fn = engine.g1_sum_segmented_jac if group == 1 else engine.g2_sum_segmented_jac
        out, inf = fn(b"".join(p.jac for p in pts), len(pts), None, off)
    else:
        fn = engine.g1_sum_segmented if group == 1 else engine.g2_sum_segmented
        out, inf = fn(b"".join(p.bytes_or_zero() for p in pts), len(pts), None, off, [1 if p.infinity else 0 for p in pts])
    pb = 96 if group == 1 else 192
    return [Point(None if inf[j] else out[pb * j:pb * (j + 1)], group) for j in range(len(committees))]


def committee_batch_args(committees, sigs):
    """the flattened keys and the signatures of a batch of VerifyAggregateCommon: (jac, keys bytes, npk, offsets, signature bytes)"""
    keys, off = flatten_committees(committees)
    if all_in_memory(keys + sigs):
        return True, b"".join(p.jac for p in keys), len(keys), off, b"".join(s.jac for s in sigs)
    return False, b"".join(p.bytes_or_zero() for p in keys), len(keys), off, b"".join(s.bytes_or_zero() for s in sigs)


def message_table(msgs):
    """equal messages once: (table, the index of msgs[j] in it) -- what the grouped randomised calls take"""
    at, table, idx = {}, [], []
    for x in msgs:
        x = bytes(x)
        if x not in at:
            at[x] = len(table)
            table.append(x)
        idx.append(at[x])
    return table, idx
