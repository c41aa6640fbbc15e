"""Host-side mirror of the reference package g1pubs (g1pubs/bls.go): PublicKey in G1, Signature in
G2, messages hashed to G2.  Same names, argument meaning and results as the Go API; every group,
pairing and hash operation runs in the HIP kernels of libblsmi.so (no CPU fallback).

    Verify(m, pub, sig)                         g1pubs/bls.go:165-168
    sig.VerifyAggregate(pubKeys, msgs)          g1pubs/bls.go:252-282
    sig.VerifyAggregateCommon(pubKeys, msg)     g1pubs/bls.go:287-290
    AggregateSignatures / AggregatePublicKeys   g1pubs/bls.go:177-204
    DeserializeSignature / DeserializePublicKey g1pubs/bls.go:33-40, 89-96
plus VerifyBatch, the batch form the one-tuple-per-call Go API lacks.
"""
from . import engine
from ._groups import DeserializeError, Point, all_in_memory, committee_batch_args, committee_sums, point_sum, points_valid  # noqa: F401
from ._groups import deserialize_objects, message_table, serialize_points, verify_serialized_randomized

SIG_GROUP, PK_GROUP = 2, 1


class Signature:
    def __init__(self, point):
        self.s = point

    def Serialize(self):                      # g1pubs/bls.go:18-20
        return self.s.serialize()

    def Copy(self):
        return Signature(self.s.copy())

    def Aggregate(self, other):               # g1pubs/bls.go:174-177
        self.s = point_sum([self.s, other.s], SIG_GROUP)

    def VerifyAggregate(self, pubKeys, msgs):
        if len(pubKeys) != len(msgs):          # g1pubs/bls.go:241-243
            return False
        if self.s.infinity or any(p.p.infinity for p in pubKeys):
            return False                       # the reference panics in MillerLoop on infinity; defined as false here
        if all_in_memory([p.p for p in pubKeys] + [self.s]):   # the points as the Go values hold them: ToAffine on the device
            return engine.g1pubs_verify_aggregate_jac(msgs, b"".join(p.p.jac for p in pubKeys), self.s.jac)
        return engine.g1pubs_verify_aggregate(msgs, b"".join(p.p.raw for p in pubKeys), self.s.raw)

    def VerifyAggregateCommon(self, pubKeys, msg):
        if all_in_memory([p.p for p in pubKeys] + [self.s]):   # key sum and Verify in one library call, Jacobian points summed as they are
            return engine.g1pubs_verify_aggregate_common_jac(msg, b"".join(p.p.jac for p in pubKeys), self.s.jac, len(pubKeys))
        return Verify(msg, AggregatePublicKeys(pubKeys), self)


class PublicKey:
    def __init__(self, point):
        self.p = point

    def Serialize(self):                      # g1pubs/bls.go:67-69
        return self.p.serialize()

    def Copy(self):
        return PublicKey(self.p.copy())

    def Equals(self, other):
        return self.p == other.p

    def Aggregate(self, other):               # g1pubs/bls.go:189-192
        self.p = point_sum([self.p, other.p], PK_GROUP)


def NewSignatureFromG2(raw192):
    return Signature(Point(raw192, SIG_GROUP))


def NewPublicKeyFromG1(raw96):
    return PublicKey(Point(raw96, PK_GROUP))


def NewSignatureFromG2Projective(jac288):
    """a Signature holding its point the way the reference's does (g1pubs/bls.go:13-15): the 288 bytes of a *bls.G2Projective"""
    return Signature(Point(None, SIG_GROUP, jac=jac288))


def NewPublicKeyFromG1Projective(jac144):
    """g1pubs/bls.go:53-55: the 144 bytes of a *bls.G1Projective"""
    return PublicKey(Point(None, PK_GROUP, jac=jac144))


def DeserializeSignature(b96):
    return Signature(Point.deserialize(b96, SIG_GROUP))


def DeserializePublicKey(b48):
    return PublicKey(Point.deserialize(b48, PK_GROUP))


def NewAggregateSignature():
    return Signature(Point(None, SIG_GROUP))


def NewAggregatePubkey():
    return PublicKey(Point(None, PK_GROUP))


def AggregateSignatures(sigs):
    return Signature(point_sum([s.s for s in sigs], SIG_GROUP))


def AggregatePublicKeys(pubs):
    return PublicKey(point_sum([p.p for p in pubs], PK_GROUP))


def VerifyBatch(msgs, pubs, sigs):
    """[Verify(msgs[i], pubs[i], sigs[i]) for i] in one launch sequence."""
    n = len(msgs)
    if not (len(pubs) == len(sigs) == n):
        raise ValueError("length mismatch")
    if n == 0:
        return []
    if all_in_memory([p.p for p in pubs] + [s.s for s in sigs]):
        ok, _ = engine.g1pubs_verify_batch_jac(msgs, b"".join(p.p.jac for p in pubs), b"".join(s.s.jac for s in sigs))
        return [bool(x) for x in ok]
    flags = [(1 if p.p.infinity else 0) | (2 if s.s.infinity else 0) for p, s in zip(pubs, sigs)]
    ok, _ = engine.g1pubs_verify_batch(msgs, b"".join(p.p.bytes_or_zero() for p in pubs), b"".join(s.s.bytes_or_zero() for s in sigs), flags)
    return [bool(x) for x in ok]


def VerifyBatchRandomized(msgs, pubs, sigs, scalars=None):
    """VerifyBatch's verdicts from ONE pairing check over the batch with random 64-bit weights (small-exponent batch verification):
    every tuple True when it holds, the per-tuple verdicts when it fails.  Keys and signatures must lie in the prime-order subgroups
    (Deserialize* guarantees it).  scalars: n nonzero 64-bit integers for tests -- soundness is then the caller's; None draws fresh ones."""
    n = len(msgs)
    if not (len(pubs) == len(sigs) == n):
        raise ValueError("length mismatch")
    if n == 0:
        return []
    if all_in_memory([p.p for p in pubs] + [s.s for s in sigs]):
        ok, _, _ = engine.g1pubs_verify_batch_rlc_jac(msgs, b"".join(p.p.jac for p in pubs), b"".join(s.s.jac for s in sigs), scalars)
        return [bool(x) for x in ok]
    flags = [(1 if p.p.infinity else 0) | (2 if s.s.infinity else 0) for p, s in zip(pubs, sigs)]
    ok, _, _ = engine.g1pubs_verify_batch_rlc(msgs, b"".join(p.p.bytes_or_zero() for p in pubs), b"".join(s.s.bytes_or_zero() for s in sigs), flags, scalars)
    return [bool(x) for x in ok]


def VerifyBatchRandomizedGrouped(msgs, msg_idx, pubs, sigs, scalars=None):
    """VerifyBatchRandomized for tuples that share messages: msgs is a table of d messages and tuple i is (msgs[msg_idx[i]], pubs[i], sigs[i]).
    The tuples of one message share one pairing of the combined check (d hashes and Miller loops, not n); the verdicts are those of
    VerifyBatchRandomized on the expanded messages.  The combined path runs at any n: choosing this form is choosing it."""
    n = len(msg_idx)
    if not (len(pubs) == len(sigs) == n):
        raise ValueError("length mismatch")
    if n == 0:
        return []
    if all_in_memory([p.p for p in pubs] + [s.s for s in sigs]):
        ok, _, _ = engine.g1pubs_verify_batch_rlc_grouped_jac(msgs, msg_idx, b"".join(p.p.jac for p in pubs), b"".join(s.s.jac for s in sigs), scalars)
        return [bool(x) for x in ok]
    flags = [(1 if p.p.infinity else 0) | (2 if s.s.infinity else 0) for p, s in zip(pubs, sigs)]
    ok, _, _ = engine.g1pubs_verify_batch_rlc_grouped(msgs, msg_idx, b"".join(p.p.bytes_or_zero() for p in pubs), b"".join(s.s.bytes_or_zero() for s in sigs), flags, scalars)
    return [bool(x) for x in ok]


def VerifyBatchRandomizedGroupedLocate(msgs, msg_idx, pubs, sigs, scalars=None, block=0):
    """VerifyBatchRandomizedGrouped for input an adversary may have touched: every message's tuples are cut into cells of at most `block`
    tuples (0: automatic; else any value >= 1), the combined check runs over the cells' sums, and when it fails one pairing equation per
    cell finds the cells that hold -- only the tuples of the others go through the per-tuple path.  Verdicts as VerifyBatch on the
    expanded messages."""
    n = len(msg_idx)
    if not (len(pubs) == len(sigs) == n):
        raise ValueError("length mismatch")
    if n == 0:
        return []
    if all_in_memory([p.p for p in pubs] + [s.s for s in sigs]):
        ok = engine.g1pubs_verify_batch_rlc_grouped_locate_jac(msgs, msg_idx, b"".join(p.p.jac for p in pubs), b"".join(s.s.jac for s in sigs), scalars, block)[0]
        return [bool(x) for x in ok]
    flags = [(1 if p.p.infinity else 0) | (2 if s.s.infinity else 0) for p, s in zip(pubs, sigs)]
    ok = engine.g1pubs_verify_batch_rlc_grouped_locate(msgs, msg_idx, b"".join(p.p.bytes_or_zero() for p in pubs), b"".join(s.s.bytes_or_zero() for s in sigs), flags, scalars, block)[0]
    return [bool(x) for x in ok]


def VerifyBatchRandomizedLocate(msgs, pubs, sigs, scalars=None, block=0):
    """VerifyBatchRandomized for input an adversary may have touched: when the combined check fails, one pairing equation per block of `block`
    tuples (0: automatic; else even and at least 2) finds the blocks that hold, and only the tuples of the others go through the per-tuple
    path -- a failed check costs the good path plus work proportional to the bad tuples' blocks.  Verdicts as VerifyBatch."""
    n = len(msgs)
    if not (len(pubs) == len(sigs) == n):
        raise ValueError("length mismatch")
    if n == 0:
        return []
    if all_in_memory([p.p for p in pubs] + [s.s for s in sigs]):
        ok = engine.g1pubs_verify_batch_rlc_locate_jac(msgs, b"".join(p.p.jac for p in pubs), b"".join(s.s.jac for s in sigs), scalars, block)[0]
        return [bool(x) for x in ok]
    flags = [(1 if p.p.infinity else 0) | (2 if s.s.infinity else 0) for p, s in zip(pubs, sigs)]
    ok = engine.g1pubs_verify_batch_rlc_locate(msgs, b"".join(p.p.bytes_or_zero() for p in pubs), b"".join(s.s.bytes_or_zero() for s in sigs), flags, scalars, block)[0]
    return [bool(x) for x in ok]


def VerifySerializedBatch(msgs, pub_bytes, sig_bytes):
    """DeserializePublicKey + DeserializeSignature + Verify per tuple, in one device pass over the 48-byte keys and
    96-byte signatures of the wire format.  A tuple whose key or signature does not deserialise (the reference returns
    an error there and Verify is never reached) or is the point at infinity yields False."""
    ok, _, _ = engine.verify_serialized_batch(__name__.rsplit(".", 1)[-1], msgs, b"".join(pub_bytes), b"".join(sig_bytes), True)
    return [bool(x) for x in ok]


def Verify(m, pub, sig):
    return VerifyBatch([m], [pub], [sig])[0]


def Sign(message, key):
    """Sign(message, key) (g1pubs/bls.go:132-135): key = the secret scalar as 32 big-endian bytes (SecretKey.Serialize()).  One call is
    one hash-to-curve plus one windowed multiplication on the latency path; not side-channel hardened (include/blsmi.h)."""
    return SignBatch([message], [key])[0]


def PrivToPub(k):
    """PrivToPub(k) (g1pubs/bls.go:144-146): k = the secret scalar as 32 big-endian bytes."""
    return PrivToPubBatch([k])[0]


def PrivToPubBatch(secret_scalars):
    """pk_i = sk_i * generator (PrivToPub, g1pubs/bls.go:144-146); scalars are 32-byte big-endian."""
    n = len(secret_scalars)
    out, inf = engine.g1_mul_generator_batch(b"".join(secret_scalars), n)
    return [PublicKey(Point(None if inf[i] else out[i].tobytes(), PK_GROUP)) for i in range(n)]


def SignBatch(msgs, secret_scalars):
    """sigma_i = sk_i * HashG2(m_i) (Sign, g1pubs/bls.go:132-135); scalars are 32-byte big-endian."""
    n = len(msgs)
    out, inf = engine.g1pubs_sign_batch(msgs, b"".join(secret_scalars))    # one call: hash, then multiply, on the device
    return [Signature(Point(None if inf[i] else out[i].tobytes(), SIG_GROUP)) for i in range(n)]


# ---- the *WithDomain family (g1pubs/bls.go:138-141, 171-174, 294-311) ---------------------------------
def VerifyWithDomainBatchRandomized(msgs32, pubs, sigs, domain8, scalars=None):
    """VerifyWithDomainBatch's verdicts through one combined pairing check (VerifyBatchRandomized)"""
    n = len(msgs32)
    if not (len(pubs) == len(sigs) == n):
        raise ValueError("length mismatch")
    if n == 0:
        return []
    if all_in_memory([p.p for p in pubs] + [s.s for s in sigs]):
        ok, _ = engine.g1pubs_verify_with_domain_batch_rlc_jac(msgs32, domain8, b"".join(p.p.jac for p in pubs), b"".join(s.s.jac for s in sigs), scalars)
        return [bool(x) for x in ok]
    flags = [(1 if p.p.infinity else 0) | (2 if s.s.infinity else 0) for p, s in zip(pubs, sigs)]
    ok, _ = engine.g1pubs_verify_with_domain_batch_rlc(msgs32, domain8, b"".join(p.p.bytes_or_zero() for p in pubs), b"".join(s.s.bytes_or_zero() for s in sigs), flags, scalars)
    return [bool(x) for x in ok]


def VerifyWithDomainBatchRandomizedGrouped(msgs32, msg_idx, pubs, sigs, domain8, scalars=None):
    """VerifyWithDomainBatchRandomized over a table of d 32-byte messages and n indices into it (VerifyBatchRandomizedGrouped)"""
    n = len(msg_idx)
    if not (len(pubs) == len(sigs) == n):
        raise ValueError("length mismatch")
    if n == 0:
        return []
    if all_in_memory([p.p for p in pubs] + [s.s for s in sigs]):
        ok, _, _ = engine.g1pubs_verify_with_domain_batch_rlc_grouped_jac(msgs32, domain8, msg_idx, b"".join(p.p.jac for p in pubs), b"".join(s.s.jac for s in sigs), scalars)
        return [bool(x) for x in ok]
    flags = [(1 if p.p.infinity else 0) | (2 if s.s.infinity else 0) for p, s in zip(pubs, sigs)]
    ok, _, _ = engine.g1pubs_verify_with_domain_batch_rlc_grouped(msgs32, domain8, msg_idx, b"".join(p.p.bytes_or_zero() for p in pubs), b"".join(s.s.bytes_or_zero() for s in sigs), flags, scalars)
    return [bool(x) for x in ok]


def VerifyWithDomainBatchRandomizedGroupedLocate(msgs32, msg_idx, pubs, sigs, domain8, scalars=None, block=0):
    """VerifyWithDomainBatchRandomizedGrouped that finds the bad tuples by cells (VerifyBatchRandomizedGroupedLocate)"""
    n = len(msg_idx)
    if not (len(pubs) == len(sigs) == n):
        raise ValueError("length mismatch")
    if n == 0:
        return []
    if all_in_memory([p.p for p in pubs] + [s.s for s in sigs]):
        ok = engine.g1pubs_verify_with_domain_batch_rlc_grouped_locate_jac(msgs32, domain8, msg_idx, b"".join(p.p.jac for p in pubs), b"".join(s.s.jac for s in sigs), scalars, block)[0]
        return [bool(x) for x in ok]
    flags = [(1 if p.p.infinity else 0) | (2 if s.s.infinity else 0) for p, s in zip(pubs, sigs)]
    ok = engine.g1pubs_verify_with_domain_batch_rlc_grouped_locate(msgs32, domain8, msg_idx, b"".join(p.p.bytes_or_zero() for p in pubs), b"".join(s.s.bytes_or_zero() for s in sigs), flags, scalars, block)[0]
    return [bool(x) for x in ok]


def VerifyWithDomainBatchRandomizedLocate(msgs32, pubs, sigs, domain8, scalars=None, block=0):
    """VerifyWithDomainBatchRandomized that finds the bad tuples by blocks (VerifyBatchRandomizedLocate)"""
    n = len(msgs32)
    if not (len(pubs) == len(sigs) == n):
        raise ValueError("length mismatch")
    if n == 0:
        return []
    if all_in_memory([p.p for p in pubs] + [s.s for s in sigs]):
        ok = engine.g1pubs_verify_with_domain_batch_rlc_locate_jac(msgs32, domain8, b"".join(p.p.jac for p in pubs), b"".join(s.s.jac for s in sigs), scalars, block)[0]
        return [bool(x) for x in ok]
    flags = [(1 if p.p.infinity else 0) | (2 if s.s.infinity else 0) for p, s in zip(pubs, sigs)]
    ok = engine.g1pubs_verify_with_domain_batch_rlc_locate(msgs32, domain8, b"".join(p.p.bytes_or_zero() for p in pubs), b"".join(s.s.bytes_or_zero() for s in sigs), flags, scalars, block)[0]
    return [bool(x) for x in ok]


def VerifyWithDomainBatch(msgs32, pubs, sigs, domain8):
    n = len(msgs32)
    if n == 0:
        return []
    if all_in_memory([p.p for p in pubs] + [s.s for s in sigs]):
        return [bool(x) for x in engine.g1pubs_verify_with_domain_batch_jac(msgs32, domain8, b"".join(p.p.jac for p in pubs), b"".join(s.s.jac for s in sigs))]
    flags = [(1 if p.p.infinity else 0) | (2 if s.s.infinity else 0) for p, s in zip(pubs, sigs)]
    ok = engine.g1pubs_verify_with_domain_batch(msgs32, domain8, b"".join(p.p.bytes_or_zero() for p in pubs), b"".join(s.s.bytes_or_zero() for s in sigs), flags)
    return [bool(x) for x in ok]


def VerifyWithDomain(m32, pub, sig, domain8):
    return VerifyWithDomainBatch([m32], [pub], [sig], domain8)[0]


def VerifyAggregateCommonWithDomain(sig, pubKeys, msg32, domain8):
    if all_in_memory([p.p for p in pubKeys] + [sig.s]):
        return engine.g1pubs_verify_aggregate_common_with_domain_jac(msg32, domain8, b"".join(p.p.jac for p in pubKeys), sig.s.jac, len(pubKeys))
    return VerifyWithDomain(msg32, AggregatePublicKeys(pubKeys), sig, domain8)


def VerifyAggregateWithDomain(sig, pubKeys, msgs32, domain8):
    if len(pubKeys) != len(msgs32):
        return False
    if sig.s.infinity or any(p.p.infinity for p in pubKeys):
        return False
    if all_in_memory([p.p for p in pubKeys] + [sig.s]):
        return engine.g1pubs_verify_aggregate_with_domain_jac(msgs32, domain8, b"".join(p.p.jac for p in pubKeys), sig.s.jac)
    return engine.g1pubs_verify_aggregate_with_domain(msgs32, domain8, b"".join(p.p.raw for p in pubKeys), sig.s.raw)


def SignWithDomainBatch(msgs32, secret_scalars, domain8):
    n = len(msgs32)
    out, inf = engine.g1pubs_sign_with_domain_batch(msgs32, domain8, b"".join(secret_scalars))
    return [Signature(Point(None if inf[i] else out[i].tobytes(), SIG_GROUP)) for i in range(n)]


def AggregatePublicKeysBatch(committees):
    """[AggregatePublicKeys(c) for c in committees] as one segmented sum on the device"""
    return [PublicKey(p) for p in committee_sums([[k.p for k in c] for c in committees], PK_GROUP)]


def VerifyAggregateCommonBatch(sigs, committees, msgs):
    """[sigs[j].VerifyAggregateCommon(committees[j], msgs[j]) for j] in one call: the committee sums beside the hash, then one verify batch"""
    m = len(sigs)
    if not (len(committees) == len(msgs) == m):
        raise ValueError("length mismatch")
    if m == 0:
        return []
    jac, keys, npk, off, sg = committee_batch_args([[k.p for k in c] for c in committees], [s.s for s in sigs])
    fn = engine.g1pubs_verify_aggregate_common_batch_jac if jac else engine.g1pubs_verify_aggregate_common_batch
    ok, _ = fn(msgs, keys, npk, None, off, sg)
    return [bool(x) for x in ok]


def VerifyAggregateCommonWithDomainBatch(sigs, committees, msgs32, domain8):
    """[VerifyAggregateCommonWithDomain(sigs[j], committees[j], msgs32[j], domain8) for j] in one call"""
    m = len(sigs)
    if not (len(committees) == len(msgs32) == m):
        raise ValueError("length mismatch")
    if m == 0:
        return []
    if any(len(x) != 32 for x in msgs32):
        raise ValueError("messages must be 32 bytes")
    jac, keys, npk, off, sg = committee_batch_args([[k.p for k in c] for c in committees], [s.s for s in sigs])
    fn = engine.g1pubs_verify_aggregate_common_with_domain_batch_jac if jac else engine.g1pubs_verify_aggregate_common_with_domain_batch
    ok, _ = fn(b"".join(bytes(x) for x in msgs32), domain8, keys, npk, None, off, sg)
    return [bool(x) for x in ok]


def VerifyAggregateCommonBatchRandomized(sigs, committees, msgs, scalars=None):
    """VerifyAggregateCommonBatch under ONE pairing equation with random 64-bit weights (scalars: m nonzero integers, or None to have them
    drawn): one Miller loop per distinct message and one final exponentiation; equal messages are put into the table once here.  The
    verdicts are VerifyAggregateCommonBatch's -- when the equation fails, or an item is flagged, they come from its m checks."""
    m = len(sigs)
    if not (len(committees) == len(msgs) == m) or (scalars is not None and len(scalars) != m):
        raise ValueError("length mismatch")
    if m == 0:
        return []
    table, idx = message_table(msgs)
    jac, keys, npk, off, sg = committee_batch_args([[k.p for k in c] for c in committees], [s.s for s in sigs])
    fn = engine.g1pubs_verify_aggregate_common_batch_rlc_jac if jac else engine.g1pubs_verify_aggregate_common_batch_rlc
    return [bool(x) for x in fn(table, idx, keys, npk, None, off, sg, scalars)[0]]


def VerifyAggregateCommonWithDomainBatchRandomized(sigs, committees, msgs32, domain8, scalars=None):
    """VerifyAggregateCommonWithDomainBatch under one pairing equation (VerifyAggregateCommonBatchRandomized)"""
    m = len(sigs)
    if not (len(committees) == len(msgs32) == m) or (scalars is not None and len(scalars) != m):
        raise ValueError("length mismatch")
    if m == 0:
        return []
    if any(len(x) != 32 for x in msgs32):
        raise ValueError("messages must be 32 bytes")
    table, idx = message_table(msgs32)
    jac, keys, npk, off, sg = committee_batch_args([[k.p for k in c] for c in committees], [s.s for s in sigs])
    fn = engine.g1pubs_verify_aggregate_common_with_domain_batch_rlc_jac if jac else engine.g1pubs_verify_aggregate_common_with_domain_batch_rlc
    return [bool(x) for x in fn(table, domain8, idx, keys, npk, None, off, sg, scalars)[0]]


def ValidatePublicKeys(pubs):
    """[pub is on the curve and in the prime-order subgroup] -- what the randomised batch verifications and the default multiplications
    presuppose and Deserialize* guarantees -- for keys built any other way, held in either form, in one call; infinity counts as valid,
    as in the reference's IsOnCurve / IsInCorrectSubgroupAssumingOnCurve"""
    return points_valid([p.p for p in pubs], PK_GROUP)


def ValidateSignatures(sigs):
    return points_valid([s.s for s in sigs], SIG_GROUP)


# ---- the wire format in batches (blsmi 0.15): 48-byte keys and 96-byte signatures <-> objects that hold in-memory points ----------------------
def DeserializePublicKeys(blobs):
    """[DeserializePublicKey(b) for b in blobs] in one library call -> (keys, errors): errors[i] is the decode error code (0: fine; the
    messages: _groups._DECODE_ERRORS) and keys[i] is None where it is not 0.  The keys hold in-memory points: every batch call takes them as
    they are."""
    return deserialize_objects(blobs, PK_GROUP, PublicKey)


def DeserializeSignatures(blobs):
    return deserialize_objects(blobs, SIG_GROUP, Signature)


def SerializePublicKeys(pubs):
    """[pub.Serialize() for pub in pubs] in one library call: ToAffine and Compress on the device"""
    return serialize_points([p.p for p in pubs], PK_GROUP)


def SerializeSignatures(sigs):
    return serialize_points([s.s for s in sigs], SIG_GROUP)


def VerifySerializedBatchRandomized(msgs, pub_bytes, sig_bytes, block=0):
    """VerifySerializedBatch's verdicts by VerifyBatchRandomizedLocate: the keys and signatures are deserialised (subgroup check included) into
    in-memory points on the device and go through the combined check.  A tuple with an undecodable element gets False and sends only its own
    block of `block` tuples (0: automatic; else even and at least 2) through the per-tuple path."""
    return [bool(x) for x in verify_serialized_randomized(__name__.rsplit(".", 1)[-1], PK_GROUP, SIG_GROUP, msgs, pub_bytes, sig_bytes, block)[0]]
