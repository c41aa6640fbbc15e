"""-m gpu: BASELINE.json configs at FULL size, checked through size-independent properties (the oracle
needs ~3 ms per pairing, so bit-for-bit comparison is done on seeded samples and the rest through
identities that hold only if every element is right).

config 3: 2^20-point G1 and G2 scalar multiplication + grand sum
config 4: 2^20-signature g2pubs VerifyAggregate with distinct messages (single GPU here; the 8-way shard
          is the same call per rank + the Fq12 partial-product gather)
config 5: 262 144 g1pubs tuples with a corruption schedule
"""
import hashlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from gpu_common import P, RC

pytestmark = pytest.mark.gpu
R = P.R_ORDER
CORES = max(1, min(32, len(os.sched_getaffinity(0))))      # the oracle's C calls release the interpreter lock


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    return engine


def scalars(n, seed):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 0] &= 0x3f                       # < 2^254 < r
    return raw


def to_int_sum(raw):
    """sum of big-endian 256-bit scalars mod r, vectorised over 32-bit words"""
    w = raw.reshape(raw.shape[0], 8, 4).astype(np.uint64)
    words = (w[:, :, 0] << 24) | (w[:, :, 1] << 16) | (w[:, :, 2] << 8) | w[:, :, 3]
    tot = 0
    for j in range(8):
        tot = (tot << 32) + int(words[:, j].sum())
    return tot % R


def test_config3_msm_1m_points(eng):
    n = 1 << 20
    k = scalars(n, 3)
    for gen, mul, summ, msm, ref_mul, pb in [(RC.g1_generator(), eng.g1_mul_batch, eng.g1_sum, eng.g1_msm, RC.g1_mul, 96),
                                              (RC.g2_generator(), eng.g2_mul_batch, eng.g2_sum, eng.g2_msm, RC.g2_mul, 192)]:
        # base points: 4096 distinct multiples of the generator, tiled; scalars all distinct
        base = 4096
        bk = scalars(base, 33)
        bpts, _ = mul(gen * base, bk.reshape(-1), base)
        pts = np.tile(bpts, (n // base, 1))
        out, inf = mul(pts.reshape(-1), k.reshape(-1), n)
        assert not inf.any()
        # (1) bit-for-bit against the oracle: one contiguous 16 384-row block (256 whole workgroups, every lane position) and every
        #     64th row of the whole batch (every workgroup-sized stretch of it), the oracle's cores in parallel
        rows = sorted(set(range(n // 2 - 8192, n // 2 + 8192)) | set(range(0, n, 64)) | {1, 4095, 4096, n - 1})
        with ThreadPoolExecutor(CORES) as ex:
            want = list(ex.map(lambda i: ref_mul(pts[i].tobytes(), k[i].tobytes()), rows))
        bad = [i for i, w in zip(rows, want) if out[i].tobytes() != w]
        assert not bad, bad[:8]
        # (2) grand sum identity: sum_i k_i * (b_{i mod base} G) = (sum_i k_i b_{i mod base}) G  -- wrong in any element => wrong sum
        total = summ(out.reshape(-1), n)
        bints = [int.from_bytes(bk[j].tobytes(), "big") for j in range(base)]
        acc = 0
        kk = k.reshape(n // base, base, 32)
        for j in range(base):
            acc = (acc + bints[j] * to_int_sum(kk[:, j, :])) % R
        assert total == ref_mul(gen, acc.to_bytes(32, "big"))
        # (3) the one-pass multi-scalar multiplication entry point (multiples never leave the device) gives the same point
        assert msm(pts.reshape(-1), k.reshape(-1), n) == total


def test_msm_bucket_method_edge_cases(eng):
    """the bucket method (n >= 2^17) with inputs that leave windows empty or make the sum vanish: short scalars (the upper 12 of the
    16 windows hold the point at infinity), and a multiset {P_i, -P_i} with equal scalars (every window's sum is the point at
    infinity; the result is flagged infinite)."""
    n = 1 << 17
    base = 1024
    bk = scalars(base, 71)
    for gen, mul, msm, ref_mul, pb in [(RC.g1_generator(), eng.g1_mul_batch, eng.g1_msm, RC.g1_mul, 96),
                                       (RC.g2_generator(), eng.g2_mul_batch, eng.g2_msm, RC.g2_mul, 192)]:
        bpts, _ = mul(gen * base, bk.reshape(-1), base)
        pts = np.tile(bpts, (n // base, 1))
        rng = np.random.default_rng(5)
        k = np.zeros((n, 32), dtype=np.uint8)
        k[:, 24:] = rng.integers(0, 256, size=(n, 8), dtype=np.uint8)            # 64-bit scalars
        bints = [int.from_bytes(bk[j].tobytes(), "big") for j in range(base)]
        acc = 0
        kk = k.reshape(n // base, base, 32)
        for j in range(base):
            acc = (acc + bints[j] * to_int_sum(kk[:, j, :])) % R
        assert msm(pts.reshape(-1), k.reshape(-1), n) == ref_mul(gen, acc.to_bytes(32, "big"))
        # second half = negated first half, same scalars: the sum is the point at infinity
        half = n // 2
        neg = pts[:half].copy().reshape(half, pb // 48, 48)
        ycols = range(pb // 96, pb // 48)                                        # the y coordinate's field elements
        for c in ycols:
            y = np.array([int.from_bytes(neg[i, c].tobytes(), "big") for i in range(base)], dtype=object)
            for i in range(base):
                neg[i::base, c] = np.frombuffer(((P.Q - y[i]) % P.Q).to_bytes(48, "big"), dtype=np.uint8)
        both = np.concatenate([pts[:half], neg.reshape(half, pb)])
        k2 = scalars(half, 72)
        assert msm(both.reshape(-1), np.concatenate([k2, k2]).reshape(-1), n) is None


def _distinct_msgs(n):
    idx = np.arange(n, dtype=np.uint64)
    return [hashlib.sha256(int(i).to_bytes(8, "little")).digest() for i in idx]


def test_config4_verify_aggregate_1m(eng):
    import bls_amd.g2pubs as g2p
    n = 1 << 20
    msgs = _distinct_msgs(n)
    # 1024 distinct signers, each signing 1024 distinct messages; sigma = sum_i sk_{i mod 1024} H(m_i)
    nk = 1024
    sk = scalars(nk, 4)
    pks, _ = eng.g2_mul_batch(RC.g2_generator() * nk, sk.reshape(-1), nk)
    for j in (0, nk - 1):
        assert pks[j].tobytes() == RC.g2pubs.priv_to_pub(sk[j].tobytes())
    h = eng.hash_g1_batch(msgs)
    for i in (0, 77777, n - 1):
        assert h[i].tobytes() == RC.hash_g1(msgs[i])
    sks = np.tile(sk, (n // nk, 1))
    sig_pts, inf = eng.g1_mul_batch(h.reshape(-1), sks.reshape(-1), n)
    assert not inf.any()
    agg = eng.g1_sum(sig_pts.reshape(-1), n)
    all_pks = np.tile(pks, (n // nk, 1))
    assert eng.g2pubs_verify_aggregate(msgs, all_pks.reshape(-1), agg) is True
    # one corrupted public key (swap two signers) must flip the verdict
    bad = all_pks.copy(); bad[12345] = all_pks[12346]
    assert eng.g2pubs_verify_aggregate(msgs, bad.reshape(-1), agg) is False
    # a duplicated message gives False (g2pubs/bls.go:245-261) -- here under the aggregate of the original messages, so the pairing equation
    # fails as well and this does not show which of the two rejected; test_gpu_dup_rule.py has the cases where the rule alone decides
    dup = list(msgs); dup[999] = dup[5]
    assert eng.g2pubs_verify_aggregate(dup, all_pks.reshape(-1), agg) is False


@pytest.mark.parametrize("group", ["g2pubs", "g1pubs"])
def test_verify_aggregate_odd_count_on_the_throughput_kernels(eng, group):
    """n = 8195 .. 8192 (above the latency threshold): two tuples share a Miller loop in the throughput kernels, the last one of
    an odd count runs alone; true aggregate -> 1, one swapped key (the last tuple, one in the body) -> 0."""
    n = 8195
    nk = 64
    sk = scalars(nk, 9)
    msgs = _distinct_msgs(n)
    if group == "g2pubs":
        pks, _ = eng.g2_mul_batch(RC.g2_generator() * nk, sk.reshape(-1), nk)
        h = eng.hash_g1_batch(msgs); mul, summ, va = eng.g1_mul_batch, eng.g1_sum, eng.g2pubs_verify_aggregate
    else:
        pks, _ = eng.g1_mul_batch(RC.g1_generator() * nk, sk.reshape(-1), nk)
        h = eng.hash_g2_batch(msgs); mul, summ, va = eng.g2_mul_batch, eng.g2_sum, eng.g1pubs_verify_aggregate
    sks = np.tile(sk, (n // nk + 1, 1))[:n]
    all_pks = np.tile(pks, (n // nk + 1, 1))[:n]
    sig_pts, inf = mul(h.reshape(-1), sks.reshape(-1), n)
    assert not inf.any()
    for m in (n, n - 1, n - 2, n - 3):
        agg = summ(sig_pts[:m].reshape(-1), m)
        assert va(msgs[:m], all_pks[:m].reshape(-1), agg) is True
        bad = all_pks[:m].copy(); bad[m - 1] = all_pks[m - 2]                # the last tuple: the one that runs alone when m is odd
        assert va(msgs[:m], bad.reshape(-1), agg) is False
        bad = all_pks[:m].copy(); bad[100] = all_pks[101]
        assert va(msgs[:m], bad.reshape(-1), agg) is False


def test_config5_g1pubs_256k(eng):
    n = 262144
    nk = 256
    sk = scalars(nk, 5)
    pks, _ = eng.g1_mul_batch(RC.g1_generator() * nk, sk.reshape(-1), nk)
    msgs = [b"Hello world! 16 characters %d" % i for i in range(n)]
    h = eng.hash_g2_batch(msgs)
    assert h[n - 1].tobytes() == RC.hash_g2(msgs[n - 1])
    sks = np.tile(sk, (n // nk, 1))
    sigs, inf = eng.g2_mul_batch(h.reshape(-1), sks.reshape(-1), n)
    assert not inf.any()
    assert sigs[4242].tobytes() == RC.g1pubs.sign(msgs[4242], sks[4242].tobytes())
    all_pks = np.tile(pks, (n // nk, 1))
    # corruption schedule: every 16th tuple broken in rotation (wrong message / wrong key / negated signature)
    expect = np.ones(n, dtype=bool)
    msgs2 = list(msgs); pk2 = all_pks.copy(); sg2 = sigs.copy()
    q = P.Q
    for i in range(15, n, 16):
        expect[i] = False
        kind = (i // 16) % 3
        if kind == 0:
            msgs2[i] = msgs[i] + b"!"
        elif kind == 1:
            pk2[i] = all_pks[(i + 1) % n]
        else:
            for off in (96, 144):
                v = int.from_bytes(sg2[i, off:off + 48].tobytes(), "big")
                sg2[i, off:off + 48] = np.frombuffer(((q - v) % q).to_bytes(48, "big"), dtype=np.uint8)
    ok, bitmap = eng.g1pubs_verify_batch(msgs2, pk2.reshape(-1), sg2.reshape(-1))
    assert np.array_equal(ok, expect)
    assert np.array_equal(np.unpackbits(bitmap, bitorder="little")[:n].astype(bool), expect)
    for i in (15, 31, 47, 100):
        assert RC.g1pubs.verify(msgs2[i], pk2[i].tobytes(), sg2[i].tobytes()) == bool(expect[i])


def test_config5_literal_g1pubs_256k_verify_aggregate(eng):
    """BASELINE configs[4] as worded: "g1pubs path (G2 pubkeys, G1 sigs): 256k aggregate verify" -- ONE
    (*Signature).VerifyAggregate over 262 144 distinct messages (g1pubs/bls.go:252-282): true, one swapped pair of keys
    -> false, a duplicated message -> false (under the aggregate of the original messages: the equation fails there too; the rule on its
    own is test_gpu_dup_rule.py's).  Exercises the k_miller1 + Fq12 product tree path with G2 hashes at size."""
    n = 262144
    nk = 256
    sk = scalars(nk, 55)
    pks, _ = eng.g1_mul_batch(RC.g1_generator() * nk, sk.reshape(-1), nk)
    for j in (0, nk - 1):
        assert pks[j].tobytes() == RC.g1pubs.priv_to_pub(sk[j].tobytes())
    msgs = _distinct_msgs(n)
    h = eng.hash_g2_batch(msgs)
    for i in (0, 131071, n - 1):
        assert h[i].tobytes() == RC.hash_g2(msgs[i])
    sks = np.tile(sk, (n // nk, 1))
    sig_pts, inf = eng.g2_mul_batch(h.reshape(-1), sks.reshape(-1), n)
    assert not inf.any()
    assert sig_pts[777].tobytes() == RC.g1pubs.sign(msgs[777], sks[777].tobytes())
    agg = eng.g2_sum(sig_pts.reshape(-1), n)
    all_pks = np.tile(pks, (n // nk, 1))
    assert eng.g1pubs_verify_aggregate(msgs, all_pks.reshape(-1), agg) is True
    bad = all_pks.copy(); bad[200001] = all_pks[200002]; bad[200002] = all_pks[200001]
    assert eng.g1pubs_verify_aggregate(msgs, bad.reshape(-1), agg) is False
    dup = list(msgs); dup[n - 1] = dup[17]
    assert eng.g1pubs_verify_aggregate(dup, all_pks.reshape(-1), agg) is False
    # the small-n form of the same entry point agrees with the oracle's VerifyAggregate (n + 1 full pairings)
    m8, p8 = msgs[:8], [all_pks[i].tobytes() for i in range(8)]
    a8 = eng.g2_sum(sig_pts[:8].reshape(-1), 8)
    assert eng.g1pubs_verify_aggregate(m8, b"".join(p8), a8) is True and RC.g1pubs.verify_aggregate(a8, p8, m8) is True
