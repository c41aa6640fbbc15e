"""-m gpu: the lane-pair pairing kernels with the wave-priority yield (pair_kernels.inc: every wave enters at s_setprio 1 and drops to 0
late in its work).  Priority changes when a wave issues, never what it computes: the results stay those of the oracle at partly filled
workgroups, in a Verify with a bad tuple, and at the one size where two waves actually share every SIMD (65 536 tuples = 2 048 waves)."""
import numpy as np
import pytest

from gpu_common import P, RC, rand_g1, rand_g2, sk_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    """every size through the lane-pair kernels (the switch of test_gpu_pairing.py's four-layout fixture)"""
    from bls_amd import engine
    engine.init(0)
    engine.set_latency_threshold(0); engine.set_quad_threshold(0); engine.set_row_threshold(0, 0)
    yield engine
    engine.set_latency_threshold(8192); engine.set_quad_threshold(16384); engine.set_row_threshold(*engine.ROW_DEFAULT)


@pytest.mark.parametrize("n", [1, 33, 95])
def test_pairing_partly_filled_workgroups(eng, n):
    """32 tuples per workgroup: 1 (one lane pair), 33 (a full group and one pair), 95 (two full groups and 31 pairs)"""
    xs = P.XORShift(900 + n)
    g1 = b"".join(rand_g1(xs) for _ in range(n)); g2 = b"".join(rand_g2(xs) for _ in range(n))
    assert np.array_equal(eng.pairing_batch(g1, g2, n), RC.pairing_batch(g1, g2, n))


def test_g2pubs_verify_with_one_corrupted_tuple(eng):
    """k_miller2_pair + k_final_exp_is_one_pair: 33 tuples, tuple 17 signed over another message"""
    import bls_amd.g2pubs as g2p
    n, bad = 33, 17
    xs = P.XORShift(933)
    msgs, pks, sigs = [], [], []
    for i in range(n):
        sk = sk_bytes(xs)
        m = b"Hello world! 16 characters %d" % i
        pks.append(RC.g2pubs.priv_to_pub(sk)); sigs.append(RC.g2pubs.sign(m, sk))
        msgs.append(m + b"!" if i == bad else m)
    got = g2p.VerifyBatch(msgs, [g2p.NewPublicKeyFromG2(p) for p in pks], [g2p.NewSignatureFromG1(s) for s in sigs])
    assert got == [i != bad for i in range(n)]
    for i in (0, bad, n - 1):
        assert RC.g2pubs.verify(msgs[i], pks[i], sigs[i]) == (i != bad)


def test_64k_pairings_two_waves_per_simd(eng):
    """65 536 tuples: 2 048 waves on 1 024 SIMDs, the grid on which the yield acts.  Every row equals the same inputs run as two 32 768-tuple
    halves (one wave per SIMD: nothing to yield to), and 64 seeded rows equal the oracle's Pairing()."""
    n, base = 65536, 512
    xs = P.XORShift(965)
    sc = b"".join(sk_bytes(xs) for _ in range(2 * base))
    g1b, _ = eng.g1_mul_generator_batch(sc[:32 * base], base)
    g2b, _ = eng.g2_mul_generator_batch(sc[32 * base:], base)
    reps = n // base
    g1 = np.ascontiguousarray(np.tile(g1b, (reps, 1)))                     # tile r pairs P-row i with Q-row (i + r) mod base: all distinct
    g2 = np.ascontiguousarray(np.concatenate([np.roll(g2b, -r, axis=0) for r in range(reps)]))
    out = eng.pairing_batch(g1.reshape(-1), g2.reshape(-1), n)
    h = n // 2
    halves = np.concatenate([eng.pairing_batch(g1[:h].reshape(-1), g2[:h].reshape(-1), h), eng.pairing_batch(g1[h:].reshape(-1), g2[h:].reshape(-1), h)])
    bad = np.nonzero((out != halves).any(axis=1))[0]
    assert bad.size == 0, "rows differing between one 65 536 call and two 32 768 calls: %s" % bad[:8]
    rows = np.sort(np.random.RandomState(965).choice(n, 64, replace=False))
    want = np.concatenate([RC.pairing_batch(g1[i].tobytes(), g2[i].tobytes(), 1) for i in rows])
    assert np.array_equal(out[rows], want)
