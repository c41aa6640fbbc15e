"""-m gpu: every device form of HashG2WithDomain's try-and-increment search (g2.go:1041-1085) at CHOSEN search counters.

hash.cuh has four forms of the loop; which of their code runs depends on the counter at which x0 + counter first gives a square, and a
random message has counter >= c with probability 2^-c.  tests/tai_corpus.py holds messages found by search (tools/tai_search.py) with every
counter 0 .. 20 and 25, and batches laid out so that a form reaches a given state; tests/test_tai_corpus_cpu.py proves the counters and the
states on the CPU.  Here every output record of every call is compared byte for byte with the oracle's HashG2WithDomain, and the form is
confirmed by the kernel names of blsmi_last_profile:

  k_tai_g2_waves8                 eight waves a message: up to 4 rounds (counter 25), the LDS verdict words re-used, the stride of a round
  k_tai_g2_lanes8 + k_lat:cofac2  eight lanes a message: 4 rounds, early finishers wait, the slowest message at every group position
  k_tai_g2_wave + k_cofac2_pair   the wave shares its open messages' candidates: 26 rounds of one candidate, k = 7, 10, 21, 64, ragged waves
  k_hash_g2_domain_redo           one lane a message: finished lanes keep their point while the wave goes on to counter 25
"""
import numpy as np
import pytest

import tai_corpus as T
from gpu_common import P, RC, sk_bytes
from test_gpu_miller_variants import names_of

pytestmark = pytest.mark.gpu

_WANT = {}


def want(i):
    """the oracle's 192 bytes for message(i), computed once"""
    if i not in _WANT:
        _WANT[i] = RC.hash_g2_with_domain(T.message(i), T.DOMAIN)
    return _WANT[i]


def check(out, indices, what):
    assert out.shape == (len(indices), 192)
    for r, i in enumerate(indices):
        assert out[r].tobytes() == want(i), (what, "record", r, "message", i, "counter", T.COUNTER_OF[i])


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    engine.set_latency_threshold(8192)
    yield engine
    engine.set_latency_threshold(8192)


def hashed(eng, indices, threshold, kernels, what):
    """HashG2WithDomain of the messages at this latency threshold -> the records, after checking the call ran `kernels`"""
    try:
        eng.set_latency_threshold(threshold)
        out, names = names_of(eng, lambda: eng.hash_g2_with_domain_batch(T.messages(indices), T.DOMAIN))
    finally:
        eng.set_latency_threshold(8192)
    assert all(k in names for k in kernels), (what, names)
    return out


WAVES8 = ("k_tai_g2_waves8", "k_lat:cofac2")
LANES8 = ("k_tai_g2_lanes8", "k_lat:cofac2")
SHARED = ("k_tai_g2_wave", "k_cofac2_pair")


def test_eight_waves_per_message_beyond_the_first_round(eng):
    """k_tai_g2_waves8 (calls of up to 128 messages): every corpus message with counter >= 7 -- a call of its own each, all in one call, and
    with counter-0 messages up to the hand-over size.  Counters 8 .. 15 take a second round, 16 .. 20 a third, 25 a fourth: the stride
    `step`, the verdict words written again after the barrier, the winner scan after a round without one."""
    idx = T.indices_with(7)
    assert T.rounds_of_eight(T.counters_of(idx)) == 4 and len(idx) <= 128
    for i in idx:
        check(hashed(eng, [i], 8192, WAVES8, "single"), [i], "single")
    check(hashed(eng, idx, 8192, WAVES8, "together"), idx, "together")
    full = (idx[::-1] + T.COUNTERS[0])[:128]                                # the largest call the form serves, the slow messages first
    check(hashed(eng, full, 8192, WAVES8, "128"), full, "128")


def test_eight_lanes_per_message_with_the_slowest_message_at_every_group_position(eng):
    """k_tai_g2_lanes8 + the cofac2 level program (129 messages and more at the default threshold): batch (g) -- waves of eight messages with
    counters 0, 7, 8, 15, 16, 17 and 25, the 25 at each of the eight group positions in turn (`pass >> base` for base 0 .. 56), groups that
    finish in round 0 holding their winner through three more rounds -- padded with counter-0 messages to 133, no multiple of eight"""
    g = T.BATCHES["g"]
    idx = g + T.COUNTERS[0][:133 - len(g)]
    assert len(idx) == 133
    check(hashed(eng, idx, 8192, LANES8, "g"), idx, "g")
    idx = T.COUNTERS[0][:61] + g                                            # ... and with the ragged wave of (g) at the very end of the call
    assert len(idx) == 130
    check(hashed(eng, idx, 8192, LANES8, "g at the end"), idx, "g at the end")


@pytest.mark.parametrize("name", T.WAVE_BATCHES + ["all"])
def test_shared_wave_search_in_the_states_of_the_named_batches(eng, name):
    """k_tai_g2_wave + k_cofac2_pair (latency threshold 0): the batches (a) .. (f) of tests/tai_corpus.py, whose rounds -- open counts, candidates
    per message, who closes where -- tests/test_tai_corpus_cpu.py derives from the model; each as a call of its own, then all in one call"""
    idx = [i for b in T.WAVE_BATCHES for i in T.BATCHES[b]] if name == "all" else T.BATCHES[name]
    assert len(idx) < 600
    check(hashed(eng, idx, 0, SHARED, name), idx, name)


def test_one_lane_loop_keeps_finished_lanes_while_the_wave_goes_on(eng):
    """hash_g2_with_domain (hash.cuh), one lane per message, the wave looping until its slowest lane is done: 70 messages -- a wave and a ragged
    one -- with counters 0 and 25, through blsmi_debug_hash_redo with every good flag 0.  That entry point launches k_hash_g2_domain_redo
    unconditionally (it leaves no profile mark); the kernel is also the redo pass behind the latency path's cofac2 program.  In the source,
    k_hash_g2_domain -- the fused kernel a start-up switch selects -- calls hash_g2_with_domain_wave, i.e. the SHARED search of the test above
    followed by scale_by_cofactor_g2, not this loop; tests/test_gpu_hash_pair.py and tests/test_gpu_startup_switches.py run it."""
    top = T.COUNTERS[T.MAX_COUNTER][0]
    idx = [top if j % 9 == 4 else T.COUNTERS[0][j % 64] for j in range(70)]
    assert idx[67] == top and idx[69] != top
    out = eng.debug_hash_redo(2, T.messages(idx), np.zeros(70, dtype=np.uint8), np.full((70, 192), 0xAA, dtype=np.uint8), domain8=T.DOMAIN)
    check(out, idx, "one lane")
    flags = np.array([j % 2 for j in range(70)], dtype=np.uint8)            # and every other message left alone
    out = eng.debug_hash_redo(2, T.messages(idx), flags, np.full((70, 192), 0xAA, dtype=np.uint8), domain8=T.DOMAIN)
    for j, i in enumerate(idx):
        assert out[j].tobytes() == (b"\xaa" * 192 if flags[j] else want(i)), j


@pytest.mark.parametrize("threshold,kernels", [(8192, WAVES8), (0, SHARED)], ids=["latency", "throughput"])
def test_sign_and_verify_with_domain_over_the_slowest_messages(eng, threshold, kernels):
    """the consumers of the hash, over the messages with counter >= 15: SignWithDomain gives the oracle's signature bytes (g1pubs/bls.go:138-141),
    VerifyWithDomain accepts them and rejects them under the neighbouring message (g1pubs/bls.go:171-174)"""
    idx = T.indices_with(15)
    n = len(idx)
    xs = P.XORShift(20261020)
    sks = [sk_bytes(xs) for _ in range(n)]
    msgs = T.messages(idx)
    pks = b"".join(RC.g1pubs.priv_to_pub(k) for k in sks)
    sigs = [RC.g1pubs.sign_with_domain(m, k, T.DOMAIN) for m, k in zip(msgs, sks)]
    near = T.messages([i + 1 for i in idx])
    try:
        eng.set_latency_threshold(threshold)
        (got, inf), names = names_of(eng, lambda: eng.g1pubs_sign_with_domain_batch(msgs, T.DOMAIN, b"".join(sks)))
        assert kernels[0] in names, names
        ok, names = names_of(eng, lambda: eng.g1pubs_verify_with_domain_batch(msgs, T.DOMAIN, pks, b"".join(sigs)))
        assert kernels[0] in names, names
        bad = eng.g1pubs_verify_with_domain_batch(near, T.DOMAIN, pks, b"".join(sigs))
    finally:
        eng.set_latency_threshold(8192)
    assert not inf.any()
    for j in range(n):
        assert got[j].tobytes() == sigs[j], (j, idx[j])
    assert ok.all() and not bad.any()
    assert RC.g1pubs.verify_with_domain(msgs[0], pks[:96], sigs[0], T.DOMAIN) and not RC.g1pubs.verify_with_domain(near[0], pks[:96], sigs[0], T.DOMAIN)
