"""The searched corpus of tests/tai_corpus.py is what it says: every listed message has the listed try-and-increment counter under the
big-integer oracle (g2.go:1065-1084), the C oracle's HashG2WithDomain is the point at x0 + counter scaled by the cofactor, and every named
batch reaches -- by wave_schedule, the plain model of tai_g2_wave's rounds -- exactly the states tests/test_gpu_tai_search.py needs it for.
A batch that misses its state is a failure of the test data."""
import os

import pytest

import tai_corpus as T
from oracle import pyref as P
from oracle import refcpu as RC


def _x0(msg32):
    return (int.from_bytes(P._sha(msg32 + T.DOMAIN + b"\x01"), "big"), int.from_bytes(P._sha(msg32 + T.DOMAIN + b"\x02"), "big"))


def _is_square(x):
    """x^3 + b a square in Fq2 <=> fq2_sqrt finds a root (fq2.go:198-232)"""
    return P.fq2_sqrt(P.fq2_add(P.fq2_mul(P.fq2_sqr(x), x), P.B_COEFF_FQ2)) is not None


def _counter(msg32):
    x, c = _x0(msg32), 0
    while not _is_square(x):
        x, c = P.fq2_add(x, P.FQ2_ONE), c + 1
    return c


def _scaled(msg32, counter):
    """the wire bytes of ScaleByCofactor of the point at x0 + counter with the y that has Parity() (g2.go:1074-1080), all in pyref"""
    x0 = _x0(msg32)
    x = ((x0[0] + counter) % P.Q, x0[1])
    y = P.fq2_sqrt(P.fq2_add(P.fq2_mul(P.fq2_sqr(x), x), P.B_COEFF_FQ2))
    assert y is not None
    if not P.fq2_parity(y):
        y = P.fq2_neg(y)
    return P.g2_serialize(P.jac_to_affine(P.F2, P.affine_mul(P.F2, (x, y), P.G2_COFACTOR)))


def test_the_table_holds_what_the_tests_need():
    assert T.DOMAIN == bytes(range(1, 9)) and T.message(0) == __import__("hashlib").sha256(b"tai-corpus-0").digest()
    assert all(c in T.COUNTERS for c in range(18))                          # every counter 0 .. 17
    assert all(len(T.COUNTERS[c]) >= 2 for c in (7, 8, 15, 16))            # the round boundaries of the eight-per-round forms
    assert T.MAX_COUNTER >= 17
    flat = [i for idx in T.COUNTERS.values() for i in idx]
    assert len(set(flat)) == len(flat) and all(0 <= i < 1 << 21 for i in flat)
    assert all(idx == sorted(idx) for idx in T.COUNTERS.values())
    assert T.rounds_of_eight([T.MAX_COUNTER]) >= 3


@pytest.mark.parametrize("counter", sorted(T.COUNTERS))
def test_every_listed_message_has_its_counter(counter):
    for i in T.COUNTERS[counter]:
        assert _counter(T.message(i)) == counter, i


def test_the_c_oracle_returns_the_point_at_x0_plus_counter():
    """every message with counter >= 15, and two of each smaller value"""
    picked = T.indices_with(15) + [i for c in range(15) for i in T.COUNTERS[c][:2]]
    for i in picked:
        m = T.message(i)
        assert RC.hash_g2_with_domain(m, T.DOMAIN) == _scaled(m, T.COUNTER_OF[i]), i


def test_the_search_tool_counts_the_same_way():
    import importlib.util
    spec = importlib.util.spec_from_file_location("tai_search", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "tai_search.py"))
    tool = importlib.util.module_from_spec(spec); spec.loader.exec_module(tool)
    assert tool.DOMAIN == T.DOMAIN and 1 << tool.FAMILY_BITS == 1 << 21
    for i in [T.COUNTERS[c][-1] for c in sorted(T.COUNTERS)]:
        assert tool.message(i) == T.message(i) and tool.counter(T.message(i)) == T.COUNTER_OF[i], i


# ---- wave_schedule itself, on cases small enough to follow by hand ----------------------------------------------------------------------
def test_wave_schedule_on_hand_checked_cases():
    r = T.wave_schedule([0] * 64)
    assert len(r) == 1 and r[0]["k"] == 1 and r[0]["idle"] == 0 and r[0]["own_x0"] and r[0]["closes"] == list(range(64))
    r = T.wave_schedule([5])                                                # one message: all 64 candidates in round 0
    assert len(r) == 1 and r[0]["k"] == 64 and r[0]["first"] == {0: 0} and not r[0]["own_x0"]
    r = T.wave_schedule([64])                                               # ... the 65th needs a second round from candidate 64
    assert [x["first"][0] for x in r] == [0, 64]
    r = T.wave_schedule([0, 3, 0])                                          # three: k = 21, one lane idle
    assert len(r) == 1 and r[0]["k"] == 21 and r[0]["idle"] == 1
    r = T.wave_schedule([0] * 61 + [1, 2, 30])                              # 64 -> 3 (k 21, candidates 1 .. 21) -> 1 (k 64, from 22)
    assert [(len(x["open"]), x["k"]) for x in r] == [(64, 1), (3, 21), (1, 64)]
    assert r[1]["first"] == {61: 1, 62: 1, 63: 1} and r[1]["closes"] == [61, 62] and r[2]["first"] == {63: 22}
    r = T.wave_schedule([1] * 33 + [0] * 31)                                # 33 open: still one candidate each, 31 lanes idle
    assert r[1]["k"] == 1 and r[1]["idle"] == 31 and not r[1]["own_x0"]


# ---- the named batches ------------------------------------------------------------------------------------------------------------------
def _schedules(name):
    return [T.wave_schedule(T.counters_of(w)) for w in T.waves_of(T.BATCHES[name])]


def test_every_batch_is_made_of_listed_messages_and_stays_small():
    for name, idx in T.BATCHES.items():
        assert all(i in T.COUNTER_OF for i in idx), name
    assert sum(len(T.BATCHES[b]) for b in T.WAVE_BATCHES) < 600


def test_batch_a_keeps_all_lanes_open_for_three_rounds_and_runs_max_plus_one_rounds():
    idx = T.BATCHES["a"]
    cs = T.counters_of(idx)
    assert len(idx) == 64 and min(cs) >= 2 and max(cs) == T.MAX_COUNTER
    (r,) = _schedules("a")
    assert all(x["own_x0"] and x["k"] == 1 and len(x["open"]) == 64 for x in r[:3])      # rounds 0, 1, 2: all 64 lanes open
    assert len(r) == T.MAX_COUNTER + 1 and all(x["k"] == 1 for x in r)                  # one candidate a round up to the last
    assert [x["first"][0] for x in r] == list(range(T.MAX_COUNTER + 1))
    assert len(r[-1]["open"]) == 33 and r[-1]["closes"] == r[-1]["open"]
    # the wave of 64 DIFFERENT messages: the same three rounds, then wider ranges; a message stays open beyond candidate 12
    idx = T.BATCHES["a_distinct"]
    cs = T.counters_of(idx)
    assert len(set(idx)) == 64 and min(cs) >= 2 and max(cs) == T.MAX_COUNTER
    (r,) = _schedules("a_distinct")
    assert all(x["own_x0"] and len(x["open"]) == 64 for x in r[:3]) and not r[3]["own_x0"]
    assert [(len(x["open"]), x["k"]) for x in r[3:]] == [(58, 1), (52, 1), (46, 1), (40, 1), (34, 1), (28, 2), (16, 4), (4, 16)]   # six of each counter 2 .. 11
    assert any(min(x["first"].values()) > 12 for x in r)


def test_batch_b_closes_on_the_first_and_the_last_candidate_of_two_ranges():
    idx = T.BATCHES["b"]
    cs = T.counters_of(idx)
    assert len(idx) == 64 and sorted(c for c in cs if c) == [1, 4, 7, 8, 10, 13, 16, 17, 18]
    (r,) = _schedules("b")
    assert [(len(x["open"]), x["k"], x["idle"]) for x in r] == [(64, 1, 0), (9, 7, 1), (6, 10, 4), (1, 64, 0)]
    assert set(r[1]["first"].values()) == {1} and sorted(cs[m] for m in r[1]["closes"]) == [1, 4, 7]          # range 1 .. 7
    assert set(r[2]["first"].values()) == {8} and sorted(cs[m] for m in r[2]["closes"]) == [8, 10, 13, 16, 17]  # range 8 .. 17
    assert r[3]["first"] == {47: 18} and r[3]["closes"] == [47]


def test_batches_c_and_d_leave_one_and_three_messages_open():
    (r,) = _schedules("c")
    assert [(len(x["open"]), x["k"], x["idle"]) for x in r] == [(64, 1, 0), (1, 64, 0)] and r[1]["first"] == {41: 1}
    (r,) = _schedules("d")
    assert [(len(x["open"]), x["k"], x["idle"]) for x in r] == [(64, 1, 0), (3, 21, 1)] and r[1]["first"] == {0: 1, 30: 1, 63: 1}
    assert sorted(T.counters_of([T.BATCHES["d"][m] for m in r[1]["closes"]])) == [1, 12, 19]                  # 1: the first candidate of 1 .. 21


def test_batch_e_repeats_messages_within_a_wave():
    idx = T.BATCHES["e"]
    assert len(idx) == 10 and len(set(idx)) == 7
    (r,) = _schedules("e")
    assert [(len(x["open"]), x["k"], x["idle"]) for x in r] == [(10, 6, 4), (4, 16, 0)]
    assert r[1]["open"] == [1, 3, 6, 8] and idx[1] == idx[3] and idx[6] == idx[8] and set(r[1]["first"].values()) == {6}


def test_batches_f_end_in_ragged_waves():
    a, b = _schedules("f1")
    assert len(T.BATCHES["f1"]) == 65 and [(len(x["open"]), x["k"]) for x in a] == [(64, 1), (3, 21)] and [(len(x["open"]), x["k"]) for x in b] == [(1, 64)] and b[0]["first"] == {0: 0}
    assert T.counters_of(T.BATCHES["f1"][64:]) == [17]
    a, b = _schedules("f37")
    assert len(T.BATCHES["f37"]) == 101 and [(len(x["open"]), x["k"], x["idle"]) for x in b] == [(37, 1, 27), (7, 9, 1), (1, 64, 0)]
    assert b[1]["first"][0] == 1 and b[2]["first"] == {0: 10} and T.counters_of(T.BATCHES["f37"][64:])[0] == 14


def test_batch_g_puts_the_largest_counter_at_every_group_position():
    idx = T.BATCHES["g"]
    assert len(idx) == 69 and len(idx) % 8
    for w in range(8):
        cs = T.counters_of(idx[8 * w:8 * w + 8])
        assert cs.index(T.MAX_COUNTER) == w and sorted(cs) == [0, 0, 7, 8, 15, 16, 17, T.MAX_COUNTER], w
        assert T.rounds_of_eight(cs) == T.MAX_COUNTER // 8 + 1 >= 3                       # the groups that finish in round 0 wait two more rounds at least
    assert T.counters_of(idx[64:]) == [16, 0, 7, 15, 8] and T.rounds_of_eight(T.counters_of(idx[64:])) == 3
